// MX-fp8 linear for the SD3 q | k | v projections (BASELINE config 5: "MFMA fp8 QKV"), CDNA4 only.
//
// Format: OCP MX, e4m3fn elements, blocks of 32 consecutive K elements, one E8M0 scale byte per block.
//   scale rule  e = floor(log2(amax)) - 8, +1 when amax * 2^-e > 448 (so no element ever saturates); amax == 0 -> e = 0; byte = e + 127
//   elements    x * 2^-e (exact) rounded to e4m3 to nearest even (v_cvt_pk_fp8_f32; the clamp to +-448 is a guard only)
//
//   mxfp8_quantize_kernel   fp16 rows -> e4m3 bytes [rows][K] + E8M0 bytes [rows][K/32]; four lanes per block, 16-byte loads, 8-byte stores
//   linear_mxfp8_kernel     Y[M,N] = deq(X) deq(W)^T + bias on v_mfma_scale_f32_16x16x128_f8f6f4 (cbsz = blgp = 0: e4m3 x e4m3).
//       Two tiles, both 128 deep: 256 x 256 of 8 waves as 4 (M) x 2 (N), 64 x 128 per wave = 4 x 8 MFMA tiles (248 VGPR, 128 KB LDS, one block per
//       CU), taken when M and N are both at least 256; else 128 x 128 of 4 waves as 2 x 2, 64 x 64 per wave (170 VGPR, 64 KB LDS, two blocks per CU).
//       fp32 accumulators, bias in fp32, one rounding on store.
//       Staging is global_load_lds (16-byte form) into two LDS buffers: rows are UNPADDED 128 B (one K tile of one row), the lane-linear
//       image is swizzled on the SOURCE address: 16-byte chunk c of row r sits at chunk c ^ sw(r), sw(r) = (r >> 1) & 7, which makes the
//       fragment reads (lane: row l & 15, chunks g and 4 + g with g = l >> 4, two ds_read_b128) conflict-free for the 16-lane groups of that read.
//       Operand lane map of the scaled MFMA with 8-bit operands, MEASURED (one-block operands with a different scale per block; then held by the
//       exact-value test of tests/test_gpu_mxfp8.py): lane l, row l & 15, g = l >> 4, holds K bytes 16 g .. 16 g + 15 in its first four operand
//       registers and 64 + 16 g .. 64 + 16 g + 15 in the last four — NOT 32 consecutive bytes — while its scale operand is the scale byte of that
//       row's MX block g (K 32 g .. 32 g + 31), in the byte of the VGPR that opsel names.  So a lane's elements belong to blocks g >> 1 and
//       2 + (g >> 1), whose scales lanes of other groups supply.  The four fragments of a wave's operand keep their scale bytes in ONE VGPR
//       (byte i = fragment i).
//       As in gemm.hip the weight is the A operand (D = W X^T), so a lane holds four consecutive n of one row m: 8-byte stores.
#include <type_traits>

#include "common.h"
#include "kernels.h"
#include "../../include/univst.h"

namespace {

typedef int v8i __attribute__((ext_vector_type(8)));
typedef int v4i __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void mxfp8_quantize_kernel(const half_t* __restrict__ X, long ldx, long rows, int K, uint8_t* __restrict__ Q,
                                                              uint8_t* __restrict__ S) {
    const int cpr = K >> 3;                                   // 8-element chunks per row (a multiple of 4: four chunks = one MX block)
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const bool ok = idx < rows * cpr;                         // whole quads are in or out (rows * cpr % 4 == 0): every shuffle partner is live
    const long r = ok ? idx / cpr : 0;
    const int c = ok ? (int)(idx - r * cpr) : 0;
    const h8 v = ok ? *reinterpret_cast<const h8*>(X + r * ldx + (long)c * 8) : h8{0, 0, 0, 0, 0, 0, 0, 0};
    float f[8];
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        f[i] = (float)v[i];
        amax = fmaxf(amax, fabsf(f[i]));
    }
    amax = fmaxf(amax, __shfl_xor(amax, 1, 64));
    amax = fmaxf(amax, __shfl_xor(amax, 2, 64));
    int e = 0;
    if (amax > 0.f) {                                         // an fp16 value, subnormals included, is a normal fp32: the exponent field is floor(log2)
        e = (int)((__float_as_uint(amax) >> 23) & 0xff) - 127 - 8;
        if (ldexpf(amax, -e) > 448.f) ++e;
    }
    int w0 = 0, w1 = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = __builtin_amdgcn_fmed3f(ldexpf(f[i], -e), -448.f, 448.f);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[0], f[1], w0, false);
    w0 = __builtin_amdgcn_cvt_pk_fp8_f32(f[2], f[3], w0, true);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[4], f[5], w1, false);
    w1 = __builtin_amdgcn_cvt_pk_fp8_f32(f[6], f[7], w1, true);
    if (ok) {
        *reinterpret_cast<int2*>(Q + r * K + (long)c * 8) = int2{w0, w1};
        if ((c & 3) == 0) S[r * (K >> 5) + (c >> 2)] = (uint8_t)(e + 127);
    }
}

constexpr int MX_BK = 128;                                  // one scaled MFMA deep: four MX blocks

struct MxParams {
    const uint8_t *Xq, *Xs, *Wq, *Ws;
    const half_t* bias;
    half_t* Y;
    long ldy, M;
    int N, K, tiles_n, tiles;
};

template <int N, class F>
__device__ __forceinline__ void mx_static_for(F&& f) {      // f(integral_constant<int, 0>) .. f(integral_constant<int, N - 1>): opsel is an immediate
    if constexpr (N > 0) {
        mx_static_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// WM x WN waves, each FM x FN MFMA tiles of 16 x 16: a (WM FM 16) x (WN FN 16) x 128 block tile.  FN % 4 == 0 and FM == 4: one scale VGPR per four fragments.
template <int WM, int WN, int FM, int FN>
__global__ __launch_bounds__(WM * WN * 64, 2) void linear_mxfp8_kernel(const MxParams p) {
    constexpr int NW = WM * WN, BM = WM * FM * 16, BN = WN * FN * 16, STAGE = (BM + BN) * MX_BK;
    constexpr int PW = BN / (8 * NW), PX = BM / (8 * NW);               // 8-row staging pieces per wave
    static_assert(FM == 4 && FN % 4 == 0 && BN % (8 * NW) == 0 && BM % (8 * NW) == 0, "tile shape");
    extern __shared__ __attribute__((aligned(16))) uint8_t mx_smem[];
    const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, g = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wave % WM, wn = wave / WM;
    const int bid = xcd_remap(blockIdx.x, p.tiles);
    const int tm = bid / p.tiles_n, tn = bid - tm * p.tiles_n;          // the column tiles of one row tile are neighbours: they share its X rows in L2
    const long m0 = (long)tm * BM;
    const int n0 = tn * BN;
    const int KB = p.K >> 5;                                            // scale bytes per row

    // staging: a wave instruction fills 8 rows x 128 B, lane -> (row lane >> 3, chunk lane & 7) of its piece; wave w owns pieces PW w .. of W, PX w .. of X
    const uint8_t *wsrc[PW], *xsrc[PX];
#pragma unroll
    for (int j = 0; j < PW; ++j) {
        const int row = (wave * PW + j) * 8 + (lane >> 3);
        const int n = min(n0 + row, p.N - 1);                           // rows past the edge re-read the last one; their results are never stored
        wsrc[j] = p.Wq + (long)n * p.K + (((lane & 7) ^ ((row >> 1) & 7)) << 4);
    }
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const int row = (wave * PX + j) * 8 + (lane >> 3);
        const long m = min(m0 + row, p.M - 1);
        xsrc[j] = p.Xq + m * p.K + (((lane & 7) ^ ((row >> 1) & 7)) << 4);
    }
    auto issue_tile = [&](int k0, int buf) {
        uint8_t* wd = mx_smem + buf * STAGE + wave * PW * 1024;
        uint8_t* xd = mx_smem + buf * STAGE + BN * MX_BK + wave * PX * 1024;
#pragma unroll
        for (int j = 0; j < PW; ++j)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(wsrc[j] + k0),
                                             (__attribute__((address_space(3))) void*)(wd + j * 1024), 16, 0, 0);
#pragma unroll
        for (int j = 0; j < PX; ++j)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)(xsrc[j] + k0),
                                             (__attribute__((address_space(3))) void*)(xd + j * 1024), 16, 0, 0);
    };
    // scales: one dword per (row, K tile) = the four block bytes of that tile; the lane needs byte g of the row of each of its fragments
    const uint8_t *wsc[FN], *xsc[FM];
#pragma unroll
    for (int i = 0; i < FN; ++i) wsc[i] = p.Ws + (long)min(n0 + wn * FN * 16 + i * 16 + l15, p.N - 1) * KB;
#pragma unroll
    for (int i = 0; i < FM; ++i) xsc[i] = p.Xs + min(m0 + wm * FM * 16 + i * 16 + l15, p.M - 1) * KB;
    unsigned rs_w[FN], rs_x[FM];
    auto load_scales = [&](int kt) {
#pragma unroll
        for (int i = 0; i < FN; ++i) rs_w[i] = *reinterpret_cast<const unsigned*>(wsc[i] + kt * 4);
#pragma unroll
        for (int i = 0; i < FM; ++i) rs_x[i] = *reinterpret_cast<const unsigned*>(xsc[i] + kt * 4);
    };
    auto pack = [&](const unsigned* rs) {           // byte i <- this lane's block byte of fragment i
        unsigned o = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) o |= ((rs[i] >> (8 * g)) & 0xffu) << (8 * i);
        return (int)o;
    };

    f4 acc[FN][FM];
#pragma unroll
    for (int i = 0; i < FN; ++i)
#pragma unroll
        for (int j = 0; j < FM; ++j) acc[i][j] = f4{0.f, 0.f, 0.f, 0.f};

    const int nk = p.K / MX_BK;
    issue_tile(0, 0);
    load_scales(0);
    const int sw = (l15 >> 1) & 7;
    const int o0 = l15 * MX_BK + ((g ^ sw) << 4), o1 = l15 * MX_BK + (((4 + g) ^ sw) << 4);      // K bytes 16 g .. and 64 + 16 g ..
    auto frag = [&](const uint8_t* base) {
        const v4i lo = *reinterpret_cast<const v4i*>(base + o0), hi = *reinterpret_cast<const v4i*>(base + o1);
        return v8i{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    };
    for (int kt = 0; kt < nk; ++kt) {
        const uint8_t* Wt = mx_smem + (kt & 1) * STAGE + wn * FN * 16 * MX_BK;
        const uint8_t* Xt = mx_smem + (kt & 1) * STAGE + BN * MX_BK + wm * FM * 16 * MX_BK;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's DMA of tile kt (and its scale loads) landed: stated, not left to where the
        __syncthreads();                                      // compiler waits for the scale registers; then every wave's, and buffer (kt + 1) & 1 is free
        int sa[FN / 4];
#pragma unroll
        for (int h = 0; h < FN / 4; ++h) sa[h] = pack(rs_w + 4 * h);
        const int sb = pack(rs_x);
        if (kt + 1 < nk) {                // the next tile's DMA and scale loads fly under this tile's MFMAs
            issue_tile((kt + 1) * MX_BK, (kt + 1) & 1);
            load_scales(kt + 1);
        }
        v8i b[FM];
#pragma unroll
        for (int j = 0; j < FM; ++j) b[j] = frag(Xt + j * 16 * MX_BK);
        mx_static_for<FN / 4>([&](auto hc) {          // four weight fragments at a time: 32 operand VGPRs live, not 8 FN
            constexpr int h = decltype(hc)::value;
            v8i a[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = frag(Wt + (h * 4 + i) * 16 * MX_BK);
            mx_static_for<4>([&](auto ic) {
                mx_static_for<FM>([&](auto jc) {
                    constexpr int i = decltype(ic)::value, j = decltype(jc)::value;
                    acc[h * 4 + i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[i], b[j], acc[h * 4 + i][j], 0, 0, i, sa[h], j, sb);
                });
            });
        });
    }

    // epilogue: the lane holds n = nb + 4 g + r (r < 4) of row m = mb + l15
#pragma unroll
    for (int j = 0; j < FM; ++j) {
        const long m = m0 + wm * FM * 16 + j * 16 + l15;
        if (m >= p.M) continue;
        half_t* row = p.Y + m * p.ldy;
#pragma unroll
        for (int i = 0; i < FN; ++i) {
            const int n = n0 + wn * FN * 16 + i * 16 + g * 4;
            if (n >= p.N) continue;                                     // N % 16 == 0: a 16-column fragment is in or out as a whole
            f4 v = acc[i][j];
            if (p.bias) {
                const h4 bv = *reinterpret_cast<const h4*>(p.bias + n);
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] += (float)bv[r];
            }
            *reinterpret_cast<h4*>(row + n) = h4{(half_t)v[0], (half_t)v[1], (half_t)v[2], (half_t)v[3]};
        }
    }
}

template <int WM, int WN, int FM, int FN>
int mx_launch(MxParams p, const char* sym, hipStream_t s) {
    constexpr int BM = WM * FM * 16, BN = WN * FN * 16;
    const long tiles_m = (p.M + BM - 1) / BM;
    p.tiles_n = (p.N + BN - 1) / BN;
    UV_REQUIRE(tiles_m * p.tiles_n <= 0x7fffffffL, "linear_mxfp8: %ld x %d tiles are too many for one launch", tiles_m, p.tiles_n);
    p.tiles = (int)(tiles_m * p.tiles_n);
    uv_prof_begin(UV_CLS_MXFP8, 2.0 * (double)p.M * p.N * p.K,
                  ((double)p.M + p.N) * p.K * (1.0 + 1.0 / 32) + 2.0 * (double)p.M * p.N, s, sym);
    hipLaunchKernelGGL((linear_mxfp8_kernel<WM, WN, FM, FN>), dim3((unsigned)p.tiles), dim3(WM * WN * 64), 2 * (BM + BN) * MX_BK, s, p);
    uv_prof_end(s);
    UV_LAUNCH_CHECK();
    return UV_OK;
}

}  // namespace

int uv_launch_mxfp8_quantize(const half_t* X, long ldx, long rows, int K, uint8_t* Q, uint8_t* S, hipStream_t s) {
    UV_REQUIRE(X && Q && S, "mxfp8_quantize: null argument");
    UV_REQUIRE(rows >= 1 && K >= 32 && K % 32 == 0, "mxfp8_quantize: rows=%ld must be positive and K=%d a positive multiple of the 32-element MX block",
               rows, K);
    UV_REQUIRE(ldx >= K && ldx % 8 == 0 && ((uintptr_t)X & 15) == 0 && ((uintptr_t)Q & 7) == 0,
               "mxfp8_quantize: ldx=%ld must be a multiple of 8 and at least K=%d, X 16-byte and Q 8-byte aligned", ldx, K);
    const long n = rows * (K / 8);
    UV_REQUIRE((n + 255) / 256 <= 0x7fffffffL, "mxfp8_quantize: rows * K = %ld * %d is too large for one launch", rows, K);
    hipLaunchKernelGGL(mxfp8_quantize_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, X, ldx, rows, K, Q, S);
    UV_LAUNCH_CHECK();
    return UV_OK;
}

int uv_launch_linear_mxfp8(const uint8_t* Xq, const uint8_t* Xs, const uint8_t* Wq, const uint8_t* Ws, const half_t* bias, half_t* Y, long ldy, long M,
                           int N, int K, hipStream_t s) {
    UV_REQUIRE(Xq && Xs && Wq && Ws && Y, "linear_mxfp8: null argument");
    UV_REQUIRE(M >= 1 && N >= 16 && N % 16 == 0 && K >= 128 && K % 128 == 0,
               "linear_mxfp8: M=%ld must be positive, N=%d a multiple of 16 and K=%d a multiple of 128 (one scaled MFMA spans four MX blocks)", M, N, K);
    UV_REQUIRE(ldy >= N && ldy % 4 == 0 && ((uintptr_t)Y & 7) == 0 && ((uintptr_t)bias & 7) == 0,
               "linear_mxfp8: ldy=%ld must be a multiple of 4 and at least N=%d, Y and bias 8-byte aligned", ldy, N);
    UV_REQUIRE((((uintptr_t)Xq | (uintptr_t)Wq) & 15) == 0 && (((uintptr_t)Xs | (uintptr_t)Ws) & 3) == 0,
               "linear_mxfp8: element pointers must be 16-byte and scale pointers 4-byte aligned");
    MxParams p;
    p.Xq = Xq; p.Xs = Xs; p.Wq = Wq; p.Ws = Ws; p.bias = bias; p.Y = Y; p.ldy = ldy; p.M = M; p.N = N; p.K = K;
    // at least two full small tiles each way: the 256 x 256 tile of 8 waves (half the operand traffic per FLOP, twice the MFMAs per barrier); else 128 x 128 of 4
    if (M >= 256 && N >= 256) return mx_launch<4, 2, 4, 8>(p, "linear_mxfp8_kernel<4,2,4,8>", s);
    return mx_launch<2, 2, 4, 4>(p, "linear_mxfp8_kernel<2,2,4,4>", s);
}

extern "C" {

int univst_mxfp8_quantize(const void* X, int64_t ldx, int64_t rows, int K, void* Q, void* S, void* stream) {
    return uv_launch_mxfp8_quantize((const half_t*)X, (long)ldx, (long)rows, K, (uint8_t*)Q, (uint8_t*)S, (hipStream_t)stream);
}

int univst_linear_mxfp8(const void* Xq, const void* Xs, const void* Wq, const void* Ws, const void* bias, void* Y, int64_t ldy, int64_t M, int N, int K,
                        void* stream) {
    return uv_launch_linear_mxfp8((const uint8_t*)Xq, (const uint8_t*)Xs, (const uint8_t*)Wq, (const uint8_t*)Ws, (const half_t*)bias, (half_t*)Y,
                                  (long)ldy, (long)M, N, K, (hipStream_t)stream);
}

}  // extern "C"
