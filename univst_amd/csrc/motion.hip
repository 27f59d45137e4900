// The AnimateDiff-v2 motion module (VanillaTemporalModule -> TemporalTransformer3DModel of backbones/animatediff/models/motion_module.py) as ONE
// host-side graph of the library's gfx950 kernels per call, on the library's own activation order: row (b F + f) N + n, frame-major NHWC.
//
//   h  = proj_in(GroupNorm_per_frame(x))
//   per block:  per Temporal_Self attention:  h += to_out(frame_attention(q|k|v(LN h) + Wqkv pe[f]))      then  h += ff2(geglu(ff1(LN h)))
//   y  = proj_out(h) + x
//
// New kernel here: the attention along the FRAME axis (F <= 32 tokens per (branch, pixel, head)), which reads its rows in place through the frame
// stride N * ldx — no regrouped "(b n) f c" copy of the activations exists.  The norms run on uv_launch_groupnorm / uv_launch_layernorm, the
// projections on uv_launch_gemm (mode 0: bias, residual and GEGLU epilogues).
//
// The position rows: to_q / to_k / to_v have no bias, so W (x + pe_f) = W x + W pe_f.  finalize projects the table once (pe_qkv[f] = Wqkv pe[f],
// fp32 accumulation, fp16 rows) and the attention kernel adds row f to every q|k|v row of frame f as it loads it.
//
// Two owners of the activations: univst_motion_forward carves them from the handle's own arena (Motion::reserve); the AnimateDiff UNet3D graph
// (unet.hip Fwd::motion) calls Motion::run with buffers of ITS arena and its split-K workspace, so the 21 modules of a UNet hold no arena at all.
#include <math.h>
#include <string.h>

#include "kernels.h"
#include "motion.h"

namespace {

constexpr float LOG2E = 1.4426950408889634f;

constexpr int ta_vstr(int KT) { return KT * 16 + 4; }      // halfs per V^T row in LDS (8-byte aligned rows)
// waves per block: eight (all heads of one pixel at 8 heads) unless the V^T images of eight waves would take more than 64 KB of LDS
constexpr int ta_waves(int D, int KT) { return D * ta_vstr(KT) * 2 * 8 <= 64 * 1024 ? 8 : 4; }

// Attention over the F frames of one (branch b, pixel n, head) per WAVE; a block owns TA_WAVES consecutive (pixel, head) items of branch b = blockIdx.y,
// head fastest, so the block's bytes of every frame are one contiguous run of the q|k|v rows.
//   F <= 16 KT: KT tiles of 16 frames (queries and keys alike), D = head dim, padded in REGISTERS to KS 32-wide k steps (40 -> 64, 80 -> 96)
//   scores: S^T tile = K_tile Q_tile^T by KS v_mfma_f32_16x16x32_f16: lane (g, c) = lane (l >> 4, l & 15) holds keys 16 kt + 4g .. + 3 of query c;
//     its operands are 16-byte loads straight from the rows (lane (g, c): frame c of the tile, columns 32 ks + 8g ..), zeros for frames >= F and
//     columns >= D — neither is ever read from memory.
//   softmax in fp32 over registers and the four lane groups g; a padding key f' >= F gets -inf by select, so its probability is an exact 0.
//   O^T = V^T P^T by one v_mfma_f32_16x16x32_f16 per 16 head columns: the score accumulator IS its B operand (k slot 8g + j <-> key 4g + j for j < 4,
//     16 + 4g + j - 4 for j >= 4), so P never moves between lanes.  V^T comes from the wave's own LDS image [D][16 KT + 4], written from 16-byte row
//     loads, with zeros in the key columns F .. 16 KT - 1 (0 x NaN cannot arise).  The result has 4 consecutive head columns of one query per lane.
template <int D, int KT>
__global__ __launch_bounds__(ta_waves(D, KT) * 64) void temporal_attn_kernel(const half_t* __restrict__ qkv, long ldx, const half_t* __restrict__ pe,
                                                                            half_t* __restrict__ out, long ldo, int F, int N, int heads) {
    constexpr int WAVES = ta_waves(D, KT), KS = (D + 31) / 32, DT = (D + 15) / 16, VSTR = ta_vstr(KT), CH = D / 8, NV = (KT * 16 * CH + 63) / 64;
    __shared__ __attribute__((aligned(16))) half_t Vs[WAVES * D * VSTR];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const int b = blockIdx.y, C = heads * D;
    const long item = (long)blockIdx.x * WAVES + w;
    const bool live = item < (long)N * heads;      // (wave uniform; a dead wave only meets the barrier)
    const int n = (int)(item / heads), hd = (int)(item % heads);
    half_t* Vt = Vs + w * D * VSTR;
    const long fs = (long)N * ldx;                 // halfs between the rows of consecutive frames
    const half_t* base = qkv + ((long)b * F * N + n) * ldx + hd * D;
    const half_t* pbase = pe ? pe + hd * D : nullptr;
    const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    const f4 z4 = {0.f, 0.f, 0.f, 0.f};
    // row f, columns col .. col + 7 of part (0 q, 1 k, 2 v), with the projected position row added (one fp16 rounding of the sum)
    auto load8 = [&](int part, int f, int col) {
        h8 v = *reinterpret_cast<const h8*>(base + f * fs + part * C + col);
        if (pbase) v += *reinterpret_cast<const h8*>(pbase + (long)f * 3 * C + part * C + col);
        return v;
    };

    h8 qf[KT][KS], kf[KT][KS];
    float l[KT];
    h8 pb[KT];
    if (live) {
#pragma unroll
        for (int t = 0; t < KT; ++t)
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) {
                const int f = t * 16 + l15, col = ks * 32 + g * 8;
                const bool in = f < F && col < D;
                kf[t][ks] = in ? load8(1, f, col) : zero8;
                qf[t][ks] = in ? load8(0, f, col) : zero8;
            }
        // ---- V rows -> V^T in LDS: chunk idx = (frame, 8 columns); frames F .. 16 KT - 1 are zeros
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = lane + 64 * i, f = idx / CH, c = (idx % CH) * 8;
            if (f < KT * 16) {
                const h8 v = f < F ? load8(2, f, c) : zero8;
#pragma unroll
                for (int e = 0; e < 8; ++e) Vt[(c + e) * VSTR + f] = v[e];
            }
        }
        // ---- scores: sc[kt][qt][r] = <k[16 kt + 4g + r], q[16 qt + l15]>
        f4 sc[KT][KT];
#pragma unroll
        for (int kt = 0; kt < KT; ++kt)
#pragma unroll
            for (int qt = 0; qt < KT; ++qt) {
                sc[kt][qt] = z4;
#pragma unroll
                for (int ks = 0; ks < KS; ++ks) sc[kt][qt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[kt][ks], qf[qt][ks], sc[kt][qt], 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r) sc[kt][qt][r] = kt * 16 + 4 * g + r < F ? sc[kt][qt][r] : -INFINITY;
            }
        // ---- softmax over the keys of query 16 qt + l15: registers, then the four lane groups g
#pragma unroll
        for (int qt = 0; qt < KT; ++qt) {
            float m = -INFINITY;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) m = fmaxf(m, sc[kt][qt][r]);
            m = fmaxf(m, __shfl_xor(m, 16, 64));
            m = fmaxf(m, __shfl_xor(m, 32, 64));      // finite: key 0 exists (F >= 1) and every operand of a padding QUERY is zero
            float sum = 0.f;
#pragma unroll
            for (int kt = 0; kt < KT; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    sc[kt][qt][r] = __builtin_amdgcn_exp2f((sc[kt][qt][r] - m) * LOG2E);      // exp2(-inf) = 0: a padding key
                    sum += sc[kt][qt][r];
                }
            sum += __shfl_xor(sum, 16, 64);
            sum += __shfl_xor(sum, 32, 64);
            l[qt] = sum;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pb[qt][j] = (half_t)sc[0][qt][j];
                pb[qt][4 + j] = KT == 2 ? (half_t)sc[KT - 1][qt][j] : (half_t)0.f;
            }
        }
    }
    __syncthreads();      // the V^T image is complete (every wave reads its own image only)
    if (!live) return;
#pragma unroll
    for (int qt = 0; qt < KT; ++qt) {
        const int f = qt * 16 + l15;
        const float inv = 1.f / l[qt];
        half_t* orow = out + (((long)b * F + f) * N + n) * ldo + hd * D + 4 * g;
#pragma unroll
        for (int dt = 0; dt < DT; ++dt) {
            const int dc = dt * 16 + l15;          // the head column this lane feeds as the A operand's row
            h8 a = zero8;
            if (dc < D) {
                const half_t* vr = Vt + dc * VSTR + 4 * g;
                const h4 lo = *reinterpret_cast<const h4*>(vr);
                const h4 hi = KT == 2 ? *reinterpret_cast<const h4*>(vr + 16) : h4{0, 0, 0, 0};
                a = h8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            }
            const f4 o = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pb[qt], z4, 0, 0, 0);      // o[r]: head column 16 dt + 4g + r of query f
            if (f < F && dt * 16 + 4 * g < D) {    // frames F .. and columns D .. are the kernel's own padding: never stored
                const h4 r = {(half_t)(o[0] * inv), (half_t)(o[1] * inv), (half_t)(o[2] * inv), (half_t)(o[3] * inv)};
                *reinterpret_cast<h4*>(orow + dt * 16) = r;
            }
        }
    }
}

template <int D, int KT>
void ta_launch(const half_t* qkv, long ldx, const half_t* pe, int B, int F, int N, int heads, half_t* out, long ldo, hipStream_t s) {
    constexpr int WAVES = ta_waves(D, KT);
    const unsigned gx = (unsigned)(((long)N * heads + WAVES - 1) / WAVES);
    hipLaunchKernelGGL((temporal_attn_kernel<D, KT>), dim3(gx, (unsigned)B), dim3(WAVES * 64), 0, s, qkv, ldx, pe, out, ldo, F, N, heads);
}

}  // namespace

int uv_launch_temporal_attention(const half_t* qkv, long ldx, const half_t* pe_qkv, int B, int F, int N, int heads, int head_dim, half_t* out, long ldo,
                                 hipStream_t s) {
    UV_REQUIRE(qkv && out, "temporal_attention: null qkv / out");
    UV_REQUIRE(head_dim == 40 || head_dim == 80 || head_dim == 160, "temporal_attention: head_dim=%d (the kernel has 40, 80 and 160)", head_dim);
    UV_REQUIRE(F >= 1 && F <= UV_MOTION_MAX_F, "temporal_attention: F=%d (1 <= F <= %d frames)", F, UV_MOTION_MAX_F);
    UV_REQUIRE(heads >= 1 && heads <= 64, "temporal_attention: heads=%d (1 .. 64)", heads);
    UV_REQUIRE(B >= 1 && B <= 65535 && N >= 1, "temporal_attention: B=%d (1 .. 65535), N=%d (>= 1)", B, N);
    UV_REQUIRE((long)B * F * N < (1L << 31), "temporal_attention: B * F * N = %ld rows (the row index is 31 bits)", (long)B * F * N);
    // grid.x = ceil(N * heads / waves per block), at least N * heads / 8 blocks of at most 512 threads: HIP takes fewer than 2^32 threads per grid dimension
    UV_REQUIRE((long)N * heads <= (1L << 24), "temporal_attention: N * heads = %ld (pixel, head) problems per branch (at most 2^24: the grid's x dimension)",
               (long)N * heads);
    const long C = (long)heads * head_dim;
    UV_REQUIRE(ldx >= 3 * C && ldx % 8 == 0, "temporal_attention: ldx=%ld (>= 3 * heads * head_dim = %ld, a multiple of 8 halfs: 16-byte row loads)", ldx, 3 * C);
    UV_REQUIRE(ldo >= C && ldo % 4 == 0, "temporal_attention: ldo=%ld (>= heads * head_dim = %ld, a multiple of 4 halfs: 8-byte row stores)", ldo, C);
    UV_REQUIRE((reinterpret_cast<uintptr_t>(qkv) & 15) == 0 && (reinterpret_cast<uintptr_t>(pe_qkv) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 7) == 0,
               "temporal_attention: qkv and pe_qkv must be 16-byte aligned, out 8-byte aligned");
    const bool two = F > 16;
#define TA_CASE(D)                                                                                     \
    if (head_dim == D) {                                                                               \
        if (two) ta_launch<D, 2>(qkv, ldx, pe_qkv, B, F, N, heads, out, ldo, s);                       \
        else ta_launch<D, 1>(qkv, ldx, pe_qkv, B, F, N, heads, out, ldo, s);                           \
    }
    TA_CASE(40)
    TA_CASE(80)
    TA_CASE(160)
#undef TA_CASE
    UV_LAUNCH_CHECK();
    return UV_OK;
}

int uv_motion_check_cfg(const univst_motion_cfg& c) {
    UV_REQUIRE(c.channels >= 8 && c.channels <= 2048 && c.channels % 8 == 0, "motion_create: channels %d (a multiple of 8, at most 2048: the LayerNorm kernel's width)", c.channels);
    UV_REQUIRE(c.num_heads >= 1 && c.channels % c.num_heads == 0, "motion_create: channels %d is not a multiple of num_heads %d", c.channels, c.num_heads);
    const int d = c.channels / c.num_heads;
    UV_REQUIRE(d == 40 || d == 80 || d == 160, "motion_create: channels %d / num_heads %d is a head dim of %d; the attention kernel has 40, 80 and 160", c.channels,
               c.num_heads, d);
    UV_REQUIRE(c.norm_groups >= 1 && c.channels % c.norm_groups == 0, "motion_create: channels %d is not a multiple of norm_groups %d", c.channels, c.norm_groups);
    UV_REQUIRE(c.max_len >= 1 && c.max_len <= UV_MOTION_MAX_F, "motion_create: max_len %d must be in 1..%d", c.max_len, UV_MOTION_MAX_F);
    UV_REQUIRE(c.num_blocks >= 1 && c.num_blocks <= 64 && c.attn_per_block >= 0 && c.attn_per_block <= 64, "motion_create: num_blocks %d (1..64), attn_per_block %d (0..64)",
               c.num_blocks, c.attn_per_block);
    UV_REQUIRE(c.position_encoding == 0 || c.position_encoding == 1, "motion_create: position_encoding %d (0 or 1)", c.position_encoding);
    UV_REQUIRE(c.gn_eps > 0.f && c.ln_eps > 0.f, "motion_create: gn_eps %g and ln_eps %g must be positive", (double)c.gn_eps, (double)c.ln_eps);
    return UV_OK;
}

int Motion::finalize(hipStream_t s) {
    clear_derived();
    clear_missing();
    blocks.clear();
    const long C = cfg.channels, L = cfg.max_len;
    const int d = cfg.channels / cfg.num_heads;
    const std::string tt = "temporal_transformer.";
    UV_SHAPED(gn_g, tt + "norm.weight", C);
    UV_SHAPED(gn_b, tt + "norm.bias", C);
    UV_SHAPED(in_w, tt + "proj_in.weight", C, C);
    UV_SHAPED(in_b, tt + "proj_in.bias", C);
    UV_SHAPED(outp_w, tt + "proj_out.weight", C, C);
    UV_SHAPED(outp_b, tt + "proj_out.bias", C);
    // the sinusoid of PositionalEncoding (d_model = C): pe[f][2i] = sin(f w_i), pe[f][2i + 1] = cos(f w_i), w_i = 10000^(-2i / C)
    std::vector<half_t> pe_host;
    if (cfg.position_encoding) {
        pe_host.resize((size_t)(L * C));
        for (long f = 0; f < L; ++f)
            for (long c = 0; c < C; ++c) {
                const double ang = (double)f * exp((double)(c & ~1L) * (-log(10000.0) / (double)C));
                pe_host[(size_t)(f * C + c)] = (half_t)(float)((c & 1) ? cos(ang) : sin(ang));
            }
    }
    for (int bl = 0; bl < cfg.num_blocks; ++bl) {
        const std::string p = tt + "transformer_blocks." + std::to_string(bl) + ".";
        MotionBlock Bk;
        for (int i = 0; i < cfg.attn_per_block; ++i) {
            const std::string a = p + "attention_blocks." + std::to_string(i) + ".";
            MotionAttn A;
            UV_SHAPED(A.ln_g, p + "norms." + std::to_string(i) + ".weight", C);
            UV_SHAPED(A.ln_b, p + "norms." + std::to_string(i) + ".bias", C);
            UV_SHAPED(A.out_w, a + "to_out.0.weight", C, C);
            UV_SHAPED(A.out_b, a + "to_out.0.bias", C);
            const half_t *qw, *kw, *vw;
            UV_SHAPED(qw, a + "to_q.weight", C, C);
            UV_SHAPED(kw, a + "to_k.weight", C, C);
            UV_SHAPED(vw, a + "to_v.weight", C, C);
            // fused q|k|v projection [3C, C]; the score scale d^-0.5 rides on the q rows, which leaves the kernel the factor log2(e) only
            UV_RUN(derive_concat(a + "#qkv_w", {qw, kw, vw}, C, C, s, 1.f / sqrtf((float)d), &A.qkv_w));
            A.pe_qkv = nullptr;
            if (cfg.position_encoding) {
                // the table: a checkpoint's pos_encoder.pe [1, max_len, C] when it was loaded, else the formula; then pe_qkv[f] = Wqkv pe[f]
                const half_t* pe = nullptr;
                if (find(a + "pos_encoder.pe")) UV_SHAPED(pe, a + "pos_encoder.pe", 1, L, C);
                else {
                    half_t* dpe;
                    UV_RUN(derive(a + "#pe", {L, C}, &dpe));
                    UV_HIP(hipMemcpyAsync(dpe, pe_host.data(), pe_host.size() * sizeof(half_t), hipMemcpyHostToDevice, s));
                    pe = dpe;
                }
                half_t* pq;
                UV_RUN(derive(a + "#pe_qkv", {L, 3 * C}, &pq));
                UV_RUN(uv_launch_gemm(lin_params(pe, L, (int)C, A.qkv_w, (int)(3 * C), pq), 0, s));
                A.pe_qkv = pq;
            }
            Bk.attn.push_back(A);
        }
        UV_SHAPED(Bk.ffn_g, p + "ff_norm.weight", C);
        UV_SHAPED(Bk.ffn_b, p + "ff_norm.bias", C);
        UV_SHAPED(Bk.ff2_w, p + "ff.net.2.weight", C, 4 * C);
        UV_SHAPED(Bk.ff2_b, p + "ff.net.2.bias", C);
        const half_t *w1, *b1;
        UV_SHAPED(w1, p + "ff.net.0.proj.weight", 8 * C, C);
        UV_SHAPED(b1, p + "ff.net.0.proj.bias", 8 * C);
        // GEGLU projection in the row order of the `geglu = 1` epilogue: 16 value rows, then their 16 gate rows
        half_t *gw, *gb;
        UV_RUN(derive(p + "ff.net.0.proj.weight#geglu", {8 * C, C}, &gw));
        UV_RUN(derive(p + "ff.net.0.proj.bias#geglu", {8 * C}, &gb));
        UV_RUN(uv_launch_geglu_interleave(w1, gw, (int)(8 * C), (int)C, s));
        UV_RUN(uv_launch_geglu_interleave(b1, gb, (int)(8 * C), 1, s));
        Bk.ff1_w = gw;
        Bk.ff1_b = gb;
        blocks.push_back(Bk);
    }
    UV_HIP(hipStreamSynchronize(s));      // (pe_host is read by the copies above until here)
    finalized = true;
    return UV_OK;
}

// the activations of one (B, F, N): a new size re-carves the arena (growing the slab synchronises the device); the same size touches nothing
int Motion::reserve(int B, int F, int N) {
    if (B == rB && F == rF && N == rN) return UV_OK;
    rB = rF = rN = 0;
    const long M = (long)B * F * N;
    const int C = cfg.channels;
    // split-K partials of the linears, as the GEMM launcher will plan them: {N, K, geglu, bias, residual} of proj_in, q|k|v, to_out / proj_out, ff1, ff2, with
    // the null pattern run() passes; the 256-aligned norm weight stands in for the operands (run() holds every launch to what is reserved here)
    UV_RUN(uv_plan_splitk_bytes(M, gn_g, {{C, C, 0, 1, 0}, {3 * C, C, 0, 0, 0}, {C, C, 0, 1, 1}, {8 * C, C, 1, 1, 0}, {C, 4 * C, 0, 1, 1}}, &splitk_bytes));
    const size_t mc = (size_t)M * C * 2;
    UV_RUN(carve({{&x[0], mc}, {&x[1], mc}, {&h, mc}, {&att, mc}, {&qkv, (size_t)M * 3 * C * 2}, {&ff, (size_t)M * 4 * C * 2},
                  {&gn_ws, (size_t)uv_groupnorm_workspace_floats(B * F, cfg.norm_groups) * sizeof(float)}, {&splitk, splitk_bytes}}));
    rB = B;
    rF = F;
    rN = N;
    return UV_OK;
}

int Motion::check_shape(const char* who, int B, int F, int N) const {
    UV_REQUIRE(finalized, "%s: call the handle's finalize after loading weights", who);
    UV_REQUIRE(B >= 1 && B <= 65535 && N >= 1, "%s: B=%d (1..65535), N=%d (>= 1)", who, B, N);
    UV_REQUIRE(F >= 1 && F <= UV_MOTION_MAX_F, "%s: F=%d frames (1..%d: what the attention kernel holds)", who, F, UV_MOTION_MAX_F);
    UV_REQUIRE(!cfg.position_encoding || F <= cfg.max_len, "%s: F=%d frames (1..max_len %d: the position table has max_len rows)", who, F, cfg.max_len);
    UV_REQUIRE((long)B * F * N < (1L << 31) / 8, "%s: B * F * N = %ld rows (at most 2^28)", who, (long)B * F * N);
    return UV_OK;
}

int Motion::forward(const half_t* X, half_t* Y, int B, int F, int N, hipStream_t s) {
    UV_REQUIRE(finalized, "motion_forward: call univst_motion_finalize after loading weights");
    UV_REQUIRE(X && Y, "motion_forward: null X / Y");
    UV_RUN(check_shape("motion_forward", B, F, N));
    UV_RUN(reserve(B, F, N));
    MotionBufs b;
    b.x[0] = x[0]; b.x[1] = x[1]; b.h = h; b.att = att; b.qkv = qkv; b.ff = ff;
    b.gn_ws = gn_ws; b.splitk = splitk; b.splitk_bytes = splitk_bytes;
    return run(X, Y, B, F, N, b, s);
}

int Motion::run(const half_t* X, half_t* Y, int B, int F, int N, const MotionBufs& b, hipStream_t s) {
    const long M = (long)B * F * N;
    const int C = cfg.channels;
    const int ncu = uv_num_cus();
    auto linear = [&](const half_t* Xi, int K, const half_t* Wt, const half_t* bias, int Nn, half_t* Yo, const half_t* R, int geglu) {
        const GemmParams g = lin_params(Xi, M, K, Wt, Nn, Yo, bias, R, geglu, b.splitk, b.splitk_bytes);
        // the workspace holds what its owner planned: a launch that wanted more (an operand of another alignment) would allocate behind the caller's back
        const GemmPlan pl = uv_gemm_plan(g, 0, ncu);
        if (pl.rc == UV_OK && pl.ws_bytes > b.splitk_bytes) {
            uv_set_error("motion_forward: the %d x %d linear plans %zu bytes of split-K partials, the workspace holds %zu (X / Y must be 16-byte aligned)", Nn, K,
                         pl.ws_bytes, b.splitk_bytes);
            return UV_ERR_STATE;
        }
        return uv_launch_gemm(g, 0, s);
    };
    half_t* const x[2] = {b.x[0], b.x[1]};
    UV_RUN(uv_launch_groupnorm(X, nullptr, C, 0, M, N, cfg.norm_groups, cfg.gn_eps, gn_g, gn_b, 0, b.h, b.gn_ws, s));
    int cur = 0;
    UV_RUN(linear(b.h, C, in_w, in_b, C, x[cur], nullptr, 0));
    for (const MotionBlock& bk : blocks) {
        for (const MotionAttn& a : bk.attn) {
            UV_RUN(uv_launch_layernorm(x[cur], C, b.h, C, a.ln_g, a.ln_b, M, C, cfg.ln_eps, s));
            UV_RUN(linear(b.h, C, a.qkv_w, nullptr, 3 * C, b.qkv, nullptr, 0));
            UV_RUN(uv_launch_temporal_attention(b.qkv, 3L * C, a.pe_qkv, B, F, N, cfg.num_heads, C / cfg.num_heads, b.att, C, s));
            UV_RUN(linear(b.att, C, a.out_w, a.out_b, C, x[cur ^ 1], x[cur], 0));
            cur ^= 1;
        }
        UV_RUN(uv_launch_layernorm(x[cur], C, b.h, C, bk.ffn_g, bk.ffn_b, M, C, cfg.ln_eps, s));
        UV_RUN(linear(b.h, C, bk.ff1_w, bk.ff1_b, 8 * C, b.ff, nullptr, 1));
        UV_RUN(linear(b.ff, 4 * C, bk.ff2_w, bk.ff2_b, C, x[cur ^ 1], x[cur], 0));
        cur ^= 1;
    }
    return linear(x[cur], C, outp_w, outp_b, C, Y, X, 0);
}
