// RAFT-large optical flow (the `flow_fn` of src/cal_optica_flow.py; reference call sites cal_optica_flow.py:51-99 get_warp and
// stable_diffusion.py:731-747, 116 inferences per smoothing step) as ONE host-side graph of gfx950 kernels per image pair.
//
// The network is torchvision's `raft_large` (models/optical_flow/raft.py) — THIRD-PARTY code that is absent from the reference tree and from both
// boxes.  Its structure is restated here from the published definition with that model's state-dict keys, so a stock checkpoint loads as is;
// tests/raft_ref.py is a second restatement (fp32, plain torch) that the kernels are held against.  12 flow updates, final flow only, eval mode.
//
//   encoders   convnormrelu 7x7/2 3->64 | layer1 (64) layer2 (96, /2) layer3 (128, /2): two ResidualBlocks each | conv 1x1 128->256
//              feature encoder: InstanceNorm (per image, per channel; the pair is a batch of two); context encoder: BatchNorm folded into the convs
//   volume     corr[i][j] = <fmap1[i], fmap2[j]> / 16 (fp16 x fp16 -> fp32 MFMA), 4 levels by 2x2 average pooling (floor)
//   12 x       lookup (radius 4, bilinear, zeros outside; channel l*81 + a*9 + b samples x + (a - 4), y + (b - 4)) -> motion encoder ->
//              separable ConvGRU (1x5 then 5x1 over [h | context | motion]) -> flow head -> coords1 += delta
//   upsample   mask predictor on the last hidden state, convex combination of the 3x3 neighbourhood of 8 * flow per 8x8 sub-pixel
//
// Numerics: conv inputs / outputs fp16 with fp32 accumulation; the volume, its lookups, the coordinates, the flow and the GRU state are fp32 (the
// state is rounded to fp16 only where a conv reads it).  The 3x3 and 1x1 convs are the library's NHWC implicit GEMM (gemm.hip, mode 1); the 7x7
// convs (Cin = 3 / 2) and the 1x5 / 5x1 GRU convs gather their operand rows here (im2col) and run as plain GEMMs.
#include <math.h>

#include "kernels.h"
#include "model.h"
#include "raft.h"

namespace {

// ---------------------------------------------------------------- weight preparation
__global__ void r_convert_f16_f32_kernel(const half_t* __restrict__ in, float* __restrict__ out, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (float)in[i];
}
// eval-mode BatchNorm as a per-channel scale / shift of the conv in front of it
__global__ void r_bn_fold_kernel(const float* g, const float* b, const float* mean, const float* var, float* scale, float* shift, int C) {
    int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= C) return;
    const float sc = g[i] / sqrtf(var[i] + 1e-5f);
    scale[i] = sc;
    shift[i] = b[i] - mean[i] * sc;
}
// [Co][Ci][taps] fp32 -> [CoP][Kp] fp16, k = tap * CiP + c, zero padded; scale (may be null): per output channel
__global__ void r_prep_w_kernel(const float* __restrict__ w, const float* __restrict__ scale, half_t* __restrict__ out, int Co, int Ci, int taps, int CiP, int Kp,
                                int CoP) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)CoP * Kp) return;
    const int k = (int)(i % Kp), o = (int)(i / Kp);
    float v = 0.f;
    if (o < Co && k < taps * CiP) {
        const int t = k / CiP, c = k % CiP;
        if (c < Ci) v = w[((long)o * Ci + c) * taps + t] * (scale ? scale[o] : 1.f);
    }
    out[i] = (half_t)v;
}
__global__ void r_prep_b_kernel(const float* __restrict__ b, const float* __restrict__ scale, const float* __restrict__ shift, half_t* __restrict__ out, int Co,
                                int CoP) {
    int o = blockIdx.x * blockDim.x + threadIdx.x;
    if (o >= CoP) return;
    out[o] = o < Co ? (half_t)(b[o] * (scale ? scale[o] : 1.f) + (shift ? shift[o] : 0.f)) : (half_t)0.f;
}

// ---------------------------------------------------------------- im2col of the 7x7 convs (padding 3): rows [imgs*Ho*Wo][Kp], k = (ky*7 + kx)*C + c
// mode 0: uint8 images [imgs][Hs][Ws][3], value / 255 (preprocess_image of the reference); mode 1: coords1 fp32 [Hs][Ws][2], value = coords1 - grid (the flow)
__global__ __launch_bounds__(256) void r_im2col7_kernel(const void* __restrict__ src, int mode, int C, int imgs, int Hs, int Ws, int stride, int Ho, int Wo, int Kp,
                                                        half_t* __restrict__ out) {
    const int kc = Kp / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)imgs * Ho * Wo * kc) return;
    const int ch = (int)(i % kc);
    const long row = i / kc;
    const int ox = (int)(row % Wo), oy = (int)((row / Wo) % Ho), img = (int)(row / ((long)Wo * Ho));
    h8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int k = ch * 8 + e;
        float x = 0.f;
        if (k < 49 * C) {
            const int t = k / C, c = k % C, ky = t / 7, kx = t % 7;
            const int iy = oy * stride + ky - 3, ix = ox * stride + kx - 3;
            if (iy >= 0 && iy < Hs && ix >= 0 && ix < Ws) {
                const long pix = ((long)img * Hs + iy) * Ws + ix;
                if (mode == 0) x = (float)((const uint8_t*)src)[pix * C + c] / 255.0f;
                else x = ((const float*)src)[pix * 2 + c] - (float)(c == 0 ? ix : iy);
            }
        }
        v[e] = (half_t)x;
    }
    *reinterpret_cast<h8*>(out + row * Kp + ch * 8) = v;
}

// ---------------------------------------------------------------- InstanceNorm2d (no affine, eps 1e-5, biased variance) on NHWC [imgs][P][C], per image and channel
__global__ __launch_bounds__(256) void r_in_stats_kernel(const half_t* __restrict__ x, int P, int C, int S, float* __restrict__ part) {
    __shared__ float red[256][17];
    const int c8 = blockIdx.x, sp = blockIdx.y, img = blockIdx.z;
    const long r0 = (long)sp * P / S, r1 = (long)(sp + 1) * P / S;
    float s1[8], s2[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) s1[e] = s2[e] = 0.f;
    for (long r = r0 + threadIdx.x; r < r1; r += 256) {
        const h8 v = *reinterpret_cast<const h8*>(x + ((long)img * P + r) * C + c8 * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const float f = (float)v[e];
            s1[e] += f;
            s2[e] = fmaf(f, f, s2[e]);
        }
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        red[threadIdx.x][e] = s1[e];
        red[threadIdx.x][8 + e] = s2[e];
    }
    __syncthreads();
    if (threadIdx.x < 16) {
        float a = 0.f;
        for (int t = 0; t < 256; ++t) a += red[t][threadIdx.x];
        const int e = threadIdx.x & 7, which = threadIdx.x >> 3;
        part[(((long)img * S + sp) * C + c8 * 8 + e) * 2 + which] = a;
    }
}
__global__ void r_in_finalize_kernel(const float* __restrict__ part, int P, int C, int S, int imgs, float* __restrict__ stat) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= imgs * C) return;
    const int img = i / C, c = i % C;
    double a = 0.0, b = 0.0;
    for (int sp = 0; sp < S; ++sp) {
        a += (double)part[(((long)img * S + sp) * C + c) * 2];
        b += (double)part[(((long)img * S + sp) * C + c) * 2 + 1];
    }
    const double mean = a / P;
    double var = b / P - mean * mean;
    if (var < 0.0) var = 0.0;
    stat[i * 2] = (float)mean;
    stat[i * 2 + 1] = (float)(1.0 / sqrt(var + 1e-5));
}
__global__ __launch_bounds__(256) void r_in_apply_kernel(half_t* __restrict__ x, const float* __restrict__ stat, int P, int C, long n8, int relu) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const int c8 = (int)(i % (C / 8));
    const int img = (int)(i / ((long)(C / 8) * P));
    h8 v = *reinterpret_cast<h8*>(x + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float2 st = *reinterpret_cast<const float2*>(stat + ((long)img * C + c8 * 8 + e) * 2);
        float f = ((float)v[e] - st.x) * st.y;
        if (relu) f = fmaxf(f, 0.f);
        v[e] = (half_t)f;
    }
    *reinterpret_cast<h8*>(x + i * 8) = v;
}

// out = relu(a + b) (b may be null), 8 halfs per thread
__global__ __launch_bounds__(256) void r_add_relu_kernel(const half_t* __restrict__ a, const half_t* __restrict__ b, half_t* __restrict__ out, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    h8 v = *reinterpret_cast<const h8*>(a + i * 8);
    if (b) {
        const h8 w = *reinterpret_cast<const h8*>(b + i * 8);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (half_t)fmaxf((float)v[e] + (float)w[e], 0.f);
    } else {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (half_t)fmaxf((float)v[e], 0.f);
    }
    *reinterpret_cast<h8*>(out + i * 8) = v;
}

// context encoder output [N][256] -> hidden = tanh(first 128) (fp32 state + fp16 copy), context = relu(last 128)
__global__ __launch_bounds__(256) void r_ctx_split_kernel(const half_t* __restrict__ co, float* __restrict__ h32, half_t* __restrict__ h16, half_t* __restrict__ ctx, long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long p = i >> 7;
    const int c = (int)(i & 127);
    const float t = tanhf((float)co[p * 256 + c]);
    h32[i] = t;
    h16[i] = (half_t)t;
    ctx[i] = (half_t)fmaxf((float)co[p * 256 + 128 + c], 0.f);
}

// ---------------------------------------------------------------- all-pairs correlation: out[i][j] = <f1[i], f2[j]> / 16, K = 256, one 64 x 64 tile per block
// (4 waves x (16 rows x 4 column fragments)); the operand rows are read straight into MFMA registers (16 bytes per lane), reuse comes out of L2
__global__ __launch_bounds__(256) void r_corr_kernel(const half_t* __restrict__ f1, const half_t* __restrict__ f2, float* __restrict__ out, int N) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const int i0 = blockIdx.y * 64 + wave * 16, j0 = blockIdx.x * 64;
    const int ai = i0 + l15;
    f4 acc[4];
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[f] = f4{0.f, 0.f, 0.f, 0.f};
    const h8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int ks = 0; ks < 8; ++ks) {
        const h8 a = ai < N ? *reinterpret_cast<const h8*>(f1 + (long)ai * 256 + ks * 32 + g * 8) : zero;
#pragma unroll
        for (int f = 0; f < 4; ++f) {
            const int bj = j0 + f * 16 + l15;
            const h8 b = bj < N ? *reinterpret_cast<const h8*>(f2 + (long)bj * 256 + ks * 32 + g * 8) : zero;
            acc[f] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, acc[f], 0, 0, 0);
        }
    }
#pragma unroll
    for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = i0 + g * 4 + r, col = j0 + f * 16 + l15;
            if (row < N && col < N) out[(long)row * N + col] = acc[f][r] * 0.0625f;
        }
}
// 2x2 / stride-2 average pooling of the last two axes of [N][hl][wl] (floor: an odd last row / column is dropped)
__global__ __launch_bounds__(256) void r_pool_kernel(const float* __restrict__ in, float* __restrict__ out, long N, int hl, int wl) {
    const int ho = hl / 2, wo = wl / 2;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N * ho * wo) return;
    const int x = (int)(i % wo), y = (int)((i / wo) % ho);
    const long p = i / ((long)wo * ho);
    const float* r = in + (p * hl + 2 * y) * wl + 2 * x;
    out[i] = ((r[0] + r[1]) + (r[wl] + r[wl + 1])) * 0.25f;
}

// ---------------------------------------------------------------- pyramid lookup: one block per pixel, 4 levels x 9 x 9 bilinear samples of its correlation rows.
// Threads walk x fastest (a pixel's window is contiguous in x inside a level: 9 taps of a row = two or three 64-byte segments), the 324 values are
// transposed to the channel order l*81 + a*9 + b (a moves x) through LDS and leave as one contiguous row.
__global__ __launch_bounds__(128) void r_lookup_kernel(const float* __restrict__ pyr, const float* __restrict__ coords, int hh, int ww, float* __restrict__ out32,
                                                       half_t* __restrict__ out16) {
    __shared__ float val[328];
    const long N = (long)hh * ww, p = blockIdx.x;
    const float cx = coords[p * 2], cy = coords[p * 2 + 1];
    for (int t = threadIdx.x; t < 328; t += 128) {
        float r = 0.f;
        int ch = t;
        if (t < 324) {
            const int l = t / 81, rem = t % 81, b = rem / 9, a = rem % 9;
            ch = l * 81 + a * 9 + b;
            long off = 0;
            for (int m = 0; m < l; ++m) off += N * (hh >> m) * (ww >> m);
            const int hl = hh >> l, wl = ww >> l;
            const float* lv = pyr + off + p * hl * wl;
            const float sc = 1.f / (float)(1 << l);
            const float x = cx * sc + (float)(a - 4), y = cy * sc + (float)(b - 4);
            const float xf = floorf(x), yf = floorf(y);
            if (xf >= -1.f && xf < (float)wl && yf >= -1.f && yf < (float)hl) {        // (also false for NaN coordinates)
                const int x0 = (int)xf, y0 = (int)yf;
                const float wx1 = x - xf, wx0 = (xf + 1.f) - x, wy1 = y - yf, wy0 = (yf + 1.f) - y;
                const bool xa = x0 >= 0, xb = x0 + 1 < wl, ya = y0 >= 0, yb = y0 + 1 < hl;
                const float nw = (xa && ya) ? lv[y0 * wl + x0] : 0.f, ne = (xb && ya) ? lv[y0 * wl + x0 + 1] : 0.f;
                const float sw = (xa && yb) ? lv[(y0 + 1) * wl + x0] : 0.f, se = (xb && yb) ? lv[(y0 + 1) * wl + x0 + 1] : 0.f;
                r = nw * (wx0 * wy0) + ne * (wx1 * wy0) + sw * (wx0 * wy1) + se * (wx1 * wy1);
            }
        }
        val[ch] = r;
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 328; t += 128) {
        if (out32 && t < 324) out32[p * 324 + t] = val[t];
        if (out16) out16[p * 328 + t] = (half_t)val[t];
    }
}

// ---------------------------------------------------------------- separable ConvGRU
// operand rows of a 1x5 (dir 0) / 5x1 (dir 1) conv over the virtual concat [h | context | motion] (3 x 128 channels): [N][5][384]; zr != null: the h part is
// r (.) h with r = sigmoid(zr[.][128 + c]) (the convq input)
__global__ __launch_bounds__(256) void r_gru_im2col_kernel(const float* __restrict__ h32, const half_t* __restrict__ ctx, const half_t* __restrict__ mot,
                                                           const half_t* __restrict__ zr, int dir, int hh, int ww, half_t* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)hh * ww * 240) return;
    const int ch = (int)(i % 48), tap = (int)((i / 48) % 5);
    const long p = i / 240;
    const int x = (int)(p % ww) + (dir == 0 ? tap - 2 : 0), y = (int)(p / ww) + (dir == 1 ? tap - 2 : 0);
    h8 v = {0, 0, 0, 0, 0, 0, 0, 0};
    if (x >= 0 && x < ww && y >= 0 && y < hh) {
        const long q = (long)y * ww + x;
        if (ch < 16) {
            const float* hp = h32 + q * 128 + ch * 8;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                float f = hp[e];
                if (zr) f *= 1.f / (1.f + expf(-(float)zr[q * 256 + 128 + ch * 8 + e]));
                v[e] = (half_t)f;
            }
        } else if (ch < 32) {
            v = *reinterpret_cast<const h8*>(ctx + q * 128 + (ch - 16) * 8);
        } else {
            v = *reinterpret_cast<const h8*>(mot + q * 128 + (ch - 32) * 8);
        }
    }
    *reinterpret_cast<h8*>(out + p * 1920 + tap * 384 + ch * 8) = v;
}
// h <- (1 - z) h + z tanh(q), z = sigmoid(zr[.][c]); fp32 state + the fp16 copy the next convs read
__global__ __launch_bounds__(256) void r_gru_blend_kernel(const half_t* __restrict__ zr, const half_t* __restrict__ qpre, float* __restrict__ h32, half_t* __restrict__ h16,
                                                          long n) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const long p = i >> 7;
    const int c = (int)(i & 127);
    const float z = 1.f / (1.f + expf(-(float)zr[p * 256 + c]));
    const float q = tanhf((float)qpre[i]);
    const float h = (1.f - z) * h32[i] + z * q;
    h32[i] = h;
    h16[i] = (half_t)h;
}

// ---------------------------------------------------------------- coordinates
__global__ void r_init_coords_kernel(float* __restrict__ c, int hh, int ww) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hh * ww) return;
    *reinterpret_cast<float2*>(c + (long)i * 2) = float2{(float)(i % ww), (float)(i / ww)};
}
// motion[.][126..127] = flow = coords1 - coords0 (cat[conv out, flow] of the motion encoder)
__global__ void r_set_flow_kernel(half_t* __restrict__ motion, const float* __restrict__ c, int hh, int ww) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= hh * ww) return;
    h2 v;
    v[0] = (half_t)(c[(long)i * 2] - (float)(i % ww));
    v[1] = (half_t)(c[(long)i * 2 + 1] - (float)(i / ww));
    *reinterpret_cast<h2*>(motion + (long)i * 128 + 126) = v;
}
__global__ void r_update_coords_kernel(float* __restrict__ c, const half_t* __restrict__ delta, long N) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= N) return;
    float2 v = *reinterpret_cast<float2*>(c + i * 2);
    v.x += (float)delta[i * 8];
    v.y += (float)delta[i * 8 + 1];
    *reinterpret_cast<float2*>(c + i * 2) = v;
}

// ---------------------------------------------------------------- convex upsampling: out[8y+i][8x+j] = sum_k softmax_k(0.25 mask[p][k*64 + i*8 + j]) * 8 flow[y+ky-1][x+kx-1]
// (zeros outside: F.unfold padding 1).  One thread per (pixel, sub-pixel): the 64 sub-pixels of a tap are one contiguous 128-byte read.
__global__ __launch_bounds__(256) void r_upsample_kernel(const float* __restrict__ flow, int is_coords, const half_t* __restrict__ mask, int hh, int ww,
                                                         float* __restrict__ out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)hh * ww * 64) return;
    const int sp = (int)(i & 63);
    const long p = i >> 6;
    const int x = (int)(p % ww), y = (int)(p / ww);
    float m[9], mx = -INFINITY;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        m[k] = 0.25f * (float)mask[p * 576 + k * 64 + sp];
        mx = fmaxf(mx, m[k]);
    }
    float den = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        m[k] = expf(m[k] - mx);
        den += m[k];
    }
    float fx = 0.f, fy = 0.f;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        const int yy = y + k / 3 - 1, xx = x + k % 3 - 1;
        if (yy < 0 || yy >= hh || xx < 0 || xx >= ww) continue;
        float2 f = *reinterpret_cast<const float2*>(flow + ((long)yy * ww + xx) * 2);
        if (is_coords) {
            f.x -= (float)xx;
            f.y -= (float)yy;
        }
        const float w = m[k] / den;
        fx = fmaf(w, 8.f * f.x, fx);
        fy = fmaf(w, 8.f * f.y, fy);
    }
    const int oy = y * 8 + (sp >> 3), ox = x * 8 + (sp & 7);
    *reinterpret_cast<float2*>(out + ((long)oy * ww * 8 + ox) * 2) = float2{fx, fy};
}

}  // namespace

// ================================================================== stand-alone stages
long uv_raft_pyramid_floats(int hh, int ww) {
    long n = 0;
    for (int l = 0; l < 4; ++l) n += (long)hh * ww * (hh >> l) * (ww >> l);
    return n;
}
int uv_raft_corr_pyramid(const half_t* f1, const half_t* f2, int hh, int ww, float* pyr, hipStream_t s) {
    UV_REQUIRE(hh >= 16 && ww >= 16 && (long)hh * ww <= 65535L * 64, "raft_corr_pyramid: feature map %d x %d (at least 16 x 16)", hh, ww);
    const int N = hh * ww;
    const unsigned t = (unsigned)((N + 63) / 64);
    hipLaunchKernelGGL(r_corr_kernel, dim3(t, t), dim3(256), 0, s, f1, f2, pyr, N);
    float* lv = pyr;
    for (int l = 0; l < 3; ++l) {
        const int hl = hh >> l, wl = ww >> l;
        float* nx = lv + (long)N * hl * wl;
        hipLaunchKernelGGL(r_pool_kernel, dim3(nb((long)N * (hl / 2) * (wl / 2))), dim3(256), 0, s, lv, nx, (long)N, hl, wl);
        lv = nx;
    }
    UV_LAUNCH_CHECK();
    return UV_OK;
}
int uv_raft_corr_lookup(const float* pyr, const float* coords, int hh, int ww, float* out32, half_t* out16, hipStream_t s) {
    UV_REQUIRE(hh >= 16 && ww >= 16 && (out32 || out16), "raft_corr_lookup: feature map %d x %d (at least 16 x 16), one output", hh, ww);
    hipLaunchKernelGGL(r_lookup_kernel, dim3((unsigned)(hh * ww)), dim3(128), 0, s, pyr, coords, hh, ww, out32, out16);
    UV_LAUNCH_CHECK();
    return UV_OK;
}
int uv_raft_convex_upsample(const float* flow, int is_coords, const half_t* mask, int hh, int ww, float* out, hipStream_t s) {
    UV_REQUIRE(hh > 0 && ww > 0, "raft_convex_upsample: %d x %d", hh, ww);
    hipLaunchKernelGGL(r_upsample_kernel, dim3(nb((long)hh * ww * 64)), dim3(256), 0, s, flow, is_coords, mask, hh, ww, out);
    UV_LAUNCH_CHECK();
    return UV_OK;
}

// ================================================================== the handle
Raft::~Raft() {
    for (auto& kv : weights) (void)hipFree(kv.second.ptr);
    for (void* p : derived) (void)hipFree(p);
    if (slab) (void)hipFree(slab);
    if (splitk) (void)hipFree(splitk);
}

int Raft::load_tensor(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s) {
    UV_REQUIRE(key && dev_ptr && ndim >= 0 && ndim <= 4, "raft_load_tensor: bad arguments");
    UV_REQUIRE(dtype == UNIVST_F16 || dtype == UNIVST_F32, "raft_load_tensor: dtype %d", dtype);
    long n = 1;
    for (int i = 0; i < ndim; ++i) n *= shape[i];
    UV_REQUIRE(n > 0, "%s: empty tensor", key);
    RaftW32 t;
    t.n = n;
    UV_HIP(hipMalloc((void**)&t.ptr, (size_t)n * sizeof(float)));
    if (dtype == UNIVST_F32) UV_HIP(hipMemcpyAsync(t.ptr, dev_ptr, (size_t)n * sizeof(float), hipMemcpyDeviceToDevice, s));
    else hipLaunchKernelGGL(r_convert_f16_f32_kernel, dim3(nb(n)), dim3(256), 0, s, (const half_t*)dev_ptr, t.ptr, n);
    UV_LAUNCH_CHECK();
    auto it = weights.find(key);
    if (it != weights.end()) {
        UV_HIP(hipStreamSynchronize(s));
        (void)hipFree(it->second.ptr);
    }
    weights[key] = t;
    finalized = false;
    return UV_OK;
}

int Raft::finalize(hipStream_t s) {
    UV_HIP(hipStreamSynchronize(s));
    for (void* p : derived) (void)hipFree(p);
    derived.clear();
    convs.clear();
    auto get = [&](const std::string& k, long n) -> const float* {
        auto it = weights.find(k);
        if (it == weights.end()) {
            uv_set_error("raft: weight '%s' was never loaded", k.c_str());
            return nullptr;
        }
        if (it->second.n != n) {
            uv_set_error("raft: weight '%s' has %ld elements, raft_large has %ld", k.c_str(), it->second.n, n);
            return nullptr;
        }
        return it->second.ptr;
    };
    auto dmalloc = [&](size_t bytes) -> void* {
        void* p = nullptr;
        if (hipMalloc(&p, bytes) != hipSuccess) {
            uv_set_error("raft_finalize: out of device memory");
            return nullptr;
        }
        derived.push_back(p);
        return p;
    };
    // name: conv module (weight at name + ".weight"); bn: BatchNorm module or ""; rows [row0, row0 + Co) of the derived conv `dst` (stacked z | r)
    auto prep = [&](const std::string& dst, const std::string& name, const std::string& bn, int Co, int Ci, int taps, int CiP, int Kp, int CoP, int row0) -> int {
        const float *w = get(name + ".weight", (long)Co * Ci * taps), *b = get(name + ".bias", Co);
        if (!w || !b) return UV_ERR_STATE;
        RaftConv& c = convs[dst];
        if (!c.W) {
            c.W = (half_t*)dmalloc((size_t)CoP * Kp * 2);
            c.b = (half_t*)dmalloc((size_t)CoP * 2);
            if (!c.W || !c.b) return UV_ERR_HIP;
            c.Co = c.CoP = CoP;
            c.Ci = Ci;
            c.CiP = CiP;
            c.taps = taps;
            c.Kp = Kp;
        }
        float *scale = nullptr, *shift = nullptr;
        if (!bn.empty()) {
            const float *g = get(bn + ".weight", Co), *be = get(bn + ".bias", Co), *mu = get(bn + ".running_mean", Co), *var = get(bn + ".running_var", Co);
            if (!g || !be || !mu || !var) return UV_ERR_STATE;
            scale = (float*)dmalloc((size_t)Co * 8);
            if (!scale) return UV_ERR_HIP;
            shift = scale + Co;
            hipLaunchKernelGGL(r_bn_fold_kernel, dim3(nb(Co)), dim3(256), 0, s, g, be, mu, var, scale, shift, Co);
        }
        const int rows = row0 ? Co : CoP;       // a stacked second half fills exactly its rows
        hipLaunchKernelGGL(r_prep_w_kernel, dim3(nb((long)rows * Kp)), dim3(256), 0, s, w, scale, c.W + (long)row0 * Kp, Co, Ci, taps, CiP, Kp, rows);
        hipLaunchKernelGGL(r_prep_b_kernel, dim3(nb(rows)), dim3(256), 0, s, b, scale, shift, c.b + row0, Co, rows);
        return UV_OK;
    };
#define RP(...)                   \
    do {                          \
        int _rc = prep(__VA_ARGS__); \
        if (_rc) return _rc;      \
    } while (0)
    for (int e = 0; e < 2; ++e) {
        const std::string enc = e ? "context_encoder" : "feature_encoder";
        auto cna = [&](const std::string& m, int Co, int Ci, int taps, int CiP, int Kp) { return prep(m, m + ".0", e ? m + ".1" : "", Co, Ci, taps, CiP, Kp, Co, 0); };
        int rc = cna(enc + ".convnormrelu", 64, 3, 49, 3, 152);
        if (rc) return rc;
        const int chans[4] = {64, 64, 96, 128};
        for (int L = 1; L <= 3; ++L)
            for (int B = 0; B < 2; ++B) {
                const std::string pre = enc + ".layer" + std::to_string(L) + "." + std::to_string(B);
                const int Cin = B == 0 ? chans[L - 1] : chans[L], Co = chans[L];
                if ((rc = cna(pre + ".convnormrelu1", Co, Cin, 9, Cin, 9 * Cin))) return rc;
                if ((rc = cna(pre + ".convnormrelu2", Co, Co, 9, Co, 9 * Co))) return rc;
                if (B == 0 && L > 1 && (rc = cna(pre + ".downsample", Co, Cin, 1, Cin, Cin))) return rc;
            }
        RP(enc + ".conv", enc + ".conv", "", 256, 128, 1, 128, 128, 256, 0);
    }
    const std::string me = "update_block.motion_encoder.", rb = "update_block.recurrent_block.", fhd = "update_block.flow_head.";
    RP(me + "convcorr1", me + "convcorr1.0", "", 256, 324, 1, 328, 328, 256, 0);
    RP(me + "convcorr2", me + "convcorr2.0", "", 192, 256, 9, 256, 2304, 192, 0);
    RP(me + "convflow1", me + "convflow1.0", "", 128, 2, 49, 2, 104, 128, 0);
    RP(me + "convflow2", me + "convflow2.0", "", 64, 128, 9, 128, 1152, 64, 0);
    RP(me + "conv", me + "conv.0", "", 126, 256, 9, 256, 2304, 128, 0);
    for (int d = 1; d <= 2; ++d) {
        const std::string g = rb + "convgru" + std::to_string(d);
        {   // z | r stacked: one launch
            RaftConv& c = convs[g + ".zr"];
            c.W = (half_t*)dmalloc((size_t)256 * 1920 * 2);
            c.b = (half_t*)dmalloc(256 * 2);
            if (!c.W || !c.b) return UV_ERR_HIP;
            c.Co = c.CoP = 256;
            c.Ci = c.CiP = 384;
            c.taps = 5;
            c.Kp = 1920;
        }
        RP(g + ".zr", g + ".convz", "", 128, 384, 5, 384, 1920, 128, 0);
        RP(g + ".zr", g + ".convr", "", 128, 384, 5, 384, 1920, 128, 128);
        RP(g + ".convq", g + ".convq", "", 128, 384, 5, 384, 1920, 128, 0);
    }
    RP(fhd + "conv1", fhd + "conv1", "", 256, 128, 9, 128, 1152, 256, 0);
    RP(fhd + "conv2", fhd + "conv2", "", 2, 256, 9, 256, 2304, 8, 0);
    RP("mask_predictor.convrelu", "mask_predictor.convrelu.0", "", 256, 128, 9, 128, 1152, 256, 0);
    RP("mask_predictor.conv", "mask_predictor.conv", "", 576, 256, 1, 256, 256, 576, 0);
#undef RP
    UV_LAUNCH_CHECK();
    if (!splitk) UV_HIP(hipMalloc((void**)&splitk, UV_SPLITK_WS_BYTES));
    UV_HIP(hipStreamSynchronize(s));
    finalized = true;
    return UV_OK;
}

int Raft::reserve(int Hn, int Wn) {
    if (slab && Hn == H && Wn == W) return UV_OK;
    const long P2 = (long)(Hn / 2) * (Wn / 2), N = (long)(Hn / 8) * (Wn / 8);
    size_t off = 0;
    auto carve = [&](size_t bytes) {
        const size_t o = off;
        off += (bytes + 255) / 256 * 256;
        return o;
    };
    const size_t o_col7 = carve((size_t)2 * P2 * 152 * 2);
    size_t o_act[4];
    for (int i = 0; i < 4; ++i) o_act[i] = carve((size_t)2 * P2 * 64 * 2);
    const size_t o_part = carve((size_t)2 * 64 * 128 * 2 * 4), o_stat = carve((size_t)2 * 128 * 2 * 4);
    const size_t o_fmap = carve((size_t)2 * N * 256 * 2), o_ctxout = carve((size_t)N * 256 * 2), o_h32 = carve((size_t)N * 128 * 4), o_h16 = carve((size_t)N * 128 * 2),
                 o_ctx16 = carve((size_t)N * 128 * 2), o_pyr = carve((size_t)uv_raft_pyramid_floats(Hn / 8, Wn / 8) * 4), o_coords = carve((size_t)N * 2 * 4),
                 o_corr16 = carve((size_t)N * 328 * 2), o_c1 = carve((size_t)N * 256 * 2), o_c2 = carve((size_t)N * 256 * 2), o_colf = carve((size_t)N * 104 * 2),
                 o_f1 = carve((size_t)N * 128 * 2), o_motion = carve((size_t)N * 128 * 2), o_gcol = carve((size_t)N * 1920 * 2), o_zr = carve((size_t)N * 256 * 2),
                 o_qpre = carve((size_t)N * 128 * 2), o_fh = carve((size_t)N * 256 * 2), o_delta = carve((size_t)N * 8 * 2), o_mh = carve((size_t)N * 256 * 2),
                 o_mask = carve((size_t)N * 576 * 2);
    UV_RUN(uv_slab_grow(&slab, &slab_bytes, off));
    col7 = (half_t*)(slab + o_col7);
    for (int i = 0; i < 4; ++i) act[i] = (half_t*)(slab + o_act[i]);
    in_part = (float*)(slab + o_part);
    in_stat = (float*)(slab + o_stat);
    fmap = (half_t*)(slab + o_fmap);
    ctxout = (half_t*)(slab + o_ctxout);
    h32 = (float*)(slab + o_h32);
    h16 = (half_t*)(slab + o_h16);
    ctx16 = (half_t*)(slab + o_ctx16);
    pyr = (float*)(slab + o_pyr);
    coords1 = (float*)(slab + o_coords);
    corr16 = (half_t*)(slab + o_corr16);
    c1 = (half_t*)(slab + o_c1);
    c2 = (half_t*)(slab + o_c2);
    colf = (half_t*)(slab + o_colf);
    f1 = (half_t*)(slab + o_f1);
    motion = (half_t*)(slab + o_motion);
    gcol = (half_t*)(slab + o_gcol);
    zr = (half_t*)(slab + o_zr);
    qpre = (half_t*)(slab + o_qpre);
    fh = (half_t*)(slab + o_fh);
    delta = (half_t*)(slab + o_delta);
    mh = (half_t*)(slab + o_mh);
    mask = (half_t*)(slab + o_mask);
    H = Hn;
    W = Wn;
    return UV_OK;
}

namespace {
struct RFwd {
    Raft& u;
    hipStream_t s;
    const RaftConv* cv(const std::string& k) {
        auto it = u.convs.find(k);
        return it == u.convs.end() ? nullptr : &it->second;
    }
    // 3x3 (padding 1) / 1x1 conv at the given stride on NHWC [imgs, Hs, Ws, CiP] through the implicit GEMM
    int conv(const std::string& k, const half_t* X, int imgs, int Hs, int Ws, int stride, half_t* Y, int ldy) {
        const RaftConv* c = cv(k);
        UV_REQUIRE(c && (c->taps == 9 || c->taps == 1), "raft: conv %s", k.c_str());
        GemmParams g;
        g.X = X;
        g.C1 = c->CiP;
        g.Hs = Hs;
        g.Ws = Ws;
        g.stride = stride;
        g.taps = c->taps;
        g.Ho = (Hs - 1) / stride + 1;       // 3x3 / padding 1 and 1x1 / padding 0 alike
        g.Wo = (Ws - 1) / stride + 1;
        g.M = imgs * g.Ho * g.Wo;
        g.N = c->CoP;
        g.K = c->Kp;
        g.W = c->W;
        g.bias = c->b;
        g.Y = Y;
        g.ldy = ldy;
        g.partial = u.splitk;
        g.partial_bytes = UV_SPLITK_WS_BYTES;
        return uv_launch_gemm(g, 1, s);
    }
    int lin(const std::string& k, const half_t* X, long M, half_t* Y, int ldy) {
        const RaftConv* c = cv(k);
        UV_REQUIRE(c, "raft: conv %s", k.c_str());
        GemmParams g;
        g.X = X;
        g.ldx = c->Kp;
        g.M = (int)M;
        g.K = c->Kp;
        g.N = c->CoP;
        g.W = c->W;
        g.bias = c->b;
        g.Y = Y;
        g.ldy = ldy;
        g.partial = u.splitk;
        g.partial_bytes = UV_SPLITK_WS_BYTES;
        return uv_launch_gemm(g, 0, s);
    }
    int relu(half_t* x, long n) {
        hipLaunchKernelGGL(r_add_relu_kernel, dim3(nb(n / 8)), dim3(256), 0, s, x, (const half_t*)nullptr, x, n / 8);
        UV_LAUNCH_CHECK();
        return UV_OK;
    }
    // the norm (+ ReLU) behind a conv: InstanceNorm for the feature encoder; the context encoder's BatchNorm is already inside the conv
    int norm(bool inorm, half_t* x, int imgs, long P, int C, int relu_) {
        if (!inorm) return relu_ ? relu(x, imgs * P * C) : UV_OK;
        int S = (int)((P + 1023) / 1024);
        if (S > 64) S = 64;
        hipLaunchKernelGGL(r_in_stats_kernel, dim3(C / 8, S, imgs), dim3(256), 0, s, x, (int)P, C, S, u.in_part);
        hipLaunchKernelGGL(r_in_finalize_kernel, dim3(nb(imgs * C)), dim3(256), 0, s, u.in_part, (int)P, C, S, imgs, u.in_stat);
        hipLaunchKernelGGL(r_in_apply_kernel, dim3(nb(imgs * P * C / 8)), dim3(256), 0, s, x, u.in_stat, (int)P, C, imgs * P * C / 8, relu_);
        UV_LAUNCH_CHECK();
        return UV_OK;
    }
    int encoder(const std::string& enc, bool inorm, int imgs, int H, int W, half_t* dst) {
        int hc = H / 2, wc = W / 2, C = 64;
        int ix = 0, iy1 = 1, iy2 = 2, id = 3;
        UV_RUN(lin(enc + ".convnormrelu", u.col7, (long)imgs * hc * wc, u.act[ix], 64));
        UV_RUN(norm(inorm, u.act[ix], imgs, (long)hc * wc, 64, 1));
        const int chans[3] = {64, 96, 128};
        for (int L = 1; L <= 3; ++L)
            for (int B = 0; B < 2; ++B) {
                const std::string pre = enc + ".layer" + std::to_string(L) + "." + std::to_string(B);
                const int st = (B == 0 && L > 1) ? 2 : 1, Co = chans[L - 1];
                const int ho = (hc - 1) / st + 1, wo = (wc - 1) / st + 1;
                const long Po = (long)ho * wo;
                UV_RUN(conv(pre + ".convnormrelu1", u.act[ix], imgs, hc, wc, st, u.act[iy1], Co));
                UV_RUN(norm(inorm, u.act[iy1], imgs, Po, Co, 1));
                UV_RUN(conv(pre + ".convnormrelu2", u.act[iy1], imgs, ho, wo, 1, u.act[iy2], Co));
                UV_RUN(norm(inorm, u.act[iy2], imgs, Po, Co, 1));
                const half_t* res = u.act[ix];
                if (st == 2) {
                    UV_RUN(conv(pre + ".downsample", u.act[ix], imgs, hc, wc, 2, u.act[id], Co));
                    UV_RUN(norm(inorm, u.act[id], imgs, Po, Co, 0));
                    res = u.act[id];
                }
                hipLaunchKernelGGL(r_add_relu_kernel, dim3(nb(imgs * Po * Co / 8)), dim3(256), 0, s, res, (const half_t*)u.act[iy2], u.act[iy1], imgs * Po * Co / 8);
                UV_LAUNCH_CHECK();
                std::swap(ix, iy1);
                hc = ho;
                wc = wo;
                C = Co;
            }
        (void)C;
        return conv(enc + ".conv", u.act[ix], imgs, hc, wc, 1, dst, 256);
    }
};
}  // namespace

static int raft_check_size(int H, int W) {
    UV_REQUIRE(H > 0 && W > 0 && H % 8 == 0 && W % 8 == 0, "input image H and W should be divisible by 8, but got %d (h) and %d (w)", H, W);
    UV_REQUIRE(H / 8 >= 16 && W / 8 >= 16 && (long)H * W <= (1L << 24),
               "Feature maps are too small to be down-sampled by the correlation pyramid. H and W of feature maps should be at least 16; got: (%d, %d). "
               "Remember that input images to the model are downsampled by 8, so that means their dimensions should be at least 8 * 16 = 128", H / 8, W / 8);
    return UV_OK;
}

// fills fmap [2][N][256], h32 / h16 (tanh half of the context encoder) and ctx16 (relu half); img1 / img2 uint8 [H][W][3]
int Raft::encode(const uint8_t* img1, const uint8_t* img2, int Hn, int Wn, hipStream_t s) {
    UV_RUN(raft_check_size(Hn, Wn));
    if (!finalized) UV_RUN(finalize(s));
    UV_RUN(reserve(Hn, Wn));
    RFwd f{*this, s};
    const int Ho = Hn / 2, Wo = Wn / 2;
    const long P2 = (long)Ho * Wo, N = (long)(Hn / 8) * (Wn / 8);
    hipLaunchKernelGGL(r_im2col7_kernel, dim3(nb(P2 * 19)), dim3(256), 0, s, (const void*)img1, 0, 3, 1, Hn, Wn, 2, Ho, Wo, 152, col7);
    hipLaunchKernelGGL(r_im2col7_kernel, dim3(nb(P2 * 19)), dim3(256), 0, s, (const void*)img2, 0, 3, 1, Hn, Wn, 2, Ho, Wo, 152, col7 + P2 * 152);
    UV_LAUNCH_CHECK();
    UV_RUN(f.encoder("feature_encoder", true, 2, Hn, Wn, fmap));
    UV_RUN(f.encoder("context_encoder", false, 1, Hn, Wn, ctxout));
    hipLaunchKernelGGL(r_ctx_split_kernel, dim3(nb(N * 128)), dim3(256), 0, s, ctxout, h32, h16, ctx16, N * 128);
    UV_LAUNCH_CHECK();
    return UV_OK;
}

// one RecurrentBlock step: convgru1 (1x5) then convgru2 (5x1) over [h | ctx | motion]; hs fp32 [N][128] in place, hh16 its fp16 copy (output)
int Raft::gru(float* hs, half_t* hh16, const half_t* ctx, const half_t* mot, int hh, int ww, hipStream_t s) {
    RFwd f{*this, s};
    const long N = (long)hh * ww;
    for (int d = 0; d < 2; ++d) {
        const std::string g = "update_block.recurrent_block.convgru" + std::to_string(d + 1);
        hipLaunchKernelGGL(r_gru_im2col_kernel, dim3(nb(N * 240)), dim3(256), 0, s, hs, ctx, mot, (const half_t*)nullptr, d, hh, ww, gcol);
        UV_LAUNCH_CHECK();
        UV_RUN(f.lin(g + ".zr", gcol, N, zr, 256));
        hipLaunchKernelGGL(r_gru_im2col_kernel, dim3(nb(N * 240)), dim3(256), 0, s, hs, ctx, mot, (const half_t*)zr, d, hh, ww, gcol);
        UV_LAUNCH_CHECK();
        UV_RUN(f.lin(g + ".convq", gcol, N, qpre, 128));
        hipLaunchKernelGGL(r_gru_blend_kernel, dim3(nb(N * 128)), dim3(256), 0, s, zr, qpre, hs, hh16, N * 128);
        UV_LAUNCH_CHECK();
    }
    return UV_OK;
}

// one flow update: lookup -> motion encoder -> ConvGRU -> flow head -> coords1 += delta
int Raft::update(int hh, int ww, hipStream_t s) {
    RFwd f{*this, s};
    const long N = (long)hh * ww;
    const std::string me = "update_block.motion_encoder.";
    UV_RUN(uv_raft_corr_lookup(pyr, coords1, hh, ww, nullptr, corr16, s));
    UV_RUN(f.conv(me + "convcorr1", corr16, 1, hh, ww, 1, c1, 256));
    UV_RUN(f.relu(c1, N * 256));
    UV_RUN(f.conv(me + "convcorr2", c1, 1, hh, ww, 1, c2, 256));                 // cat[corr, flow]: columns 0..191 | 192..255 of one buffer
    hipLaunchKernelGGL(r_im2col7_kernel, dim3(nb(N * 13)), dim3(256), 0, s, (const void*)coords1, 1, 2, 1, hh, ww, 1, hh, ww, 104, colf);
    UV_LAUNCH_CHECK();
    UV_RUN(f.lin(me + "convflow1", colf, N, f1, 128));
    UV_RUN(f.relu(f1, N * 128));
    UV_RUN(f.conv(me + "convflow2", f1, 1, hh, ww, 1, c2 + 192, 256));
    UV_RUN(f.relu(c2, N * 256));
    UV_RUN(f.conv(me + "conv", c2, 1, hh, ww, 1, motion, 128));                  // 126 channels + 2 zero rows ...
    UV_RUN(f.relu(motion, N * 128));
    hipLaunchKernelGGL(r_set_flow_kernel, dim3(nb(N)), dim3(256), 0, s, motion, coords1, hh, ww);      // ... that take the flow
    UV_LAUNCH_CHECK();
    UV_RUN(gru(h32, h16, ctx16, motion, hh, ww, s));
    UV_RUN(f.conv("update_block.flow_head.conv1", h16, 1, hh, ww, 1, fh, 256));
    UV_RUN(f.relu(fh, N * 256));
    UV_RUN(f.conv("update_block.flow_head.conv2", fh, 1, hh, ww, 1, delta, 8));
    hipLaunchKernelGGL(r_update_coords_kernel, dim3(nb(N)), dim3(256), 0, s, coords1, delta, N);
    UV_LAUNCH_CHECK();
    return UV_OK;
}

int Raft::forward(const uint8_t* img1, const uint8_t* img2, int Hn, int Wn, float* flow, hipStream_t s) {
    UV_RUN(encode(img1, img2, Hn, Wn, s));
    RFwd f{*this, s};
    const int hh = Hn / 8, ww = Wn / 8;
    const long N = (long)hh * ww;
    UV_RUN(uv_raft_corr_pyramid(fmap, fmap + N * 256, hh, ww, pyr, s));
    hipLaunchKernelGGL(r_init_coords_kernel, dim3(nb(N)), dim3(256), 0, s, coords1, hh, ww);
    UV_LAUNCH_CHECK();
    for (int it = 0; it < 12; ++it) UV_RUN(update(hh, ww, s));
    // only the final flow is returned: the mask predictor runs once, on the last hidden state
    UV_RUN(f.conv("mask_predictor.convrelu", h16, 1, hh, ww, 1, mh, 256));
    UV_RUN(f.relu(mh, N * 256));
    UV_RUN(f.conv("mask_predictor.conv", mh, 1, hh, ww, 1, mask, 576));
    return uv_raft_convex_upsample(coords1, 1, mask, hh, ww, flow, s);
}
