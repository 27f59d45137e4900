// The T5 encoder stack (transformers T5EncoderModel, v1.1 gated-gelu form: SD3 / SD3.5's text_encoder_3, T5 v1.1-XXL) as ONE host-side graph of the
// library's gfx950 kernels per call, behind `pipeline.text_encoder_3(ids)[0]` (custom_pipeline.py encode_prompt).  THIRD-PARTY network, restated from
// its published definition (models/t5/modeling_t5.py) with that class's state-dict keys; tests/t5_ref.py is the yardstick and tests/test_t5_ref.py
// holds it to transformers itself.
//
//   x0 = embed[ids]                                                          (fp32 residual stream)
//   per layer:  h = rms(x) g1;  q|k|v = h Wqkv^T                             (no 1/sqrt(d) scaling in T5)
//               a = softmax(q k^T + bias[head][bucket(j - i)]) v             (bidirectional, no mask)
//               x += a Wo^T
//               h = rms(x) g2;  x += (gelu_new(h Wi0^T) * (h Wi1^T)) Wwo^T
//   last = rms(x_L) g_final                                                  (fp16 out)
//
// The residual stream is fp32: T5's stream outgrows the fp16 range (transformers clamps at inf and keeps `wo` in fp32; an all-fp16 module has
// neither protection).  RMSNorm reads fp32 rows and writes fp16 rows, the linears run fp16 with fp32 accumulation on uv_launch_gemm (mode 0, split-K
// partials in the handle's arena), and each sub-layer's fp16 output is added into the fp32 stream by its own pass.
// New kernels here: the embedding gather, RMSNorm, the bidirectional d = 64 attention with the relative-position bias, the gated activation, the add.
#include <math.h>
#include <string.h>

#include "t5.h"
#include "kernels.h"

namespace {

constexpr int TA_D = 64;                                   // head dim
constexpr int TA_KC = 64;                                  // keys per online-softmax step
constexpr int TA_KSTR = lds_stride_bytes(TA_D * 2) / 2;    // halfs per K row in LDS (80)
constexpr int TA_VSTR = 72;                                // halfs per V^T row: 64 key columns, 16-byte aligned rows
constexpr float LOG2E = 1.4426950408889634f;

// x[row, :] = float(embed[id]).  The id is clamped into [0, vocab): a bad id never reads out of bounds (the Python wrapper range-checks and raises
// before it gets here).
__global__ __launch_bounds__(256) void t5_embed_kernel(const int64_t* __restrict__ ids, const half_t* __restrict__ embed, float* __restrict__ x, long rows, int C,
                                                       int vocab) {
    const int c8 = C / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * c8) return;
    const long row = i / c8;
    const int c = (int)(i % c8) * 8;
    int64_t id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const h8 t = *reinterpret_cast<const h8*>(embed + id * C + c);
    float* o = x + row * C + c;
    *reinterpret_cast<f4*>(o) = f4{(float)t[0], (float)t[1], (float)t[2], (float)t[3]};
    *reinterpret_cast<f4*>(o + 4) = f4{(float)t[4], (float)t[5], (float)t[6], (float)t[7]};
}

// T5LayerNorm: out[row, c] = fp16(x[row, c] * rsqrt(mean_c x^2 + eps) * g[c]) — no mean subtraction, no bias.  One block per fp32 row of any width
// C % 4 == 0; the statistics are fp32 over the full width; one rounding per element.
__global__ __launch_bounds__(256) void t5_rmsnorm_kernel(const float* __restrict__ x, const half_t* __restrict__ g, half_t* __restrict__ out, int C, float eps) {
    __shared__ float part[4];
    const float* xr = x + (long)blockIdx.x * C;
    float ss = 0.f;
    for (int c = threadIdx.x * 4; c < C; c += 1024) {
        const f4 v = *reinterpret_cast<const f4*>(xr + c);
        ss += v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
    }
    ss = wave_sum(ss);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = ss;
    __syncthreads();
    const float rstd = 1.f / sqrtf((part[0] + part[1] + part[2] + part[3]) / (float)C + eps);
    half_t* orow = out + (long)blockIdx.x * C;
    for (int c = threadIdx.x * 4; c < C; c += 1024) {
        const f4 v = *reinterpret_cast<const f4*>(xr + c);
        const h4 gg = *reinterpret_cast<const h4*>(g + c);
        const h4 r = {(half_t)(v[0] * rstd * (float)gg[0]), (half_t)(v[1] * rstd * (float)gg[1]), (half_t)(v[2] * rstd * (float)gg[2]),
                      (half_t)(v[3] * rstd * (float)gg[3])};
        *reinterpret_cast<h4*>(orow + c) = r;
    }
}

// Bidirectional self-attention of one (batch, head, group of 64 queries): d = 64, no score scaling, additive relative-position bias.
//   block = 4 waves; wave w owns queries 64 qg + 16 w .. + 15 and walks ALL keys in steps of 64 with an online softmax, so registers and LDS do not
//   depend on S.  Per step the block stages the head's 64 K rows (row-major, [64][TA_KSTR]) and V rows (transposed, [64][TA_VSTR]) in LDS; a key
//   row at or beyond S is stored as ZERO, so no value from outside the element's own S rows is ever loaded.
//   scores: S^T tile = K_tile Q_tile^T by two v_mfma_f32_16x16x32_f16 (k = 64): lane (g, c) holds keys 4g .. 4g+3 of query c, which is the B operand
//   layout of the P V product, so P never moves between lanes (the layout of clip_attn_kernel).
//   bias: the head's row of the table over delta = j - i (all 1023 fp32 entries) sits in LDS and is added to the score before the maximum.
//   keys j >= S get -inf by SELECT before the maximum: their probability is an exact 0, and their V^T column in LDS is an exact 0, so the P V
//   product never multiplies anything read from outside the S rows.
//   softmax in fp32 (exp2 of log2(e) (s - max)); P rounded to fp16 for the MFMA steps; O = acc / l rounded once.
__global__ __launch_bounds__(256) void t5_attn_kernel(const half_t* __restrict__ qkv, const float* __restrict__ bias, half_t* __restrict__ out, int S, int heads,
                                                      int nqg) {
    __shared__ __attribute__((aligned(16))) half_t Ks[TA_KC * TA_KSTR];
    __shared__ __attribute__((aligned(16))) half_t Vt[TA_D * TA_VSTR];
    __shared__ float Bs[UV_T5_BIAS_W];
    const int qg = blockIdx.x % nqg, hd = (blockIdx.x / nqg) % heads, b = blockIdx.x / (nqg * heads), C = heads * TA_D;
    const long ld = 3L * C;
    const half_t* base = qkv + (long)b * S * ld + hd * TA_D;
    const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < UV_T5_BIAS_W; i += 256) Bs[i] = bias[(long)hd * UV_T5_BIAS_W + i];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    const int qi = qg * 64 + w * 16 + l15;                 // this lane's query (column of the score tile)
    const bool wave_live = qg * 64 + w * 16 < S;           // wave-uniform: a wave without queries still stages and meets the barriers
    h8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = qi < S ? *reinterpret_cast<const h8*>(base + qi * ld + ks * 32 + g * 8) : zero8;
    const f4 z4 = {0.f, 0.f, 0.f, 0.f};
    f4 o[4] = {z4, z4, z4, z4};                            // O^T[d = 16 dt + 4g + r][query l15]
    float m = -INFINITY, l = 0.f;
    for (int c0 = 0; c0 < S; c0 += TA_KC) {
        __syncthreads();                                   // the previous step's reads are done
        for (int i = threadIdx.x; i < TA_KC * 8; i += 256) {
            const int row = i >> 3, c = (i & 7) * 8;
            const bool live = c0 + row < S;
            const half_t* src = base + (long)(c0 + row) * ld + c;
            *reinterpret_cast<h8*>(Ks + row * TA_KSTR + c) = live ? *reinterpret_cast<const h8*>(src + C) : zero8;
            const h8 v = live ? *reinterpret_cast<const h8*>(src + 2 * C) : zero8;
#pragma unroll
            for (int e = 0; e < 8; ++e) Vt[(c + e) * TA_VSTR + row] = v[e];
        }
        __syncthreads();
        if (!wave_live) continue;
        // ---- scores of 64 keys: sc[kt][r] = <k[c0 + 16 kt + 4g + r], q[qi]> + bias[j - i]
        f4 sc[4];
        float mc = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const half_t* kr = Ks + (kt * 16 + l15) * TA_KSTR + g * 8;
            sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const h8*>(kr), qf[0], z4, 0, 0, 0);
            sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const h8*>(kr + 32), qf[1], sc[kt], 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = c0 + kt * 16 + 4 * g + r;
                const float sb = sc[kt][r] + Bs[j - qi + (UV_T5_MAX_S - 1)];      // j, qi in [0, 512): the index is in [0, 1022]
                sc[kt][r] = j < S ? sb : -INFINITY;
                mc = fmaxf(mc, sc[kt][r]);
            }
        }
        mc = fmaxf(mc, __shfl_xor(mc, 16, 64));
        mc = fmaxf(mc, __shfl_xor(mc, 32, 64));
        const float mn = fmaxf(m, mc);                     // finite: key c0 < S is in this step
        const float alpha = __builtin_amdgcn_exp2f((m - mn) * LOG2E);      // first step: exp2(-inf) = 0
        float ps = 0.f;
#pragma unroll
        for (int kt = 0; kt < 4; ++kt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[kt][r] = __builtin_amdgcn_exp2f((sc[kt][r] - mn) * LOG2E);      // exp2(-inf) = 0: a key beyond S
                ps += sc[kt][r];
            }
        ps += __shfl_xor(ps, 16, 64);
        ps += __shfl_xor(ps, 32, 64);
        l = l * alpha + ps;
        m = mn;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) o[dt] *= alpha;
        // ---- O^T += V^T P^T, two key tiles per MFMA: k slot 8g + e <-> key 16 t0 + 4g + e (e < 4), 16 t1 + 4g + e - 4 (e >= 4)
#pragma unroll
        for (int pr = 0; pr < 2; ++pr) {
            const int t0 = 2 * pr, t1 = 2 * pr + 1;
            h8 pb;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                pb[e] = (half_t)sc[t0][e];
                pb[4 + e] = (half_t)sc[t1][e];
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const half_t* vr = Vt + (dt * 16 + l15) * TA_VSTR + 4 * g;
                const h4 lo = *reinterpret_cast<const h4*>(vr + t0 * 16), hi = *reinterpret_cast<const h4*>(vr + t1 * 16);
                const h8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pb, o[dt], 0, 0, 0);
            }
        }
    }
    if (qi < S) {      // queries S .. are the block's own padding: never stored
        const float inv = 1.f / l;
        half_t* orow = out + ((long)b * S + qi) * C + hd * TA_D + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const h4 r = {(half_t)(o[dt][0] * inv), (half_t)(o[dt][1] * inv), (half_t)(o[dt][2] * inv), (half_t)(o[dt][3] * inv)};
            *reinterpret_cast<h4*>(orow + dt * 16) = r;
        }
    }
}

// T5DenseGatedActDense's middle: in [M, 2 F] = (h Wi0^T | h Wi1^T) -> out [M, F] = fp16(gelu_new(a) * b), fp32 math, one rounding
__global__ __launch_bounds__(256) void t5_gated_act_kernel(const half_t* __restrict__ in, half_t* __restrict__ out, long rows, int F) {
    const int f8 = F / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * f8) return;
    const long row = i / f8;
    const int c = (int)(i % f8) * 8;
    const h8 a = *reinterpret_cast<const h8*>(in + row * 2 * F + c), bb = *reinterpret_cast<const h8*>(in + row * 2 * F + F + c);
    h8 r;
#pragma unroll
    for (int e = 0; e < 8; ++e) r[e] = (half_t)(gelu_tanh_f((float)a[e]) * (float)bb[e]);
    *reinterpret_cast<h8*>(out + row * F + c) = r;
}

// x += float(y) over n8 groups of 8: a sub-layer's fp16 output into the fp32 stream
__global__ __launch_bounds__(256) void t5_add_kernel(float* __restrict__ x, const half_t* __restrict__ y, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    const h8 v = *reinterpret_cast<const h8*>(y + i * 8);
    f4 a = *reinterpret_cast<const f4*>(x + i * 8), c = *reinterpret_cast<const f4*>(x + i * 8 + 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        a[e] += (float)v[e];
        c[e] += (float)v[4 + e];
    }
    *reinterpret_cast<f4*>(x + i * 8) = a;
    *reinterpret_cast<f4*>(x + i * 8 + 4) = c;
}

}  // namespace

int uv_t5_bucket_table(int num_buckets, int max_distance, int n, int* out) {
    UV_REQUIRE(out && n >= 1 && n <= (1 << 20), "t5_bucket_table: n=%d must be in 1..2^20", n);
    UV_REQUIRE(num_buckets >= 4, "t5_bucket_table: num_buckets %d must be at least 4", num_buckets);
    const int nbk = num_buckets / 2, max_exact = nbk / 2;      // bidirectional: half the buckets per sign, half of those exact
    UV_REQUIRE(max_distance > max_exact, "t5_bucket_table: max_distance %d must exceed num_buckets / 4 = %d", max_distance, max_exact);
    for (int d = -(n - 1); d <= n - 1; ++d) {
        const int a = d < 0 ? -d : d;
        int v = a;
        if (a >= max_exact) {      // logarithmic bins up to max_distance, the last bucket beyond (the quotient truncates, as .to(torch.long) does)
            v = max_exact + (int)(log((double)a / max_exact) / log((double)max_distance / max_exact) * (nbk - max_exact));
            if (v > nbk - 1) v = nbk - 1;
        }
        out[d + n - 1] = (d > 0 ? nbk : 0) + v;
    }
    return UV_OK;
}

int uv_launch_t5_attention(const half_t* qkv, const float* bias_table, int B, int S, int heads, half_t* out, hipStream_t s) {
    UV_REQUIRE(qkv && bias_table && out, "t5_attention: null argument");
    UV_REQUIRE(B >= 1 && heads >= 1 && S >= 1 && S <= UV_T5_MAX_S && (long)B * heads * ((S + 63) / 64) < (1L << 30), "t5_attention: B=%d heads=%d S=%d (1 <= S <= %d)",
               B, heads, S, UV_T5_MAX_S);
    UV_REQUIRE((reinterpret_cast<uintptr_t>(qkv) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0 && (reinterpret_cast<uintptr_t>(bias_table) & 3) == 0,
               "t5_attention: qkv / out must be 16-byte aligned (bias_table 4-byte)");
    const int nqg = (S + 63) / 64;
    hipLaunchKernelGGL(t5_attn_kernel, dim3((unsigned)(B * heads * nqg)), dim3(256), 0, s, qkv, bias_table, out, S, heads, nqg);
    UV_LAUNCH_CHECK();
    return UV_OK;
}

int uv_t5_check_cfg(const univst_t5_cfg& c) {
    UV_REQUIRE(c.vocab_size >= 1, "t5_create: vocab_size %d must be positive", c.vocab_size);
    UV_REQUIRE(c.num_layers >= 1, "t5_create: num_layers %d must be positive", c.num_layers);
    UV_REQUIRE(c.num_heads >= 1 && c.num_heads <= 4096, "t5_create: num_heads %d must be in 1..4096", c.num_heads);
    UV_REQUIRE(c.d_kv == TA_D, "t5_create: d_kv %d (the attention kernel has a head dim of 64 only)", c.d_kv);
    UV_REQUIRE(c.d_model >= 8 && c.d_model % 8 == 0, "t5_create: d_model %d must be a positive multiple of 8", c.d_model);
    UV_REQUIRE(c.d_ff >= 8 && c.d_ff % 8 == 0, "t5_create: d_ff %d must be a positive multiple of 8", c.d_ff);
    UV_REQUIRE(c.num_buckets >= 4, "t5_create: num_buckets %d must be at least 4", c.num_buckets);
    UV_REQUIRE(c.max_distance > c.num_buckets / 4, "t5_create: max_distance %d must exceed num_buckets / 4 = %d", c.max_distance, c.num_buckets / 4);
    UV_REQUIRE(c.layer_norm_eps > 0.f, "t5_create: layer_norm_eps %g must be positive", (double)c.layer_norm_eps);
    return UV_OK;
}

int T5::load_tensor(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s) {
    UV_REQUIRE(key, "t5_load_tensor: null key");
    // the embedding is tied: a checkpoint carries it as shared.weight, encoder.embed_tokens.weight or both — one copy under the first name
    if (!strcmp(key, "encoder.embed_tokens.weight")) key = "shared.weight";
    return Model::load_tensor(key, dev_ptr, dtype, shape, ndim, s);
}

int T5::finalize(hipStream_t s) {
    clear_derived();
    clear_missing();
    layers.clear();
    bias_table = nullptr;
    const int C = cfg.d_model, F = cfg.d_ff, Hn = cfg.num_heads, I = Hn * TA_D;
    const half_t* rel;
    UV_SHAPED(embed, "shared.weight", cfg.vocab_size, C);
    UV_SHAPED(fln_g, "encoder.final_layer_norm.weight", C);
    UV_SHAPED(rel, "encoder.block.0.layer.0.SelfAttention.relative_attention_bias.weight", cfg.num_buckets, Hn);
    for (int l = 0; l < cfg.num_layers; ++l) {
        const std::string p = "encoder.block." + std::to_string(l) + ".layer.";
        T5Layer L;
        const half_t *qw, *kw, *vw, *w0, *w1;
        UV_SHAPED(L.ln1_g, p + "0.layer_norm.weight", C);
        UV_SHAPED(qw, p + "0.SelfAttention.q.weight", I, C);
        UV_SHAPED(kw, p + "0.SelfAttention.k.weight", I, C);
        UV_SHAPED(vw, p + "0.SelfAttention.v.weight", I, C);
        UV_SHAPED(L.o_w, p + "0.SelfAttention.o.weight", C, I);
        UV_SHAPED(L.ln2_g, p + "1.layer_norm.weight", C);
        UV_SHAPED(w0, p + "1.DenseReluDense.wi_0.weight", F, C);
        UV_SHAPED(w1, p + "1.DenseReluDense.wi_1.weight", F, C);
        UV_SHAPED(L.wo_w, p + "1.DenseReluDense.wo.weight", C, F);
        // fused q|k|v [3 I, C] and wi_0|wi_1 [2 F, C]: one projection each (T5 has no attention scale to fold)
        UV_RUN(derive_concat(p + "0.SelfAttention#qkv_w", {qw, kw, vw}, I, C, s, 1.f, &L.qkv_w));
        UV_RUN(derive_concat(p + "1.DenseReluDense#wi_w", {w0, w1}, F, C, s, 1.f, &L.wi_w));
        layers.push_back(L);
    }
    UV_HIP(hipStreamSynchronize(s));      // the uploads queued on s are in place
    // the per-head bias table [heads][delta + 511] (fp32, kept in a derived slot of twice as many halfs): block 0's relative_attention_bias
    // [num_buckets, heads] read through the bucket of every delta; built on the host, once
    std::vector<int> bucket(UV_T5_BIAS_W);
    UV_RUN(uv_t5_bucket_table(cfg.num_buckets, cfg.max_distance, UV_T5_MAX_S, bucket.data()));
    std::vector<half_t> relh((size_t)cfg.num_buckets * Hn);
    UV_HIP(hipMemcpy(relh.data(), rel, relh.size() * sizeof(half_t), hipMemcpyDeviceToHost));
    std::vector<float> table((size_t)Hn * UV_T5_BIAS_W);
    for (int hd = 0; hd < Hn; ++hd)
        for (int d = 0; d < UV_T5_BIAS_W; ++d) table[(size_t)hd * UV_T5_BIAS_W + d] = (float)relh[(size_t)bucket[d] * Hn + hd];
    half_t* slot;
    UV_RUN(derive("encoder.block.0.layer.0.SelfAttention#bias_table", {Hn, 2L * UV_T5_BIAS_W}, &slot));
    UV_HIP(hipMemcpy(slot, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    bias_table = reinterpret_cast<const float*>(slot);
    finalized = true;
    return UV_OK;
}

// the activations of one (B, S): a new size re-carves the arena (growing the slab synchronises the device); the same size touches nothing
int T5::reserve(int B, int S) {
    if (B == rB && S == rS) return UV_OK;
    rB = rS = 0;
    const long M = (long)B * S;
    const int C = cfg.d_model, F = cfg.d_ff, I = cfg.num_heads * TA_D;
    // split-K partials of the four linears (q|k|v, o, wi_0|wi_1, wo: none has a bias or a residual), as the GEMM launcher will plan them; the 256-aligned
    // embedding table stands in for the operands
    UV_RUN(uv_plan_splitk_bytes(M, embed, {{3 * I, C, 0, 0, 0}, {C, I, 0, 0, 0}, {2 * F, C, 0, 0, 0}, {C, F, 0, 0, 0}}, &splitk_bytes));
    const size_t bh = (size_t)M * C * 2;
    UV_RUN(carve({{&x, (size_t)M * C * 4}, {&h, bh}, {&y, bh}, {&qkv, (size_t)M * 3 * I * 2}, {&att, (size_t)M * I * 2}, {&ff2, (size_t)M * 2 * F * 2},
                  {&ff, (size_t)M * F * 2}, {&splitk, splitk_bytes}}));
    rB = B;
    rS = S;
    return UV_OK;
}

int T5::encode(const int64_t* ids, int B, int S, half_t* last_hidden, hipStream_t s) {
    UV_REQUIRE(finalized, "t5_encode: call univst_t5_finalize after loading weights");
    UV_REQUIRE(ids && last_hidden && B >= 1 && B <= 4096 && S >= 1 && S <= UV_T5_MAX_S, "t5_encode: B=%d (1..4096), S=%d (1..%d)", B, S, UV_T5_MAX_S);
    UV_REQUIRE((reinterpret_cast<uintptr_t>(last_hidden) & 7) == 0, "t5_encode: last_hidden must be 8-byte aligned");
    UV_RUN(reserve(B, S));
    const long M = (long)B * S;
    const int C = cfg.d_model, F = cfg.d_ff, I = cfg.num_heads * TA_D;
    auto linear = [&](const half_t* X, int K, const half_t* Wt, int N, half_t* Y) { return uv_launch_gemm(lin_params(X, M, K, Wt, N, Y, nullptr, nullptr, 0, splitk, splitk_bytes), 0, s); };
    auto rms = [&](const half_t* g, half_t* dst) { hipLaunchKernelGGL(t5_rmsnorm_kernel, dim3((unsigned)M), dim3(256), 0, s, x, g, dst, C, cfg.layer_norm_eps); };
    auto add = [&]() { hipLaunchKernelGGL(t5_add_kernel, dim3(nb(M * C / 8)), dim3(256), 0, s, x, y, M * C / 8); };
    hipLaunchKernelGGL(t5_embed_kernel, dim3(nb(M * (C / 8))), dim3(256), 0, s, ids, embed, x, M, C, cfg.vocab_size);
    UV_LAUNCH_CHECK();
    for (const T5Layer& w : layers) {
        rms(w.ln1_g, h);
        UV_LAUNCH_CHECK();
        UV_RUN(linear(h, C, w.qkv_w, 3 * I, qkv));
        UV_RUN(uv_launch_t5_attention(qkv, bias_table, B, S, cfg.num_heads, att, s));
        UV_RUN(linear(att, I, w.o_w, C, y));
        add();
        rms(w.ln2_g, h);
        UV_LAUNCH_CHECK();
        UV_RUN(linear(h, C, w.wi_w, 2 * F, ff2));
        hipLaunchKernelGGL(t5_gated_act_kernel, dim3(nb(M * (F / 8))), dim3(256), 0, s, ff2, ff, M, F);
        UV_LAUNCH_CHECK();
        UV_RUN(linear(ff, F, w.wo_w, C, y));
        add();
        UV_LAUNCH_CHECK();
    }
    rms(fln_g, last_hidden);
    UV_LAUNCH_CHECK();
    return UV_OK;
}
