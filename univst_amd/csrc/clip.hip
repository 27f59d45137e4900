// The CLIP text tower (transformers CLIPTextModel / CLIPTextModelWithProjection: SD-v1.5's CLIP-L, SD-v2.1's OpenCLIP-H, SD3's CLIP-L and CLIP-bigG) as
// ONE host-side graph of the library's gfx950 kernels per call, behind `pipeline.text_encoder(ids)` (stable_diffusion.py _encode_prompt,
// ddim_inversion.py, custom_pipeline.py _get_clip_prompt_embeds).  THIRD-PARTY network, restated from its published definition
// (models/clip/modeling_clip.py) with that class's state-dict keys, with or without the `text_model.` prefix; tests/clip_ref.py is the yardstick and
// tests/test_clip_ref.py holds it to transformers itself.
//
//   x0 = token_embedding[ids] + position_embedding[0..S)
//   per layer:  x += out_proj(causal_attention(q|k|v(LN1 x)));  x += fc2(act(fc1(LN2 x)))       act = quick_gelu or gelu (erf)
//   last = final_layer_norm(x_L);  pooled = last[b, eos position];  text_embeds = text_projection(pooled)
//
// New kernels here: the embedding gather, the causal d = 64 attention (one block per (batch, head), the head's Q / K / V in LDS, MFMA for the full
// key tiles and a select-guarded vector pass for the diagonal tile), the activation pass and the EOS pooling.  The projections run on uv_launch_gemm
// (mode 0, bias / residual epilogues), the norms on uv_launch_layernorm, text_projection on uv_launch_linear_small.
#include <math.h>
#include <string.h>

#include "clip.h"
#include "kernels.h"

namespace {

constexpr int CA_D = 64;                                   // head dim
constexpr int CA_QSTR = lds_stride_bytes(CA_D * 2) / 2;    // halfs per Q / K row in LDS (80)
constexpr int CA_VK = 96;                                  // key columns of the transposed V: three 32-key steps, zero beyond S
constexpr int CA_VSTR = 104;                               // halfs per V^T row (16-byte aligned rows)
constexpr float LOG2E = 1.4426950408889634f;

// out[b, s, :] = fp16(tok[id] + pos[s]) (fp32 add, one rounding).  The id is clamped into [0, vocab): a bad id never reads out of bounds (the
// Python wrapper range-checks and raises before it gets here).
__global__ __launch_bounds__(256) void clip_embed_kernel(const int64_t* __restrict__ ids, const half_t* __restrict__ tok, const half_t* __restrict__ pos,
                                                         half_t* __restrict__ out, long rows, int S, int C, int vocab) {
    const int c8 = C / 8;
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows * c8) return;
    const long row = i / c8;
    const int c = (int)(i % c8) * 8, s = (int)(row % S);
    int64_t id = ids[row];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const h8 t = *reinterpret_cast<const h8*>(tok + id * C + c), p = *reinterpret_cast<const h8*>(pos + (long)s * C + c);
    h8 o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)t[e] + (float)p[e]);
    *reinterpret_cast<h8*>(out + row * C + c) = o;
}

// Causal self-attention of one (batch, head): S <= 80 queries and keys, d = 64, q rows already scaled by 1/8.
//   block = 5 waves; wave w owns query tile w (rows 16w .. 16w+15) and key tiles 0 .. w: 15 of the 25 score tiles exist.
//   LDS: Q and K row-major [80][CA_QSTR], V transposed [64][CA_VSTR] over 96 key columns; everything beyond row S is ZERO, so no value
//   from outside the head's S rows is ever loaded.
//   scores: S^T tile = K_tile Q_tile^T by two v_mfma_f32_16x16x32_f16 (k = 64): lane (g, c) holds keys 4g .. 4g+3 of query c, which is the B operand
//   layout of the P V product, so P never moves between lanes.
//   key tiles below the diagonal are visible to all 16 queries: O^T += V^T P^T by MFMA, two key tiles per 32-wide step (an odd tile out pairs with
//   zeros in both operands).  The diagonal tile is where j > i occurs: its P V runs on the vector unit with a SELECT per (query, key), so a masked
//   key's V row is never multiplied — 0 x NaN and 0 x Inf cannot arise, whatever lies in the rows a query may not see.  Masked scores are replaced
//   (select) by -inf before the maximum, so their probability is an exact 0 and a NaN score in a masked slot is dropped.
//   softmax in fp32 (exp2 of log2(e) (s - max)); P rounded to fp16 for the MFMA steps; O = acc / l rounded once.
__global__ __launch_bounds__(320) void clip_attn_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ out, int S, int heads) {
    __shared__ __attribute__((aligned(16))) half_t Qs[UV_CLIP_MAX_S * CA_QSTR];
    __shared__ __attribute__((aligned(16))) half_t Ks[UV_CLIP_MAX_S * CA_QSTR];
    __shared__ __attribute__((aligned(16))) half_t Vt[CA_D * CA_VSTR];
    const int b = blockIdx.x / heads, hd = blockIdx.x % heads, C = heads * CA_D;
    const long ld = 3L * C;
    const half_t* base = qkv + (long)b * S * ld + hd * CA_D;
    const h8 zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int i = threadIdx.x; i < UV_CLIP_MAX_S * 8; i += 320) {
        const int row = i >> 3, c = (i & 7) * 8;
        const bool live = row < S;
        *reinterpret_cast<h8*>(Qs + row * CA_QSTR + c) = live ? *reinterpret_cast<const h8*>(base + row * ld + c) : zero8;
        *reinterpret_cast<h8*>(Ks + row * CA_QSTR + c) = live ? *reinterpret_cast<const h8*>(base + row * ld + C + c) : zero8;
    }
    for (int i = threadIdx.x; i < CA_VK * 8; i += 320) {
        const int row = i >> 3, c = (i & 7) * 8;
        const h8 v = row < S ? *reinterpret_cast<const h8*>(base + row * ld + 2 * C + c) : zero8;
#pragma unroll
        for (int e = 0; e < 8; ++e) Vt[(c + e) * CA_VSTR + row] = v[e];
    }
    __syncthreads();
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63, l15 = lane & 15, g = lane >> 4;
    if (w * 16 >= S) return;      // (no barrier behind this point)

    const f4 z4 = {0.f, 0.f, 0.f, 0.f};
    h8 qf[2];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) qf[ks] = *reinterpret_cast<const h8*>(Qs + (w * 16 + l15) * CA_QSTR + ks * 32 + g * 8);
    // ---- scores: sc[kt][r] = <k[16 kt + 4g + r], q[16 w + l15]>
    f4 sc[5];
#pragma unroll
    for (int kt = 0; kt < 5; ++kt) {
        sc[kt] = z4;
        if (kt <= w) {
            const half_t* kr = Ks + (kt * 16 + l15) * CA_QSTR + g * 8;
            sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const h8*>(kr), qf[0], sc[kt], 0, 0, 0);
            sc[kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(*reinterpret_cast<const h8*>(kr + 32), qf[1], sc[kt], 0, 0, 0);
        }
        if (kt == w) {      // the diagonal tile: key j visible to query i iff j <= i and j < S
#pragma unroll
            for (int r = 0; r < 4; ++r) sc[kt][r] = (4 * g + r <= l15 && w * 16 + 4 * g + r < S) ? sc[kt][r] : -INFINITY;
        }
    }
    // ---- softmax over the keys of query l15: registers, then the four lane groups g
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < 5; ++kt)
        if (kt <= w)
#pragma unroll
            for (int r = 0; r < 4; ++r) m = fmaxf(m, sc[kt][r]);
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));      // finite: key 0 is visible to every query
    float l = 0.f;
#pragma unroll
    for (int kt = 0; kt < 5; ++kt)
        if (kt <= w)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                sc[kt][r] = __builtin_amdgcn_exp2f((sc[kt][r] - m) * LOG2E);      // exp2(-inf) = 0: a masked slot
                l += sc[kt][r];
            }
    l += __shfl_xor(l, 16, 64);
    l += __shfl_xor(l, 32, 64);
    // ---- O^T[d][query] over the full key tiles (kt < w), two per MFMA step: k slot 8g + j <-> key 16 t0 + 4g + j (j < 4), 16 t1 + 4g + j - 4 (j >= 4)
    f4 o[4] = {z4, z4, z4, z4};
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
        const int t0 = 2 * pr, t1 = 2 * pr + 1;
        if (t0 < w) {
            const bool two = t1 < w;
            h8 pb;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pb[j] = (half_t)sc[t0][j];
                pb[4 + j] = two ? (half_t)sc[t1][j] : (half_t)0.f;
            }
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const half_t* vr = Vt + (dt * 16 + l15) * CA_VSTR + 4 * g;
                const h4 lo = *reinterpret_cast<const h4*>(vr + t0 * 16);
                const h4 hi = two ? *reinterpret_cast<const h4*>(vr + t1 * 16) : h4{0, 0, 0, 0};
                const h8 a = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
                o[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a, pb, o[dt], 0, 0, 0);
            }
        }
    }
    // ---- the diagonal tile on the vector unit: o[dt][r] (d = 16 dt + 4g + r, query l15) += p[j] v[16 w + j][d] for the VISIBLE j only
    f4 pd = z4;
#pragma unroll
    for (int kt = 0; kt < 5; ++kt)
        if (kt == w) pd = sc[kt];
    float pj[16];
#pragma unroll
    for (int gg = 0; gg < 4; ++gg)
#pragma unroll
        for (int r = 0; r < 4; ++r) pj[gg * 4 + r] = __shfl(pd[r], gg * 16 + l15, 64);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const half_t* vr = Vt + (dt * 16 + 4 * g + r) * CA_VSTR + w * 16;
            const h8 v0 = *reinterpret_cast<const h8*>(vr), v1 = *reinterpret_cast<const h8*>(vr + 8);
            float acc = o[dt][r];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const float v = (float)(j < 8 ? v0[j & 7] : v1[j & 7]);
                acc = (j <= l15 && w * 16 + j < S) ? fmaf(pj[j], v, acc) : acc;
            }
            o[dt][r] = acc;
        }
    const int i = w * 16 + l15;
    if (i < S) {      // rows S .. 79 are the kernel's own padding: never stored
        const float inv = 1.f / l;
        half_t* orow = out + ((long)b * S + i) * C + hd * CA_D + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
            const h4 r = {(half_t)(o[dt][0] * inv), (half_t)(o[dt][1] * inv), (half_t)(o[dt][2] * inv), (half_t)(o[dt][3] * inv)};
            *reinterpret_cast<h4*>(orow + dt * 16) = r;
        }
    }
}

// x <- act(x) in place over n8 groups of 8 halfs: act 0 = quick_gelu x sigmoid(1.702 x), 1 = gelu 0.5 x (1 + erf(x / sqrt 2)) (libm erff)
template <int ACT>
__global__ __launch_bounds__(256) void clip_act_kernel(half_t* __restrict__ x, long n8) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n8) return;
    h8 v = *reinterpret_cast<const h8*>(x + i * 8);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float f = (float)v[e];
        v[e] = (half_t)(ACT == 0 ? f / (1.f + __expf(-1.702f * f)) : 0.5f * f * (1.f + erff(f * 0.70710678118654752f)));
    }
    *reinterpret_cast<h8*>(x + i * 8) = v;
}

// pooled row of one batch element: position by the legacy rule (eos == 2: the first largest id) or the first id == eos (0 when there is none),
// then the row of `last` [B, S, C] at it -> out [B, C].  One block per batch element; S <= 80.
__global__ __launch_bounds__(256) void clip_pool_kernel(const int64_t* __restrict__ ids, const half_t* __restrict__ last, half_t* __restrict__ out, int S, int C,
                                                        int eos) {
    __shared__ int spos;
    const int b = blockIdx.x;
    if (threadIdx.x == 0) {
        int p = 0;
        if (eos == 2) {
            int64_t best = ids[(long)b * S];
            for (int s = 1; s < S; ++s) {
                const int64_t v = ids[(long)b * S + s];
                if (v > best) {
                    best = v;
                    p = s;
                }
            }
        } else {
            for (int s = 0; s < S; ++s)
                if (ids[(long)b * S + s] == eos) {
                    p = s;
                    break;
                }
        }
        spos = p;
    }
    __syncthreads();
    const half_t* src = last + ((long)b * S + spos) * C;
    for (int c = threadIdx.x * 8; c < C; c += 256 * 8) *reinterpret_cast<h8*>(out + (long)b * C + c) = *reinterpret_cast<const h8*>(src + c);
}

}  // namespace

int uv_launch_clip_attention(const half_t* qkv, int B, int S, int heads, half_t* out, hipStream_t s) {
    UV_REQUIRE(qkv && out, "clip_attention: null argument");
    UV_REQUIRE(B >= 1 && heads >= 1 && S >= 1 && S <= UV_CLIP_MAX_S && (long)B * heads < (1L << 30), "clip_attention: B=%d heads=%d S=%d (1 <= S <= %d)", B, heads, S,
               UV_CLIP_MAX_S);
    UV_REQUIRE((reinterpret_cast<uintptr_t>(qkv) & 15) == 0 && (reinterpret_cast<uintptr_t>(out) & 15) == 0, "clip_attention: qkv / out must be 16-byte aligned");
    hipLaunchKernelGGL(clip_attn_kernel, dim3((unsigned)(B * heads)), dim3(320), 0, s, qkv, out, S, heads);
    UV_LAUNCH_CHECK();
    return UV_OK;
}

int uv_clip_check_cfg(const univst_clip_cfg& c) {
    UV_REQUIRE(c.vocab_size >= 1 && c.num_layers >= 1 && c.num_heads >= 1 && c.hidden_size >= 1 && c.intermediate_size >= 8 && c.intermediate_size % 8 == 0,
               "clip_create: bad config (vocab %d, layers %d, heads %d, hidden %d, intermediate %d)", c.vocab_size, c.num_layers, c.num_heads, c.hidden_size,
               c.intermediate_size);
    UV_REQUIRE(c.hidden_size == c.num_heads * CA_D, "clip_create: hidden_size %d / num_heads %d must be a head dim of 64", c.hidden_size, c.num_heads);
    UV_REQUIRE(c.hidden_size <= 2048, "clip_create: hidden_size %d > 2048 (the LayerNorm kernel's width)", c.hidden_size);
    UV_REQUIRE(c.max_positions >= 1 && c.max_positions <= UV_CLIP_MAX_S, "clip_create: max_positions %d must be in 1..%d", c.max_positions, UV_CLIP_MAX_S);
    UV_REQUIRE(c.hidden_act == 0 || c.hidden_act == 1, "clip_create: hidden_act %d (0 = quick_gelu, 1 = gelu)", c.hidden_act);
    UV_REQUIRE(c.projection_dim >= 0 && c.layer_norm_eps > 0.f, "clip_create: projection_dim %d, layer_norm_eps %g", c.projection_dim, (double)c.layer_norm_eps);
    return UV_OK;
}

int Clip::load_tensor(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s) {
    UV_REQUIRE(key, "clip_load_tensor: null key");
    if (!strncmp(key, "text_model.", 11)) key += 11;      // checkpoints (and CLIPTextModelWithProjection) prefix the tower's keys; text_projection.weight is top level
    return Model::load_tensor(key, dev_ptr, dtype, shape, ndim, s);
}

int Clip::finalize(hipStream_t s) {
    clear_derived();
    clear_missing();
    layers.clear();
    const int C = cfg.hidden_size, I = cfg.intermediate_size;
    UV_SHAPED(tok, "embeddings.token_embedding.weight", cfg.vocab_size, C);
    UV_SHAPED(pos, "embeddings.position_embedding.weight", cfg.max_positions, C);
    UV_SHAPED(fln_g, "final_layer_norm.weight", C);
    UV_SHAPED(fln_b, "final_layer_norm.bias", C);
    proj = nullptr;
    if (cfg.projection_dim) UV_SHAPED(proj, "text_projection.weight", cfg.projection_dim, C);
    for (int l = 0; l < cfg.num_layers; ++l) {
        const std::string p = "encoder.layers." + std::to_string(l) + ".";
        ClipLayer L;
        UV_SHAPED(L.ln1_g, p + "layer_norm1.weight", C);
        UV_SHAPED(L.ln1_b, p + "layer_norm1.bias", C);
        UV_SHAPED(L.ln2_g, p + "layer_norm2.weight", C);
        UV_SHAPED(L.ln2_b, p + "layer_norm2.bias", C);
        UV_SHAPED(L.out_w, p + "self_attn.out_proj.weight", C, C);
        UV_SHAPED(L.out_b, p + "self_attn.out_proj.bias", C);
        UV_SHAPED(L.fc1_w, p + "mlp.fc1.weight", I, C);
        UV_SHAPED(L.fc1_b, p + "mlp.fc1.bias", I);
        UV_SHAPED(L.fc2_w, p + "mlp.fc2.weight", C, I);
        UV_SHAPED(L.fc2_b, p + "mlp.fc2.bias", C);
        const half_t *qw, *kw, *vw, *qb, *kb, *vb;
        UV_SHAPED(qw, p + "self_attn.q_proj.weight", C, C);
        UV_SHAPED(kw, p + "self_attn.k_proj.weight", C, C);
        UV_SHAPED(vw, p + "self_attn.v_proj.weight", C, C);
        UV_SHAPED(qb, p + "self_attn.q_proj.bias", C);
        UV_SHAPED(kb, p + "self_attn.k_proj.bias", C);
        UV_SHAPED(vb, p + "self_attn.v_proj.bias", C);
        // fused q|k|v projection [3C, C] + [3C]; the attention scale d^-0.5 = 1/8 rides on the q rows (a power of two: exact in fp16 short of
        // underflow), which leaves the kernel the factor log2(e) only
        UV_RUN(derive_concat(p + "self_attn#qkv_w", {qw, kw, vw}, C, C, s, 0.125f, &L.qkv_w));
        UV_RUN(derive_concat(p + "self_attn#qkv_b", {qb, kb, vb}, C, 0, s, 0.125f, &L.qkv_b));
        layers.push_back(L);
    }
    UV_HIP(hipStreamSynchronize(s));
    finalized = true;
    return UV_OK;
}

// the activations of one (B, S): a new size re-carves the arena (growing the slab synchronises the device); the same size touches nothing
int Clip::reserve(int B, int S) {
    if (B == rB && S == rS) return UV_OK;
    rB = rS = 0;
    const long M = (long)B * S;
    const int C = cfg.hidden_size, I = cfg.intermediate_size;
    // split-K partials of the four linears (q|k|v, out + residual, fc1, fc2 + residual), as the GEMM launcher will plan them; the 256-aligned embedding table
    // stands in for the operands
    UV_RUN(uv_plan_splitk_bytes(M, tok, {{3 * C, C, 0, 1, 0}, {C, C, 0, 1, 1}, {I, C, 0, 1, 0}, {C, I, 0, 1, 1}}, &splitk_bytes));
    const size_t mc = (size_t)M * C * 2;
    UV_RUN(carve({{&x[0], mc}, {&x[1], mc}, {&h, mc}, {&att, mc}, {&mid, mc}, {&last, mc}, {&qkv, (size_t)M * 3 * C * 2}, {&ff, (size_t)M * I * 2},
                  {&prow, (size_t)B * C * 2}, {&splitk, splitk_bytes}}));
    rB = B;
    rS = S;
    return UV_OK;
}

int Clip::encode(const int64_t* ids, int B, int S, half_t* last_hidden, half_t* hidden_states, half_t* pooled, hipStream_t s) {
    UV_REQUIRE(finalized, "clip_encode: call univst_clip_finalize after loading weights");
    UV_REQUIRE(ids && B >= 1 && B <= 4096 && S >= 1 && S <= cfg.max_positions, "clip_encode: B=%d (1..4096), S=%d (1..max_positions %d)", B, S, cfg.max_positions);
    UV_RUN(reserve(B, S));
    const long M = (long)B * S;
    const int C = cfg.hidden_size, I = cfg.intermediate_size, L = cfg.num_layers;
    auto linear = [&](const half_t* X, int K, const half_t* Wt, const half_t* bias, int N, half_t* Y, const half_t* R) {
        return uv_launch_gemm(lin_params(X, M, K, Wt, N, Y, bias, R, 0, splitk, splitk_bytes), 0, s);
    };
    // residual stream l: the caller's hidden_states[l] when it wants them, else two arena buffers in turn
    auto xl = [&](int l) { return hidden_states ? hidden_states + (long)l * M * C : x[l & 1]; };
    hipLaunchKernelGGL(clip_embed_kernel, dim3(nb(M * (C / 8))), dim3(256), 0, s, ids, tok, pos, xl(0), M, S, C, cfg.vocab_size);
    UV_LAUNCH_CHECK();
    for (int l = 0; l < L; ++l) {
        const ClipLayer& w = layers[l];
        const half_t* xi = xl(l);
        UV_RUN(uv_launch_layernorm(xi, C, h, C, w.ln1_g, w.ln1_b, M, C, cfg.layer_norm_eps, s));
        UV_RUN(linear(h, C, w.qkv_w, w.qkv_b, 3 * C, qkv, nullptr));
        UV_RUN(uv_launch_clip_attention(qkv, B, S, cfg.num_heads, att, s));
        UV_RUN(linear(att, C, w.out_w, w.out_b, C, mid, xi));
        UV_RUN(uv_launch_layernorm(mid, C, h, C, w.ln2_g, w.ln2_b, M, C, cfg.layer_norm_eps, s));
        UV_RUN(linear(h, C, w.fc1_w, w.fc1_b, I, ff, nullptr));
        const long n8 = M * I / 8;
        if (cfg.hidden_act == 0) hipLaunchKernelGGL(clip_act_kernel<0>, dim3(nb(n8)), dim3(256), 0, s, ff, n8);
        else hipLaunchKernelGGL(clip_act_kernel<1>, dim3(nb(n8)), dim3(256), 0, s, ff, n8);
        UV_LAUNCH_CHECK();
        UV_RUN(linear(ff, I, w.fc2_w, w.fc2_b, C, xl(l + 1), mid));
    }
    if (!last_hidden && !pooled) return UV_OK;
    half_t* lh = last_hidden ? last_hidden : last;
    UV_RUN(uv_launch_layernorm(xl(L), C, lh, C, fln_g, fln_b, M, C, cfg.layer_norm_eps, s));
    if (!pooled) return UV_OK;
    hipLaunchKernelGGL(clip_pool_kernel, dim3((unsigned)B), dim3(256), 0, s, ids, lh, proj ? prow : pooled, S, C, cfg.eos_token_id);
    UV_LAUNCH_CHECK();
    if (proj)      // text_projection has no bias; the small-M kernel takes 8 rows per launch
        for (int m0 = 0; m0 < B; m0 += 8)
            UV_RUN(uv_launch_linear_small(prow + (long)m0 * C, proj, nullptr, pooled + (long)m0 * cfg.projection_dim, B - m0 < 8 ? B - m0 : 8, cfg.projection_dim, C, 0, s));
    return UV_OK;
}
