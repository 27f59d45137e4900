// The temporal VAE behind the pipeline's decode / encode call sites (reference call sites
// backbones/video_diffusion_sd/pipelines/stable_diffusion.py:369-394 decode_latents, :793-818 get_images_from_latents, :820-834 get_latent_image,
// inversion_tools/ddim_inversion.py:28-31,52-55) as ONE host-side graph of the library's gfx950 kernels per call.
//
// The network itself is diffusers' AutoencoderKLTemporalDecoder (the SVD VAE: src/sd/run_*_sd.py:36-42 load it from
// stabilityai/stable-video-diffusion-img2vid) — THIRD-PARTY code that is absent from the reference tree and from both boxes.  Its structure is
// restated here from the published definition (diffusers 0.35: models/autoencoders/autoencoder_kl_temporal_decoder.py, vae.py Encoder,
// unets/unet_3d_blocks.py MidBlockTemporalDecoder / UpBlockTemporalDecoder, resnet.py ResnetBlock2D / TemporalResnetBlock /
// SpatioTemporalResBlock / AlphaBlender, attention_processor.py Attention) with the state-dict keys of that class, so a `vae/` checkpoint loads
// as is; PARITY UNPINNED (the oracle oracle/vae_ref.py is a second restatement of the same definition, not the third-party code).
//
//   encoder  conv_in 3->C0 | 4 x [2 ResnetBlock2D, stride-2 conv (input padded bottom / right only)] | mid: resnet, 1-head attention, resnet |
//            GroupNorm + SiLU + conv_out -> 2*latent | quant_conv 1x1                                      (per frame; no temporal layers)
//   decoder  conv_in latent->C3 | mid: ST-resblock, 1-head attention (head_dim = C3), ST-resblock | 4 x [3 ST-resblocks, nearest x2 + conv] |
//            GroupNorm + SiLU + conv_out -> 3 | time_conv_out: Conv3d (3,1,1) over the frames
//   ST-resblock = ResnetBlock2D (per-frame GroupNorm) -> TemporalResnetBlock (GroupNorm over (C/G, F, H, W), two Conv3d (3,1,1)) -> AlphaBlender
//            (merge "learned", switch_spatial_to_temporal_mix: x = (1 - sigmoid(mix)) * spatial + sigmoid(mix) * temporal)
//
// Kernels: the NHWC implicit-GEMM convs (gemm.hip; the Conv3d (3,1,1) is the 3x1 tap geometry on "image rows = frames, columns = pixels" — no
// wasted taps; nearest x2 folded into the conv addressing; the encoder's asymmetric padding is a tap-geometry parameter), GroupNorm (+SiLU)
// (norm.hip), the linears and — for the single 512-wide head over H/8 x W/8 tokens, which no flash kernel of the library is shaped for — the
// attention as two GEMMs per frame around a row softmax (scores of one frame: N x N fp16, 32 MB at 512 x 512).
#include <math.h>
#include <string.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "kernels.h"
#include "vae.h"

namespace {

// softmax over the rows of S [rows][N] fp16, in place, fp32 arithmetic; one wave per row (N % 8 == 0).  The scores arrive ROUNDED TO fp16: a logit beyond
// 65504 is +inf there and exp(inf - inf) would turn the whole row into NaN (SD-family VAE mid-block activations are large: force_upcast in the stock
// config) — scores are clamped to the fp16 range on load, so such a row degrades to a tie between its saturated keys instead
__global__ __launch_bounds__(256) void v_softmax_rows_kernel(half_t* __restrict__ S, long rows, int N) {
    const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    half_t* r = S + row * N;
    float m = -INFINITY;
    for (int c = lane * 8; c < N; c += 512) {
        const h8 v = *reinterpret_cast<const h8*>(r + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) m = fmaxf(m, fminf((float)v[e], 65504.f));
    }
    m = wave_max(m);
    float l = 0.f;
    for (int c = lane * 8; c < N; c += 512) {
        const h8 v = *reinterpret_cast<const h8*>(r + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) l += __expf(fminf((float)v[e], 65504.f) - m);
    }
    l = wave_sum(l);
    const float inv = 1.f / l;
    for (int c = lane * 8; c < N; c += 512) {
        h8 v = *reinterpret_cast<const h8*>(r + c);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = (half_t)(__expf(fminf((float)v[e], 65504.f) - m) * inv);
        *reinterpret_cast<h8*>(r + c) = v;
    }
}
// [R][C] -> [C][R] through a 32 x 33 LDS tile
__global__ __launch_bounds__(256) void v_transpose_kernel(const half_t* __restrict__ in, half_t* __restrict__ out, int R, int C) {
    __shared__ half_t t[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int i = threadIdx.x; i < 1024; i += 256) {
        const int r = i >> 5, c = i & 31;
        t[r][c] = (r0 + r < R && c0 + c < C) ? in[(long)(r0 + r) * C + c0 + c] : (half_t)0.f;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 1024; i += 256) {
        const int c = i >> 5, r = i & 31;
        if (c0 + c < C && r0 + r < R) out[(long)(c0 + c) * R + r0 + r] = t[r][c];
    }
}
// time_conv_out (Conv3d Cc -> Cc, kernel (3,1,1)) on the NHWC rows of conv_out, written straight into the caller's [B*F, Cc, HW] layout
__global__ __launch_bounds__(256) void v_time_conv_out_kernel(const half_t* __restrict__ x, int ldx, half_t* __restrict__ y, const half_t* __restrict__ w,
                                                              const half_t* __restrict__ bias, int B, int F, long HW, int Cc) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * F * HW) return;
    const long pix = i % HW;
    const long bf = i / HW;
    const int f = (int)(bf % F);
    for (int co = 0; co < Cc; ++co) {
        float acc = (float)bias[co];
        for (int t = 0; t < 3; ++t) {
            const int ff = f + t - 1;
            if (ff < 0 || ff >= F) continue;
            const half_t* xr = x + (i + (long)(t - 1) * HW) * ldx;
            for (int ci = 0; ci < Cc; ++ci) acc += (float)w[((long)co * Cc + ci) * 3 + t] * (float)xr[ci];
        }
        y[(bf * Cc + co) * HW + pix] = (half_t)acc;
    }
}

}  // namespace

// query rows per chunk of the one-head attention under a score budget: the largest multiple of the 128-row GEMM tile whose [Qc, N] fp16 scores fit,
// at least one tile, at most N (the attention and the arena formula both size from it)
long uv_vae_attn_chunk_rows(long score_bytes, long N) {
    long Qc = score_bytes / (2L * N) / 128 * 128;
    if (Qc < 128) Qc = 128;
    return Qc > N ? N : Qc;
}

int Vae::finalize(hipStream_t s) {
    clear_derived();
    mix.clear();
    std::vector<std::string> keys;
    for (auto& kv : weights) keys.push_back(kv.first);
    auto ends = [](const std::string& a, const char* suf) {
        size_t n = strlen(suf);
        return a.size() >= n && a.compare(a.size() - n, n, suf) == 0;
    };
    for (const std::string& k : keys) {
        const WTensor& t = weights[k];
        if ((t.shape.size() == 4 || t.shape.size() == 5) && ends(k, ".weight") && k != "decoder.time_conv_out.weight") {
            // Conv2d [Co,Ci,kh,kw] / Conv3d [Co,Ci,3,1,1] -> [Co][taps][CiP] (+ the tap-inner copy for the 256x320 tile's fast im2col addressing)
            int taps = 1;
            for (size_t d = 2; d < t.shape.size(); ++d) taps *= (int)t.shape[d];
            if (t.shape.size() == 4) UV_REQUIRE((taps == 1 || taps == 9) && t.shape[2] == t.shape[3], "%s: only 1x1 / 3x3 Conv2d", k.c_str());
            else UV_REQUIRE(taps == 3 && t.shape[2] == 3, "%s: only (3,1,1) Conv3d", k.c_str());
            UV_RUN(uv_derive_conv_layouts(*this, k, s));
        } else if (ends(k, ".to_q.weight") || ends(k, ".to_q.bias")) {
            // the attention scale 1/sqrt(head_dim) (one head: head_dim = C) rides on the q projection, so the fp16 scores are the scaled ones
            long n = 1;
            for (long v : t.shape) n *= v;
            half_t* d;
            UV_RUN(derive(k + "#qs", t.shape, &d));
            UV_RUN(uv_launch_scale_f16(t.ptr, d, n, 1.f / sqrtf((float)t.shape[0]), s));
        }
    }
    UV_LAUNCH_CHECK();
    // AlphaBlender mix factors: one scalar per ST-resblock, read once
    for (const std::string& k : keys) {
        if (!ends(k, ".time_mixer.mix_factor")) continue;
        half_t h;
        UV_HIP(hipMemcpyAsync(&h, weights[k].ptr, sizeof(half_t), hipMemcpyDeviceToHost, s));
        UV_HIP(hipStreamSynchronize(s));
        mix[k.substr(0, k.size() - strlen(".time_mixer.mix_factor"))] = (float)h;
    }
    // The AlphaBlender folded into the temporal block's second conv: blended = alpha * s + (1 - alpha) * (s + h) = s + sigmoid(mix) * h with h = conv2(...) + bias,
    // so conv2's weight and bias are scaled by sigmoid(mix) once and the residual add of its epilogue IS the blend (one pass over three tensors less per block)
    for (auto& kv : mix) {
        const float sig = 1.f / (1.f + expf(-kv.second));
        for (const char* suf : {".temporal_res_block.conv2.weight#nhwc", ".temporal_res_block.conv2.bias"}) {
            const WTensor* t = find(kv.first + suf);
            UV_REQUIRE(t, "%s%s missing", kv.first.c_str(), suf);
            long n = 1;
            for (long v : t->shape) n *= v;
            half_t* d;
            UV_RUN(derive(kv.first + suf + "#mix", t->shape, &d));
            UV_RUN(uv_launch_scale_f16(t->ptr, d, n, sig, s));
        }
    }
    UV_LAUNCH_CHECK();
    UV_HIP(hipStreamSynchronize(s));
    finalized = true;
    return UV_OK;
}

namespace {
struct VFwd {
    Vae& u;
    hipStream_t s;
    float* gn_ws = nullptr;

    half_t* alloc(long elems) {
        half_t* p = (half_t*)u.arena.alloc((size_t)elems * sizeof(half_t));
        if (!p) uv_set_error("vae: activation arena exhausted (%zu bytes)", u.arena.size);
        return p;
    }
    void free(void* p) { u.arena.release(p); }
    half_t* W(const std::string& k) { return u.W(k); }

    int groupnorm(const Act& a, long rows_per_stat, const std::string& p, int silu, half_t* out, float eps = 1e-6f) {
        half_t *g = W(p + ".weight"), *b = W(p + ".bias");
        if (!g || !b) return u.missing_error("vae");
        return uv_launch_groupnorm(a.p, nullptr, a.C, 0, a.rows(), (int)rows_per_stat, u.cfg.norm_num_groups, eps, g, b, silu, out, gn_ws, s);
    }
    // 2-D conv on [imgs, H, W, C]; asym: the encoder's stride-2 conv (input padded at the bottom / right only)
    // ldy > Cout (the plain VAE's post_quant_conv in front of a conv that reads channels padded to 8): rows of ldy halfs, the columns behind Cout zero
    int conv(const Act& a, const std::string& p, int Cout, int taps, int stride, int up, bool asym, const half_t* R, Act* out, int ldy = 0) {
        GemmParams g = conv_params(a, nullptr, taps, stride, up, asym);
        g.N = Cout;
        g.korder = (taps == 9 && !asym && stride == 1 && a.C % 64 == 0 && u.find(p + ".weight#ti")) ? 1 : 0;
        g.W = W(p + (g.korder ? ".weight#ti" : ".weight#nhwc"));
        g.bias = W(p + ".bias");
        if (!g.W || !g.bias) return u.missing_error("vae");
        g.R = R;
        g.ldr = Cout;
        out->imgs = a.imgs;
        out->H = g.Ho;
        out->W = g.Wo;
        out->C = ldy > Cout ? ldy : Cout;
        out->p = alloc(out->rows() * out->C);
        if (!out->p) return UV_ERR_STATE;
        if (out->C > Cout) UV_HIP(hipMemsetAsync(out->p, 0, (size_t)out->rows() * out->C * sizeof(half_t), s));
        g.Y = out->p;
        g.ldy = out->C;
        return uv_launch_gemm(g, 1, s);
    }
    // Conv3d (3,1,1) over the F frames of every pixel: the 3x1 tap geometry on (image rows = frames, image columns = pixels)
    int frame_conv(const Act& a, int F, const std::string& p, const half_t* R, half_t* out, const char* mixsuf = "") {
        GemmParams g;
        g.X = a.p;
        g.C1 = a.C;
        g.Hs = F;
        g.Ws = a.H * a.W;
        g.taps = 3;
        g.tapw = 1;
        g.pady = 1;
        g.padx = 0;
        g.Ho = F;
        g.Wo = g.Ws;
        g.M = (int)a.rows();
        g.N = a.C;
        g.K = 3 * a.C;
        g.W = W(p + ".weight#nhwc" + mixsuf);
        g.bias = W(p + ".bias" + mixsuf);
        if (!g.W || !g.bias) return u.missing_error("vae");
        g.R = R;
        g.ldr = a.C;
        g.Y = out;
        g.ldy = a.C;
        return uv_launch_gemm(g, 1, s);
    }
    int linear(const half_t* X, long M, int K, const half_t* Wt, const half_t* bias, int N, half_t* Y, const half_t* R = nullptr) {
        return uv_launch_gemm(lin_params(X, M, K, Wt, N, Y, bias, R), 0, s);
    }
    // diffusers ResnetBlock2D without a time embedding: GroupNorm (per image) + SiLU -> conv -> GroupNorm + SiLU -> conv, + (1x1 conv of) the input
    int resnet2d(const std::string& p, const Act& x, int Cout, Act* out) {
        const long hw = (long)x.H * x.W;
        half_t* n1 = alloc(x.rows() * x.C);
        if (!n1) return UV_ERR_STATE;
        UV_RUN(groupnorm(x, hw, p + ".norm1", 1, n1));
        Act n1a{n1, x.imgs, x.H, x.W, x.C}, h;
        UV_RUN(conv(n1a, p + ".conv1", Cout, 9, 1, 0, false, nullptr, &h));
        free(n1);
        half_t* n2 = alloc(h.rows() * Cout);
        if (!n2) return UV_ERR_STATE;
        UV_RUN(groupnorm(h, hw, p + ".norm2", 1, n2));
        free(h.p);
        const half_t* res = x.p;
        Act sc{};
        if (u.find(p + ".conv_shortcut.weight")) {
            UV_RUN(conv(x, p + ".conv_shortcut", Cout, 1, 1, 0, false, nullptr, &sc));
            res = sc.p;
        } else {
            UV_REQUIRE(x.C == Cout, "%s: no conv_shortcut but %d -> %d channels", p.c_str(), x.C, Cout);
        }
        Act n2a{n2, x.imgs, x.H, x.W, Cout};
        UV_RUN(conv(n2a, p + ".conv2", Cout, 9, 1, 0, false, res, out));
        free(n2);
        if (sc.p) free(sc.p);
        return UV_OK;
    }
    // diffusers TemporalResnetBlock (in == out channels, no time embedding) on [B, F, H, W, C]: GroupNorm over (C/G, F, H, W), eps 1e-5
    // (Mid / UpBlockTemporalDecoder build their ST-resblocks with eps = 1e-6, temporal_eps = 1e-5), with the ST-resblock's AlphaBlender in its last epilogue
    int resnet_temporal(const std::string& p, const Act& x, int F, half_t* out) {
        const long rps = (long)F * x.H * x.W;
        half_t* n1 = alloc(x.rows() * x.C);
        if (!n1) return UV_ERR_STATE;
        UV_RUN(groupnorm(x, rps, p + ".norm1", 1, n1, 1e-5f));
        half_t* h = alloc(x.rows() * x.C);
        if (!h) return UV_ERR_STATE;
        Act n1a{n1, x.imgs, x.H, x.W, x.C};
        UV_RUN(frame_conv(n1a, F, p + ".conv1", nullptr, h));
        Act ha{h, x.imgs, x.H, x.W, x.C};
        UV_RUN(groupnorm(ha, rps, p + ".norm2", 1, n1, 1e-5f));
        UV_RUN(frame_conv(n1a, F, p + ".conv2", x.p, out, "#mix"));     // x + sigmoid(mix) * (conv2 + bias): the block's output AND the AlphaBlender (finalize)
        free(h);
        free(n1);
        return UV_OK;
    }
    // diffusers SpatioTemporalResBlock with AlphaBlender("learned", switch_spatial_to_temporal_mix = True)
    int st_resblock(const std::string& p, const Act& x, int F, int Cout, Act* out) {
        Act sp;
        UV_RUN(resnet2d(p + ".spatial_res_block", x, Cout, &sp));
        auto it = u.mix.find(p);
        UV_REQUIRE(it != u.mix.end(), "%s: time_mixer.mix_factor missing", p.c_str());
        half_t* tp = alloc(sp.rows() * Cout);
        if (!tp) return UV_ERR_STATE;
        UV_RUN(resnet_temporal(p + ".temporal_res_block", sp, F, tp));      // = alpha * spatial + (1 - alpha) * temporal, alpha = 1 - sigmoid(mix): folded into conv2
        free(sp.p);
        sp.p = tp;
        *out = sp;
        return UV_OK;
    }
    // diffusers Attention(heads = 1, dim_head = C, norm_num_groups, residual_connection, bias) over the H*W tokens of every image.
    // Numerics: the scaled scores of a frame are stored in fp16 between the QK^T GEMM and the row softmax (|ds| <= 2^-11 |s|: for logits of a few tens
    // that is the size of the error the fp16 q and k rows themselves carry — the reference runs this VAE in fp16 too, `vae.to(weight_dtype)`); the softmax
    // arithmetic and the PV accumulation are fp32.  A d = 512 flash kernel would avoid the N x N round trip; at 64 x 64 tokens the two GEMMs take 2 % of a decode.
    // score_bytes > 0 (the plain VAE): the query rows of a frame go through in chunks of Qc rows against all N keys, Qc the largest multiple of the
    // 128-row GEMM tile whose [Qc, N] fp16 scores fit the budget (at least one tile).  Every chunk sees every key, so a chunk's softmax rows are final:
    // nothing is merged.  score_bytes == 0 (the temporal VAE): one chunk, the whole frame.
    int attention(const std::string& p, const Act& x, Act* out, long score_bytes = 0, long* chunks = nullptr) {
        const int C = x.C, N = x.H * x.W;
        const long rows = x.rows();
        UV_REQUIRE(N % 8 == 0 && C % 8 == 0, "%s: %d tokens x %d channels", p.c_str(), N, C);
        const long Qc = score_bytes > 0 ? uv_vae_attn_chunk_rows(score_bytes, N) : N;
        if (chunks) *chunks = (N + Qc - 1) / Qc;
        half_t* gn = alloc(rows * C);
        if (!gn) return UV_ERR_STATE;
        UV_RUN(groupnorm(x, N, p + ".group_norm", 0, gn));
        half_t *q = alloc(rows * C), *k = alloc(rows * C), *v = alloc(rows * C);
        if (!q || !k || !v) return UV_ERR_STATE;
        half_t *wq = W(p + ".to_q.weight#qs"), *bq = W(p + ".to_q.bias#qs"), *wk = W(p + ".to_k.weight"), *bk = W(p + ".to_k.bias"), *wv = W(p + ".to_v.weight"),
               *bv = W(p + ".to_v.bias"), *wo = W(p + ".to_out.0.weight"), *bo = W(p + ".to_out.0.bias");
        if (!wq || !bq || !wk || !bk || !wv || !bv || !wo || !bo) return u.missing_error("vae");
        UV_RUN(linear(gn, rows, C, wq, bq, C, q));
        UV_RUN(linear(gn, rows, C, wk, bk, C, k));
        UV_RUN(linear(gn, rows, C, wv, bv, C, v));
        half_t *S = alloc(Qc * N), *vT = alloc((long)N * C);
        if (!S || !vT) return UV_ERR_STATE;
        for (int f = 0; f < x.imgs; ++f) {
            const long o = (long)f * N * C;
            for (long c0 = 0; c0 < N; c0 += Qc) {
                const long qc = N - c0 < Qc ? N - c0 : Qc;                                      // the last chunk may be ragged (a multiple of 8 rows)
                UV_RUN(linear(q + o + c0 * C, qc, C, k + o, nullptr, N, S));                    // scores [qc, N] (already scaled: the scale rides on q)
                hipLaunchKernelGGL(v_softmax_rows_kernel, dim3((unsigned)((qc + 3) / 4)), dim3(256), 0, s, S, qc, N);
                // V^T once per frame, behind the first chunk's softmax
                if (c0 == 0) hipLaunchKernelGGL(v_transpose_kernel, dim3((C + 31) / 32, (N + 31) / 32), dim3(256), 0, s, v + o, vT, N, C);
                UV_LAUNCH_CHECK();
                UV_RUN(linear(S, qc, N, vT, nullptr, C, gn + o + c0 * C));                      // O = P V  (gn is free by now)
            }
        }
        free(S);
        free(vT);
        free(q);
        free(k);
        free(v);
        out->imgs = x.imgs; out->H = x.H; out->W = x.W; out->C = C;
        out->p = alloc(rows * C);
        if (!out->p) return UV_ERR_STATE;
        UV_RUN(linear(gn, rows, C, wo, bo, C, out->p, x.p));
        free(gn);
        return UV_OK;
    }

    // ---- the walks.  The arena is first-fit, so where a buffer is taken and given back is part of the graph: a stage takes what it needs, then its
    // input is released
    // one step of a walk: stage(&y) runs on `cur` into a fresh y, cur's buffer is released, cur = y
    template <class Stage>
    int step(Act& cur, Stage stage) {
        Act nxt;
        UV_RUN(stage(&nxt));
        free(cur.p);
        cur = nxt;
        return UV_OK;
    }
    int take_gn_ws(long imgs) {
        gn_ws = (float*)u.arena.alloc((size_t)uv_groupnorm_workspace_floats((int)imgs, u.cfg.norm_num_groups) * 4);
        return gn_ws ? UV_OK : UV_ERR_STATE;
    }
    // the caller's [imgs, C, H, W] as NHWC rows with the channels zero padded to 8
    int load_nchw(const half_t* src, long imgs, int C, int H, int Wd, Act* out) {
        const int Cp = (C + 7) / 8 * 8;
        *out = Act{alloc(imgs * H * Wd * Cp), (int)imgs, H, Wd, Cp};
        if (!out->p) return UV_ERR_STATE;
        return uv_launch_ncfhw_to_nhwc(src, out->p, (int)imgs, C, 1, H * Wd, Cp, s);
    }
    // the end of the encoder and of the decoder: GroupNorm + SiLU + conv_out.  Not a step: cur goes back as soon as it is normalised, before the conv takes its output
    int norm_conv_out(const std::string& side, Act& cur, int Cout) {
        Act na{alloc(cur.rows() * cur.C), cur.imgs, cur.H, cur.W, cur.C};
        if (!na.p) return UV_ERR_STATE;
        UV_RUN(groupnorm(cur, (long)cur.H * cur.W, side + ".conv_norm_out", 1, na.p));
        free(cur.p);
        UV_RUN(conv(na, side + ".conv_out", Cout, 9, 1, 0, false, nullptr, &cur));
        free(na.p);
        return UV_OK;
    }
    // The encoder of both handles (it has no temporal layer): x [imgs, in_channels, H, W] -> moments [imgs, 2*latent, H/8, W/8].  quant_conv: the 1x1 conv
    // behind conv_out runs (the temporal VAE always has it, the plain one by its config); score_bytes / chunks: the attention's (0 / null: one chunk)
    int encoder(const half_t* xin, long imgs, int H, int Wd, half_t* moments, bool quant_conv, long score_bytes, long* chunks) {
        const int* boc = u.cfg.block_out_channels;
        const int L2 = 2 * u.cfg.latent_channels;
        UV_RUN(take_gn_ws(imgs));
        Act cur;
        UV_RUN(load_nchw(xin, imgs, u.cfg.in_channels, H, Wd, &cur));
        UV_RUN(step(cur, [&](Act* y) { return conv(cur, "encoder.conv_in", boc[0], 9, 1, 0, false, nullptr, y); }));
        for (int b = 0; b < 4; ++b) {
            const std::string down = "encoder.down_blocks." + std::to_string(b);
            for (int l = 0; l < u.cfg.layers_per_block; ++l)
                UV_RUN(step(cur, [&](Act* y) { return resnet2d(down + ".resnets." + std::to_string(l), cur, boc[b], y); }));
            if (b < 3) UV_RUN(step(cur, [&](Act* y) { return conv(cur, down + ".downsamplers.0.conv", boc[b], 9, 2, 0, true, nullptr, y); }));
        }
        UV_RUN(step(cur, [&](Act* y) { return resnet2d("encoder.mid_block.resnets.0", cur, boc[3], y); }));
        UV_RUN(step(cur, [&](Act* y) { return attention("encoder.mid_block.attentions.0", cur, y, score_bytes, chunks); }));
        UV_RUN(step(cur, [&](Act* y) { return resnet2d("encoder.mid_block.resnets.1", cur, boc[3], y); }));
        UV_RUN(norm_conv_out("encoder", cur, L2));
        if (quant_conv) UV_RUN(step(cur, [&](Act* y) { return conv(cur, "quant_conv", L2, 1, 1, 0, false, nullptr, y); }));
        UV_RUN(uv_launch_nhwc_to_ncfhw(cur.p, L2, moments, (int)imgs, L2, 1, cur.H * cur.W, s));
        free(cur.p);
        free(gn_ws);
        return UV_OK;
    }
    // The decoder of both handles from conv_in through conv_out, on cur = the latents as NHWC rows (channels padded to 8); cur leaves as conv_out's
    // rows.  F > 0: the temporal decoder on clips of F frames (ST-resblocks; MidBlockTemporalDecoder.forward zips resnets[1:] with its ONE attention, so
    // resnets[1] runs behind it only where layers_per_block >= 2).  F == 0: the plain one (ResnetBlock2D; UNetMidBlock2D always has resnets[1]).
    int decoder(Act& cur, int F, long score_bytes, long* chunks) {
        const int* boc = u.cfg.block_out_channels;
        auto resblock = [&](const std::string& p, int Cout, Act* y) { return F > 0 ? st_resblock(p, cur, F, Cout, y) : resnet2d(p, cur, Cout, y); };
        UV_RUN(step(cur, [&](Act* y) { return conv(cur, "decoder.conv_in", boc[3], 9, 1, 0, false, nullptr, y); }));
        UV_RUN(step(cur, [&](Act* y) { return resblock("decoder.mid_block.resnets.0", boc[3], y); }));
        UV_RUN(step(cur, [&](Act* y) { return attention("decoder.mid_block.attentions.0", cur, y, score_bytes, chunks); }));
        if (F == 0 || u.cfg.layers_per_block >= 2) UV_RUN(step(cur, [&](Act* y) { return resblock("decoder.mid_block.resnets.1", boc[3], y); }));
        for (int b = 0; b < 4; ++b) {
            const int Cout = boc[3 - b];
            const std::string up = "decoder.up_blocks." + std::to_string(b);
            for (int l = 0; l < u.cfg.layers_per_block + 1; ++l)
                UV_RUN(step(cur, [&](Act* y) { return resblock(up + ".resnets." + std::to_string(l), Cout, y); }));
            if (b < 3) UV_RUN(step(cur, [&](Act* y) { return conv(cur, up + ".upsamplers.0.conv", Cout, 9, 1, 1, false, nullptr, y); }));
        }
        return norm_conv_out("decoder", cur, u.cfg.out_channels);
    }
};
}  // namespace

// The arena for imgs images of H x W pixels.  The largest live set is at the output resolution: ~5 tensors of `wide` channels (the last upsampler's
// output and the GroupNorm copies around it; the widest width a graph has there) plus the attention at 1/8 resolution: its score matrix of
// score_rows x N and the token tensors around it
size_t Vae::arena_need(long imgs, int H, int Wd, int wide, long score_rows) const {
    const size_t rows = (size_t)imgs * H * Wd;
    const size_t N = (size_t)(H / 8) * (Wd / 8);
    return rows * wide * 2 * 5 + (size_t)score_rows * N * 2 + (size_t)imgs * N * cfg.block_out_channels[3] * 2 * 8 + (256u << 20);
}

int Vae::reserve(long imgs, int H, int Wd) {
    // the second-narrowest width at the output resolution, the whole score matrix of one frame
    return arena.ensure(arena_need(imgs, H, Wd, cfg.block_out_channels[1], (long)(H / 8) * (Wd / 8)));
}

// z [imgs, latent, h, w] fp16 (already divided by the scaling factor) -> out [imgs, out_channels, 8h, 8w] fp16; imgs = clips x num_frames
int Vae::decode(const half_t* z, long imgs, int num_frames, int h, int w, half_t* out, hipStream_t s) {
    UV_REQUIRE(finalized, "vae_decode: call univst_vae_finalize after loading weights");
    UV_REQUIRE(imgs > 0 && num_frames > 0 && imgs % num_frames == 0 && h > 0 && w > 0, "vae_decode: %ld images are not whole clips of %d frames", imgs, num_frames);
    UV_RUN(reserve(imgs, h * 8, w * 8));
    clear_missing();
    VFwd f{*this, s};
    UV_RUN(f.take_gn_ws(imgs));
    Act cur;
    UV_RUN(f.load_nchw(z, imgs, cfg.latent_channels, h, w, &cur));
    UV_RUN(f.decoder(cur, num_frames, 0, nullptr));
    half_t *tw = W("decoder.time_conv_out.weight"), *tb = W("decoder.time_conv_out.bias");
    if (!tw || !tb) return missing_error("vae");
    const long HW = (long)cur.H * cur.W;
    hipLaunchKernelGGL(v_time_conv_out_kernel, dim3(nb(imgs * HW)), dim3(256), 0, s, cur.p, cfg.out_channels, out, tw, tb, (int)(imgs / num_frames), num_frames, HW,
                       cfg.out_channels);
    UV_LAUNCH_CHECK();
    f.free(cur.p);
    return UV_OK;
}

// x [imgs, in_channels, H, W] fp16 in [-1, 1] -> moments [imgs, 2*latent, H/8, W/8] fp16 (mean | logvar; the caller samples)
int Vae::encode(const half_t* xin, long imgs, int H, int Wd, half_t* moments, hipStream_t s) {
    UV_REQUIRE(finalized, "vae_encode: call univst_vae_finalize after loading weights");
    UV_REQUIRE(imgs > 0 && H % 8 == 0 && Wd % 8 == 0, "vae_encode: %ld images of %d x %d (multiples of 8)", imgs, H, Wd);
    UV_RUN(reserve(imgs, H, Wd));
    clear_missing();
    VFwd f{*this, s};
    return f.encoder(xin, imgs, H, Wd, moments, true, 0, nullptr);
}

// ------------------------------------------------------------------------------------------ the plain AutoencoderKL (univst_klvae)
// diffusers 0.35 AutoencoderKL (models/autoencoders/autoencoder_kl.py; vae.py Encoder / Decoder, unet_2d_blocks.py DownEncoderBlock2D / UpDecoderBlock2D /
// UNetMidBlock2D with mid_block_add_attention) under that class's state-dict names — THIRD-PARTY, restated from the published definition; PARITY UNPINNED
// (tests/klvae_ref.py is a second restatement).  Both handles run VFwd::encoder (quant_conv only where the config has one) and VFwd::decoder, here with
// plain resblocks:
//   [post_quant_conv 1x1] | conv_in | mid: resnet, 1-head attention, resnet | 4 x [layers_per_block + 1 ResnetBlock2D, nearest x2 + conv on the first three] |
//   GroupNorm + SiLU + conv_out
// with no temporal layer.  No layer couples images, so a call runs its batch in groups whose arena need stays under pass_bytes, and the attention's
// score matrix is bounded by attn_score_bytes (VFwd::attention).
size_t KlVae::need_bytes(long imgs, int H, int Wd) const {
    // the widest tensor at the full resolution (a config may have its first width above its second), the score matrix bounded by the budget
    const int* boc = cfg.block_out_channels;
    return arena_need(imgs, H, Wd, boc[0] > boc[1] ? boc[0] : boc[1], uv_vae_attn_chunk_rows(score_bytes(), (long)(H / 8) * (Wd / 8)));
}

long KlVae::group_of(long imgs, int H, int Wd) const {
    const size_t budget = kcfg.pass_bytes > 0 ? (size_t)kcfg.pass_bytes : (size_t)8 << 30;
    const size_t one = need_bytes(1, H, Wd), per = need_bytes(2, H, Wd) - one;      // the need is linear in the image count
    long g = budget > one ? 1 + (long)((budget - one) / per) : 1;
    return g < imgs ? g : imgs;
}

// z [imgs, latent, h, w] fp16 (already z / scaling_factor + shift_factor) -> out [imgs, out_channels, 8h, 8w] fp16
int KlVae::decode(const half_t* z, long imgs, int h, int w, half_t* out, hipStream_t s) {
    UV_REQUIRE(finalized, "klvae_decode: call univst_klvae_finalize after loading weights");
    UV_REQUIRE(imgs > 0 && h > 0 && w > 0, "klvae_decode: %ld images of %d x %d latents", imgs, h, w);
    UV_REQUIRE(((long)h * w) % 8 == 0, "klvae_decode: %d x %d latents: the token count of the mid-block attention must be a multiple of 8", h, w);
    const long g = group_of(imgs, h * 8, w * 8);
    UV_RUN(arena.ensure(need_bytes(g, h * 8, w * 8)));
    clear_missing();
    passes = 0;
    for (long i0 = 0; i0 < imgs; i0 += g, ++passes) {
        const long n = imgs - i0 < g ? imgs - i0 : g;
        UV_RUN(decode_pass(z + i0 * cfg.latent_channels * h * w, n, h, w, out + i0 * cfg.out_channels * 64L * h * w, s));
    }
    return UV_OK;
}

// one group: the head (post_quant_conv, written with its channels padded to 8 as conv_in reads them), VFwd::decoder, the layout of the caller
int KlVae::decode_pass(const half_t* z, long imgs, int h, int w, half_t* out, hipStream_t s) {
    VFwd f{*this, s};
    UV_RUN(f.take_gn_ws(imgs));
    Act cur;
    UV_RUN(f.load_nchw(z, imgs, cfg.latent_channels, h, w, &cur));
    if (kcfg.use_post_quant_conv)
        UV_RUN(f.step(cur, [&](Act* y) { return f.conv(cur, "post_quant_conv", cfg.latent_channels, 1, 1, 0, false, nullptr, y, cur.C); }));
    UV_RUN(f.decoder(cur, 0, score_bytes(), &attn_chunks));
    UV_RUN(uv_launch_nhwc_to_ncfhw(cur.p, cfg.out_channels, out, (int)imgs, cfg.out_channels, 1, cur.H * cur.W, s));
    f.free(cur.p);
    f.free(f.gn_ws);
    return UV_OK;
}

// x [imgs, in_channels, H, W] fp16 in [-1, 1] -> moments [imgs, 2*latent, H/8, W/8] fp16 (mean | logvar; the caller samples)
int KlVae::encode(const half_t* xin, long imgs, int H, int Wd, half_t* moments, hipStream_t s) {
    UV_REQUIRE(finalized, "klvae_encode: call univst_klvae_finalize after loading weights");
    UV_REQUIRE(imgs > 0 && H > 0 && Wd > 0 && H % 8 == 0 && Wd % 8 == 0, "klvae_encode: %ld images of %d x %d (multiples of 8)", imgs, H, Wd);
    UV_REQUIRE(((long)(H / 8) * (Wd / 8)) % 8 == 0, "klvae_encode: %d x %d pixels: the token count of the mid-block attention (H/8 * W/8) must be a multiple of 8", H, Wd);
    const long g = group_of(imgs, H, Wd);
    UV_RUN(arena.ensure(need_bytes(g, H, Wd)));
    clear_missing();
    passes = 0;
    for (long i0 = 0; i0 < imgs; i0 += g, ++passes) {
        const long n = imgs - i0 < g ? imgs - i0 : g;
        VFwd f{*this, s};
        UV_RUN(f.encoder(xin + i0 * cfg.in_channels * H * Wd, n, H, Wd, moments + i0 * 2 * cfg.latent_channels * (H / 8) * (Wd / 8), kcfg.use_quant_conv, score_bytes(),
                         &attn_chunks));
    }
    return UV_OK;
}
