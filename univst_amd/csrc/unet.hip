// The whole pseudo-3D SD UNet forward as ONE host-side graph of gfx950 kernels (one C-ABI call per
// denoising step).  Activations live in NHWC fp16 ([B*F*H*W, C] == the transformer's token layout), chosen
// once at conv_in, so every rearrange/permute/cat/upsample of the reference disappears into kernel
// addressing.  Weights are owned by the handle (device fp16 copies keyed by the reference state-dict
// names) plus derived layouts built by finalize().  A first-fit arena supplies all activations; nothing is
// allocated inside forward() after the first call for a geometry.
//
// Structure restated from: unet_3d_condition.py:306-443, unet_3d_blocks.py:129-645, attention.py:104-346,
// resnet.py:335-394, pnp_utils.py:20-111.  Dead work of the reference that is skipped because it is an
// exact identity for 2-D-initialised weights (verified at finalize): temporal conv1d (dirac, resnet.py:53-55)
// and temporal attention (zero to_out weight => adds its bias, attention.py:233).
//
// The same graph serves the AnimateDiff UNet3D (univst_unet_create_animatediff; backbones/animatediff/models/unet.py, unet_blocks.py:271-276,
// :382-421, :621-667, resnet.py:10-29, attention.py:327-371, pnp_utils.py:18-109 of that backbone): GroupNorms per frame, attn1 over the frame's own
// keys, no attn_temp / temporal convs, and a motion module (motion.hip) behind every resnet / transformer pair, its chain on this handle's arena.
#include <math.h>
#include <string.h>

#include <map>
#include <string>
#include <unordered_map>
#include <vector>

#include "comm.h"
#include "kernels.h"
#include "unet.h"

namespace {

// [Co,Ci,3,3] -> [Co][Ci/32][9][32] (conv_patch_kernel: a k tile is two consecutive (32-channel slab, tap) units)
__global__ void permute_conv_weight_t32_kernel(const half_t* __restrict__ in, half_t* __restrict__ out, int Co, int Ci) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    long total = (long)Co * Ci * 9;
    if (i >= total) return;
    int j = (int)(i % 32);
    int t = (int)((i / 32) % 9);
    int q = (int)((i / (32 * 9)) % (Ci / 32));
    int o = (int)(i / ((long)Ci * 9));
    out[i] = in[((long)o * Ci + q * 32 + j) * 9 + t];
}

// LayerNorm folded into the following linear (GemmParams::ln_stats): W'[n][k] = fp16(gamma[k] * W[n][k]), wsum[n] = sum_k W'[n][k]
// (of the ROUNDED values: it has to cancel mean * sum_k W' exactly), lnb[n] = bias[n] + sum_k beta[k] * W[n][k].  One wave per row.
__global__ __launch_bounds__(64) void ln_fold_weight_kernel(const half_t* __restrict__ W, const half_t* __restrict__ gamma,
                                                            const half_t* __restrict__ beta, const half_t* __restrict__ bias,
                                                            half_t* __restrict__ Wout, float* __restrict__ wsum, float* __restrict__ lnb, int K) {
    const int n = blockIdx.x, lane = threadIdx.x;
    float s = 0.f, b = 0.f;
    for (int k = lane; k < K; k += 64) {
        const float w = (float)W[(long)n * K + k];
        const half_t wp = (half_t)(w * (float)gamma[k]);
        Wout[(long)n * K + k] = wp;
        s += (float)wp;
        b = fmaf((float)beta[k], w, b);
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        s += __shfl_xor(s, o, 64);
        b += __shfl_xor(b, o, 64);
    }
    if (lane == 0) {
        wsum[n] = s;
        lnb[n] = b + (bias ? (float)bias[n] : 0.f);
    }
}

__global__ void count_nonzero_kernel(const half_t* __restrict__ w, long n, unsigned* cnt) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && (float)w[i] != 0.f) atomicAdd(cnt, 1u);
}

// per-unit variants (slot i of a counter array): which temporal layers are trained?
__global__ void count_not_dirac_slot_kernel(const half_t* __restrict__ w, int Co, int Ci, int k, unsigned* cnt) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)Co * Ci * k) return;
    int t = (int)(i % k), ci = (int)((i / k) % Ci), co = (int)(i / ((long)k * Ci));
    float expect = (co == ci && t == k / 2) ? 1.f : 0.f;
    if ((float)w[i] != expect) atomicAdd(cnt, 1u);
}
// Conv1d weight [C][C][3] over frames -> a 3x3 conv weight [C][ky][kx][CP] on the geometry (rows = frames, columns = pixels) whose
// side columns (kx != 1) are zero: the temporal conv runs through the ordinary implicit-GEMM conv kernels
__global__ void embed_temporal_weight_kernel(const half_t* __restrict__ in, half_t* __restrict__ out, int C) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)C * 9 * C) return;
    const int ci = (int)(i % C), tap = (int)((i / C) % 9), co = (int)(i / ((long)C * 9));
    const int ky = tap / 3, kx = tap % 3;
    out[i] = kx == 1 ? in[((long)co * C + ci) * 3 + ky] : (half_t)0.f;
}
// trained temporal conv on few channels (conv_out: 4): y[b,f,p,co] = bias[co] + sum_t sum_ci W[co][ci][t] x[b,f+t-1,p,ci]
__global__ void temporal_conv_small_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, const half_t* __restrict__ w,
                                           const half_t* __restrict__ bias, int B, int F, long HW, int C) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * F * HW * C) return;
    const int co = (int)(i % C);
    const long row = i / C;
    const int f = (int)((row / HW) % F);
    float acc = (float)bias[co];
    for (int t = 0; t < 3; ++t) {
        const int ff = f + t - 1;
        if (ff < 0 || ff >= F) continue;
        const half_t* xr = x + (row + (long)(t - 1) * HW) * C;
        for (int ci = 0; ci < C; ++ci) acc += (float)w[((long)co * C + ci) * 3 + t] * (float)xr[ci];
    }
    y[i] = (half_t)acc;
}
// trained temporal attention (attention.py:336-346): every pixel attends over the F frames of its clip.  One thread per
// (branch, pixel, head, query frame); q | k | v rows [(b f) n, 3C]; F <= 32.  A fine-tuned-checkpoint path: correctness first.
template <int D8>
__global__ __launch_bounds__(256) void temporal_attn_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ out, int B, int F, int N, int C,
                                                            int heads, float scale) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long)B * N * heads * F) return;
    const int n = (int)(i % N);
    const int f = (int)((i / N) % F);
    const int h = (int)((i / ((long)N * F)) % heads);
    const int b = (int)(i / ((long)N * F * heads));
    const long ld = 3L * C;
    const half_t* base = qkv + ((long)b * F * N + n) * ld + h * (D8 * 8);      // frame 0 of this pixel
    const long fs = (long)N * ld;                                             // frame stride
    h8 q[D8];
#pragma unroll
    for (int c = 0; c < D8; ++c) q[c] = *reinterpret_cast<const h8*>(base + f * fs + c * 8);
    float p[32];
    float mx = -INFINITY;
#pragma unroll
    for (int g = 0; g < 32; ++g) {
        p[g] = -INFINITY;
        if (g < F) {
            float s = 0.f;
#pragma unroll
            for (int c = 0; c < D8; ++c) {
                const h8 k8 = *reinterpret_cast<const h8*>(base + g * fs + C + c * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) s += (float)q[c][e] * (float)k8[e];
            }
            p[g] = s * scale;
            mx = fmaxf(mx, p[g]);
        }
    }
    float l = 0.f;
#pragma unroll
    for (int g = 0; g < 32; ++g) {
        p[g] = g < F ? __expf(p[g] - mx) : 0.f;
        l += p[g];
    }
    const float inv = 1.f / l;
    half_t* op = out + (((long)b * F + f) * N + n) * C + h * (D8 * 8);
#pragma unroll 1
    for (int c = 0; c < D8; ++c) {
        float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int g = 0; g < 32; ++g) {
            if (g < F) {
                const h8 v8 = *reinterpret_cast<const h8*>(base + g * fs + 2 * C + c * 8);
#pragma unroll
                for (int e = 0; e < 8; ++e) o[e] += p[g] * (float)v8[e];
            }
        }
        h8 r;
#pragma unroll
        for (int e = 0; e < 8; ++e) r[e] = (half_t)(o[e] * inv);
        *reinterpret_cast<h8*>(op + c * 8) = r;
    }
}

// the decoder attn1 layers that carry the PnP forward: [up block][attention] (pnp_utils.py:104-111)
const int kPnpLayers[4][3] = {{0, 0, 0}, {0, 1, 1}, {1, 1, 1}, {1, 1, 1}};

}  // namespace

// ------------------------------------------------------------------------------------------ handle
bool UNet::pnp_window_active(bool animatediff, const univst_pnp* pnp) {
    if (!pnp || !pnp->registered) return false;
    // AnimateDiff's closure (pnp_utils.py:45 of that backbone): eta1 * 50 <= idx < eta2 * 50, evaluated in double as Python does
    return animatediff ? (double)pnp->idx >= (double)pnp->eta1 * 50.0 && (double)pnp->idx < (double)pnp->eta2 * 50.0
                       : pnp->idx >= pnp->eta1 && pnp->idx <= pnp->eta2 * 50.f;
}

std::vector<long> UNet::style_bank_layout(int H, int Wd) const {
    std::vector<long> off;
    long at = 0;
    for (int i = 1; i < 4; ++i)                                    // up_blocks.i runs on level 3 - i
        for (int j = 0; j < cfg.layers_per_block + 1 && j < 3; ++j) {
            if (!kPnpLayers[i][j]) continue;
            off.push_back(at);
            const long N = (long)(H >> (3 - i)) * (Wd >> (3 - i));
            at += (N * 2 * cfg.block_out_channels[3 - i] * (long)sizeof(half_t) + 255) & ~255L;
        }
    off.push_back(at);
    return off;
}

int UNet::static_style_check(const char* entry) const {
    const char* why = animatediff ? "the AnimateDiff UNet: the motion modules' position encoding makes identical frames differ"
                      : !temporal_conv_active.empty() || !temporal_attn_active.empty()
                          ? "a checkpoint with trained temporal layers: they couple the frames, so a repeated style frame does not give identical frames"
                      : world > 1 || native_comm ? "a handle with a communicator attached: the halo phase of a frame shard shifts against the style's hidden rows"
                                                 : nullptr;
    if (why) {
        uv_set_error("%s: the static style is not available on %s", entry, why);
        return UV_ERR_UNSUPPORTED;
    }
    UV_REQUIRE(finalized, "%s: call univst_unet_finalize after loading weights", entry);
    return UV_OK;
}

UNet::~UNet() {
    for (auto& kv : idx_tables) (void)hipFree(kv.second);
    if (d_counter) (void)hipFree(d_counter);
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (xstream) (void)hipStreamDestroy(xstream);
    if (emu_flag) (void)hipFree(emu_flag);
}

int UNet::comm_streams() {
    if (xstream) return UV_OK;
    int lo = 0, hi = 0;                         // (numerically lowest = greatest priority): the exchange's few kernels go ahead of the queued compute
    UV_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    UV_HIP(hipStreamCreateWithPriority(&xstream, hipStreamNonBlocking, hi));
    UV_HIP(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
    UV_HIP(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    return UV_OK;
}

int UNet::load_tensor(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s) {
    if (animatediff && key) {      // "<block>.motion_modules.<j>.<the module's own key>" goes to that module's store
        const std::string k(key);
        const size_t pos = k.find(".motion_modules.");
        if (pos != std::string::npos) {
            const size_t dot = k.find('.', pos + strlen(".motion_modules."));
            auto it = dot == std::string::npos ? motions.end() : motions.find(k.substr(0, dot));
            UV_REQUIRE(it != motions.end(), "unet_load_tensor: key %s: the config of this handle (motion_levels_mask / motion_mid_block) has no such motion module", key);
            finalized = false;
            return it->second->load_tensor(key + dot + 1, dev_ptr, dtype, shape, ndim, s);
        }
    }
    return Model::load_tensor(key, dev_ptr, dtype, shape, ndim, s);
}

int UNet::finalize(hipStream_t s) {
    clear_derived();
    std::vector<std::string> keys;
    for (auto& kv : weights) keys.push_back(kv.first);
    // one counter per temporal UNIT (a conv's temporal weight + bias, a block's attn_temporal.to_out weight): non-zero = trained
    std::vector<std::pair<std::string, int>> tunits;          // (prefix, 0 conv / 1 attention)
    std::unordered_map<std::string, int> tslot;
    for (const std::string& k : keys) {
        size_t pos;
        if ((pos = k.find(".conv_temporal.")) != std::string::npos) {
            const std::string pre = k.substr(0, pos);
            if (!tslot.count(pre)) { tslot[pre] = (int)tunits.size(); tunits.push_back({pre, 0}); }
        } else if ((pos = k.find(".attn_temporal.to_out.0.weight")) != std::string::npos) {
            const std::string pre = k.substr(0, pos);
            if (!tslot.count(pre + "#a")) { tslot[pre + "#a"] = (int)tunits.size(); tunits.push_back({pre, 1}); }
        }
    }
    const size_t ncnt = tunits.size() + 1;
    if (d_counter) (void)hipFree(d_counter);
    d_counter = nullptr;
    UV_HIP(hipMalloc(&d_counter, ncnt * sizeof(unsigned)));
    UV_HIP(hipMemsetAsync(d_counter, 0, ncnt * sizeof(unsigned), s));
    temporal_conv_active.clear();
    temporal_attn_active.clear();
    auto ends = [](const std::string& a, const char* suf) {
        size_t n = strlen(suf);
        return a.size() >= n && a.compare(a.size() - n, n, suf) == 0;
    };
    auto level_of = [](const std::string& a) {      // resolution level (0 = finest) of a state-dict key
        int i = 0;
        if (sscanf(a.c_str(), "down_blocks.%d.", &i) == 1) return i;
        if (sscanf(a.c_str(), "up_blocks.%d.", &i) == 1) return 3 - i;
        return 3;                                    // mid_block
    };
    for (const std::string& k : keys) {
        const WTensor& t = weights[k];
        if (k.find("conv_temporal.weight") != std::string::npos) {
            UV_REQUIRE(t.shape.size() == 3 && t.shape[0] == t.shape[1] && t.shape[2] == 3, "%s: expected a [C,C,3] Conv1d weight", k.c_str());
            long n = t.shape[0] * t.shape[1] * t.shape[2];
            hipLaunchKernelGGL(count_not_dirac_slot_kernel, dim3(nb(n)), dim3(256), 0, s, t.ptr, (int)t.shape[0], (int)t.shape[1],
                               (int)t.shape[2], d_counter + tslot[k.substr(0, k.find(".conv_temporal."))]);
        } else if (k.find("conv_temporal.bias") != std::string::npos) {
            long n = t.shape[0];
            hipLaunchKernelGGL(count_nonzero_kernel, dim3(nb(n)), dim3(256), 0, s, t.ptr, n, d_counter + tslot[k.substr(0, k.find(".conv_temporal."))]);
        } else if (ends(k, "attn_temporal.to_out.0.weight")) {
            long n = 1;
            for (long v : t.shape) n *= v;
            hipLaunchKernelGGL(count_nonzero_kernel, dim3(nb(n)), dim3(256), 0, s, t.ptr, n,
                               d_counter + tslot[k.substr(0, k.find(".attn_temporal.to_out.0.weight")) + "#a"]);
        } else if (t.shape.size() == 4 && k.find("_temporal") == std::string::npos) {
            // conv weights -> [Co][taps][CiP] (+ the tap-inner copy)
            int Co = (int)t.shape[0], Ci = (int)t.shape[1], taps = (int)(t.shape[2] * t.shape[3]);
            UV_REQUIRE(taps == 1 || taps == 9, "%s: only 1x1 / 3x3 convs are supported", k.c_str());
            UV_RUN(uv_derive_conv_layouts(*this, k, s));
            if (taps == 9 && Ci % 64 == 0 && Co % 320 == 0 && k.find("downsamplers") == std::string::npos) {      // LDS-patch copy (GemmParams::W32; stride-1 convs)
                half_t* d3;
                UV_RUN(derive(k + "#t32", {Co, Ci / 32, 9, 32}, &d3));
                hipLaunchKernelGGL(permute_conv_weight_t32_kernel, dim3(nb((long)Co * Ci * 9)), dim3(256), 0, s, t.ptr, d3, Co, Ci);
                if (k.find("upsamplers") != std::string::npos) {      // phase copy (GemmParams::W4): the conv over the nearest-x2 upsampled input as four 2x2-tap convs
                    half_t* d4;
                    UV_RUN(derive(k + "#ph4", {4, Co, Ci / 32, 4, 32}, &d4));
                    UV_RUN(uv_launch_conv_up2_phase_weights(t.ptr, d4, Co, Ci, s));
                }
            }
        } else if (ends(k, ".attn1.to_q.weight")) {
            std::string p = k.substr(0, k.size() - strlen("to_q.weight"));
            const WTensor *tk = find(p + "to_k.weight"), *tv = find(p + "to_v.weight");
            UV_REQUIRE(tk && tv, "%s: to_k / to_v missing", p.c_str());
            long C = t.shape[0], K = t.shape[1];
            UV_RUN(derive_concat(p + "qkv#fused", {t.ptr, tk->ptr, tv->ptr}, C, K, s));
            const int hd = (int)C / cfg.attention_heads[level_of(k)];
            // second copy whose Q rows carry log2(e)/sqrt(d) (AttnParams::q_prescaled): the software-pipelined kernels (head_dim 40: SD-v1.5; 64: the
            // SD-v2.1 layout) take the scale from the weights
            if (hd == 40 || hd == 64 || hd == 80 || hd == 160)
                UV_RUN(derive_concat(p + "qkv#fused#qs", {t.ptr, tk->ptr, tv->ptr}, C, K, s, 1.4426950408889634f / sqrtf((float)hd)));
        } else if (ends(k, ".attn2.to_q.weight")) {
            const long C = t.shape[0], K = t.shape[1];
            const int hd = (int)C / cfg.attention_heads[level_of(k)];
            if (hd == 40) {
                half_t* d2;
                UV_RUN(derive(k + "#qs", {C, K}, &d2));
                UV_RUN(uv_launch_scale_f16(t.ptr, d2, C * K, 1.4426950408889634f / sqrtf((float)hd), s));
            }
        } else if (ends(k, ".attn2.to_k.weight")) {
            std::string p = k.substr(0, k.size() - strlen("to_k.weight"));
            const WTensor* tv = find(p + "to_v.weight");
            UV_REQUIRE(tv, "%s: to_v missing", p.c_str());
            UV_RUN(derive_concat(p + "kv#fused", {t.ptr, tv->ptr}, t.shape[0], t.shape[1], s));
        } else if (ends(k, ".ff.net.0.proj.weight") || ends(k, ".ff.net.0.proj.bias")) {
            int rows = (int)t.shape[0], cols = t.shape.size() > 1 ? (int)t.shape[1] : 1;
            UV_REQUIRE(rows % 32 == 0, "%s: GEGLU width %d must be a multiple of 32", k.c_str(), rows);
            half_t* d;
            UV_RUN(derive(k + "#geglu", {rows, cols}, &d));
            UV_RUN(uv_launch_geglu_interleave(t.ptr, d, rows, cols, s));
            // K = 320 (the 64x64 level): a second copy in the row order of the X-resident kernel (gemm.hip geglu_xres_kernel)
            int kdim = cols;
            if (!ends(k, ".weight")) {      // the bias: the reduction length is its weight's (a checkpoint that carries the bias without the weight is refused)
                const WTensor* wt = find(k.substr(0, k.size() - strlen("bias")) + "weight");
                UV_REQUIRE(wt && wt->shape.size() == 2, "%s: the projection's weight is missing", k.c_str());
                kdim = (int)wt->shape[1];
            }
            if (uv_geglu_xres_ok(rows, kdim)) {
                half_t* dx;
                UV_RUN(derive(k + "#xres", {rows, cols}, &dx));
                UV_RUN(uv_launch_geglu_xres_permute(t.ptr, dx, rows, cols, s));
            }
        }
    }
    // LayerNorm-folded copies of the three linears that follow norm1 / norm2 / norm3 of every transformer block
    for (const std::string& k : keys) {
        if (!ends(k, ".transformer_blocks.0.norm1.weight")) continue;
        const std::string b = k.substr(0, k.size() - strlen(".norm1.weight"));
        struct FoldJob { const char* norm; std::string w; std::string bias; };
        std::vector<FoldJob> jobs = {
            {".norm1", b + (find(b + ".attn1.qkv#fused#qs") ? ".attn1.qkv#fused#qs" : ".attn1.qkv#fused"), ""},
            {".norm2", b + (find(b + ".attn2.to_q.weight#qs") ? ".attn2.to_q.weight#qs" : ".attn2.to_q.weight"), ""},
            {".norm3", b + ".ff.net.0.proj.weight#geglu", b + ".ff.net.0.proj.bias#geglu"}};
        if (find(b + ".ff.net.0.proj.weight#xres")) jobs.push_back({".norm3", b + ".ff.net.0.proj.weight#xres", b + ".ff.net.0.proj.bias#xres"});
        for (auto& j : jobs) {
            const WTensor *w = find(j.w), *gm = find(b + j.norm + ".weight"), *bt = find(b + j.norm + ".bias");
            const WTensor* bi = j.bias.empty() ? nullptr : find(j.bias);
            UV_REQUIRE(w && gm && bt && (j.bias.empty() || bi) && w->shape.size() == 2 && gm->shape[0] == w->shape[1],
                       "%s: LayerNorm / linear pair incomplete", (b + j.norm).c_str());
            const long N = w->shape[0], K = w->shape[1];
            half_t *wo, *ws, *lb;
            int rc = derive(j.w + "#ln", {N, K}, &wo);
            if (!rc) rc = derive(j.w + "#ln.wsum", {2 * N}, &ws);      // fp32 [N]
            if (!rc) rc = derive(j.w + "#ln.bias", {2 * N}, &lb);      // fp32 [N]
            if (rc) return rc;
            hipLaunchKernelGGL(ln_fold_weight_kernel, dim3((unsigned)N), dim3(64), 0, s, w->ptr, gm->ptr, bt->ptr, bi ? bi->ptr : nullptr, wo,
                               (float*)ws, (float*)lb, (int)K);
        }
    }
    // the fused text cross-attention (fused.hip, the 64x64 level of SD-v1.x): to_q (plain and LayerNorm-folded) and to_out in MFMA operand order
    for (const std::string& k : keys) {
        if (!ends(k, ".attn2.to_out.0.weight")) continue;
        const std::string b = k.substr(0, k.size() - strlen(".attn2.to_out.0.weight"));
        const WTensor& t = weights[k];
        if (t.shape.size() != 2 || t.shape[0] != t.shape[1] || !uv_attn2_fused_ok((int)t.shape[0], cfg.attention_heads[level_of(k)], 64, 77)) continue;
        const std::string wq = b + (find(b + ".attn2.to_q.weight#qs") ? ".attn2.to_q.weight#qs" : ".attn2.to_q.weight");
        for (const std::string& src : {k, wq, wq + "#ln", b + ".attn1.to_out.0.weight"}) {
            const WTensor* w = find(src);
            if (!w) continue;
            half_t* d;
            UV_RUN(derive(src + "#frag", {w->shape[0], w->shape[1]}, &d));
            UV_RUN(uv_launch_frag_pack(w->ptr, d, (int)w->shape[0], (int)w->shape[1], s));
        }
    }
    {   // all resnets' time_emb_proj stacked into one [sum Cout, 4*C0] matrix: one projection launch per forward instead of 22
        std::vector<std::string> tk;
        for (const std::string& k : keys)
            if (ends(k, ".time_emb_proj.weight")) tk.push_back(k);
        std::sort(tk.begin(), tk.end());
        temb_off.clear();
        temb_total = 0;
        for (const std::string& k : tk) {
            temb_off[k.substr(0, k.size() - strlen(".time_emb_proj.weight"))] = temb_total;
            temb_total += weights[k].shape[0];
        }
        if (!tk.empty()) {
            const long K = weights[tk[0]].shape[1];
            half_t *wa, *ba;
            UV_RUN(derive("time_emb_proj#all.weight", {temb_total, K}, &wa));
            UV_RUN(derive("time_emb_proj#all.bias", {temb_total}, &ba));
            for (const std::string& k : tk) {
                const std::string pre = k.substr(0, k.size() - strlen(".time_emb_proj.weight"));
                const WTensor& wt = weights[k];
                const WTensor* bt = find(pre + ".time_emb_proj.bias");
                UV_REQUIRE(bt && wt.shape[1] == K, "%s: time_emb_proj bias missing or width mismatch", pre.c_str());
                UV_HIP(hipMemcpyAsync(wa + temb_off[pre] * K, wt.ptr, wt.shape[0] * K * sizeof(half_t), hipMemcpyDeviceToDevice, s));
                UV_HIP(hipMemcpyAsync(ba + temb_off[pre], bt->ptr, wt.shape[0] * sizeof(half_t), hipMemcpyDeviceToDevice, s));
            }
        }
    }
    UV_LAUNCH_CHECK();
    std::vector<unsigned> hc(ncnt, 0);
    UV_HIP(hipMemcpyAsync(hc.data(), d_counter, ncnt * sizeof(unsigned), hipMemcpyDeviceToHost, s));
    UV_HIP(hipStreamSynchronize(s));
    // trained temporal layers: derived layouts for the units that need them (resnet.py:70-80, attention.py:336-346)
    for (size_t i = 0; i < tunits.size(); ++i) {
        if (!hc[i]) continue;
        const std::string& pre = tunits[i].first;
        if (tunits[i].second == 0) {
            const WTensor* w = find(pre + ".conv_temporal.weight");
            UV_REQUIRE(w && find(pre + ".conv_temporal.bias"), "%s: conv_temporal weight / bias incomplete", pre.c_str());
            const int C = (int)w->shape[0];
            if (C % 8 == 0) {
                half_t* d;
                UV_RUN(derive(pre + ".conv_temporal.weight#t3x3", {C, 9, C}, &d));
                hipLaunchKernelGGL(embed_temporal_weight_kernel, dim3(nb((long)C * 9 * C)), dim3(256), 0, s, w->ptr, d, C);
            }
            temporal_conv_active[pre] = 1;
        } else {
            const WTensor *tq = find(pre + ".attn_temporal.to_q.weight"), *tk = find(pre + ".attn_temporal.to_k.weight"),
                          *tv = find(pre + ".attn_temporal.to_v.weight");
            UV_REQUIRE(tq && tk && tv && find(pre + ".norm_temporal.weight") && find(pre + ".norm_temporal.bias") &&
                       find(pre + ".attn_temporal.to_out.0.bias"), "%s: attn_temporal / norm_temporal parameters incomplete", pre.c_str());
            UV_RUN(derive_concat(pre + ".attn_temporal.qkv#fused", {tq->ptr, tk->ptr, tv->ptr}, tq->shape[0], tq->shape[1], s));
            temporal_attn_active[pre] = 1;
        }
    }
    // proj_out folded into ff.net.2 (kcat_fold; Fwd::transformer): nothing non-linear lies between the two, so
    //   Wp (W2 mid + b2 + tb + h3) + bp = [Wp W2 | Wp] [mid | h3] + (Wp (b2 + tb) + bp)
    // is ONE GEMM with K = 5C over the row [mid | h3].  Product and bias are accumulated in fp32 from the fp16 weights and rounded to fp16 once (the
    // bias too: the 128-wide kernel and the split-K reduction, which run the deep levels, have no fp32 bias).  Keys as Fwd::conv looks them up.
    // Derived whatever kcat_fold says (the option may change after finalize), but not for a block with a trained temporal attention, which never takes
    // the fold.  Cost: C x 5C fp16 per block beside the retained ff.net.2 / proj_out weights — 124 MB for the 16 blocks of SD-v1.5.
    for (const std::string& k : keys) {
        if (!ends(k, ".transformer_blocks.0.ff.net.2.weight")) continue;
        const std::string b = k.substr(0, k.size() - strlen(".ff.net.2.weight")), p = b.substr(0, b.size() - strlen(".transformer_blocks.0"));
        const WTensor *w2 = find(k), *wp = find(p + ".proj_out.weight#nhwc");
        if (!wp) wp = find(p + ".proj_out.weight");
        const WTensor *b2 = find(b + ".ff.net.2.bias"), *tb = find(b + ".attn_temporal.to_out.0.bias"), *bp = find(p + ".proj_out.bias");
        if (temporal_attn_active.count(b) || !wp || !b2 || (!tb && !animatediff) || !bp || w2->shape.size() != 2) continue;            // (the graph reports what is missing; the AnimateDiff block has no attn_temporal)
        const long C = w2->shape[0], K2 = w2->shape[1];
        long nwp = 1;
        for (long v : wp->shape) nwp *= v;
        if (wp->shape[0] != C || nwp != C * C || C % 8 != 0 || K2 != 4 * C || b2->shape[0] != C || (tb && tb->shape[0] != C) || bp->shape[0] != C) continue;
        half_t *wo, *bo;
        UV_RUN(derive(p + ".proj_out#kcat.weight#nhwc", {C, 1, K2 + C}, &wo));
        UV_RUN(derive(p + ".proj_out#kcat.bias", {C}, &bo));
        UV_RUN(uv_launch_linear_compose(wp->ptr, w2->ptr, b2->ptr, tb ? tb->ptr : nullptr, bp->ptr, (int)C, (int)K2, wo, bo, s));
    }
    UV_LAUNCH_CHECK();
    UV_HIP(hipStreamSynchronize(s));
    // the motion modules: derived layouts of each, and which of them do anything — a proj_out (weight and bias) that is still all zeros
    // (zero_initialize: no motion checkpoint loaded) makes the module proj_out(h) + x = x, and the graph skips it exactly
    motion_active.clear();
    if (!motions.empty()) {
        std::vector<std::string> mk;
        for (auto& kv : motions)
            if (!kv.second->weights.empty()) mk.push_back(kv.first);      // (a module none of whose tensors was loaded: as if zero-initialised)
        unsigned* dc = nullptr;
        UV_HIP(hipMalloc(&dc, (mk.size() + 1) * sizeof(unsigned)));
        int rc = hipMemsetAsync(dc, 0, (mk.size() + 1) * sizeof(unsigned), s) == hipSuccess ? UV_OK : UV_ERR_HIP;
        for (size_t i = 0; i < mk.size() && !rc; ++i) {
            Motion& m = *motions[mk[i]];
            rc = m.finalize(s);
            if (rc) break;
            for (const char* nm : {"temporal_transformer.proj_out.weight", "temporal_transformer.proj_out.bias"}) {
                const WTensor* t = m.find(nm);
                long n = 1;
                for (long v : t->shape) n *= v;
                hipLaunchKernelGGL(count_nonzero_kernel, dim3(nb(n)), dim3(256), 0, s, t->ptr, n, dc + i);
            }
        }
        std::vector<unsigned> hm(mk.size() + 1, 0);
        if (!rc && hipMemcpyAsync(hm.data(), dc, hm.size() * sizeof(unsigned), hipMemcpyDeviceToHost, s) != hipSuccess) rc = UV_ERR_HIP;
        if (!rc && hipStreamSynchronize(s) != hipSuccess) rc = UV_ERR_HIP;
        (void)hipFree(dc);
        if (rc == UV_ERR_HIP) uv_set_error("unet_finalize: a HIP call failed while inspecting the motion modules");
        if (rc) return rc;
        for (size_t i = 0; i < mk.size(); ++i)
            if (hm[i]) motion_active[mk[i]] = 1;
    }
    finalized = true;
    return UV_OK;
}

int UNet::reserve(int B, int F, int H, int Wd) {
    const long rows0 = (long)B * F * H * Wd;
    // activations (28 level-0-sized tensors at the high-water mark of the graph) + the small workspaces + split-K partials + the pool of the
    // producers' GroupNorm statistics (Fwd::gst_pool: rows0 / 16 fragments x 32 sub-group slots x 64 tensors x (sum, sumsq) fp32 = 1 KB per row)
    size_t need = (size_t)rows0 * cfg.block_out_channels[0] * 2 * 28 + (64u << 20) + UV_SPLITK_WS_BYTES + (gn_producer ? (size_t)rows0 * 1024 : 0);
    // a motion chain holds 9 level-sized tensors (x0, x1, h, the 4C-wide q|k|v / hidden buffer, the output, its input) where a transformer block's peak is 8
    if (animatediff) need += (size_t)rows0 * cfg.block_out_channels[0] * 2 * 4;
    UV_RUN(arena.ensure(need));
    // K/V source tables for this (B,F)
    long key = ((long)B << 20) | F | ((long)rank << 40) | ((long)world << 50);
    if (!idx_tables.count(key)) {
        std::vector<int> t;
        // frame shard: ranks > 0 find the previous frame of their first local frame and the clip's frame 0 in the
        // extra K/V frames appended after the B*F local ones ([B prev | B first], filled by Fwd::kv_exchange)
        const bool ext = world > 1 && rank > 0;
        auto prev = [&](int b, int f) { return f > 0 ? b * F + f - 1 : (ext ? B * F + b : b * F); };
        auto first = [&](int b) { return ext ? B * F + B + b : b * F; };
        // Duplicate sources are merged: at f = 0 the reference's key set is {0,0,0} (stock) / {0,0} (PnP), at f = 1 it is
        // {0,1,0} / {0,0}.  Softmax over a key set that contains frame X m times equals reading X once with log2(m) added
        // to its scores, so the table keeps unique sources + (count, log2 multiplicity) — exact, 6 % fewer key tiles.
        std::vector<int> cnt;
        std::vector<float> lw;
        auto emit = [&](std::vector<int> srcs, int width) {
            std::vector<int> uniq;
            std::vector<int> mult;
            for (int sidx : srcs) {
                size_t j = 0;
                for (; j < uniq.size(); ++j)
                    if (uniq[j] == sidx) break;
                if (j == uniq.size()) { uniq.push_back(sidx); mult.push_back(1); }
                else mult[j]++;
            }
            cnt.push_back((int)uniq.size());
            for (int j = 0; j < width; ++j) {
                t.push_back(j < (int)uniq.size() ? uniq[j] : uniq[0]);
                lw.push_back(j < (int)uniq.size() ? log2f((float)mult[j]) : 0.f);
            }
        };
        // Round 6, ranks > 0 of a frame shard: the key set of every query is split into the frames this rank HOLDS (phase 1, runs while the halo frames
        // are on the wire) and the two halo frames (phase 2, continues from phase 1's softmax state): the primary tables carry the local sources — a
        // frame may have none: PnP at f = 0 — and a second block [idx stock 3BF | idx pnp 2BF | cnt stock BF | cnt pnp BF] behind them the halo ones
        // (never duplicates: prev and first are different row blocks even where they are the same global frame).
        auto emit_split = [&](std::vector<int> local, std::vector<int> halo, int width, std::vector<int>& t2, std::vector<int>& cnt2, int self) {
            cnt.push_back((int)local.size());
            for (int j = 0; j < width; ++j) {
                t.push_back(j < (int)local.size() ? local[j] : self);
                lw.push_back(0.f);
            }
            cnt2.push_back((int)halo.size());
            for (int j = 0; j < width; ++j) t2.push_back(j < (int)halo.size() ? halo[j] : self);
        };
        std::vector<int> t2s, t2p, c2s, c2p;
        for (int b = 0; b < B; ++b)
            for (int f = 0; f < F; ++f) {                                             // stock: [-1, 0, 'first'] (attention.py:356)
                if (!ext) emit({prev(b, f), b * F + f, first(b)}, 3);
                else if (f == 0) emit_split({b * F + f}, {prev(b, f), first(b)}, 3, t2s, c2s, b * F + f);
                else emit_split({prev(b, f), b * F + f}, {first(b)}, 3, t2s, c2s, b * F + f);
            }
        for (int b = 0; b < B; ++b)
            for (int f = 0; f < F; ++f) {                                             // PnP: [-1, 'first'] (pnp_utils.py:25)
                if (!ext) emit({prev(b, f), first(b)}, 2);
                else if (f == 0) emit_split({}, {prev(b, f), first(b)}, 2, t2p, c2p, b * F + f);
                else emit_split({prev(b, f)}, {first(b)}, 2, t2p, c2p, b * F + f);
            }
        for (int b = 0; b < B; ++b)
            for (int f = 0; f < F; ++f) t.push_back(b);   // text: one [77, C] block per branch
        // layout of the device table: [idx stock 3BF | idx pnp 2BF | idx text BF | cnt stock BF | cnt pnp BF | logw stock 3BF | logw pnp 2BF]
        // (+ on ranks > 0 of a shard: [idx stock2 3BF | idx pnp2 2BF | cnt stock2 BF | cnt pnp2 BF])
        for (int v : cnt) t.push_back(v);
        for (float v : lw) {
            int bits;
            memcpy(&bits, &v, 4);
            t.push_back(bits);
        }
        for (auto* v : {&t2s, &t2p, &c2s, &c2p})
            for (int x : *v) t.push_back(x);
        if (animatediff)                              // (never sharded: this block sits at 13 BF) attn1 of the per-frame UNet: one key source, the frame itself
            for (int i = 0; i < B * F; ++i) t.push_back(i);
        int* d;
        UV_HIP(hipMalloc(&d, t.size() * sizeof(int)));
        UV_HIP(hipMemcpy(d, t.data(), t.size() * sizeof(int), hipMemcpyHostToDevice));
        idx_tables[key] = d;
    }
    return UV_OK;
}

// ------------------------------------------------------------------------------------------ forward
// the optional arguments of Fwd::conv / Fwd::linear, set by name
struct ConvOpt {
    int stride = 1, up = 0;
    const half_t* rowbias = nullptr;      // the time-embedding row bias, ldrb halfs apart (0: Cout)
    long ldrb = 0;
    const half_t* R = nullptr;            // residual [rows, Cout]
    bool want_gst = false;                // let the epilogue leave the GroupNorm statistics of the output (Act::gst) for a following GroupNorm
};
struct LinOpt {
    const half_t* R = nullptr;            // residual rows, ldr halfs apart
    long ldr = 0;
    const half_t* bias2 = nullptr;        // GemmParams::bias2
    int geglu = 0;
    float* stats_out = nullptr;           // emit the per-row (sum, sumsq) of Y for a following folded LayerNorm
    const float* ln_in = nullptr;         // fold LayerNorm(X) (statistics in ln_in, K / 160 slots per row) into this linear: `wkey` names the "#ln" weight, whose bias comes with it
    const float** gst_out = nullptr;      // where to leave the GroupNorm statistics of Y when the epilogue wrote them (else null)
    // the weight in place of W(wkey) — with rows_per_set: per-frame weight sets + fp32 bias (a GroupNorm folded into this linear: uv_launch_groupnorm's fold)
    const half_t* wsets = nullptr;
    const float* bias32 = nullptr;
    int rows_per_set = 0;
};
// One spatial transformer block (attention.py:104-153 + :280-346, + pnp_utils.py:20-100 when pnp_layer) runs as a sequence of stages over this
// context: the names, the shapes, the decisions `decide` takes once from shapes and options, and the buffers that live across stages.  The arena is
// first-fit, so WHERE a stage takes and releases a buffer is part of the graph (the high-water mark depends on it): no scope-bound guards.
struct Block {
    std::string p, b;                  // "<block>.attentions.<j>" and its ".transformer_blocks.0"
    const Act* x = nullptr;            // the block's input: proj_in reads it, proj_out adds it
    int C = 0, d = 0, N = 0, heads = 0, nbands = 1;
    long rows = 0;
    float scale_log2e = 0.f, beta = 0.f;
    bool gnf = false, fold = false, fold3 = false, qs = false, qs2 = false, registered = false, shift = false, kcat = false, a2pre = false,
         a2fused = false, t_attn = false;
    std::string wpi, wqkv, wq2, pkc;   // proj_in / attn1 q|k|v / attn2 to_q weights as the decisions picked them; the composed K = 5C operand
    half_t *t0 = nullptr, *h = nullptr, *h2 = nullptr, *h3 = nullptr, *h4 = nullptr, *kv = nullptr, *q2 = nullptr, *mid = nullptr;
    float* lnst = nullptr;             // [rows][C/160][2] fp32: row statistics for the folded LayerNorms
    half_t *gm2 = nullptr, *bt2 = nullptr, *gm3 = nullptr, *bt3 = nullptr, *tb = nullptr;      // norm2 / norm3, the bias-only temporal attention
};
struct Band {      // one band of whole frames of the row-local chain (the whole tensor when nbands == 1)
    int bd, imgs;
    long rows, o;  // rows of the band; offset of its first row in a C-wide tensor (halfs)
    float* lb;     // its rows of Block::lnst
};

struct Fwd {
    UNet& u;
    hipStream_t s;
    int B, F, text_len;
    const univst_pnp* pnp;
    half_t* emb = nullptr;     // [B, 4*C0]
    const half_t* text = nullptr;
    const int *idx_stock = nullptr, *idx_pnp = nullptr, *idx_text = nullptr, *cnt_stock = nullptr, *cnt_pnp = nullptr;
    const float *lw_stock = nullptr, *lw_pnp = nullptr;
    const int *idx2_stock = nullptr, *idx2_pnp = nullptr, *cnt2_stock = nullptr, *cnt2_pnp = nullptr;   // halo phase (ranks > 0 of a frame shard)
    const int* idx_self = nullptr;     // AnimateDiff: the identity table (frame i reads the keys of frame i)
    float* gn_ws = nullptr;
    float* mgn_ws = nullptr;           // AnimateDiff: GroupNorm partials of the motion modules (their own group count)
    float* sk_ws = nullptr;        // split-K fp32 partials (UV_SPLITK_WS_BYTES)
    half_t* temb_all = nullptr;    // [B, temb_total]: every resnet's time_emb_proj(SiLU(emb)), one launch per forward
    float* ad_ws = nullptr;
    float* gst_pool = nullptr;     // bump region for the producers' GroupNorm statistics (never reused inside a forward)
    size_t gst_left = 0;           // floats
    // static style (UNet::StyleBank): the bank of this call, its layers' byte offsets, the next PnP layer, and "the last layer has left its rows"
    const UNet::StyleBank* sb = nullptr;
    std::vector<long> sb_off;
    size_t sb_layer = 0;
    bool sb_done = false;

    float* gst_take(long rows, int C) {   // [C/10][rows/16][2] floats, or null (pool exhausted / switched off: the consumer runs its own pass)
        const size_t n = (size_t)(rows / 16) * (C / 10) * 2;
        if (!u.gn_producer || !gst_pool || rows % 16 != 0 || C % 10 != 0 || n > gst_left) return nullptr;
        float* p = gst_pool;
        gst_pool += n;
        gst_left -= n;
        return p;
    }
    void gst_give_back(long rows, int C) {
        const size_t n = (size_t)(rows / 16) * (C / 10) * 2;
        gst_pool -= n;
        gst_left += n;
    }

    half_t* alloc(long elems) {
        half_t* p = (half_t*)u.arena.alloc((size_t)elems * sizeof(half_t));
        if (!p) uv_set_error("unet: activation arena exhausted (%zu bytes); call univst_unet_reserve with the right geometry", u.arena.size);
        return p;
    }
    void free(void* p) { u.arena.release(p); }
    half_t* W(const std::string& k) { return u.W(k); }

    // the K/V source tables of this (B, F) (layout: UNet::reserve) and the workspaces every forward holds from its start to its end
    int workspaces(const int* tab, int H, int Wd) {
        const long BF_ = (long)B * F;
        idx_stock = tab; idx_pnp = tab + BF_ * 3; idx_text = tab + BF_ * 5;
        cnt_stock = tab + BF_ * 6; cnt_pnp = tab + BF_ * 7;
        lw_stock = (const float*)(tab + BF_ * 8); lw_pnp = (const float*)(tab + BF_ * 11);
        if (u.world > 1 && u.rank > 0) {
            idx2_stock = tab + BF_ * 13; idx2_pnp = tab + BF_ * 16;
            cnt2_stock = tab + BF_ * 18; cnt2_pnp = tab + BF_ * 19;
        }
        gn_ws = (float*)u.arena.alloc((size_t)uv_groupnorm_workspace_floats(B * F, u.cfg.norm_num_groups) * sizeof(float));
        ad_ws = (float*)u.arena.alloc((size_t)F * 2 * u.cfg.block_out_channels[3] * 2 * sizeof(float) + 1024);
        sk_ws = (float*)u.arena.alloc(UV_SPLITK_WS_BYTES);
        UV_REQUIRE(gn_ws && ad_ws && sk_ws, "forward: arena too small");
        if (u.animatediff) {
            idx_self = tab + BF_ * 13;
            if (!u.motions.empty()) {       // (without modules the motion config is not validated and not used)
                mgn_ws = (float*)u.arena.alloc((size_t)uv_groupnorm_workspace_floats(B * F, u.ad.motion.norm_groups) * sizeof(float) + 256);
                UV_REQUIRE(mgn_ws, "forward: arena too small");
            }
        }
        if (u.gn_producer) {           // statistics of up to 64 level-0-sized tensors: [rows/16][G][2] fp32 each (3 MB per tensor at 3 x 16 x 64 x 64: 201 MB, counted in
                                       // reserve()); taken AFTER the mandatory workspaces, so it is the part that degrades first (consumers fall back to their own pass)
            gst_left = (size_t)(((long)B * F * H * Wd + 15) / 16) * u.cfg.norm_num_groups * 2 * 64;
            gst_pool = (float*)u.arena.alloc(gst_left * sizeof(float));
            if (!gst_pool) gst_left = 0;
        }
        return UV_OK;
    }
    // time embedding (unet_3d_condition.py:359-365): emb, and every resnet's time_emb_proj of it in one launch (resnet.py:349-351)
    int time_embedding(float timestep) {
        const int C0 = u.cfg.block_out_channels[0], TED = 4 * C0;
        half_t* tsin = alloc((long)B * C0);
        half_t* e1 = alloc((long)B * TED);
        emb = alloc((long)B * TED);
        if (!tsin || !e1 || !emb) return UV_ERR_STATE;
        UV_RUN(uv_launch_timestep_embed(timestep, tsin, B, C0, u.cfg.flip_sin_to_cos, u.cfg.freq_shift, s));
        half_t *w1 = W("time_embedding.linear_1.weight"), *b1 = W("time_embedding.linear_1.bias");
        half_t *w2 = W("time_embedding.linear_2.weight"), *b2 = W("time_embedding.linear_2.bias");
        if (!w1 || !b1 || !w2 || !b2) return u.missing_error("unet");
        UV_RUN(uv_launch_linear_small(tsin, w1, b1, e1, B, TED, C0, 0, s));
        UV_RUN(uv_launch_linear_small(e1, w2, b2, emb, B, TED, TED, 1, s));
        if (u.temb_total == 0) return UV_OK;
        half_t *wa = W("time_emb_proj#all.weight"), *ba = W("time_emb_proj#all.bias");
        temb_all = alloc((long)B * u.temb_total);
        if (!wa || !ba || !temb_all) return u.missing_error("unet");
        return uv_launch_linear_small(emb, wa, ba, temb_all, B, (int)u.temb_total, TED, 1, s);
    }

    int groupnorm(const Act& a, const Act* b, int rows_per_stat, float eps, const std::string& p, int silu, half_t* out,
                  bool cross_frame = false, const UvGnFold* fold = nullptr) {
        UvGnComm gc;
        const bool sharded = cross_frame && u.world > 1;
        if (sharded) {             // 5-D GroupNorm statistics span all frames of a branch => sum the partials over ranks
            gc.world = u.world;
            gc.red = (float*)u.comm_ws;
            gc.byte_off = 0;
            gc.allreduce = u.allreduce;
            gc.user = u.comm_user;
        }
        half_t *gm = W(p + ".weight"), *bt = W(p + ".bias");
        if (!gm || !bt) return u.missing_error("unet");      // (the kernels read both unconditionally)
        return uv_launch_groupnorm(a.p, b ? b->p : nullptr, a.C, b ? b->C : 0, a.rows(), rows_per_stat, u.cfg.norm_num_groups,
                                   eps, gm, bt, silu, out, gn_ws, s, sharded ? &gc : nullptr,
                                   rows_per_stat % 16 == 0 ? a.gst : nullptr, b ? b->gst : nullptr, fold);
    }
    // launches g on the split-K workspace of the graph.  gst: let the epilogue leave the GroupNorm statistics of Y there ([N/10][M/16][2], from the pool) —
    // null when the pool is exhausted or the launch took a kernel that does not write them (the consumer then runs its own pass)
    int gemm(GemmParams& g, int mode, const float** gst = nullptr) {
        int emitted = 0;
        if (gst) *gst = nullptr;
        if (gst && (g.gn_out = gst_take(g.M, g.N))) {
            g.gn_G = g.N / 10;           // sub-groups of 10 channels: every group width of the UNet (10 .. 80) is a multiple
            g.gn_gw = 10;
            g.gn_emitted = &emitted;
        }
        g.partial = sk_ws; g.partial_bytes = UV_SPLITK_WS_BYTES;
        UV_RUN(uv_launch_gemm(g, mode, s));
        if (g.gn_out && emitted) *gst = g.gn_out;
        else if (g.gn_out) gst_give_back(g.M, g.N);
        return UV_OK;
    }
    int conv(const Act& a, const Act* b, const std::string& p, int Cout, int taps, Act* out, const ConvOpt& o = ConvOpt()) {
        GemmParams g = conv_params(a, b, taps, o.stride, o.up);
        g.N = Cout;
        g.korder = (taps == 9 && g.C1 % 64 == 0 && g.C2 % 64 == 0 && u.find(p + ".weight#ti")) ? 1 : 0;
        g.W = W(p + (g.korder ? ".weight#ti" : ".weight#nhwc"));
        if (taps == 9 && o.stride == 1 && u.find(p + ".weight#t32")) g.W32 = W(p + ".weight#t32");
        if (taps == 9 && o.stride == 1 && o.up == 1 && !b && u.find(p + ".weight#ph4")) g.W4 = W(p + ".weight#ph4");      // the plan takes it or keeps the 9-tap form
        g.bias = W(p + ".bias");
        g.rowbias = o.rowbias; g.ldrb = o.ldrb; g.rows_per_rb = F * g.Ho * g.Wo;
        g.R = o.R; g.ldr = Cout;
        out->imgs = a.imgs; out->H = g.Ho; out->W = g.Wo; out->C = Cout; out->gst = nullptr;
        if (!(out->p = alloc(out->rows() * Cout))) return UV_ERR_STATE;
        g.Y = out->p; g.ldy = Cout;
        if (!g.W || !g.bias) return u.missing_error("unet");
        if (taps != 9 || !u.temporal_conv_active.count(p)) return gemm(g, 1, o.want_gst ? &out->gst : nullptr);
        // TRAINED temporal conv (resnet.py:70-80): spatial conv (+ its bias) -> Conv1d over the frames of every pixel -> whatever the
        // caller wanted fused behind the PseudoConv3d (time-embedding row bias, residual).  The Conv1d runs as a 3x3 conv on the
        // geometry (image rows = frames, image columns = pixels) with zero side taps (embed_temporal_weight_kernel).
        half_t* mid = alloc(out->rows() * Cout);
        if (!mid) return UV_ERR_STATE;
        g.Y = mid; g.rowbias = nullptr; g.R = nullptr;
        UV_RUN(gemm(g, 1));
        half_t *tw = W(p + ".conv_temporal.weight"), *tb = W(p + ".conv_temporal.bias");
        if (!tw || !tb) return u.missing_error("unet");
        const long HWo = (long)g.Ho * g.Wo;
        if (Cout % 8 != 0) {
            UV_REQUIRE(!o.rowbias && !o.R, "%s: temporal conv on %d channels cannot carry a fused epilogue", p.c_str(), Cout);
            hipLaunchKernelGGL(temporal_conv_small_kernel, dim3(nb(out->rows() * Cout)), dim3(256), 0, s, mid, out->p, tw, tb, B, F, HWo, Cout);
            UV_LAUNCH_CHECK();
        } else {
            GemmParams t;
            t.X = mid; t.C1 = Cout; t.Hs = t.Ho = F; t.Ws = t.Wo = (int)HWo; t.taps = 9;
            t.M = (int)out->rows(); t.N = Cout; t.K = 9 * Cout;
            t.W = W(p + ".conv_temporal.weight#t3x3"); t.bias = tb;
            t.rowbias = o.rowbias; t.ldrb = o.ldrb; t.rows_per_rb = (int)(F * HWo);
            t.R = o.R; t.ldr = Cout;
            t.Y = out->p; t.ldy = Cout;
            if (!t.W) return u.missing_error("unet");
            UV_RUN(gemm(t, 1));
        }
        free(mid);
        return UV_OK;
    }
    int linear(const half_t* X, long ldx, long M, int K, const std::string& wkey, const std::string& bkey, int N, half_t* Y, long ldy,
               const LinOpt& o = LinOpt()) {
        const bool own_bias = !bkey.empty() && !o.ln_in && !o.wsets;
        GemmParams g = lin_params(X, M, K, o.wsets ? o.wsets : W(wkey), N, Y, own_bias ? W(bkey) : nullptr, o.R, o.geglu);
        g.ldx = ldx; g.ldy = ldy; g.ldr = o.ldr;      // (the graph's rows are not always contiguous: bands, the q|k|v rows, the GEGLU hidden tensor)
        g.bias2 = o.bias2; g.stats_out = o.stats_out;
        g.w_rows_per_set = o.wsets ? o.rows_per_set : 0; g.bias32 = o.wsets ? o.bias32 : nullptr;
        if (o.ln_in) {
            g.ln_stats = o.ln_in; g.ln_slots = K / 160; g.ln_eps = 1e-5f;
            g.ln_wsum = (const float*)W(wkey + ".wsum"); g.ln_bias = (const float*)W(wkey + ".bias");
        }
        if (!g.W || (own_bias && !g.bias) || (o.ln_in && (!g.ln_wsum || !g.ln_bias))) return u.missing_error("unet");
        return gemm(g, 0, o.gst_out);
    }

    // frame shard (SURVEY §8e coupling 2): every frame attends to {prev, (cur), first}; the previous frame of this rank's first frame lives on
    // rank-1 and frame 0 on rank 0.  Round 6: what travels is the block's HIDDEN rows of the boundary frame ([B, N, C] fp16 per pack: the input of
    // norm1 -> to_k | to_v, attention.py:311,375-377; half the bytes of the K|V pack) — the receiver projects (and, inside the PnP window, shifts:
    // the shift needs per-frame statistics only, pnp_utils.py:114-125) the two halo frames itself — and it travels on a FORKED stream as soon as
    // proj_in has written the rows, beside this rank's own q|k|v projection, AdaIN shift and the LOCAL phase of its attention:
    //   kv_post (after proj_in):  pack on s -> fork (one event) -> [xstream: multicast to the peers -> raise their flags]
    //   kv_join (after phase 1):  the wait kernel on s spins on this rank's own flags; the packs are then in the inbox slots of comm_ws
    // The streams meet through the flags only; xstream is joined back into s ONCE, at the end of the forward (UNet::forward).
    // A host-callback communicator (torch.distributed / gloo / the host-thread loopback of the tests) is driven from kv_join on s: same packs, serial.
    struct KvSlots {
        long o_send = 0, o_first = 0, o_prev = 0, o_rfirst = 0, nbytes = 0;
        bool emu = false;
    } kvs;
    int kv_post(const half_t* h, int C, int N) {
        kvs = KvSlots();
        kvs.nbytes = (long)B * N * C * sizeof(half_t);
        // host-callback communicator: 4 slots [send | first | recv prev | recv first].  Native (IPC) communicator: the two receive slots
        // are double-buffered by exchange parity (peers write them without an acknowledgement, comm.hip): 6 slots
        const int nslot = u.native_comm ? 6 : 4;
        const long slot = ((u.comm_ws_bytes - 65536) / nslot) & ~255L;
        UV_REQUIRE(kvs.nbytes <= slot, "kv_exchange: comm workspace too small (%ld B per slot, need %ld)", slot, kvs.nbytes);
        const long par = u.native_comm ? uv_comm_kv_parity(u.native_comm) : 0;
        kvs.o_send = 65536;
        kvs.o_first = kvs.o_send + slot;
        kvs.o_prev = kvs.o_first + slot * (1 + 2 * par);
        kvs.o_rfirst = kvs.o_prev + slot;
        if (u.rank < u.world - 1) UV_RUN(uv_launch_rows_pack(h, C, 0, C, N, B, F, F - 1, (half_t*)(u.comm_ws + kvs.o_send), s));
        if (u.rank == 0) UV_RUN(uv_launch_rows_pack(h, C, 0, C, N, B, F, 0, (half_t*)(u.comm_ws + kvs.o_first), s));
        kvs.emu = !u.native_comm && u.emu_wire_gbps > 0;
        if (!u.native_comm && !kvs.emu) return UV_OK;
        const bool sends = u.rank < u.world - 1 || kvs.emu;           // (the last rank posts nothing)
        hipStream_t x = s;
        if (u.kv_overlap && sends) {
            UV_RUN(u.comm_streams());
            x = u.xstream;
            UV_HIP(hipEventRecord(u.ev_fork, s));
            UV_HIP(hipStreamWaitEvent(x, u.ev_fork, 0));
            u.x_dirty = true;
        }
        if (u.native_comm) {
            UV_RUN(uv_comm_kv_post(u.native_comm, kvs.o_send, kvs.o_first, kvs.o_prev, kvs.o_rfirst, kvs.nbytes, x));
        } else {
            // the slowest transfer of this exchange on a node this box does not have: one pack per link (the first-frame pack reaches every rank over
            // its own link from rank 0, the halo pack over the link from rank - 1) except on rank 1, whose one link from rank 0 carries both.  The delay
            // kernel + a raise of this process's own flag word stand in for the peer's multicast + raise
            const double us = u.emu_wire_lat_us + (u.rank == 1 ? 2.0 : 1.0) * (double)kvs.nbytes / (u.emu_wire_gbps * 1e3);
            u.emu_wire_us += us;
            if (!u.emu_flag) {
                UV_HIP(hipMalloc((void**)&u.emu_flag, 64));
                UV_HIP(hipMemsetAsync(u.emu_flag, 0, 64, s));
                UV_HIP(hipStreamSynchronize(s));
            }
            UV_RUN(uv_launch_delay_us(us, x));
            UV_RUN(uv_comm_launch_raise(u.emu_flag, ++u.emu_epoch, x));
        }
        return UV_OK;
    }
    int kv_join() {
        if (u.native_comm) return uv_comm_kv_wait(u.native_comm, s);
        int rc = u.kv_exchange(u.comm_user, kvs.o_send, kvs.o_first, kvs.o_prev, kvs.o_rfirst, kvs.nbytes);
        if (rc) {
            uv_set_error("kv_exchange callback failed (%d)", rc);
            return UV_ERR_STATE;
        }
        if (kvs.emu && u.rank > 0) UV_RUN(uv_comm_launch_wait(u.emu_flag, u.emu_epoch, (int*)(u.emu_flag + 1), s));
        return UV_OK;
    }

    // resnet.py:335-394
    int resblock(const std::string& p, const Act& x, const Act* skip, int Cout, Act* out) {
        const int Cin = x.C + (skip ? skip->C : 0);
        const int rps = (u.animatediff && u.ad.inflated_groupnorm ? 1 : F) * x.H * x.W;      // InflatedGroupNorm (resnet.py:21-29): per frame
        half_t* n1 = alloc(x.rows() * Cin);
        if (!n1) return UV_ERR_STATE;
        UV_RUN(groupnorm(x, skip, rps, u.cfg.norm_eps, p + ".norm1", 1, n1, true));
        auto to = u.temb_off.find(p);
        UV_REQUIRE(to != u.temb_off.end() && temb_all, "%s: time_emb_proj missing", p.c_str());
        Act n1a{n1, x.imgs, x.H, x.W, Cin}, h;
        ConvOpt c1;
        c1.rowbias = temb_all + to->second; c1.ldrb = u.temb_total; c1.want_gst = true;
        UV_RUN(conv(n1a, nullptr, p + ".conv1", Cout, 9, &h, c1));
        free(n1);
        half_t* n2 = alloc(h.rows() * Cout);
        if (!n2) return UV_ERR_STATE;
        UV_RUN(groupnorm(h, nullptr, rps, u.cfg.norm_eps, p + ".norm2", 1, n2, true));
        free(h.p);
        const half_t* res = x.p;
        Act sc{};
        if (u.find(p + ".conv_shortcut.weight")) {
            UV_RUN(conv(x, skip, p + ".conv_shortcut", Cout, 1, &sc));
            res = sc.p;
        } else {
            UV_REQUIRE(!skip && x.C == Cout, "%s: no conv_shortcut but channel mismatch", p.c_str());
        }
        Act n2a{n2, x.imgs, x.H, x.W, Cout};
        ConvOpt c2;
        c2.R = res; c2.want_gst = true;
        UV_RUN(conv(n2a, nullptr, p + ".conv2", Cout, 9, out, c2));
        free(n2);
        if (sc.p) free(sc.p);
        return UV_OK;
    }

    // Everything that is a predicate on shapes and options: no launch, no allocation
    int decide(Block& k, bool pnp_layer) {
        const Act& x = *k.x;
        const int C = k.C, N = k.N, heads = k.heads;
        const long rows = k.rows;
        const std::string &p = k.p, &b = k.b;
        k.scale_log2e = 1.4426950408889634f / sqrtf((float)k.d);
        // The block's per-frame GroupNorm (attention.py:121) folded into proj_in where that pays (round 5): per frame a weight set gamma * rstd (.) W and
        // an fp32 bias carrying the mean term, proj_in then reads the RAW tensor — the apply pass (read + write of the tensor) goes for B*F weight copies
        // (9.8 MB against 252 MB at the 64x64 level; at the 32x32 level the copies are a third of the pass: not taken)
        k.wpi = p + (u.find(p + ".proj_in.weight#nhwc") ? ".proj_in.weight#nhwc" : ".proj_in.weight");
        const long set_bytes = (long)x.imgs * C * C * 2, apply_bytes = rows * C * 4;
        k.gnf = u.gn_fold && uv_linear_takes_big_direct(rows, C, C) && (N % 256 == 0 || N % 192 == 0) && 8 * set_bytes <= apply_bytes;
        // The three LayerNorms of the block are folded into the linears around them when all of those take the direct 256x320 path
        // (levels with >= 150 tiles: the 64x64 .. 16x16 levels of an unsharded clip): the producing linear's epilogue leaves the row
        // statistics, the consuming one runs on the raw rows — no LayerNorm launch, no normalised copy in HBM.
        // norm3 -> GEGLU projection is folded only on request (ln_fold = 2): its epilogue is the longest of the block and the fold
        // costs it more than the LayerNorm launch it removes (tools/bench_ln_fold.py).
        // (round 4: also on the 128-wide kernel where that runs these linears without split-K — the 64x64 / 32x32 levels of a frame shard)
        k.fold = u.ln_fold > 0 && C % 160 == 0 && uv_linear_fold_producer_ok(rows, C, C) && uv_linear_fold_consumer_ok(rows, 3 * C, C, false) &&
                 uv_linear_fold_consumer_ok(rows, C, C, false);
        // norm3 is folded also with the statistics from a 128-wide producer (A/B: emulated rank of 8, F = 16: 12.83 ms per step
        // without the 128-wide fold, 12.81 with norm1 / norm2 only, 12.70 with all three)
        const bool xres3 = u.find(b + ".ff.net.0.proj.weight#xres") != nullptr && uv_geglu_xres_ok(8 * C, C, rows);
        k.fold3 = k.fold && u.ln_fold > 1 && (xres3 || uv_linear_fold_consumer_ok(rows, 8 * C, C, true));
        k.qs = u.find(b + ".attn1.qkv#fused#qs") != nullptr;      // head_dim 40: scale folded into to_q (finalize)
        k.wqkv = b + (k.qs ? ".attn1.qkv#fused#qs" : ".attn1.qkv#fused");
        k.qs2 = u.find(b + ".attn2.to_q.weight#qs") != nullptr;
        k.wq2 = b + (k.qs2 ? ".attn2.to_q.weight#qs" : ".attn2.to_q.weight");
        k.registered = pnp_layer && pnp && pnp->registered;
        // (the one-frame style call never shifts: the reference only ever modifies chunk 2, pnp_utils.py:53-57)
        k.shift = k.registered && UNet::pnp_window_active(u.animatediff, pnp) && !(sb && sb->mode == UNet::StyleBank::WRITE);
        if (k.shift) {
            UV_REQUIRE(B == 3 || (sb && B == 2), "PnP attention shift needs the three-branch batch (B=3), got B=%d", B);
            k.beta = (0.9f - 0.1f) / (pnp->eta1 * 50.f - pnp->eta2 * 50.f) * ((float)pnp->idx - pnp->eta2 * 50.f) + 0.1f;
        }
        // The row-local chain behind the self-attention: to_out + residual -> (norm2) -> attn2 -> to_out + residual -> (norm3) ->
        // GEGLU projection -> FF2 + residual.  Round 4: it runs BAND BY BAND over whole frames when the level is large (64x64 level of
        // an unsharded clip: 196 608 rows, every C-wide tensor 126 MB, the 4C-wide hidden one 503 MB): with bands of 65 536 rows (one
        // round of 256-row tiles on the 256 CUs) the band's intermediates (42 MB each, hidden 168 MB) are re-read by the next kernel of
        // the chain while they are still in the 256 MB Infinity Cache instead of streaming from HBM, and the hidden buffer is
        // band-sized (tools/bench_mall_bands.py: -13 % on the four FF linears; every kernel is row-local: same results up to fp32 summation order).
        // OFF by default: inside the step (same box, alternating runs) the banded graph is 0.4 ms SLOWER (linears 16.7 -> 17.0 ms: three
        // one-round launches per kernel lose more to launch tails than the cache returns).  Kept as a switch (chain_bands).
        k.nbands = 1;
        if (u.chain_bands != 1) {
            const long target = 65536;
            int want = u.chain_bands > 1 ? u.chain_bands : (int)(rows / target);
            while (want > 1 && (x.imgs % want != 0 || (u.chain_bands <= 1 && rows / want < target))) --want;
            k.nbands = want < 1 ? 1 : want;
            // the folded LayerNorms need the direct 256x320 path for the band's row count as well: a level too small for that stays unbanded
            if (k.nbands > 1 && k.fold &&
                !(uv_linear_takes_big_direct(rows / k.nbands, C, C) && (!k.fold3 || uv_linear_takes_big_direct(rows / k.nbands, 8 * C, C))))
                k.nbands = 1;
        }
        k.t_attn = u.temporal_attn_active.count(b) != 0;
        // proj_out as extra K columns of ff.net.2 (kcat_fold; weights composed at finalize): ONE GEMM with K = 5C over the row [mid | h3] — residual = the
        // block's input, GroupNorm statistics as proj_out leaves them — replaces ff.net.2 + residual and proj_out + residual: one launch and the round trip
        // of h4 less per block.  The two halves of the row stay the two buffers they are (a 1x1 conv over the channel concat [mid | h3], as conv_shortcut
        // runs over [x | skip]): a contiguous 5C-wide buffer needs 5 units of the first-fit arena in one piece where this graph needs 4 + 1, and
        // raised its high-water mark.  Not with a trained temporal attention (it sits between the two linears) and not with a banded chain.
        k.pkc = p + ".proj_out#kcat";
        k.kcat = (u.kcat_fold & 1) && !k.t_attn && k.nbands == 1 && C % 8 == 0 && u.find(k.pkc + ".weight#nhwc") && u.find(k.pkc + ".bias") &&
                 rows * 16 * C < (1L << 31);           // (the conv kernels' 32-bit offsets into the wider source)
        // The text cross-attention as ONE launch where the shape allows (round 5, fused.hip): q projection (LayerNorm folded), the 77-key attention of the
        // wave's two heads and the out projection + residual share one 64-row tile in LDS — Q and O never reach HBM.  Unbanded chains only.
        const bool a2ok = k.nbands == 1 && u.attn2_fused && uv_attn2_fused_ok(C, heads, F * N, text_len) && u.find(b + ".attn2.to_out.0.weight#frag");
        k.a2fused = a2ok && u.find(k.wq2 + (k.fold ? "#ln#frag" : "#frag"));
        // round 5, second step: the self-attention's out projection rides in FRONT of the fused text cross-attention (fused.hip, PRE): h2 = to_out(attn1) + h
        // is that kernel's input and residual and nothing else reads it, so it stays in the block's LDS
        k.a2pre = k.a2fused && k.fold && u.attn2_fused > 1 && u.find(b + ".attn1.to_out.0.weight#frag");
        return UV_OK;
    }
    // The block's GroupNorm, or its fold into proj_in: h (and the row statistics of h when the LayerNorms are folded)
    int proj_in(Block& k) {
        const Act& x = *k.x;
        const int C = k.C;
        if (!(k.t0 = alloc(k.rows * C))) return UV_ERR_STATE;
        LinOpt lo;
        half_t* wsets = nullptr;
        float* b32 = nullptr;
        if (k.gnf) {
            wsets = alloc((long)x.imgs * C * C);
            b32 = (float*)alloc((long)x.imgs * C * 2);
            if (!wsets || !b32) return UV_ERR_STATE;
            UvGnFold gf;
            gf.W = W(k.wpi); gf.bias = W(k.p + ".proj_in.bias"); gf.N = C; gf.W_out = wsets; gf.bias32 = b32;
            if (!gf.W || !gf.bias) return u.missing_error("unet");
            UV_RUN(groupnorm(x, nullptr, k.N, 1e-6f, k.p + ".norm", 0, nullptr, false, &gf));
            lo.wsets = wsets; lo.bias32 = b32; lo.rows_per_set = k.N;
        } else {
            UV_RUN(groupnorm(x, nullptr, k.N, 1e-6f, k.p + ".norm", 0, k.t0));
        }
        if (!(k.h = alloc(k.rows * C))) return UV_ERR_STATE;
        if (k.fold && !(k.lnst = (float*)alloc(k.rows * (C / 160) * 4))) return UV_ERR_STATE;
        lo.stats_out = k.lnst;
        UV_RUN(linear(k.gnf ? x.p : k.t0, C, k.rows, C, k.wpi, k.p + ".proj_in.bias", C, k.h, C, lo));
        free(wsets);      // (null without the fold: release ignores it)
        free(b32);
        return UV_OK;
    }
    // norm1, q|k|v, the AdaIN shift and the self-attention (into t0).  Frame shard: the boundary frames' hidden rows leave right behind norm1 (kv_post), the
    // attention runs over the key frames this rank holds while they travel, and on ranks > 0 a second phase over the two halo frames follows (attn1_halo)
    int attn1(Block& k) {
        const int C = k.C, N = k.N;
        const long rows = k.rows;
        half_t *gm = W(k.b + ".norm1.weight"), *bt = W(k.b + ".norm1.bias");
        if (!gm || !bt) return u.missing_error("unet");
        if (!k.fold) UV_RUN(uv_launch_layernorm(k.h, C, k.t0, C, gm, bt, rows, C, 1e-5f, s));
        const bool shard = u.world > 1, halo = shard && u.rank > 0;
        if (shard) UV_RUN(kv_post(k.h, C, N));                  // the boundary frames' hidden rows leave now, on the forked stream
        const long extra_rows = shard ? (long)2 * B * N : 0;     // the halo frames' q|k|v rows behind the local ones: [prev: B x N | first: B x N]
        half_t* qkv = alloc((rows + extra_rows) * 3 * C);
        if (!qkv) return UV_ERR_STATE;
        LinOpt lq;
        lq.ln_in = k.lnst;      // (set when `fold`: the linear then reads the raw rows)
        UV_RUN(linear(k.fold ? k.h : k.t0, C, rows, C, k.fold ? k.wqkv + "#ln" : k.wqkv, "", 3 * C, qkv, 3 * C, lq));
        if (k.registered && sb) {      // static style: this layer's K | V rows of the one style frame go to the bank, or the shift reads them from there
            UV_REQUIRE(sb_layer + 1 < sb_off.size(), "static style: more PnP layers in the graph than the bank's layout has");
            half_t* slot = (half_t*)(sb->base + sb_off[sb_layer++]);
            if (sb->mode == UNet::StyleBank::WRITE) {
                UV_HIP(hipMemcpy2DAsync(slot, 2L * C * sizeof(half_t), qkv + C, 3L * C * sizeof(half_t), 2L * C * sizeof(half_t), (size_t)N,
                                        hipMemcpyDeviceToDevice, s));
                if (sb_layer + 1 == sb_off.size()) {      // nothing behind the last PnP layer's projection is wanted (the style's eps is discarded)
                    sb_done = true;
                    return UV_OK;
                }
            } else if (k.shift) {
                UV_RUN(uv_launch_adain_shift_static(qkv, 3 * C, slot, 2 * C, F, N, C, ad_ws, ad_ws + 2L * C, pnp->alpha, k.beta, pnp->gamma, s));
            }
        } else if (k.shift) {
            UV_RUN(uv_launch_adain_shift(qkv, 3 * C, F, N, C, ad_ws, ad_ws + (long)F * 2 * C, pnp->alpha, k.beta, pnp->gamma, s));
        }
        AttnParams ap;
        ap.q = qkv; ap.k = qkv + C; ap.v = qkv + 2 * C;
        ap.ldq = ap.ldkv = 3 * C;
        ap.o = k.t0; ap.ldo = C;
        if (u.animatediff) {      // plain per-frame self-attention (attention.py:344: no video_length, no key frames), registered or not
            ap.src_idx = idx_self;
            ap.nsrc = 1;
        } else {
            ap.src_idx = k.registered ? idx_pnp : idx_stock;
            ap.src_cnt = k.registered ? cnt_pnp : cnt_stock;
            ap.src_logw = k.registered ? lw_pnp : lw_stock;
            ap.nsrc = k.registered ? 2 : 3;
        }
        ap.BF = k.x->imgs; ap.Nq = N; ap.Nkv = N; ap.heads = k.heads; ap.d = k.d;
        ap.scale_log2e = k.scale_log2e;
        ap.q_prescaled = k.qs;
        float* state = nullptr;
        if (halo) {               // phase 1: the key frames this rank holds; (m, l) per query stays behind for phase 2
            state = (float*)alloc((long)k.x->imgs * k.heads * N * 4);
            if (!state) return UV_ERR_STATE;
            ap.state_out = state;
        }
        UV_RUN(uv_launch_attention(ap, s));
        if (shard) UV_RUN(kv_join());
        if (halo) UV_RUN(attn1_halo(k, ap, qkv, gm, bt, state));
        free(qkv);
        return UV_OK;
    }
    // the two halo frames: LayerNorm (norm1) of the received hidden rows -> to_k | to_v (all of q|k|v inside the window: the shift kernel works on
    // the fused rows) -> the AdaIN shift of each frame -> phase 2 over them.  The sender would have computed the same K | V from the same fp16 rows
    // (with the LayerNorm folded into the GEMM when `fold`: equal up to fp16 rounding of the normalised rows).
    int attn1_halo(Block& k, AttnParams& ap, half_t* qkv, const half_t* gm, const half_t* bt, float* state) {
        const int C = k.C, N = k.N;
        const long hrows = 2L * B * N;
        half_t* tn = alloc(hrows * C);
        if (!tn) return UV_ERR_STATE;
        UV_RUN(uv_launch_layernorm((const half_t*)(u.comm_ws + kvs.o_prev), C, tn, C, gm, bt, (long)B * N, C, 1e-5f, s));
        UV_RUN(uv_launch_layernorm((const half_t*)(u.comm_ws + kvs.o_rfirst), C, tn + (long)B * N * C, C, gm, bt, (long)B * N, C, 1e-5f, s));
        half_t* qh = qkv + k.rows * 3 * C;
        half_t* wfull = W(k.wqkv);
        if (!wfull) return u.missing_error("unet");
        if (k.shift) {
            UV_RUN(linear(tn, C, hrows, C, k.wqkv, "", 3 * C, qh, 3 * C));
            for (int sl = 0; sl < 2; ++sl)            // rows [slot][3 branches][N] = the shift kernel's [3][F = 1][N]
                UV_RUN(uv_launch_adain_shift(qh + (long)sl * B * N * 3 * C, 3 * C, 1, N, C, ad_ws, ad_ws + 2L * C, pnp->alpha, k.beta, pnp->gamma, s));
        } else {
            LinOpt kv_only;
            kv_only.wsets = wfull + (long)C * C;      // the to_k | to_v rows of the fused weight
            UV_RUN(linear(tn, C, hrows, C, k.wqkv, "", 2 * C, qh + C, 3 * C, kv_only));
        }
        free(tn);
        ap.src_idx = k.registered ? idx2_pnp : idx2_stock;
        ap.src_cnt = k.registered ? cnt2_pnp : cnt2_stock;
        ap.src_logw = nullptr;
        ap.state_out = nullptr;
        ap.state_in = state;
        UV_RUN(uv_launch_attention(ap, s));
        free(state);
        return UV_OK;
    }
    // Opens the row-local chain: its first buffers, the norms it reads, and the text K | V of the cross-attention (one projection for all bands).
    // (buffers are taken when first needed and, with ONE band, released as soon as the chain is past them — the arena's
    // high-water mark of the unbanded graph is unchanged; with bands the full-height tensors live until the last band, the band-sized
    // q2 / hidden buffers are reused by every band)
    int chain_begin(Block& k) {
        const int C = k.C;
        k.h2 = alloc(k.rows * C);
        k.kv = alloc((long)B * text_len * 2 * C);
        if (!k.h2 || !k.kv) return UV_ERR_STATE;
        k.gm2 = W(k.b + ".norm2.weight"); k.bt2 = W(k.b + ".norm2.bias"); k.gm3 = W(k.b + ".norm3.weight"); k.bt3 = W(k.b + ".norm3.bias");
        k.tb = u.animatediff ? nullptr : W(k.b + ".attn_temporal.to_out.0.bias");      // (the AnimateDiff block has no attn_temp)
        if (!k.gm2 || !k.bt2 || !k.gm3 || !k.bt3 || (!k.tb && !u.animatediff)) return u.missing_error("unet");
        return linear(text, u.cfg.cross_attention_dim, (long)B * text_len, u.cfg.cross_attention_dim, k.b + ".attn2.kv#fused", "", 2 * C, k.kv, 2 * C);
    }
    // attn1's out projection + residual, norm2 and the text cross-attention + residual: h3.  Three forms (decide): the fused launch with the out
    // projection in front, the fused launch behind a separate out projection, and q projection + attention + out projection
    int attn2(Block& k, const Band& r) {
        if (k.a2pre) return attn2_fused(k, r);
        LinOpt lo;
        lo.R = k.h + r.o; lo.ldr = k.C; lo.stats_out = r.lb;
        UV_RUN(linear(k.t0 + r.o, k.C, r.rows, k.C, k.b + ".attn1.to_out.0.weight", k.b + ".attn1.to_out.0.bias", k.C, k.h2 + r.o, k.C, lo));
        if (k.nbands == 1) free(k.h);
        return k.a2fused ? attn2_fused(k, r) : attn2_unfused(k, r);
    }
    int attn2_fused(Block& k, const Band& r) {      // (nbands == 1: the band is the tensor)
        const int C = k.C;
        half_t* kvf = alloc(uv_attn2_kvf_halfs(B, k.heads, k.d));
        if (!kvf || !(k.h3 = alloc(k.rows * C))) return UV_ERR_STATE;
        UV_RUN(uv_launch_kv_frag_pack(k.kv, kvf, B, text_len, C, k.heads, s));
        if (!k.fold) UV_RUN(uv_launch_layernorm(k.h2, C, k.t0, C, k.gm2, k.bt2, k.rows, C, 1e-5f, s));
        Attn2Params a2;
        a2.ldx = C; a2.M = (int)k.rows;
        a2.Wq_f = W(k.wq2 + (k.fold ? "#ln#frag" : "#frag")); a2.kvf = kvf;
        a2.rows_per_branch = F * k.N; a2.heads = k.heads; a2.Nkv = text_len;
        a2.q_prescaled = k.qs2; a2.scale_log2e = k.scale_log2e;
        a2.Wo_f = W(k.b + ".attn2.to_out.0.weight#frag"); a2.bias_o = W(k.b + ".attn2.to_out.0.bias");
        a2.Y = k.h3; a2.ldy = C;
        a2.stats_out = k.fold3 ? r.lb : nullptr;
        if (k.fold) {
            a2.ln_slots = C / 160; a2.ln_eps = 1e-5f;
            a2.ln_wsum = (const float*)W(k.wq2 + "#ln.wsum"); a2.ln_bias = (const float*)W(k.wq2 + "#ln.bias");
        }
        if (k.a2pre) {            // X = the self-attention's output; h2 = to_out(X) + h is formed (and its statistics taken) inside
            a2.X = k.t0;
            a2.Wp_f = W(k.b + ".attn1.to_out.0.weight#frag"); a2.bias_p = W(k.b + ".attn1.to_out.0.bias"); a2.Rp = k.h; a2.ldrp = C;
        } else {
            a2.X = k.fold ? k.h2 : k.t0;
            a2.ln_stats = k.fold ? r.lb : nullptr;
            a2.R = k.h2; a2.ldr = C;
        }
        if (!a2.bias_o || (k.fold && (!a2.ln_wsum || !a2.ln_bias)) || (k.a2pre && !a2.bias_p)) return u.missing_error("unet");
        UV_RUN(uv_launch_attn2_fused(a2, C, s));
        free(kvf);
        free(k.kv);
        if (k.a2pre) free(k.h);
        free(k.h2);
        return UV_OK;
    }
    int attn2_unfused(Block& k, const Band& r) {
        const int C = k.C;
        if (!k.q2 && !(k.q2 = alloc(r.rows * C))) return UV_ERR_STATE;
        if (!k.fold) UV_RUN(uv_launch_layernorm(k.h2 + r.o, C, k.t0 + r.o, C, k.gm2, k.bt2, r.rows, C, 1e-5f, s));
        LinOpt lq;
        lq.ln_in = r.lb;
        UV_RUN(linear((k.fold ? k.h2 : k.t0) + r.o, C, r.rows, C, k.fold ? k.wq2 + "#ln" : k.wq2, "", C, k.q2, C, lq));
        AttnParams ap;
        ap.q = k.q2; ap.ldq = C;
        ap.k = k.kv; ap.v = k.kv + C; ap.ldkv = 2 * C;
        ap.o = k.t0 + r.o; ap.ldo = C;
        ap.src_idx = idx_text + r.bd * r.imgs; ap.nsrc = 1;
        ap.BF = r.imgs; ap.Nq = k.N; ap.Nkv = text_len; ap.heads = k.heads; ap.d = k.d;
        ap.scale_log2e = k.scale_log2e;
        ap.q_prescaled = k.qs2;
        UV_RUN(uv_launch_attention(ap, s));
        if (k.nbands == 1) { free(k.q2); free(k.kv); }
        if (!k.h3 && !(k.h3 = alloc(k.rows * C))) return UV_ERR_STATE;
        LinOpt lo;
        lo.R = k.h2 + r.o; lo.ldr = C; lo.stats_out = k.fold3 ? r.lb : nullptr;
        UV_RUN(linear(k.t0 + r.o, C, r.rows, C, k.b + ".attn2.to_out.0.weight", k.b + ".attn2.to_out.0.bias", C, k.h3 + r.o, C, lo));
        if (k.nbands == 1) free(k.h2);
        return UV_OK;
    }
    // GEGLU feed-forward (+ the bias-only temporal attention, attention.py:233): norm3 / GEGLU projection into mid, then ff.net.2 + residual into h4 —
    // unless ff.net.2 runs inside the K = 5C GEMM behind the chain (kcat)
    int ff(Block& k, const Band& r) {
        const int C = k.C;
        if (!k.mid && !(k.mid = alloc(r.rows * 4 * C))) return UV_ERR_STATE;
        // (K = 320: the X-resident kernel and its weight order, any row count)
        const bool xres = u.find(k.b + ".ff.net.0.proj.weight#xres") != nullptr && uv_geglu_xres_ok(8 * C, C, r.rows);
        const std::string wff = k.b + (xres ? ".ff.net.0.proj.weight#xres" : ".ff.net.0.proj.weight#geglu");
        const std::string bff = k.b + (xres ? ".ff.net.0.proj.bias#xres" : ".ff.net.0.proj.bias#geglu");
        if (!k.fold3) UV_RUN(uv_launch_layernorm(k.h3 + r.o, C, k.t0 + r.o, C, k.gm3, k.bt3, r.rows, C, 1e-5f, s));
        LinOpt l1;
        l1.geglu = xres ? 2 : 1; l1.ln_in = k.fold3 ? r.lb : nullptr;
        UV_RUN(linear((k.fold3 ? k.h3 : k.t0) + r.o, C, r.rows, C, k.fold3 ? wff + "#ln" : wff, bff, 8 * C, k.mid, 4 * C, l1));
        if (k.nbands == 1 && k.lnst) free(k.lnst);
        if (k.kcat) return UV_OK;
        if (!k.h4 && !(k.h4 = alloc(k.rows * C))) return UV_ERR_STATE;
        LinOpt l2;
        l2.R = k.h3 + r.o; l2.ldr = C; l2.bias2 = k.t_attn ? nullptr : k.tb;
        return linear(k.mid, 4 * C, r.rows, 4 * C, k.b + ".ff.net.2.weight", k.b + ".ff.net.2.bias", C, k.h4 + r.o, C, l2);
    }

    // TRAINED temporal attention (attention.py:336-346): LayerNorm, q|k|v, softmax over the F frames of every pixel, to_out + residual: a new h4
    int temporal_attn(Block& k) {
        const int C = k.C, N = k.N, heads = k.heads;
        const long rows = k.rows;
        UV_REQUIRE(F <= 32, "temporal attention: clips of %d frames (kernel holds <= 32 scores per query)", F);
        half_t *gm = W(k.b + ".norm_temporal.weight"), *bt = W(k.b + ".norm_temporal.bias");
        if (!gm || !bt) return u.missing_error("unet");
        UV_RUN(uv_launch_layernorm(k.h4, C, k.t0, C, gm, bt, rows, C, 1e-5f, s));
        half_t *qkvt = alloc(rows * 3 * C), *t0 = k.t0;
        if (!qkvt) return UV_ERR_STATE;
        UV_RUN(linear(t0, C, rows, C, k.b + ".attn_temporal.qkv#fused", "", 3 * C, qkvt, 3 * C));
        const long nthr = (long)B * N * heads * F;
        const float sc = 1.f / sqrtf((float)k.d);
#define TA_CASE(D8) case 8 * D8: hipLaunchKernelGGL((temporal_attn_kernel<D8>), dim3(nb(nthr)), dim3(256), 0, s, qkvt, t0, B, F, N, C, heads, sc); break;
        switch (k.d) {
            TA_CASE(1) TA_CASE(2) TA_CASE(4) TA_CASE(5) TA_CASE(8) TA_CASE(10) TA_CASE(20)
            default: uv_set_error("temporal attention: head_dim=%d not instantiated", k.d); return UV_ERR_UNSUPPORTED;
        }
#undef TA_CASE
        UV_LAUNCH_CHECK();
        free(qkvt);
        half_t* h5 = alloc(rows * C);
        if (!h5) return UV_ERR_STATE;
        LinOpt lo;
        lo.R = k.h4; lo.ldr = C;
        UV_RUN(linear(t0, C, rows, C, k.b + ".attn_temporal.to_out.0.weight", k.b + ".attn_temporal.to_out.0.bias", C, h5, C, lo));
        free(k.h4);
        k.h4 = h5;
        return UV_OK;
    }

    // proj_out + the block's input, leaving the GroupNorm statistics of the result for the next resnet — as a plain linear over h4, or (kcat) with
    // ff.net.2 in front of it as one K = 5C GEMM over [mid | h3]
    int proj_out(Block& k, Act* out) {
        const Act& x = *k.x;
        free(k.t0);
        if (k.kcat) {
            Act am{k.mid, x.imgs, x.H, x.W, 4 * k.C}, a3{k.h3, x.imgs, x.H, x.W, k.C};
            ConvOpt co;
            co.R = x.p; co.want_gst = true;
            UV_RUN(conv(am, &a3, k.pkc, k.C, 1, out, co));
            free(k.mid);
            free(k.h3);
            return UV_OK;
        }
        out->imgs = x.imgs; out->H = x.H; out->W = x.W; out->C = k.C;
        if (!(out->p = alloc(k.rows * k.C))) return UV_ERR_STATE;
        LinOpt lo;
        lo.R = x.p; lo.ldr = k.C; lo.gst_out = &out->gst;
        UV_RUN(linear(k.h4, k.C, k.rows, k.C, k.p + (u.find(k.p + ".proj_out.weight#nhwc") ? ".proj_out.weight#nhwc" : ".proj_out.weight"), k.p + ".proj_out.bias",
                      k.C, out->p, k.C, lo));
        free(k.h4);
        return UV_OK;
    }

    int transformer(const std::string& p, const Act& x, bool pnp_layer, int heads, Act* out) {
        Block k;
        k.p = p; k.b = p + ".transformer_blocks.0"; k.x = &x;
        k.C = x.C; k.heads = heads; k.d = x.C / heads; k.N = x.H * x.W; k.rows = x.rows();
        UV_RUN(decide(k, pnp_layer));
        UV_RUN(proj_in(k));
        UV_RUN(attn1(k));
        if (sb_done) return UV_OK;      // (the style bank is complete: the call ends here, the arena is reset by the next one)
        UV_RUN(chain_begin(k));
        Band r;
        r.imgs = x.imgs / k.nbands;
        r.rows = (long)r.imgs * k.N;
        for (r.bd = 0; r.bd < k.nbands; ++r.bd) {
            r.o = r.bd * r.rows * k.C;
            r.lb = k.lnst ? k.lnst + r.bd * r.rows * (k.C / 160) * 2 : nullptr;
            UV_RUN(attn2(k, r));
            UV_RUN(ff(k, r));
        }
        if (k.nbands > 1)      // (one band released them on its way)
            for (void* q : std::initializer_list<void*>{k.h, k.q2, k.kv, k.h2, k.lnst}) free(q);
        if (!k.kcat) {
            free(k.mid);
            free(k.h3);
            if (k.t_attn) UV_RUN(temporal_attn(k));
        }
        return proj_out(k, out);
    }

    // The motion module `p` ("down_blocks.0.motion_modules.1") behind a resnet / transformer pair (unet_blocks.py:411): x becomes module(x), its old
    // buffer released.  A module whose proj_out is all zeros is the identity and is skipped.  The chain (Motion::run) takes its buffers from this
    // graph's arena for the length of the call: x0, x1, h (the attention writes its output over h), ONE 4C-wide buffer that is q|k|v during the
    // attentions and the GEGLU hidden tensor behind them, and the output.
    int motion(const std::string& p, Act* x) {
        auto it = u.motions.find(p);
        if (it == u.motions.end() || !u.motion_active.count(p)) return UV_OK;
        Motion& m = *it->second;
        const long M = x->rows();
        const int C = x->C, N = x->H * x->W;
        UV_REQUIRE(m.cfg.channels == C, "%s: the module is %d channels wide, the activation %d", p.c_str(), m.cfg.channels, C);
        UV_RUN(m.check_shape("forward", B, F, N));
        MotionBufs b;
        b.x[0] = alloc(M * C);
        b.x[1] = alloc(M * C);
        b.h = alloc(M * C);
        half_t* wide = alloc(M * 4 * C);
        half_t* y = alloc(M * C);
        if (!b.x[0] || !b.x[1] || !b.h || !wide || !y) {
            for (half_t* q : {b.x[0], b.x[1], b.h, wide, y})
                if (q) free(q);
            return UV_ERR_STATE;
        }
        b.att = b.h;
        b.qkv = b.ff = wide;
        b.gn_ws = mgn_ws;
        b.splitk = sk_ws;
        b.splitk_bytes = UV_SPLITK_WS_BYTES;
        const int rc = m.run(x->p, y, B, F, N, b, s);      // (a chain that fails half-way gives its buffers back too: the handle stays usable)
        free(b.x[0]);
        free(b.x[1]);
        free(b.h);
        free(wide);
        if (rc) {
            free(y);
            return rc;
        }
        free(x->p);
        x->p = y;
        x->gst = nullptr;
        return UV_OK;
    }
};

int UNet::forward(const half_t* sample, float timestep, const half_t* text, int B, int F, int H, int Wd, int text_len,
                  const univst_pnp* pnp, half_t* eps_out, half_t* feat_out, int ft_index, hipStream_t s, bool tap_entry, const StyleBank* bank) {
    UV_REQUIRE(finalized, "forward: call univst_unet_finalize after loading weights");
    UV_REQUIRE(world == 1 || (temporal_conv_active.empty() && temporal_attn_active.empty()),
               "forward: trained temporal layers couple all frames of a pixel; frame sharding (world=%d) is not supported with them", world);
    if (native_comm) {
        UV_RUN(uv_comm_poll(native_comm));          // a peer timed out in an earlier call: report instead of queueing more work
        uv_comm_bind_stream(native_comm, s);
    }
    UV_REQUIRE(B >= 1 && B <= 8 && F >= 1 && H >= 8 && Wd >= 8 && H % 8 == 0 && Wd % 8 == 0,
               "forward: unsupported geometry B=%d F=%d H=%d W=%d (H, W multiples of 8; B <= 8)", B, F, H, Wd);
    if (animatediff) {
        UV_REQUIRE(F <= UV_MOTION_MAX_F, "forward: F=%d frames (the AnimateDiff UNet takes at most %d: what the frame-axis attention holds)", F, UV_MOTION_MAX_F);
        UV_REQUIRE(!ad.motion.position_encoding || motions.empty() || F <= ad.motion.max_len,
                   "forward: F=%d frames exceed motion.max_len %d (the position table has max_len rows)", F, ad.motion.max_len);
        UV_REQUIRE(tap_entry || !feat_out, "forward: feat_out must be NULL: the AnimateDiff UNet has its feature tap on univst_unet_forward_tap");
        UV_REQUIRE(world == 1, "forward: the AnimateDiff UNet cannot be frame-sharded (world=%d)", world);
    }
    UV_RUN(reserve(B, F, H, Wd));
    clear_missing();
    const int* boc = cfg.block_out_channels;
    const int C0 = boc[0], L = cfg.layers_per_block;
    Fwd f{*this, s, B, F, text_len, pnp};
    f.text = text;
    if (bank) {
        f.sb = bank;
        f.sb_off = style_bank_layout(H, Wd);
    }
    UV_RUN(f.workspaces(idx_tables[((long)B << 20) | F | ((long)rank << 40) | ((long)world << 50)], H, Wd));
    UV_RUN(f.time_embedding(timestep));
    // ---- conv_in
    const int CP = (cfg.in_channels + 7) / 8 * 8;
    Act x0{f.alloc((long)B * F * H * Wd * CP), B * F, H, Wd, CP};
    if (!x0.p) return UV_ERR_STATE;
    UV_RUN(uv_launch_ncfhw_to_nhwc(sample, x0.p, B, cfg.in_channels, F, H * Wd, CP, s));
    Act x;
    ConvOpt with_gst, down2, up2;      // the three plain forms: GroupNorm statistics from the epilogue; also stride 2; also over the nearest-x2 upsampled input
    with_gst.want_gst = down2.want_gst = up2.want_gst = true;
    down2.stride = 2;
    up2.up = 1;
    UV_RUN(f.conv(x0, nullptr, "conv_in", C0, 9, &x, with_gst));
    f.free(x0.p);

    std::vector<Act> skips;
    skips.push_back(x);
    // ---- down
    for (int i = 0; i < 4; ++i) {
        const std::string p = "down_blocks." + std::to_string(i);
        const bool has_attn = i < 3;
        for (int j = 0; j < L; ++j) {
            Act y;
            UV_RUN(f.resblock(p + ".resnets." + std::to_string(j), x, nullptr, boc[i], &y));
            bool x_is_skip = false;
            for (auto& sk : skips) x_is_skip |= (sk.p == x.p);
            if (!x_is_skip) f.free(x.p);
            x = y;
            if (has_attn) {
                Act z;
                UV_RUN(f.transformer(p + ".attentions." + std::to_string(j), x, false, cfg.attention_heads[i], &z));
                f.free(x.p);
                x = z;
            }
            if (animatediff) UV_RUN(f.motion(p + ".motion_modules." + std::to_string(j), &x));
            skips.push_back(x);
        }
        if (i != 3) {
            Act y;
            UV_RUN(f.conv(x, nullptr, p + ".downsamplers.0.conv", boc[i], 9, &y, down2));
            x = y;
            skips.push_back(x);
        }
    }
    // ---- mid
    {
        Act y, z, w;
        UV_RUN(f.resblock("mid_block.resnets.0", x, nullptr, boc[3], &y));
        UV_RUN(f.transformer("mid_block.attentions.0", y, false, cfg.attention_heads[3], &z));
        f.free(y.p);
        if (animatediff) UV_RUN(f.motion("mid_block.motion_modules.0", &z));
        UV_RUN(f.resblock("mid_block.resnets.1", z, nullptr, boc[3], &w));
        f.free(z.p);
        x = w;   // previous x is skips.back(), still owned by the skip list
    }
    // ---- up
    for (int i = 0; i < 4; ++i) {
        const std::string p = "up_blocks." + std::to_string(i);
        const int Cout = boc[3 - i];
        const bool has_attn = i > 0;
        for (int j = 0; j < L + 1; ++j) {
            Act sk = skips.back();
            skips.pop_back();
            Act y;
            UV_RUN(f.resblock(p + ".resnets." + std::to_string(j), x, &sk, Cout, &y));
            f.free(x.p);
            f.free(sk.p);
            x = y;
            if (has_attn) {
                Act z;
                UV_RUN(f.transformer(p + ".attentions." + std::to_string(j), x, j < 3 && kPnpLayers[i][j], cfg.attention_heads[3 - i], &z));
                if (f.sb_done) return missing.empty() ? UV_OK : missing_error("unet");
                f.free(x.p);
                x = z;
            }
            if (animatediff) UV_RUN(f.motion(p + ".motion_modules." + std::to_string(j), &x));
        }
        if (i != 3) {
            Act y;
            UV_RUN(f.conv(x, nullptr, p + ".upsamplers.0.conv", Cout, 9, &y, up2));
            f.free(x.p);
            x = y;
        }
        if (feat_out && i == ft_index)   // sample[0].permute(1,2,3,0) == the first F*H*W NHWC rows
            UV_HIP(hipMemcpyAsync(feat_out, x.p, (size_t)F * x.H * x.W * x.C * sizeof(half_t), hipMemcpyDeviceToDevice, s));
    }
    // ---- out
    half_t* n = f.alloc(x.rows() * x.C);
    if (!n) return UV_ERR_STATE;
    UV_RUN(f.groupnorm(x, nullptr, (animatediff && ad.inflated_groupnorm ? 1 : F) * x.H * x.W, cfg.norm_eps, "conv_norm_out", 1, n, true));
    Act na{n, x.imgs, x.H, x.W, x.C}, y;
    UV_RUN(f.conv(na, nullptr, "conv_out", cfg.out_channels, 9, &y));
    UV_RUN(uv_launch_nhwc_to_ncfhw(y.p, cfg.out_channels, eps_out, B, cfg.out_channels, F, H * Wd, s));
    if (x_dirty) {                 // the forked stream's posts of this forward complete before anything the caller queues behind it (and a capture can end)
        UV_HIP(hipEventRecord(ev_join, xstream));
        UV_HIP(hipStreamWaitEvent(s, ev_join, 0));
        x_dirty = false;
    }
    if (!missing.empty()) return missing_error("unet");
    return UV_OK;
}
