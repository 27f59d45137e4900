// extern "C" surface of libunivst_hip.so (include/univst.h).  Thin argument checking + dispatch.
#include <limits.h>
#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <string.h>

#include <memory>
#include <new>
#include <string>

#include "../../include/univst.h"
#include "comm.h"
#include "kernels.h"
#include "unet.h"
#include "vae.h"
#include "raft.h"
#include "clip.h"
#include "t5.h"
#include "motion.h"

static thread_local char g_err[1024] = "";
void uv_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
const char* uv_get_error() { return g_err; }

#define H(p) ((const half_t*)(p))
#define HM(p) ((half_t*)(p))
#define S(p) ((hipStream_t)(p))

struct univst_unet {
    UNet impl;
};

// destroy / load_tensor / finalize of a handle struct univst_<name> { <Model> impl; }: the same three entries for every fp16 handle
#define UV_HANDLE_ABI(name)                                                                                                                        \
    int univst_##name##_destroy(univst_##name* h) {                                                                                                \
        delete h;                                                                                                                                  \
        return UV_OK;                                                                                                                              \
    }                                                                                                                                              \
    int univst_##name##_load_tensor(univst_##name* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* s) {        \
        UV_REQUIRE(h, "null handle");                                                                                                              \
        return h->impl.load_tensor(key, p, dtype, shape, ndim, S(s));                                                                              \
    }                                                                                                                                              \
    int univst_##name##_finalize(univst_##name* h, void* s) {                                                                                      \
        UV_REQUIRE(h, "null handle");                                                                                                              \
        return h->impl.finalize(S(s));                                                                                                             \
    }
// the read-outs every fp16 handle answers (the *_query entries try this first, then their own names)
static bool model_query(const Model& m, const char* name, double* out) {
    if (!strcmp(name, "arena_high_water")) *out = (double)m.arena.high_water;
    else if (!strcmp(name, "arena_bytes")) *out = (double)m.arena.size;      // the slab's size: changes only when a forward / reserve had to replace it by a larger one
    else if (!strcmp(name, "weight_bytes")) *out = m.weight_bytes();
    else return false;
    return true;
}

// The tuning switches of a UNet handle (include/univst.h), ONE row per option: univst_unet_create seeds the handle from `env`, univst_unet_set_option
// accepts [lo, hi] (lo > hi: a boolean, any int, stored as != 0) and refuses the rest with "<name> is <what>", univst_unet_query reads the value back.
// A seed is never refused: a boolean one is != 0, the others are clamped to [lo, seed_hi] — or (SEED_PRE) pick 2 / 1 as a boolean.  The defaults are unet.h's.
enum { SEED_PRE = -1 };
struct UNetOption {
    const char *name, *env;      // env: null = no seed
    int UNet::*member;
    int lo, hi;
    const char* what;
    int seed_hi;
};
static const UNetOption kUNetOptions[] = {
    {"ln_fold", "UNIVST_LN_FOLD", &UNet::ln_fold, 0, 2, "0, 1 or 2", 2},
    {"gn_fold", "UNIVST_GN_FOLD", &UNet::gn_fold, 1, 0, nullptr, 0},
    {"kcat_fold", "UNIVST_KCAT_FOLD", &UNet::kcat_fold, 0, 3, "0, 1 (proj_out), 2 (conv_shortcut) or 3 (both)", 3},
    {"attn2_fused", "UNIVST_ATTN2_PRE", &UNet::attn2_fused, 0, 2, "0, 1 or 2", SEED_PRE},
    {"gn_producer", "UNIVST_GN_PRODUCER", &UNet::gn_producer, 1, 0, nullptr, 0},
    {"chain_bands", "UNIVST_CHAIN_BANDS", &UNet::chain_bands, 0, 64, "0 (auto), 1 (off) or a band count <= 64", INT_MAX},      // (the seed has no upper clamp)
    {"kv_overlap", "UNIVST_KV_OVERLAP", &UNet::kv_overlap, 1, 0, nullptr, 0},
    {"emu_wire_gbps", nullptr, &UNet::emu_wire_gbps, 0, 10000, "a per-link rate in GB/s (0: off)", 0},
    {"emu_wire_lat_us", nullptr, &UNet::emu_wire_lat_us, 0, 100000, "a latency in microseconds", 0},
    {"motion_fold", nullptr, &UNet::motion_fold, 0, 1, "0 or 1", 0},      // (handles of univst_unet_create_animatediff only; 1 is not built)
};
static const UNetOption* unet_option(const char* name) {
    for (const UNetOption& o : kUNetOptions)
        if (!strcmp(name, o.name)) return &o;
    return nullptr;
}

extern "C" {

const char* univst_last_error(void) { return g_err; }
int univst_abi_version(void) { return UNIVST_ABI_VERSION; }
int univst_sd3_shift_window(int idx, double eta1, double eta2, int* active, float* beta) {
    UV_REQUIRE(active && beta, "sd3_shift_window: null argument");
    // pnp_utils.py:183-186 in double, as the reference's Python evaluates it (in fp32, 0.3f * 50 = 15.000001 and step 15 falls out of the window)
    const bool on = eta1 * 50 <= (double)idx && (double)idx <= eta2 * 50;
    *active = on ? 1 : 0;
    *beta = on ? (float)((0.9 - 0.1) / (eta1 * 50 - eta2 * 50) * ((double)idx - eta2 * 50) + 0.1) : 0.f;
    return UV_OK;
}

int univst_unet_create(const univst_unet_cfg* cfg, univst_unet** out) {
    UV_REQUIRE(cfg && out, "unet_create: null argument");
    UV_REQUIRE(cfg->norm_num_groups > 0 && cfg->layers_per_block > 0, "unet_create: bad config");
    for (int i = 0; i < 4; ++i) {
        int c = cfg->block_out_channels[i];
        const int hd = cfg->attention_heads[i];
        UV_REQUIRE(hd > 0 && c % 8 == 0 && c % cfg->norm_num_groups == 0 && c % hd == 0 && (c / hd) % 8 == 0,
                   "unet_create: block_out_channels[%d]=%d must be divisible by 8, groups and heads (head_dim multiple of 8)", i, c);
    }
    UV_REQUIRE(cfg->cross_attention_dim % 8 == 0, "unet_create: cross_attention_dim must be a multiple of 8");
    univst_unet* h = new (std::nothrow) univst_unet();
    UV_REQUIRE(h, "unet_create: out of host memory");
    h->impl.cfg = *cfg;
    for (const UNetOption& o : kUNetOptions)
        if (const char* e = o.env ? getenv(o.env) : nullptr) {
            const int v = atoi(e);
            h->impl.*o.member = o.lo > o.hi ? v != 0 : o.seed_hi == SEED_PRE ? (v ? 2 : 1) : v < o.lo ? o.lo : v > o.seed_hi ? o.seed_hi : v;
        }
    *out = h;
    return UV_OK;
}
int univst_unet_create_animatediff(const univst_unet_cfg* cfg, const univst_animatediff_cfg* ad, univst_unet** out) {
    UV_REQUIRE(cfg && ad && out, "unet_create_animatediff: null argument");
    UV_REQUIRE(ad->inflated_groupnorm == 0 || ad->inflated_groupnorm == 1, "unet_create_animatediff: inflated_groupnorm %d (0 or 1)", ad->inflated_groupnorm);
    UV_REQUIRE(ad->motion_levels_mask >= 0 && ad->motion_levels_mask <= 15, "unet_create_animatediff: motion_levels_mask %d (bits 0..3: one per level)", ad->motion_levels_mask);
    UV_REQUIRE(ad->motion_mid_block == 0 || ad->motion_mid_block == 1, "unet_create_animatediff: motion_mid_block %d (0 or 1)", ad->motion_mid_block);
    UV_REQUIRE(cfg->layers_per_block > 0 && cfg->layers_per_block <= 64, "unet_create_animatediff: layers_per_block %d", cfg->layers_per_block);
    const bool any = ad->motion_levels_mask != 0 || ad->motion_mid_block;
    if (any) {
        UV_REQUIRE(ad->motion.num_heads >= 1 && ad->motion.norm_groups >= 1, "unet_create_animatediff: motion.num_heads %d and motion.norm_groups %d must be positive",
                   ad->motion.num_heads, ad->motion.norm_groups);
        for (int l = 0; l < 4; ++l) {
            if (!((ad->motion_levels_mask >> l) & 1) && !(l == 3 && ad->motion_mid_block)) continue;
            const int c = cfg->block_out_channels[l];
            const int d = c % ad->motion.num_heads == 0 ? c / ad->motion.num_heads : 0;
            UV_REQUIRE(d == 40 || d == 80 || d == 160,
                       "unet_create_animatediff: block_out_channels[%d]=%d with motion.num_heads %d is no head dim the frame-axis attention has (40, 80, 160)", l, c,
                       ad->motion.num_heads);
            UV_REQUIRE(c % ad->motion.norm_groups == 0, "unet_create_animatediff: block_out_channels[%d]=%d is no multiple of motion.norm_groups %d", l, c,
                       ad->motion.norm_groups);
            univst_motion_cfg mc = ad->motion;
            mc.channels = c;
            UV_RUN(uv_motion_check_cfg(mc));
        }
    }
    univst_unet* h = nullptr;
    UV_RUN(univst_unet_create(cfg, &h));
    h->impl.animatediff = true;
    h->impl.ad = *ad;
    auto add = [&](const std::string& key, int width) {
        std::unique_ptr<Motion> m(new (std::nothrow) Motion());
        if (!m) return false;
        m->cfg = ad->motion;
        m->cfg.channels = width;
        h->impl.motions[key] = std::move(m);
        return true;
    };
    bool ok = true;
    for (int l = 0; l < 4 && ok; ++l) {
        if (!((ad->motion_levels_mask >> l) & 1)) continue;
        for (int j = 0; j < cfg->layers_per_block && ok; ++j) ok = add("down_blocks." + std::to_string(l) + ".motion_modules." + std::to_string(j), cfg->block_out_channels[l]);
        for (int j = 0; j <= cfg->layers_per_block && ok; ++j) ok = add("up_blocks." + std::to_string(3 - l) + ".motion_modules." + std::to_string(j), cfg->block_out_channels[l]);
    }
    if (ok && ad->motion_mid_block) ok = add("mid_block.motion_modules.0", cfg->block_out_channels[3]);
    if (!ok) {
        delete h;
        uv_set_error("unet_create_animatediff: out of host memory");
        return UV_ERR_STATE;
    }
    *out = h;
    return UV_OK;
}
int univst_unet_set_option(univst_unet* h, const char* name, int value) {
    UV_REQUIRE(h && name, "unet_set_option: null argument");
    const UNetOption* o = unet_option(name);
    if (!o) {
        uv_set_error("unet_set_option: unknown option '%s'", name);
        return UV_ERR_ARG;
    }
    const bool mf = o->member == &UNet::motion_fold;
    UV_REQUIRE(!mf || h->impl.animatediff, "unet_set_option: motion_fold belongs to a handle of univst_unet_create_animatediff");
    UV_REQUIRE(o->lo > o->hi || (value >= o->lo && value <= o->hi), "unet_set_option: %s is %s", name, o->what);
    if (mf && value == 1) {
        uv_set_error("unet_set_option: motion_fold = 1 (the motion modules' norms folded into their GEMMs) is not built; the chain runs unfolded (0)");
        return UV_ERR_UNSUPPORTED;
    }
    h->impl.*o->member = o->lo > o->hi ? value != 0 : value;
    return UV_OK;
}
int univst_unet_query(univst_unet* h, const char* name, double* out) {
    UV_REQUIRE(h && name && out, "unet_query: null argument");
    if (!strcmp(name, "emu_wire_us")) {          // modelled wire time issued since the last query (reading resets it)
        *out = h->impl.emu_wire_us;
        h->impl.emu_wire_us = 0.0;
        return UV_OK;
    }
    if (model_query(h->impl, name, out)) return UV_OK;
    if (!strcmp(name, "idx_tables")) {           // the (B, F) geometries whose K/V source tables are on the device (each uploaded once, at its first forward)
        *out = (double)h->impl.idx_tables.size();
        return UV_OK;
    }
    if (!strcmp(name, "motion_active")) {     // AnimateDiff handles: the motion modules finalize found with a non-zero proj_out
        *out = (double)h->impl.motion_active.size();
        return UV_OK;
    }
    if (const UNetOption* o = unet_option(name))      // an option's current value (motion_fold: on the handles that have it)
        if (o->member != &UNet::motion_fold || h->impl.animatediff) {
            *out = (double)(h->impl.*o->member);
            return UV_OK;
        }
    uv_set_error("unet_query: unknown quantity '%s'", name);
    return UV_ERR_ARG;
}
UV_HANDLE_ABI(unet)
int univst_unet_reserve(univst_unet* h, int B, int F, int Hh, int W) {
    UV_REQUIRE(h, "null handle");
    return h->impl.reserve(B, F, Hh, W);
}
int univst_unet_forward(univst_unet* h, const void* sample, float t, const void* text, int B, int F, int Hh, int W, int text_len,
                        const univst_pnp* pnp, void* eps, void* feat, int ft_index, void* s) {
    UV_REQUIRE(h && sample && text && eps, "unet_forward: null argument");
    return h->impl.forward(H(sample), t, H(text), B, F, Hh, W, text_len, pnp, HM(eps), HM(feat), ft_index, S(s));
}
int univst_unet_forward_tap(univst_unet* h, const void* sample, float t, const void* text, int B, int F, int Hh, int W, int text_len,
                            const univst_pnp* pnp, void* eps, void* feat, int ft_index, void* s) {
    UV_REQUIRE(h && sample && text && eps, "unet_forward_tap: null argument");
    UV_REQUIRE(feat, "unet_forward_tap: feat_out must not be NULL (univst_unet_forward is the entry without a tap)");
    UV_REQUIRE(ft_index >= 0 && ft_index <= 3, "unet_forward_tap: ft_index %d outside 0..3", ft_index);
    return h->impl.forward(H(sample), t, H(text), B, F, Hh, W, text_len, pnp, HM(eps), HM(feat), ft_index, S(s), true);
}
int64_t univst_unet_style_bank_bytes(univst_unet* h, int Hh, int W) {
    UV_REQUIRE(h && Hh >= 8 && W >= 8 && Hh % 8 == 0 && W % 8 == 0, "unet_style_bank_bytes: null handle or unsupported geometry H=%d W=%d (multiples of 8)", Hh, W);
    return h->impl.style_bank_layout(Hh, W).back();
}
int univst_unet_style_bank(univst_unet* h, const void* sample, float t, const void* text, int Hh, int W, int text_len, const univst_pnp* pnp, void* bank,
                           int64_t bank_bytes, int* active_out, void* s) {
    UV_REQUIRE(h && sample && text && active_out, "unet_style_bank: null argument");
    UV_RUN(h->impl.static_style_check("unet_style_bank"));
    UV_REQUIRE(pnp && pnp->registered, "unet_style_bank: pnp is NULL or not registered: without the PnP key sources the frame's K | V rows are not the ones the shift wants");
    UV_REQUIRE(Hh >= 8 && W >= 8 && Hh % 8 == 0 && W % 8 == 0, "unet_style_bank: unsupported geometry H=%d W=%d (multiples of 8)", Hh, W);
    *active_out = UNet::pnp_window_active(false, pnp) ? 1 : 0;
    if (!*active_out) return UV_OK;      // outside the window nothing reads the bank
    const std::vector<long> off = h->impl.style_bank_layout(Hh, W);
    UV_REQUIRE(off.size() > 1, "unet_style_bank: this configuration has no PnP layer");
    UV_REQUIRE(bank, "unet_style_bank: the PnP window is open (idx %d) and bank is NULL", pnp->idx);
    UV_REQUIRE(bank_bytes >= off.back(), "unet_style_bank: bank of %lld bytes, univst_unet_style_bank_bytes asks for %ld", (long long)bank_bytes, off.back());
    UV_REQUIRE(((uintptr_t)bank & 15) == 0, "unet_style_bank: bank must be 16-byte aligned");
    UNet::StyleBank sb;
    sb.mode = UNet::StyleBank::WRITE;
    sb.base = (char*)bank;
    return h->impl.forward(H(sample), t, H(text), 1, 1, Hh, W, text_len, pnp, nullptr, nullptr, -1, S(s), false, &sb);
}
int univst_unet_forward_static_style(univst_unet* h, const void* sample, float t, const void* text, int F, int Hh, int W, int text_len, const univst_pnp* pnp,
                                     const void* bank, int64_t bank_bytes, void* eps, void* s) {
    UV_REQUIRE(h && sample && text && eps, "unet_forward_static_style: null argument");
    UV_RUN(h->impl.static_style_check("unet_forward_static_style"));
    if (!UNet::pnp_window_active(false, pnp))      // outside the window: the ordinary two-branch forward
        return h->impl.forward(H(sample), t, H(text), 2, F, Hh, W, text_len, pnp, HM(eps), nullptr, -1, S(s));
    UV_REQUIRE(Hh >= 8 && W >= 8 && Hh % 8 == 0 && W % 8 == 0, "unet_forward_static_style: unsupported geometry H=%d W=%d (multiples of 8)", Hh, W);
    UV_REQUIRE(bank, "unet_forward_static_style: the PnP window is open (idx %d) and bank is NULL", pnp->idx);
    const long need = h->impl.style_bank_layout(Hh, W).back();
    UV_REQUIRE(bank_bytes >= need, "unet_forward_static_style: bank of %lld bytes, univst_unet_style_bank_bytes asks for %ld", (long long)bank_bytes, need);
    UV_REQUIRE(((uintptr_t)bank & 15) == 0, "unet_forward_static_style: bank must be 16-byte aligned");
    UNet::StyleBank sb;
    sb.mode = UNet::StyleBank::READ;
    sb.base = (char*)bank;
    return h->impl.forward(H(sample), t, H(text), 2, F, Hh, W, text_len, pnp, HM(eps), nullptr, -1, S(s), false, &sb);
}
int univst_unet_set_comm(univst_unet* h, int rank, int world, void* comm_ws, int64_t comm_ws_bytes, univst_allreduce_fn ar,
                         univst_kv_exchange_fn kv, void* user) {
    UV_REQUIRE(h && world >= 1 && rank >= 0 && rank < world, "set_comm: bad rank/world");
    if (h->impl.animatediff) {
        uv_set_error("set_comm: the AnimateDiff UNet cannot be frame-sharded: its frame-axis attention needs every frame on one rank");
        return UV_ERR_UNSUPPORTED;
    }
    UV_REQUIRE(world == 1 || (comm_ws && comm_ws_bytes >= (1 << 17) && ar && kv), "set_comm: world > 1 needs a workspace and both callbacks");
    h->impl.comm_ws = (char*)comm_ws;
    h->impl.comm_ws_bytes = comm_ws_bytes;
    h->impl.rank = rank;
    h->impl.world = world;
    h->impl.allreduce = ar;
    h->impl.kv_exchange = kv;
    h->impl.comm_user = user;
    h->impl.native_comm = nullptr;          // callbacks (or none, world == 1: detached) replace a library communicator
    return UV_OK;
}

int univst_unet_set_comm_native(univst_unet* h, univst_comm* comm) {
    UV_REQUIRE(h && comm, "set_comm_native: null argument");
    if (h->impl.animatediff) {
        uv_set_error("set_comm_native: the AnimateDiff UNet cannot be frame-sharded: its frame-axis attention needs every frame on one rank");
        return UV_ERR_UNSUPPORTED;
    }
    return uv_unet_attach_comm(h->impl, comm);
}

int univst_linear(const void* X, int64_t ldx, const void* W, const void* bias, const void* R, int64_t ldr, void* Y, int64_t ldy,
                  int M, int N, int K, int geglu, void* s) {
    UV_REQUIRE(X && W && Y, "linear: null argument");
    GemmParams g;
    g.X = H(X); g.ldx = ldx; g.W = H(W); g.bias = H(bias); g.R = H(R); g.ldr = ldr; g.Y = HM(Y); g.ldy = ldy;
    g.M = M; g.N = N; g.K = K; g.geglu = geglu;
    return uv_launch_gemm(g, 0, S(s));
}
int univst_linear_gated(const void* X, int64_t ldx, const void* W, const void* bias, const void* R, int64_t ldr, void* Y, int64_t ldy,
                        int M, int N, int K, int act, const void* gate, int64_t ld_gate, int rows_per_gate, void* s) {
    UV_REQUIRE(X && W && Y, "linear_gated: null argument");
    UV_REQUIRE(act == UNIVST_ACT_NONE || act == UNIVST_ACT_GELU_TANH, "linear_gated: act must be UNIVST_ACT_NONE or UNIVST_ACT_GELU_TANH");
    GemmParams g;
    g.X = H(X); g.ldx = ldx; g.W = H(W); g.bias = H(bias); g.R = H(R); g.ldr = ldr; g.Y = HM(Y); g.ldy = ldy;
    g.M = M; g.N = N; g.K = K;
    g.act = act == UNIVST_ACT_GELU_TANH ? 1 : 0;
    g.gate = H(gate); g.ld_gate = ld_gate; g.rows_per_gate = gate ? rows_per_gate : 1;
    return uv_launch_gemm(g, 0, S(s));
}
int univst_linear_epi(const void* X, int64_t ldx, const void* W, const void* bias, const void* R, int64_t ldr, void* Y, int64_t ldy,
                      int M, int N, int K, int geglu, const void* rowbias, int rows_per_rowbias, int64_t ldrb, const void* bias2,
                      void* workspace, int64_t workspace_bytes, void* s) {
    UV_REQUIRE(X && W && Y, "linear_epi: null argument");
    UV_REQUIRE(!rowbias || rows_per_rowbias >= 1, "linear_epi: rows_per_rowbias=%d must be at least 1", rows_per_rowbias);
    GemmParams g;
    g.X = H(X); g.ldx = ldx; g.W = H(W); g.bias = H(bias); g.R = H(R); g.ldr = ldr; g.Y = HM(Y); g.ldy = ldy;
    g.M = M; g.N = N; g.K = K; g.geglu = geglu;
    g.rowbias = H(rowbias); g.rows_per_rb = rowbias ? rows_per_rowbias : 1; g.ldrb = ldrb; g.bias2 = H(bias2);
    g.partial = (float*)workspace; g.partial_bytes = workspace && workspace_bytes > 0 ? (size_t)workspace_bytes : 0;
    return uv_launch_gemm(g, 0, S(s));
}
int univst_geglu_xres_permute(const void* in, void* out, int rows, int cols, void* s) {
    UV_REQUIRE(in && out, "geglu_xres_permute: null argument");
    return uv_launch_geglu_xres_permute(H(in), HM(out), rows, cols, S(s));
}
struct univst_clip {
    Clip impl;
};
int univst_clip_create(const univst_clip_cfg* cfg, univst_clip** out) {
    UV_REQUIRE(cfg && out, "clip_create: null argument");
    UV_RUN(uv_clip_check_cfg(*cfg));
    univst_clip* h = new (std::nothrow) univst_clip();
    UV_REQUIRE(h, "clip_create: out of host memory");
    h->impl.cfg = *cfg;
    *out = h;
    return UV_OK;
}
UV_HANDLE_ABI(clip)
int univst_clip_encode(univst_clip* h, const int64_t* ids, int B, int Sq, void* last_hidden, void* hidden_states, void* pooled, void* s) {
    UV_REQUIRE(h && ids, "clip_encode: null argument");
    return h->impl.encode(ids, B, Sq, HM(last_hidden), HM(hidden_states), HM(pooled), S(s));
}
int univst_clip_query(univst_clip* h, const char* name, double* out) {
    UV_REQUIRE(h && name && out, "clip_query: null argument");
    if (model_query(h->impl, name, out)) return UV_OK;
    if (!strcmp(name, "splitk_bytes")) {
        *out = (double)h->impl.splitk_bytes;
        return UV_OK;
    }
    uv_set_error("clip_query: unknown quantity '%s'", name);
    return UV_ERR_ARG;
}
int univst_clip_attention(const void* qkv, int B, int Sq, int heads, void* out, void* s) {
    return uv_launch_clip_attention(H(qkv), B, Sq, heads, HM(out), S(s));
}
struct univst_t5 {
    T5 impl;
};
int univst_t5_create(const univst_t5_cfg* cfg, univst_t5** out) {
    UV_REQUIRE(cfg && out, "t5_create: null argument");
    UV_RUN(uv_t5_check_cfg(*cfg));
    univst_t5* h = new (std::nothrow) univst_t5();
    UV_REQUIRE(h, "t5_create: out of host memory");
    h->impl.cfg = *cfg;
    *out = h;
    return UV_OK;
}
UV_HANDLE_ABI(t5)
int univst_t5_encode(univst_t5* h, const int64_t* ids, int B, int Sq, void* last_hidden, void* s) {
    UV_REQUIRE(h && ids && last_hidden, "t5_encode: null argument");
    return h->impl.encode(ids, B, Sq, HM(last_hidden), S(s));
}
int univst_t5_query(univst_t5* h, const char* name, double* out) {
    UV_REQUIRE(h && name && out, "t5_query: null argument");
    if (model_query(h->impl, name, out)) return UV_OK;
    if (!strcmp(name, "splitk_bytes")) {
        *out = (double)h->impl.splitk_bytes;
        return UV_OK;
    }
    uv_set_error("t5_query: unknown quantity '%s'", name);
    return UV_ERR_ARG;
}
int univst_t5_attention(const void* qkv, const float* bias_table, int B, int Sq, int heads, void* out, void* s) {
    return uv_launch_t5_attention(H(qkv), bias_table, B, Sq, heads, HM(out), S(s));
}
int univst_debug_t5_buckets(int num_buckets, int max_distance, int n, int* out) { return uv_t5_bucket_table(num_buckets, max_distance, n, out); }
struct univst_motion {
    Motion impl;
};
int univst_motion_create(const univst_motion_cfg* cfg, univst_motion** out) {
    UV_REQUIRE(cfg && out, "motion_create: null argument");
    UV_RUN(uv_motion_check_cfg(*cfg));
    univst_motion* h = new (std::nothrow) univst_motion();
    UV_REQUIRE(h, "motion_create: out of host memory");
    h->impl.cfg = *cfg;
    *out = h;
    return UV_OK;
}
UV_HANDLE_ABI(motion)
int univst_motion_forward(univst_motion* h, const void* X, void* Y, int B, int F, int N, void* s) {
    UV_REQUIRE(h && X && Y, "motion_forward: null argument");
    return h->impl.forward(H(X), HM(Y), B, F, N, S(s));
}
int univst_motion_query(univst_motion* h, const char* name, double* out) {
    UV_REQUIRE(h && name && out, "motion_query: null argument");
    if (model_query(h->impl, name, out)) return UV_OK;
    uv_set_error("motion_query: unknown quantity '%s'", name);
    return UV_ERR_ARG;
}
int univst_temporal_attention(const void* qkv, int64_t ldx, const void* pe_qkv, int B, int F, int N, int heads, int head_dim, void* out, int64_t ldo, void* s) {
    return uv_launch_temporal_attention(H(qkv), ldx, H(pe_qkv), B, F, N, heads, head_dim, HM(out), ldo, S(s));
}
struct univst_vae {
    Vae impl;
};
int univst_vae_create(const univst_vae_cfg* cfg, univst_vae** out) {
    UV_REQUIRE(cfg && out, "vae_create: null argument");
    UV_REQUIRE(cfg->norm_num_groups > 0 && cfg->layers_per_block >= 1 && cfg->in_channels >= 1 && cfg->in_channels <= 8 && cfg->out_channels >= 1 &&
               cfg->out_channels <= 8 && cfg->latent_channels >= 1 && cfg->latent_channels <= 8, "vae_create: bad config");
    for (int i = 0; i < 4; ++i) {
        const int c = cfg->block_out_channels[i];
        UV_REQUIRE(c > 0 && c % 8 == 0 && c % cfg->norm_num_groups == 0 && (c / cfg->norm_num_groups) % 2 == 0,
                   "vae_create: block_out_channels[%d]=%d must be a multiple of 8 and an even multiple of the group count", i, c);
    }
    univst_vae* h = new (std::nothrow) univst_vae();
    UV_REQUIRE(h, "vae_create: out of host memory");
    h->impl.cfg = *cfg;
    *out = h;
    return UV_OK;
}
UV_HANDLE_ABI(vae)
int univst_vae_decode(univst_vae* h, const void* z, int64_t imgs, int num_frames, int lat_h, int lat_w, void* out, void* s) {
    UV_REQUIRE(h && z && out, "vae_decode: null argument");
    return h->impl.decode(H(z), imgs, num_frames, lat_h, lat_w, HM(out), S(s));
}
int univst_vae_encode(univst_vae* h, const void* x, int64_t imgs, int Hh, int W, void* moments, void* s) {
    UV_REQUIRE(h && x && moments, "vae_encode: null argument");
    return h->impl.encode(H(x), imgs, Hh, W, HM(moments), S(s));
}
struct univst_klvae {
    KlVae impl;
};
int univst_klvae_create(const univst_klvae_cfg* cfg, univst_klvae** out) {
    UV_REQUIRE(cfg && out, "klvae_create: null argument");
    UV_REQUIRE(cfg->norm_num_groups > 0 && cfg->layers_per_block >= 1 && cfg->in_channels >= 1 && cfg->in_channels <= 8 && cfg->out_channels >= 1 &&
               cfg->out_channels <= 8, "klvae_create: bad config");
    UV_REQUIRE(cfg->latent_channels >= 4 && cfg->latent_channels <= 64 && cfg->latent_channels % 4 == 0,
               "klvae_create: latent_channels=%d: the moments' 2 x latent_channels must be a multiple of 8 (at most 128)", cfg->latent_channels);
    UV_REQUIRE(cfg->attn_score_bytes >= 0 && cfg->pass_bytes >= 0, "klvae_create: negative budget");
    for (int i = 0; i < 4; ++i) {
        const int c = cfg->block_out_channels[i];
        UV_REQUIRE(c > 0 && c % 8 == 0 && c % cfg->norm_num_groups == 0 && (c / cfg->norm_num_groups) % 2 == 0,
                   "klvae_create: block_out_channels[%d]=%d must be a multiple of 8 and an even multiple of the group count", i, c);
    }
    univst_klvae* h = new (std::nothrow) univst_klvae();
    UV_REQUIRE(h, "klvae_create: out of host memory");
    h->impl.kcfg = *cfg;
    univst_vae_cfg& b = h->impl.cfg;
    b.in_channels = cfg->in_channels;
    b.out_channels = cfg->out_channels;
    b.latent_channels = cfg->latent_channels;
    for (int i = 0; i < 4; ++i) b.block_out_channels[i] = cfg->block_out_channels[i];
    b.layers_per_block = cfg->layers_per_block;
    b.norm_num_groups = cfg->norm_num_groups;
    *out = h;
    return UV_OK;
}
UV_HANDLE_ABI(klvae)
int univst_klvae_decode(univst_klvae* h, const void* z, int64_t imgs, int lat_h, int lat_w, void* out, void* s) {
    UV_REQUIRE(h && z && out, "klvae_decode: null argument");
    return h->impl.decode(H(z), imgs, lat_h, lat_w, HM(out), S(s));
}
int univst_klvae_encode(univst_klvae* h, const void* x, int64_t imgs, int Hh, int W, void* moments, void* s) {
    UV_REQUIRE(h && x && moments, "klvae_encode: null argument");
    return h->impl.encode(H(x), imgs, Hh, W, HM(moments), S(s));
}
int univst_klvae_query(univst_klvae* h, const char* name, double* out) {
    UV_REQUIRE(h && name && out, "klvae_query: null argument");
    if (model_query(h->impl, name, out)) return UV_OK;
    if (!strcmp(name, "attn_chunks")) {
        *out = (double)h->impl.attn_chunks;
        return UV_OK;
    }
    if (!strcmp(name, "passes")) {
        *out = (double)h->impl.passes;
        return UV_OK;
    }
    uv_set_error("klvae_query: unknown quantity '%s'", name);
    return UV_ERR_ARG;
}
struct univst_raft {
    Raft impl;
};
int univst_raft_create(univst_raft** out) {
    UV_REQUIRE(out, "raft_create: null argument");
    univst_raft* h = new (std::nothrow) univst_raft();
    UV_REQUIRE(h, "raft_create: out of host memory");
    *out = h;
    return UV_OK;
}
int univst_raft_destroy(univst_raft* h) {
    delete h;
    return UV_OK;
}
int univst_raft_load_tensor(univst_raft* h, const char* key, const void* p, int dtype, const int64_t* shape, int ndim, void* s) {
    UV_REQUIRE(h, "null handle");
    return h->impl.load_tensor(key, p, dtype, shape, ndim, S(s));
}
int univst_raft_forward(univst_raft* h, const uint8_t* img1, const uint8_t* img2, int Hh, int W, float* flow, void* s) {
    UV_REQUIRE(h && img1 && img2 && flow, "raft_forward: null argument");
    return h->impl.forward(img1, img2, Hh, W, flow, S(s));
}
int univst_raft_encode(univst_raft* h, const uint8_t* img1, const uint8_t* img2, int Hh, int W, void* fmap, float* hidden, void* context, void* s) {
    UV_REQUIRE(h && img1 && img2, "raft_encode: null argument");
    int rc = h->impl.encode(img1, img2, Hh, W, S(s));
    if (rc) return rc;
    const size_t N = (size_t)(Hh / 8) * (W / 8);
    if (fmap) UV_HIP(hipMemcpyAsync(fmap, h->impl.fmap, 2 * N * 256 * 2, hipMemcpyDeviceToDevice, S(s)));
    if (hidden) UV_HIP(hipMemcpyAsync(hidden, h->impl.h32, N * 128 * 4, hipMemcpyDeviceToDevice, S(s)));
    if (context) UV_HIP(hipMemcpyAsync(context, h->impl.ctx16, N * 128 * 2, hipMemcpyDeviceToDevice, S(s)));
    return UV_OK;
}
int univst_raft_gru(univst_raft* h, float* hidden, const void* context, const void* motion, int fh, int fw, void* s) {
    UV_REQUIRE(h && hidden && context && motion, "raft_gru: null argument");
    UV_REQUIRE(fh >= 16 && fw >= 16 && fh <= 512 && fw <= 512, "raft_gru: feature map %d x %d (at least 16 x 16)", fh, fw);
    if (!h->impl.finalized) {
        int rc = h->impl.finalize(S(s));
        if (rc) return rc;
    }
    int rc = h->impl.reserve(fh * 8, fw * 8);
    if (rc) return rc;
    return h->impl.gru(hidden, h->impl.h16, H(context), H(motion), fh, fw, S(s));
}
int64_t univst_raft_pyramid_floats(int fh, int fw) { return fh > 0 && fw > 0 ? uv_raft_pyramid_floats(fh, fw) : 0; }
int univst_raft_corr_pyramid(const void* f1, const void* f2, int fh, int fw, float* pyr, void* s) {
    UV_REQUIRE(f1 && f2 && pyr, "raft_corr_pyramid: null argument");
    return uv_raft_corr_pyramid(H(f1), H(f2), fh, fw, pyr, S(s));
}
int univst_raft_corr_lookup(const float* pyr, const float* coords, int fh, int fw, float* out32, void* out16, void* s) {
    UV_REQUIRE(pyr && coords, "raft_corr_lookup: null argument");
    return uv_raft_corr_lookup(pyr, coords, fh, fw, out32, HM(out16), S(s));
}
int univst_raft_convex_upsample(const float* flow, const void* mask, int fh, int fw, float* out, void* s) {
    UV_REQUIRE(flow && mask && out, "raft_convex_upsample: null argument");
    return uv_raft_convex_upsample(flow, 0, H(mask), fh, fw, out, S(s));
}
int univst_frag_pack(const void* W, void* out, int N, int K, void* s) {
    UV_REQUIRE(W && out, "frag_pack: null argument");
    return uv_launch_frag_pack(H(W), HM(out), N, K, S(s));
}
int64_t univst_attn2_fused_workspace_bytes(int B, int heads, int head_dim) { return uv_attn2_kvf_halfs(B, heads, head_dim) * (int64_t)sizeof(half_t); }
int univst_attn2_fused(const void* X, int64_t ldx, const float* ln_stats, float ln_eps, const float* ln_wsum, const float* ln_bias, const void* Wq_frag,
                       int q_prescaled, const void* kv, int B, int T, int64_t rows_per_branch, const void* Wo_frag, const void* bias_o,
                       const void* residual, int64_t ldr, void* Y, int64_t ldy, int64_t M, int C, int heads, float* stats_out, void* workspace,
                       void* s) {
    UV_REQUIRE(X && Wq_frag && kv && Wo_frag && residual && Y && workspace, "attn2_fused: null argument");
    UV_REQUIRE(B >= 1 && M >= 1 && M <= (int64_t)B * rows_per_branch && M < (1LL << 31) && C % 160 == 0 && heads > 0 && C % heads == 0,
               "attn2_fused: M=%lld rows exceed B=%d branches of %lld rows (or bad C / heads)", (long long)M, B, (long long)rows_per_branch);
    UV_REQUIRE(!ln_stats || (ln_wsum && ln_bias), "attn2_fused: a folded LayerNorm needs ln_wsum and ln_bias");
    UV_REQUIRE(uv_attn2_fused_ok(C, heads, (int)rows_per_branch, T), "attn2_fused: C=%d heads=%d rows_per_branch=%lld keys=%d is not a shape this kernel serves "
               "(C = 320, 8 heads, rows per branch a multiple of 64, <= 80 keys)", C, heads, (long long)rows_per_branch, T);
    int rc = uv_launch_kv_frag_pack(H(kv), HM(workspace), B, T, C, heads, S(s));
    if (rc) return rc;
    Attn2Params p;
    p.X = H(X); p.ldx = ldx; p.M = (int)M;
    p.ln_stats = ln_stats; p.ln_slots = C / 160; p.ln_eps = ln_eps; p.ln_wsum = ln_wsum; p.ln_bias = ln_bias;
    p.Wq_f = H(Wq_frag); p.kvf = H(workspace);
    p.rows_per_branch = (int)rows_per_branch; p.heads = heads; p.Nkv = T;
    p.q_prescaled = q_prescaled; p.scale_log2e = 1.4426950408889634f / sqrtf((float)(C / heads));
    p.Wo_f = H(Wo_frag); p.bias_o = H(bias_o);
    p.R = H(residual); p.ldr = ldr;
    p.Y = HM(Y); p.ldy = ldy;
    p.stats_out = stats_out;
    return uv_launch_attn2_fused(p, C, S(s));
}
int univst_attn12_fused(const void* attn_out, int64_t ldx, const void* Wp_frag, const void* bias_p, const void* residual_in, int64_t ldr_in, float ln_eps,
                        const float* ln_wsum, const float* ln_bias, const void* Wq_frag, int q_prescaled, const void* kv, int B, int T, int64_t rows_per_branch,
                        const void* Wo_frag, const void* bias_o, void* Y, int64_t ldy, int64_t M, int C, int heads, float* stats_out, void* workspace, void* s) {
    UV_REQUIRE(attn_out && Wp_frag && residual_in && ln_wsum && ln_bias && Wq_frag && kv && Wo_frag && Y && workspace, "attn12_fused: null argument");
    UV_REQUIRE(B >= 1 && M >= 1 && M <= (int64_t)B * rows_per_branch && M < (1LL << 31) && heads > 0 && C % heads == 0, "attn12_fused: M=%lld rows exceed B=%d branches of %lld rows",
               (long long)M, B, (long long)rows_per_branch);
    UV_REQUIRE(uv_attn2_fused_ok(C, heads, (int)rows_per_branch, T), "attn12_fused: C=%d heads=%d rows_per_branch=%lld keys=%d is not a shape this kernel serves "
               "(C = 320, 8 heads, rows per branch a multiple of 64, <= 80 keys)", C, heads, (long long)rows_per_branch, T);
    int rc = uv_launch_kv_frag_pack(H(kv), HM(workspace), B, T, C, heads, S(s));
    if (rc) return rc;
    Attn2Params p;
    p.X = H(attn_out); p.ldx = ldx; p.M = (int)M;
    p.Wp_f = H(Wp_frag); p.bias_p = H(bias_p); p.Rp = H(residual_in); p.ldrp = ldr_in;
    p.ln_slots = C / 160; p.ln_eps = ln_eps; p.ln_wsum = ln_wsum; p.ln_bias = ln_bias;
    p.Wq_f = H(Wq_frag); p.kvf = H(workspace);
    p.rows_per_branch = (int)rows_per_branch; p.heads = heads; p.Nkv = T;
    p.q_prescaled = q_prescaled; p.scale_log2e = 1.4426950408889634f / sqrtf((float)(C / heads));
    p.Wo_f = H(Wo_frag); p.bias_o = H(bias_o);
    p.Y = HM(Y); p.ldy = ldy;
    p.stats_out = stats_out;
    return uv_launch_attn2_fused(p, C, S(s));
}
int univst_linear_ln(const void* X, int64_t ldx, const void* W, const void* bias, const void* R, int64_t ldr, void* Y, int64_t ldy,
                     int M, int N, int K, int geglu, const float* ln_stats, float ln_eps, const float* ln_wsum, const float* ln_bias,
                     float* stats_out, void* s) {
    UV_REQUIRE(X && W && Y, "linear_ln: null argument");
    UV_REQUIRE(!ln_stats || (ln_wsum && ln_bias && K % 160 == 0 && !bias), "linear_ln: a folded LayerNorm needs wsum, lnb (which holds the bias) and K %% 160 == 0");
    UV_REQUIRE((!stats_out || uv_linear_fold_producer_ok(M, N, K)) && (!ln_stats || geglu == 2 || uv_linear_fold_consumer_ok(M, N, K, geglu != 0)),
               "linear_ln: M=%d N=%d K=%d is not taken by the direct 256x320 path (N %% 320 == 0 and >= 150 tiles) nor by the 128-wide path without split-K", M, N, K);
    GemmParams g;
    g.X = H(X); g.ldx = ldx; g.W = H(W); g.bias = H(bias); g.R = H(R); g.ldr = ldr; g.Y = HM(Y); g.ldy = ldy;
    g.M = M; g.N = N; g.K = K; g.geglu = geglu;
    g.ln_stats = ln_stats; g.ln_slots = K / 160; g.ln_eps = ln_eps; g.ln_wsum = ln_wsum; g.ln_bias = ln_bias; g.stats_out = stats_out;
    return uv_launch_gemm(g, 0, S(s));
}
int univst_conv_nhwc(const void* X1, const void* X2, int C1, int C2, int imgs, int Hs, int Ws, int up, int stride, int taps,
                     const void* W, const void* bias, const void* rowbias, int rows_per_rb, const void* R, void* Y, int Cout,
                     void* s) {
    UV_REQUIRE(X1 && W && Y, "conv: null argument");
    UV_REQUIRE((X2 != nullptr) == (C2 > 0), "conv: X2/C2 mismatch");
    UV_REQUIRE(stride == 1 || stride == 2, "conv: stride %d", stride);
    GemmParams g;
    g.X = H(X1); g.X2 = H(X2); g.C1 = C1; g.C2 = C2; g.Hs = Hs; g.Ws = Ws; g.up = up ? 1 : 0; g.stride = stride; g.taps = taps;
    const int He = Hs << g.up, We = Ws << g.up;
    g.Ho = taps == 9 ? (He - 1) / stride + 1 : He;
    g.Wo = taps == 9 ? (We - 1) / stride + 1 : We;
    g.M = imgs * g.Ho * g.Wo; g.N = Cout; g.K = taps * (C1 + C2);
    g.W = H(W); g.bias = H(bias); g.rowbias = H(rowbias); g.rows_per_rb = rows_per_rb > 0 ? rows_per_rb : 1;
    g.R = H(R); g.ldr = Cout; g.Y = HM(Y); g.ldy = Cout;
    return uv_launch_gemm(g, 1, S(s));
}
int univst_conv_nhwc_tapinner(const void* X1, const void* X2, int C1, int C2, int imgs, int Hs, int Ws, int up, int stride,
                              const void* W, const void* bias, const void* rowbias, int rows_per_rb, const void* R, void* Y, int Cout,
                              void* s) {
    UV_REQUIRE(X1 && W && Y, "conv: null argument");
    UV_REQUIRE((X2 != nullptr) == (C2 > 0), "conv: X2/C2 mismatch");
    GemmParams g;
    g.X = H(X1); g.X2 = H(X2); g.C1 = C1; g.C2 = C2; g.Hs = Hs; g.Ws = Ws; g.up = up ? 1 : 0; g.stride = stride; g.taps = 9; g.korder = 1;
    const int He = Hs << g.up, We = Ws << g.up;
    g.Ho = (He - 1) / stride + 1;
    g.Wo = (We - 1) / stride + 1;
    g.M = imgs * g.Ho * g.Wo; g.N = Cout; g.K = 9 * (C1 + C2);
    g.W = H(W); g.bias = H(bias); g.rowbias = H(rowbias); g.rows_per_rb = rows_per_rb > 0 ? rows_per_rb : 1;
    g.R = H(R); g.ldr = Cout; g.Y = HM(Y); g.ldy = Cout;
    return uv_launch_gemm(g, 1, S(s));
}
int univst_conv3x3_patch(const void* X1, const void* X2, int C1, int C2, int imgs, int Hs, int Ws, int upsample, const void* W32,
                         const void* bias, const void* rowbias, int rows_per_rb, const void* R, void* Y, int Cout, void* s) {
    UV_REQUIRE(X1 && W32 && Y, "conv3x3_patch: null argument");
    UV_REQUIRE((X2 != nullptr) == (C2 > 0), "conv3x3_patch: X2/C2 mismatch");
    GemmParams g;
    g.X = H(X1); g.X2 = H(X2); g.C1 = C1; g.C2 = C2; g.Hs = Hs; g.Ws = Ws; g.up = upsample ? 1 : 0; g.stride = 1; g.taps = 9;
    g.Ho = Hs << g.up; g.Wo = Ws << g.up;
    g.M = imgs * g.Ho * g.Wo; g.N = Cout; g.K = 9 * (C1 + C2);
    g.W = nullptr; g.W32 = H(W32);
    g.bias = H(bias); g.rowbias = H(rowbias); g.rows_per_rb = rows_per_rb > 0 ? rows_per_rb : 1;
    g.R = H(R); g.ldr = Cout; g.Y = HM(Y); g.ldy = Cout;
    return uv_launch_gemm(g, 1, S(s));
}
int univst_linear_compose(const void* Wp, const void* W2, const void* b2, const void* tb, const void* bp, int C, int K2, void* W_out, void* bias_out, void* s) {
    return uv_launch_linear_compose(H(Wp), H(W2), H(b2), H(tb), H(bp), C, K2, HM(W_out), HM(bias_out), S(s));
}
int univst_conv_up2_phase_weights(const void* W_oihw, int Cout, int Cin, void* W4, void* s) {
    UV_REQUIRE(W_oihw && W4, "conv_up2_phase_weights: null argument");
    return uv_launch_conv_up2_phase_weights(H(W_oihw), HM(W4), Cout, Cin, S(s));
}
int univst_conv3x3_up2_phase(const void* X, int C, int imgs, int Hs, int Ws, const void* W4, const void* bias, void* Y, int Cout, float* gn_out,
                             int gn_group_width, void* s) {
    UV_REQUIRE(X && W4 && Y, "conv3x3_up2_phase: null argument");
    UV_REQUIRE(!gn_out || (gn_group_width > 0 && Cout % gn_group_width == 0), "conv3x3_up2_phase: gn_group_width=%d must divide Cout=%d", gn_group_width, Cout);
    GemmParams g;
    g.X = H(X); g.C1 = C; g.Hs = Hs; g.Ws = Ws; g.up = 1; g.stride = 1; g.taps = 9;
    g.Ho = 2 * Hs; g.Wo = 2 * Ws;
    g.M = imgs * g.Ho * g.Wo; g.N = Cout; g.K = 9 * C;
    g.W4 = H(W4); g.bias = H(bias); g.Y = HM(Y); g.ldy = Cout;
    g.tapw = 3; g.pady = g.padx = 1;
    int emitted = 0;
    if (gn_out) { g.gn_out = gn_out; g.gn_gw = gn_group_width; g.gn_G = Cout / gn_group_width; g.gn_emitted = &emitted; }
    const GemmPlan pl = uv_gemm_plan(g, 1, uv_num_cus());      // only the phase copy is given: the plan takes the phase form or names what is missing
    UV_REQUIRE(pl.rc != UV_OK || (pl.phase && (!gn_out || pl.gn_emit)), "conv3x3_up2_phase: the problem does not take the phase form with these statistics "
               "(C %% 64, Cout %% 320, whole source rows per tile, >= 150 tiles, statistics of 10 / 20 / 40-channel groups)");
    return uv_launch_gemm(g, 1, S(s));
}
int univst_groupnorm_fold_linear(const void* X, int C, int64_t rows, int rows_per_stat, int groups, float eps, const void* gamma, const void* beta,
                                 const void* W, const void* bias, int N, void* W_sets, float* bias32, void* ws, void* s) {
    UV_REQUIRE(X && gamma && beta && W && W_sets && bias32 && ws && N > 0, "groupnorm_fold_linear: null argument");
    UvGnFold f;
    f.W = H(W); f.bias = H(bias); f.N = N; f.W_out = HM(W_sets); f.bias32 = bias32;
    return uv_launch_groupnorm(H(X), nullptr, C, 0, rows, rows_per_stat, groups, eps, H(gamma), H(beta), 0, nullptr, (float*)ws, S(s), nullptr, nullptr, nullptr, &f);
}
int univst_linear_sets(const void* X, int64_t ldx, const void* W_sets, const float* bias32, int rows_per_set, const void* R, int64_t ldr, void* Y, int64_t ldy,
                       int M, int N, int K, float* stats_out, void* s) {
    UV_REQUIRE(X && W_sets && bias32 && Y && rows_per_set > 0, "linear_sets: null argument");
    GemmParams g;
    g.X = H(X); g.ldx = ldx; g.W = H(W_sets); g.bias32 = bias32; g.w_rows_per_set = rows_per_set;
    g.R = H(R); g.ldr = ldr; g.Y = HM(Y); g.ldy = ldy; g.M = M; g.N = N; g.K = K; g.stats_out = stats_out;
    UV_REQUIRE(uv_linear_takes_big_direct(M, N, K, ldx), "linear_sets: M=%d N=%d K=%d is not a problem the direct 256x320 path takes (N %% 320 == 0, >= 150 tiles)", M, N, K);
    return uv_launch_gemm(g, 0, S(s));
}
int64_t univst_groupnorm_workspace_bytes(int64_t rows, int rows_per_stat, int groups) {
    if (rows_per_stat <= 0) return 0;
    return (int64_t)uv_groupnorm_workspace_floats((int)(rows / rows_per_stat), groups) * 4;
}
int univst_groupnorm_nhwc(const void* X1, const void* X2, int C1, int C2, int64_t rows, int rows_per_stat, int groups, float eps,
                          const void* gamma, const void* beta, int silu, void* Y, void* ws, void* s) {
    UV_REQUIRE(X1 && gamma && beta && Y && ws, "groupnorm: null argument");
    return uv_launch_groupnorm(H(X1), H(X2), C1, C2, rows, rows_per_stat, groups, eps, H(gamma), H(beta), silu, HM(Y), (float*)ws,
                               S(s));
}
int univst_layernorm(const void* X, void* Y, const void* gamma, const void* beta, int64_t rows, int C, float eps, void* s) {
    UV_REQUIRE(X && Y && gamma && beta, "layernorm: null argument");
    UV_REQUIRE(rows >= 1 && rows <= INT_MAX && C >= 8, "layernorm: rows=%ld must be in 1 .. INT_MAX and C=%d at least 8", (long)rows, C);
    return uv_launch_layernorm(H(X), C, HM(Y), C, H(gamma), H(beta), rows, C, eps, S(s));
}
int univst_attention(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* out, int64_t ldo,
                     const int32_t* src_idx, const int32_t* src_cnt, const float* src_logw, int nsrc, int BF, int Nq, int Nkv, int heads,
                     int d, int q_prescaled, void* s) {
    UV_REQUIRE(q && k && v && out && src_idx, "attention: null argument");
    AttnParams a;
    a.src_cnt = src_cnt;
    a.src_logw = src_logw;
    a.q = H(q); a.k = H(k); a.v = H(v); a.o = HM(out); a.ldq = ldq; a.ldkv = ldkv; a.ldo = ldo; a.src_idx = src_idx; a.nsrc = nsrc;
    a.BF = BF; a.Nq = Nq; a.Nkv = Nkv; a.heads = heads; a.d = d;
    a.scale_log2e = 1.4426950408889634f / sqrtf((float)d);
    a.q_prescaled = q_prescaled != 0;
    return uv_launch_attention(a, S(s));
}
int univst_attention_phase(const void* q, int64_t ldq, const void* k, const void* v, int64_t ldkv, void* out, int64_t ldo,
                           const int32_t* src_idx, const int32_t* src_cnt, const float* src_logw, int nsrc, int BF, int Nq, int Nkv, int heads,
                           int d, int q_prescaled, float* state_out, const float* state_in, void* s) {
    UV_REQUIRE(q && k && v && out && src_idx && src_cnt, "attention_phase: null argument (src_cnt is required: a phase may leave a frame without sources)");
    UV_REQUIRE((state_out != nullptr) != (state_in != nullptr), "attention_phase: exactly one of state_out (first phase) / state_in (second phase)");
    AttnParams a;
    a.src_cnt = src_cnt;
    a.src_logw = src_logw;
    a.q = H(q); a.k = H(k); a.v = H(v); a.o = HM(out); a.ldq = ldq; a.ldkv = ldkv; a.ldo = ldo; a.src_idx = src_idx; a.nsrc = nsrc;
    a.BF = BF; a.Nq = Nq; a.Nkv = Nkv; a.heads = heads; a.d = d;
    a.scale_log2e = 1.4426950408889634f / sqrtf((float)d);
    a.q_prescaled = q_prescaled != 0;
    a.state_out = state_out;
    a.state_in = state_in;
    return uv_launch_attention(a, S(s));
}
int univst_attention_adain_shift(void* qkv, int64_t ld, int F, int N, int C, float alpha, float beta, float gamma, void* ws, void* s) {
    UV_REQUIRE(qkv && ws, "adain_shift: null argument");
    float* w = (float*)ws;
    return uv_launch_adain_shift(HM(qkv), ld, F, N, C, w, w + (long)F * 2 * C, alpha, beta, gamma, S(s));
}
int univst_attention_adain_shift_static(void* qkv, int64_t ld, const void* style_kv, int64_t ld_style, int F, int N, int C, float alpha, float beta,
                                        float gamma, void* ws, void* s) {
    UV_REQUIRE(qkv && style_kv && ws, "adain_shift_static: null argument");
    float* w = (float*)ws;
    return uv_launch_adain_shift_static(HM(qkv), ld, H(style_kv), ld_style, F, N, C, w, w + 2L * C, alpha, beta, gamma, S(s));
}
int univst_latent_adain(const void* cnt, const void* sty, void* out, int C, int F, int HW, void* s) {
    UV_REQUIRE(cnt && sty && out, "latent_adain: null argument");
    return uv_launch_latent_adain(H(cnt), H(sty), HM(out), C, F, HW, S(s));
}
int univst_latent_adain_stats(const void* cnt, float* stats, int C, int F, int HW, void* s) {
    UV_REQUIRE(cnt && stats, "latent_adain_stats: null argument");
    return uv_launch_latent_adain_stats(H(cnt), stats, C, F, HW, S(s));
}
int univst_latent_adain_apply(const void* cnt, const void* sty, const float* stats, int64_t n_total, void* out, int C, int F, int HW,
                              void* s) {
    UV_REQUIRE(cnt && sty && stats && out && n_total > 0, "latent_adain_apply: bad argument");
    return uv_launch_latent_adain_apply(H(cnt), H(sty), stats, n_total, HM(out), C, F, HW, S(s));
}
int univst_axpby(const void* x, const void* e, void* out, float cx, float ce, int64_t n, void* s) {
    UV_REQUIRE(x && e && out, "axpby: null argument");
    return uv_launch_axpby(H(x), H(e), HM(out), cx, ce, n, S(s));
}
int univst_mask_blend(const void* a, const void* b, const void* m, void* out, int C, int64_t FHW, void* s) {
    UV_REQUIRE(a && b && out, "mask_blend: null argument");
    return uv_launch_mask_blend(H(a), H(b), H(m), HM(out), C, FHW, S(s));
}
int univst_mask_resize(const uint8_t* mask, void* out, int F, int Hh, int W, int h, int w, void* s) {
    UV_REQUIRE(mask && out, "mask_resize: null argument");
    return uv_launch_mask_resize(mask, HM(out), F, Hh, W, h, w, S(s));
}
int univst_debug_tr16(float* out, void* s) { return uv_launch_tr16_probe(out, S(s)); }
int univst_debug_delay_us(double us, void* s) { return uv_launch_delay_us(us, S(s)); }
// host-only read-outs of the launch plans: stand-in operands (never dereferenced), 16-byte aligned with natural leading dimensions
int univst_debug_gemm_plan(int ncu, int mode, int M, int N, int K, int geglu, int flags, int rows_per_set, int C1, int C2, int Hs, int Ws, int upsample,
                           int stride, int taps, int geom, char* buf, int n) {
    UV_REQUIRE(buf && n > 0 && ncu > 0, "debug_gemm_plan: null buffer or ncu <= 0");
    if (M == 0 && N == 0) {
        snprintf(buf, (size_t)n, "%s", uv_gemm_plan_symbols().c_str());
        return UV_OK;
    }
    alignas(16) static float arena[8];                // an address to stand for every operand
    half_t* const h = (half_t*)arena;
    auto on = [&](int bit) { return (flags & bit) != 0; };
    GemmParams g;
    g.X = h; g.Y = on(UNIVST_PLAN_Y_UNALIGNED) ? h + 4 : h;
    g.W = on(UNIVST_PLAN_W32_ONLY) ? nullptr : h;
    g.W32 = on(UNIVST_PLAN_W32_ONLY) || on(UNIVST_PLAN_W32) ? h : nullptr;
    g.W4 = on(UNIVST_PLAN_W4) ? h : nullptr;
    g.N = N; g.geglu = geglu;
    const int No = geglu ? N / 2 : N;
    if (mode == 0) {
        g.M = M; g.K = K; g.ldx = K;
    } else {                                          // M: images
        g.C1 = C1; g.C2 = C2; g.X2 = C2 ? h : nullptr; g.Hs = Hs; g.Ws = Ws; g.up = upsample ? 1 : 0; g.stride = stride; g.taps = taps;
        const int He = Hs << g.up, We = Ws << g.up;
        if (geom == UNIVST_PLAN_GEOM_FRAME) {         // the 3x1 frame conv: image rows = frames, image columns = pixels
            g.tapw = 1; g.pady = 1; g.padx = 0; g.Ho = He; g.Wo = We;
        } else if (geom == UNIVST_PLAN_GEOM_PAD_END) {    // input padded at the bottom / right only
            g.tapw = 3; g.pady = g.padx = 0; g.Ho = (He + 1 - 3) / stride + 1; g.Wo = (We + 1 - 3) / stride + 1;
        } else {
            g.Ho = (He - 1) / stride + 1; g.Wo = (We - 1) / stride + 1;
        }
        g.M = M * g.Ho * g.Wo; g.K = taps * (C1 + C2);
        g.korder = on(UNIVST_PLAN_TAPINNER) ? 1 : 0;
    }
    g.ldy = on(UNIVST_PLAN_LDY_ODD) ? No + 1 : No; g.ldr = No;
    if (on(UNIVST_PLAN_BIAS)) g.bias = h;
    if (on(UNIVST_PLAN_RESIDUAL)) g.R = h;
    if (on(UNIVST_PLAN_ROWBIAS)) g.rowbias = h;
    if (on(UNIVST_PLAN_LN_STATS)) { g.ln_stats = arena; g.ln_wsum = arena; g.ln_bias = arena; g.ln_slots = g.K / 160; }
    if (on(UNIVST_PLAN_STATS_OUT)) g.stats_out = arena;
    if (on(UNIVST_PLAN_ACT)) g.act = 1;
    if (on(UNIVST_PLAN_GATE)) { g.gate = h; g.ld_gate = N; }
    if (on(UNIVST_PLAN_GN_OUT)) { g.gn_out = arena; g.gn_gw = 10; g.gn_G = N / 10; }
    if (on(UNIVST_PLAN_WORKSPACE)) { g.partial = arena; g.partial_bytes = UV_SPLITK_WS_BYTES; }
    if (rows_per_set > 0) { g.w_rows_per_set = rows_per_set; g.bias32 = arena; }
    return uv_gemm_plan_text(g, mode, ncu, buf, n);
}
int univst_debug_attention_plan(int BF, int heads, int Nq, int Nkv, int nsrc, int d, int q_prescaled, int flags, int phase, char* buf, int n) {
    UV_REQUIRE(buf && n > 0 && phase >= 0 && phase <= 2, "debug_attention_plan: null buffer or phase outside 0..2");
    if (Nq == 0 && Nkv == 0) {
        snprintf(buf, (size_t)n, "%s", uv_attention_plan_symbols().c_str());
        return UV_OK;
    }
    alignas(16) static float arena[8];
    half_t* const h = (half_t*)arena;
    AttnParams a;
    a.q = a.k = a.v = h; a.o = h; a.ldq = a.ldkv = a.ldo = (long)heads * d; a.src_idx = (const int*)arena;
    a.nsrc = nsrc; a.BF = BF; a.Nq = Nq; a.Nkv = Nkv; a.heads = heads; a.d = d; a.q_prescaled = q_prescaled != 0;
    if (flags & UNIVST_PLAN_SRC_LOGW) a.src_logw = arena;
    if (flags & UNIVST_PLAN_EXTRA_KEYS) { a.kx = a.vx = h; a.x_idx = (const int*)arena; a.ldkv_x = a.ldkv; a.Nkv_x = 77; }
    if (phase == 1) a.state_out = arena;
    if (phase == 2) a.state_in = arena;
    return uv_attention_plan_text(a, buf, n);
}
int univst_debug_groupnorm_plan(int C1, int C2, int64_t rows, int rows_per_stat, int G, int has_fold, int world, int has_producer_stats, int* out_ints) {
    UV_REQUIRE(out_ints, "debug_groupnorm_plan: null output");
    const GnPlan pl = uv_groupnorm_plan(C1, C2, rows, rows_per_stat, G, has_fold, world, has_producer_stats != 0);
    if (pl.rc != UV_OK) {
        uv_set_error("%s", pl.err);
        return pl.rc;
    }
    const int v[UNIVST_GN_PLAN_INTS] = {pl.route, pl.fold, pl.sharded, pl.block, pl.TR, pl.nchunk, pl.rpc, pl.nblk, pl.rpb, pl.lds_stats, pl.lds_tail,
                                        (int)pl.stats_grid[0], (int)pl.stats_grid[1], (int)pl.reduce_grid, (int)pl.tail_grid[0], (int)pl.tail_grid[1]};
    for (int i = 0; i < UNIVST_GN_PLAN_INTS; ++i) out_ints[i] = v[i];
    return UV_OK;
}
int univst_profile_enable(int on) {
    uv_prof_enable(on);
    return UV_OK;
}
int univst_profile_symbols(int cls, char* buf, int n) {
    UV_REQUIRE(buf && n > 0, "profile_symbols: null buffer");
    const std::string sy = uv_prof_symbols(cls);
    snprintf(buf, (size_t)n, "%s", sy.c_str());
    return UV_OK;
}
int univst_profile_collect(double* ms, int64_t* count, double* flops, double* bytes, int ncls) {
    UV_REQUIRE(ms && count && flops && bytes && ncls >= 1 && ncls <= 16, "profile_collect: bad arguments");
    long c[16];
    int rc = uv_prof_collect(ms, c, flops, bytes, ncls);
    for (int i = 0; i < ncls; ++i) count[i] = c[i];
    return rc;
}

int univst_profile_collect_aux(double* aux_bytes, int ncls) {
    UV_REQUIRE(aux_bytes && ncls >= 1 && ncls <= 16, "profile_collect_aux: bad arguments");
    uv_prof_aux(aux_bytes, ncls);
    return UV_OK;
}

int64_t univst_maskprop_workspace_bytes(int hw, int Nsrc, int C) { return uv_maskprop_workspace_bytes(hw, Nsrc, C); }
int univst_maskprop_frame(const float* feat_tar, const float* feat_src, const float* segs_src, float* segs_tar, int hw, int Nsrc,
                          int C, int ncls, float T, int topk, void* ws, void* s) {
    UV_REQUIRE(feat_tar && feat_src && segs_src && segs_tar && ws, "maskprop_frame: null argument");
    return uv_launch_maskprop_frame(feat_tar, feat_src, segs_src, segs_tar, hw, Nsrc, C, ncls, T, topk, ws, S(s));
}
int univst_maskprop_finalize(const float* segs, uint8_t* out, int ncls, int h, int w, int Hh, int W, void* ws, void* s) {
    UV_REQUIRE(segs && out && ws, "maskprop_finalize: null argument");
    return uv_launch_maskprop_finalize(segs, out, ncls, h, w, Hh, W, ws, S(s));
}
int univst_warp_accumulate(const uint8_t* key, const uint8_t* now, const float* fwd, const float* bwd, float* acc, int Hh, int W,
                           float thr, void* s) {
    UV_REQUIRE(key && now && fwd && bwd && acc, "warp_accumulate: null argument");
    return uv_launch_warp_accumulate(key, now, fwd, bwd, acc, Hh, W, thr, S(s));
}
int univst_warp_window_key(uint8_t* frames, const float* const* flows, int nn, int F, int Hh, int W, int key, int r, float thr, void* s) {
    UV_REQUIRE(frames, "warp_window_key: null argument");
    return uv_launch_warp_window_key(frames, flows, nn, F, Hh, W, key, r, thr, S(s));
}
int univst_latent_window_smooth(void* x0, const float* lflow, int C, int F, int h, int w, int r, float thr, void* s) {
    UV_REQUIRE(x0 && lflow, "latent_window_smooth: null argument");
    return uv_launch_latent_window_smooth(HM(x0), lflow, C, F, h, w, r, thr, S(s));
}
int univst_accumulate_u8(const uint8_t* f, float* acc, int64_t n, void* s) {
    UV_REQUIRE(f && acc, "accumulate_u8: null argument");
    return uv_launch_accumulate_u8(f, acc, n, S(s));
}
int univst_window_store(const float* acc, float weight, uint8_t* dst, int64_t n, void* s) {
    UV_REQUIRE(acc && dst && weight > 0.f, "window_store: bad argument");
    return uv_launch_window_store(acc, weight, dst, n, S(s));
}

}  // extern "C"
