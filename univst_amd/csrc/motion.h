// AnimateDiff motion-module handle internals and the frame-axis attention launcher (see motion.hip).  A Motion is a handle of its own
// (univst_motion_*) or one of the modules an AnimateDiff UNet handle owns (unet.h UNet::motions).
#pragma once
#include <string>
#include <vector>

#include "../../include/univst.h"
#include "model.h"

constexpr int UV_MOTION_MAX_F = 32;      // two 16-frame tiles: all scores of a (pixel, head) stay in one wave's registers

struct MotionAttn {       // one Temporal_Self attention: LayerNorm, fused q|k|v (no bias), position rows already projected, out projection
    const half_t *ln_g, *ln_b, *qkv_w, *pe_qkv, *out_w, *out_b;
};
struct MotionBlock {      // one TemporalTransformerBlock, looked up once by finalize
    std::vector<MotionAttn> attn;
    const half_t *ffn_g, *ffn_b, *ff1_w, *ff1_b, *ff2_w, *ff2_b;
};

struct MotionBufs {       // the activations of one chain run, supplied by whoever owns the memory (Motion::reserve, or the UNet graph's arena)
    half_t *x[2] = {nullptr, nullptr};      // [M, C] each: the residual stream, ping-pong
    half_t *h = nullptr;                    // [M, C]: normalised rows
    half_t *att = nullptr;                  // [M, C]: attention output (may alias h: the q|k|v projection has consumed h by then)
    half_t *qkv = nullptr;                  // [M, 3C]
    half_t *ff = nullptr;                   // [M, 4C] (may alias qkv: the two are never live together)
    float *gn_ws = nullptr, *splitk = nullptr;
    size_t splitk_bytes = 0;
};

struct Motion : Model {
    univst_motion_cfg cfg;
    std::vector<MotionBlock> blocks;
    const half_t *gn_g = nullptr, *gn_b = nullptr, *in_w = nullptr, *in_b = nullptr, *outp_w = nullptr, *outp_b = nullptr;
    // activations of one (B, F, N), carved from the arena by the first forward at that size
    int rB = 0, rF = 0, rN = 0;
    half_t *x[2] = {nullptr, nullptr}, *h = nullptr, *qkv = nullptr, *att = nullptr, *ff = nullptr;
    float *gn_ws = nullptr, *splitk = nullptr;
    size_t splitk_bytes = 0;

    Motion() : Model("motion") {}
    int finalize(hipStream_t s);
    int reserve(int B, int F, int N);
    int forward(const half_t* X, half_t* Y, int B, int F, int N, hipStream_t s);
    // the chain of forward() over caller-supplied buffers (who: the entry point named in messages); no allocation, no synchronisation
    int check_shape(const char* who, int B, int F, int N) const;
    int run(const half_t* X, half_t* Y, int B, int F, int N, const MotionBufs& b, hipStream_t s);
};

int uv_motion_check_cfg(const univst_motion_cfg& c);
// softmax attention along the frame axis of the fused q|k|v rows (row (b F + f) N + n, q already scaled): see univst_temporal_attention
int uv_launch_temporal_attention(const half_t* qkv, long ldx, const half_t* pe_qkv, int B, int F, int N, int heads, int head_dim, half_t* out, long ldo,
                                 hipStream_t s);
