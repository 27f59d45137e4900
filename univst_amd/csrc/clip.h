// CLIP text-tower handle internals (see clip.hip).
#pragma once
#include <string>
#include <vector>

#include "../../include/univst.h"
#include "model.h"

constexpr int UV_CLIP_MAX_S = 80;      // five 16-row tiles: the attention kernel keeps a whole head in LDS

struct ClipLayer {      // the weights of one encoder layer, looked up once by finalize
    const half_t *ln1_g, *ln1_b, *qkv_w, *qkv_b, *out_w, *out_b, *ln2_g, *ln2_b, *fc1_w, *fc1_b, *fc2_w, *fc2_b;
};

struct Clip : Model {
    univst_clip_cfg cfg;
    std::vector<ClipLayer> layers;
    const half_t *tok = nullptr, *pos = nullptr, *fln_g = nullptr, *fln_b = nullptr, *proj = nullptr;
    // activations of one (B, S), carved from the arena by the first encode at that size
    int rB = 0, rS = 0;
    half_t *x[2] = {nullptr, nullptr}, *h = nullptr, *qkv = nullptr, *att = nullptr, *mid = nullptr, *ff = nullptr, *last = nullptr, *prow = nullptr;
    float* splitk = nullptr;
    size_t splitk_bytes = 0;

    Clip() : Model("clip") {}
    int load_tensor(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s);
    int finalize(hipStream_t s);
    int reserve(int B, int S);
    int encode(const int64_t* ids, int B, int S, half_t* last_hidden, half_t* hidden_states, half_t* pooled, hipStream_t s);
};

int uv_clip_check_cfg(const univst_clip_cfg& c);
// causal self-attention of the fused q|k|v rows [B*S, 3*heads*64] (q already carries 1/8) -> out [B*S, heads*64]
int uv_launch_clip_attention(const half_t* qkv, int B, int S, int heads, half_t* out, hipStream_t s);
