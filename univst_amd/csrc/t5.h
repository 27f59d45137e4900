// T5 encoder handle internals (see t5.hip).
#pragma once
#include <string>
#include <vector>

#include "../../include/univst.h"
#include "model.h"

constexpr int UV_T5_MAX_S = 512;                       // the bias table spans deltas -(511) .. 511
constexpr int UV_T5_BIAS_W = 2 * UV_T5_MAX_S - 1;      // entries per head: [heads][delta + 511]

struct T5Layer {      // the weights of one encoder block, looked up once by finalize
    const half_t *ln1_g, *qkv_w, *o_w, *ln2_g, *wi_w, *wo_w;
};

struct T5 : Model {
    univst_t5_cfg cfg;
    std::vector<T5Layer> layers;
    const half_t *embed = nullptr, *fln_g = nullptr;
    const float* bias_table = nullptr;      // [heads][UV_T5_BIAS_W] fp32, derived from block 0's relative_attention_bias
    // activations of one (B, S), carved from the arena by the first encode at that size
    int rB = 0, rS = 0;
    float* x = nullptr;                     // the fp32 residual stream [B*S, d_model]
    half_t *h = nullptr, *qkv = nullptr, *att = nullptr, *y = nullptr, *ff2 = nullptr, *ff = nullptr;
    float* splitk = nullptr;
    size_t splitk_bytes = 0;

    T5() : Model("t5") {}
    int load_tensor(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s);
    int finalize(hipStream_t s);
    int reserve(int B, int S);
    int encode(const int64_t* ids, int B, int S, half_t* last_hidden, hipStream_t s);
};

int uv_t5_check_cfg(const univst_t5_cfg& c);
// transformers' T5Attention._relative_position_bucket (bidirectional) for the deltas -(n-1) .. n-1 (memory position - query position): plain host code
int uv_t5_bucket_table(int num_buckets, int max_distance, int n, int* out);
// bidirectional self-attention of the fused q|k|v rows [B*S, 3*heads*64] (no 1/sqrt(d) scaling) with the additive bias
// bias_table[head][(j - i) + 511] -> out [B*S, heads*64]
int uv_launch_t5_attention(const half_t* qkv, const float* bias_table, int B, int S, int heads, half_t* out, hipStream_t s);
