// RAFT-large handle internals (see raft.hip).
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/univst.h"
#include "common.h"

struct RaftW32 {        // a checkpoint tensor as loaded: fp32 on the device
    float* ptr = nullptr;
    long n = 0;
};
struct RaftConv {       // derived fp16 weight [CoP][Kp] (k = tap * CiP + c, zero padded) + bias [CoP]
    half_t* W = nullptr;
    half_t* b = nullptr;
    int Co = 0, CoP = 0, Ci = 0, CiP = 0, taps = 0, Kp = 0;
};

struct Raft {
    std::unordered_map<std::string, RaftW32> weights;
    std::unordered_map<std::string, RaftConv> convs;
    std::vector<void*> derived;
    bool finalized = false;
    // workspace of one image size (reserve): one slab, carved once
    char* slab = nullptr;
    size_t slab_bytes = 0;
    int H = 0, W = 0;
    float* splitk = nullptr;
    half_t *col7 = nullptr, *act[4] = {nullptr, nullptr, nullptr, nullptr}, *fmap = nullptr, *ctxout = nullptr, *h16 = nullptr, *ctx16 = nullptr;
    half_t *corr16 = nullptr, *c1 = nullptr, *c2 = nullptr, *colf = nullptr, *f1 = nullptr, *motion = nullptr, *gcol = nullptr, *zr = nullptr, *qpre = nullptr;
    half_t *fh = nullptr, *delta = nullptr, *mh = nullptr, *mask = nullptr;
    float *in_part = nullptr, *in_stat = nullptr, *h32 = nullptr, *pyr = nullptr, *coords1 = nullptr;

    ~Raft();
    int load_tensor(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s);
    int finalize(hipStream_t s);
    int reserve(int H, int W);
    int encode(const uint8_t* img1, const uint8_t* img2, int H, int W, hipStream_t s);
    int gru(float* h32, half_t* h16, const half_t* ctx, const half_t* motion, int hh, int ww, hipStream_t s);
    int update(int hh, int ww, hipStream_t s);
    int forward(const uint8_t* img1, const uint8_t* img2, int H, int W, float* flow, hipStream_t s);
};

long uv_raft_pyramid_floats(int hh, int ww);
int uv_raft_corr_pyramid(const half_t* f1, const half_t* f2, int hh, int ww, float* pyr, hipStream_t s);
int uv_raft_corr_lookup(const float* pyr, const float* coords, int hh, int ww, float* out32, half_t* out16, hipStream_t s);
int uv_raft_convex_upsample(const float* flow, int is_coords, const half_t* mask, int hh, int ww, float* out, hipStream_t s);
