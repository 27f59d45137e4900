// Plumbing shared by the model handles (unet.hip, vae.hip; raft.hip takes nb() and the slab helper only): the fp16 weight store with its
// derived layouts, the activation arena and the weight-preparation kernels (model.hip).
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "common.h"

inline unsigned nb(long n) { return (unsigned)((n + 255) / 256); }      // blocks of 256 threads over n elements

struct WTensor {
    half_t* ptr = nullptr;
    std::vector<long> shape;
};

struct Act {   // NHWC activation: [imgs, H, W, C] fp16
    half_t* p = nullptr;
    int imgs = 0, H = 0, W = 0, C = 0;
    const float* gst = nullptr;      // GroupNorm (sum, sumsq) per 16-row fragment and 10-channel sub-group, left by the producing conv / linear's epilogue ([C/10][rows/16][2]) or null
    long rows() const { return (long)imgs * H * W; }
};

// a device slab of at least `need` bytes: one that is too small is replaced after a device synchronise (its contents are lost)
int uv_slab_grow(char** base, size_t* size, size_t need);

struct Arena {   // first-fit allocator over one device slab; stream-ordered reuse
    struct Block {
        size_t off, size;
        bool free;
    };
    char* base = nullptr;
    size_t size = 0, high_water = 0;
    std::vector<Block> blocks;
    void* alloc(size_t bytes);
    void release(void* p);
    void reset();
    int ensure(size_t bytes);      // uv_slab_grow + reset
};

// device fp16 copies of a checkpoint's tensors keyed by their state-dict names, plus the layouts finalize() derives from them ("key#layout")
struct WeightStore {
    std::unordered_map<std::string, WTensor> weights, derived;
    std::string missing;           // the first key W() did not find since clear_missing()

    ~WeightStore();
    int load(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s);
    const WTensor* find(const std::string& k) const;
    half_t* W(const std::string& k);
    void clear_missing() { missing.clear(); }
    int missing_error(const char* who) const;
    int derive(const std::string& k, std::vector<long> shape, half_t** out);      // replaces a derived tensor of that key
    void clear_derived();
};

// conv weight [Co][Ci][taps...] -> "key#nhwc" [Co][taps][CiP] (input channels zero padded to 8) and, where taps == 9 && Ci % 64 == 0,
// the tap-inner "key#ti" [Co][Ci/64][9][64] (GemmParams::korder = 1)
int uv_derive_conv_layouts(WeightStore& st, const std::string& key, hipStream_t s);
// out[i] = fp16(in[i] * f)
int uv_launch_scale_f16(const half_t* in, half_t* out, long n, float f, hipStream_t s);
// [Wp W2 | Wp] and Wp (b2 + tb) + bp: two chained linears with a residual in between as ONE linear over K2 + C columns (include/univst.h univst_linear_compose)
int uv_launch_linear_compose(const half_t* Wp, const half_t* W2, const half_t* b2, const half_t* tb, const half_t* bp, int C, int K2, half_t* W_out,
                             half_t* bias_out, hipStream_t s);
