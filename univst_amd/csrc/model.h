// Plumbing shared by the model handles (model.hip): the fp16 weight store with its derived layouts, the activation arena, the weight-preparation
// kernels, and Model — the base of every fp16 handle (Clip, T5, Motion, Vae / KlVae, UNet): store + owned arena slab + finalized flag, load_tensor,
// weight_bytes, the shape-checked weight lookup of finalize (shaped / UV_SHAPED) and the fixed-buffer arena carve of reserve (carve).  raft.hip keeps
// its fp32 store and takes nb() and the slab helper only.  Nothing here needs the GEMM: model.hip links with tools/arena_check.cpp alone.
#pragma once
#include <initializer_list>
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
    // derives `k` as the row-wise concatenation of equally shaped blocks [rows, cols] (cols = 0: vectors of `rows` elements: biases), the FIRST one
    // multiplied by `scale0` unless that is 1 (an attention scale riding on the q rows): the fused q|k|v, k|v and wi_0|wi_1 operands of the handles
    int derive_concat(const std::string& k, std::initializer_list<const half_t*> blocks, long rows, long cols, hipStream_t s, float scale0 = 1.f,
                      const half_t** out = nullptr);
    void clear_derived();
};

// What the fp16 handles share on top of the store.  `who` names the handle in messages ("clip": "clip_finalize: ...", "clip: weight ... was never
// loaded", and the carve's message when the arena cannot hold the list).
struct Model : WeightStore {
    const char* const who;
    Arena arena;                   // the slab is the handle's: freed by ~Model (Arena itself owns nothing: tools/arena_check.cpp points it at host memory)
    bool finalized = false;

    explicit Model(const char* who_) : who(who_) {}
    ~Model();
    int load_tensor(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s);      // load() + finalized = false
    double weight_bytes() const;                                                                                         // loaded + derived tensors
    // finalize's lookup: the tensor of that key when its shape is `want`; else null with the missing key recorded or the shape error set (shaped_error)
    const half_t* shaped(const std::string& key, std::initializer_list<long> want);
    int shaped_error() const;
    // reserve's carve for a fixed list of buffers: the slab holds the aligned sizes of that list + 4096, *dst are allocated in list order (0 bytes: null)
    struct Buf {
        void** dst;
        size_t bytes;
        template <class T>
        Buf(T** d, size_t b) : dst(reinterpret_cast<void**>(d)), bytes(b) {}
    };
    int carve(std::initializer_list<Buf> bufs);
};
// dst = shaped(key, {dims...}), or return the error from the handle's finalize
#define UV_SHAPED(dst, key, ...)                 \
    do {                                         \
        (dst) = shaped((key), {__VA_ARGS__});    \
        if (!(dst)) return shaped_error();       \
    } while (0)

// conv weight [Co][Ci][taps...] -> "key#nhwc" [Co][taps][CiP] (input channels zero padded to 8) and, where taps == 9 && Ci % 64 == 0,
// the tap-inner "key#ti" [Co][Ci/64][9][64] (GemmParams::korder = 1)
int uv_derive_conv_layouts(WeightStore& st, const std::string& key, hipStream_t s);
// out[i] = fp16(in[i] * f)
int uv_launch_scale_f16(const half_t* in, half_t* out, long n, float f, hipStream_t s);
// GEGLU row interleave of the `geglu = 1` epilogue (16 value rows, then their 16 gate rows): out row (32q + j) = in row (16q + j), out row
// (32q + 16 + j) = in row (rows / 2 + 16q + j); rows a multiple of 32
int uv_launch_geglu_interleave(const half_t* in, half_t* out, int rows, int cols, hipStream_t s);
// [Wp W2 | Wp] and Wp (b2 + tb) + bp: two chained linears with a residual in between as ONE linear over K2 + C columns (include/univst.h univst_linear_compose)
int uv_launch_linear_compose(const half_t* Wp, const half_t* W2, const half_t* b2, const half_t* tb, const half_t* bp, int C, int K2, half_t* W_out,
                             half_t* bias_out, hipStream_t s);
