// The handle plumbing the model graphs share (model.h): weight store, activation arena, the Model base, weight-preparation kernels.  All of it runs at load,
// finalize and reserve time, or as a hash lookup in front of a launch; nothing here is on the per-step path.
#include "model.h"

#include "../../include/univst.h"

namespace {

__global__ void convert_f32_f16_kernel(const float* __restrict__ in, half_t* __restrict__ out, long n) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (half_t)in[i];
}
// [Co][Ci][taps] -> [Co][taps][CiP] (zero padded input channels): 2-D convs (taps = kh*kw) and Conv3d (3,1,1) (taps = 3) alike
__global__ void permute_conv_weight_kernel(const half_t* __restrict__ in, half_t* __restrict__ out, int Co, int Ci, int taps, int CiP) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)Co * taps * CiP) return;
    const int c = (int)(i % CiP), t = (int)((i / CiP) % taps), o = (int)(i / ((long)CiP * taps));
    out[i] = c < Ci ? in[((long)o * Ci + c) * taps + t] : (half_t)0.f;
}
// [Co][Ci][3][3] -> tap-inner [Co][Ci/64][9][64] (GemmParams::korder = 1: the nine taps of a 64-channel slab are consecutive k tiles)
__global__ void permute_conv_weight_ti_kernel(const half_t* __restrict__ in, half_t* __restrict__ out, int Co, int Ci) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)Co * Ci * 9) return;
    const int j = (int)(i % 64), t = (int)((i / 64) % 9), q = (int)((i / (64 * 9)) % (Ci / 64)), o = (int)(i / ((long)Ci * 9));
    out[i] = in[((long)o * Ci + q * 64 + j) * 9 + t];
}
__global__ void scale_f16_kernel(const half_t* __restrict__ in, half_t* __restrict__ out, long n, float f) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = (half_t)((float)in[i] * f);
}
__global__ void geglu_interleave_kernel(const half_t* __restrict__ in, half_t* __restrict__ out, int rows, int cols) {
    long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)rows * cols) return;
    int c = (int)(i % cols), r = (int)(i / cols);
    int q = r / 32, j = r % 32;
    int src = j < 16 ? 16 * q + j : rows / 2 + 16 * q + (j - 16);
    out[i] = in[(long)src * cols + c];
}

// Two chained linears composed into one (uv_launch_linear_compose): out[n][k] = sum_j Wp[n][j] W2[j][k] for k < K2, Wp[n][k - K2] for the C columns behind
// them, and (column K2 + C of the grid) the bias Wp (b2 + tb) + bp.  fp32 accumulation in j order, one fp16 rounding.  Runs once per handle: plain FMAs,
// consecutive threads on consecutive k (W2 rows read coalesced, the Wp element is a broadcast).
__global__ void linear_compose_kernel(const half_t* __restrict__ Wp, const half_t* __restrict__ W2, const half_t* __restrict__ b2, const half_t* __restrict__ tb,
                                      const half_t* __restrict__ bp, int C, int K2, half_t* __restrict__ Wout, half_t* __restrict__ bout) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x, n = blockIdx.y;
    const half_t* wp = Wp + (long)n * C;
    if (k < K2) {
        float acc = 0.f;
        for (int j = 0; j < C; ++j) acc = fmaf((float)wp[j], (float)W2[(long)j * K2 + k], acc);
        Wout[(long)n * (K2 + C) + k] = (half_t)acc;
    } else if (k < K2 + C) {
        Wout[(long)n * (K2 + C) + k] = wp[k - K2];
    } else if (k == K2 + C) {
        float acc = 0.f;
        for (int j = 0; j < C; ++j) acc = fmaf((float)wp[j], (float)b2[j] + (tb ? (float)tb[j] : 0.f), acc);
        bout[n] = (half_t)(acc + (float)bp[n]);
    }
}

}  // namespace

// ------------------------------------------------------------------------------------------ arena
int uv_slab_grow(char** base, size_t* size, size_t need) {
    if (*size >= need) return UV_OK;
    UV_HIP(hipDeviceSynchronize());
    if (*base) UV_HIP(hipFree(*base));
    *base = nullptr;
    *size = 0;
    UV_HIP(hipMalloc((void**)base, need));
    *size = need;
    return UV_OK;
}

void* Arena::alloc(size_t bytes) {
    bytes = (bytes + 255) & ~size_t(255);
    for (size_t i = 0; i < blocks.size(); ++i) {
        if (blocks[i].free && blocks[i].size >= bytes) {
            if (blocks[i].size > bytes) {
                Block rest{blocks[i].off + bytes, blocks[i].size - bytes, true};
                blocks[i].size = bytes;
                blocks.insert(blocks.begin() + i + 1, rest);
            }
            blocks[i].free = false;
            size_t used = blocks[i].off + bytes;
            if (used > high_water) high_water = used;
            return base + blocks[i].off;
        }
    }
    return nullptr;
}
void Arena::release(void* p) {
    if (!p) return;
    size_t off = (char*)p - base;
    for (size_t i = 0; i < blocks.size(); ++i) {
        if (blocks[i].off == off && !blocks[i].free) {
            blocks[i].free = true;
            if (i + 1 < blocks.size() && blocks[i + 1].free) {
                blocks[i].size += blocks[i + 1].size;
                blocks.erase(blocks.begin() + i + 1);
            }
            if (i > 0 && blocks[i - 1].free) {
                blocks[i - 1].size += blocks[i].size;
                blocks.erase(blocks.begin() + i);
            }
            return;
        }
    }
}
void Arena::reset() {
    blocks.clear();
    blocks.push_back(Block{0, size, true});
}
int Arena::ensure(size_t bytes) {
    UV_RUN(uv_slab_grow(&base, &size, bytes));
    reset();
    return UV_OK;
}

// ------------------------------------------------------------------------------------------ weight store
WeightStore::~WeightStore() {
    for (auto& kv : weights) (void)hipFree(kv.second.ptr);
    clear_derived();
}

int WeightStore::load(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s) {
    UV_REQUIRE(key && dev_ptr && ndim >= 1 && ndim <= 5, "load_tensor: bad arguments");
    UV_REQUIRE(dtype == UNIVST_F16 || dtype == UNIVST_F32, "load_tensor(%s): dtype %d unsupported", key, dtype);
    long n = 1;
    WTensor t;
    for (int i = 0; i < ndim; ++i) {
        n *= shape[i];
        t.shape.push_back(shape[i]);
    }
    UV_REQUIRE(n > 0, "load_tensor(%s): empty tensor", key);
    UV_HIP(hipMalloc((void**)&t.ptr, (size_t)n * sizeof(half_t)));
    if (dtype == UNIVST_F16) UV_HIP(hipMemcpyAsync(t.ptr, dev_ptr, (size_t)n * sizeof(half_t), hipMemcpyDeviceToDevice, s));
    else hipLaunchKernelGGL(convert_f32_f16_kernel, dim3(nb(n)), dim3(256), 0, s, (const float*)dev_ptr, t.ptr, n);
    UV_LAUNCH_CHECK();
    auto it = weights.find(key);
    if (it != weights.end()) {      // (work queued on s may still read the tensor this one replaces)
        UV_HIP(hipStreamSynchronize(s));
        (void)hipFree(it->second.ptr);
    }
    weights[key] = t;
    return UV_OK;
}

const WTensor* WeightStore::find(const std::string& k) const {
    auto it = weights.find(k);
    if (it != weights.end()) return &it->second;
    auto jt = derived.find(k);
    return jt == derived.end() ? nullptr : &jt->second;
}

half_t* WeightStore::W(const std::string& k) {
    const WTensor* t = find(k);
    if (!t) {
        if (missing.empty()) missing = k;
        return nullptr;
    }
    return t->ptr;
}

int WeightStore::missing_error(const char* who) const {
    uv_set_error("%s: weight '%s' was never loaded", who, missing.c_str());
    return UV_ERR_STATE;
}

int WeightStore::derive(const std::string& k, std::vector<long> shape, half_t** out) {
    auto it = derived.find(k);
    if (it != derived.end()) {
        (void)hipFree(it->second.ptr);
        derived.erase(it);
    }
    long n = 1;
    for (long v : shape) n *= v;
    WTensor t;
    t.shape = shape;
    UV_HIP(hipMalloc((void**)&t.ptr, (size_t)n * sizeof(half_t)));
    derived[k] = t;
    *out = t.ptr;
    return UV_OK;
}

int WeightStore::derive_concat(const std::string& k, std::initializer_list<const half_t*> blocks, long rows, long cols, hipStream_t s, float scale0,
                               const half_t** out) {
    const long nblk = (long)blocks.size(), n = rows * (cols ? cols : 1);
    half_t* d;
    UV_RUN(cols ? derive(k, {nblk * rows, cols}, &d) : derive(k, {nblk * rows}, &d));
    long i = 0;
    for (const half_t* src : blocks) {
        if (i == 0 && scale0 != 1.f) UV_RUN(uv_launch_scale_f16(src, d, n, scale0, s));
        else UV_HIP(hipMemcpyAsync(d + i * n, src, (size_t)n * sizeof(half_t), hipMemcpyDeviceToDevice, s));
        ++i;
    }
    if (out) *out = d;
    return UV_OK;
}

void WeightStore::clear_derived() {
    for (auto& kv : derived) (void)hipFree(kv.second.ptr);
    derived.clear();
}

// ------------------------------------------------------------------------------------------ what the fp16 handles share
Model::~Model() {
    if (arena.base) (void)hipFree(arena.base);
}

int Model::load_tensor(const char* key, const void* dev_ptr, int dtype, const int64_t* shape, int ndim, hipStream_t s) {
    UV_RUN(load(key, dev_ptr, dtype, shape, ndim, s));
    finalized = false;
    return UV_OK;
}

double Model::weight_bytes() const {
    double n = 0;
    for (const auto* m : {&weights, &derived})
        for (const auto& kv : *m) {
            double e = 1;
            for (long v : kv.second.shape) e *= (double)v;
            n += e * sizeof(half_t);
        }
    return n;
}

const half_t* Model::shaped(const std::string& key, std::initializer_list<long> want) {
    const WTensor* t = find(key);
    if (!t) {
        (void)W(key);      // records the missing key
        return nullptr;
    }
    if (t->shape != std::vector<long>(want)) {
        uv_set_error("%s_finalize: %s has %zu dims / first dim %ld, which the config does not give", who, key.c_str(), t->shape.size(), t->shape[0]);
        return nullptr;
    }
    return t->ptr;
}

int Model::shaped_error() const { return missing.empty() ? UV_ERR_ARG : missing_error(who); }

int Model::carve(std::initializer_list<Buf> bufs) {
    size_t need = 4096;
    for (const Buf& b : bufs) need += (b.bytes + 255) & ~size_t(255);
    UV_RUN(arena.ensure(need));
    for (const Buf& b : bufs) {
        *b.dst = b.bytes ? arena.alloc(b.bytes) : nullptr;
        if (b.bytes && !*b.dst) {
            uv_set_error("%s: activation arena exhausted (%zu bytes)", who, arena.size);
            return UV_ERR_STATE;
        }
    }
    return UV_OK;
}

// ------------------------------------------------------------------------------------------ weight preparation
int uv_derive_conv_layouts(WeightStore& st, const std::string& key, hipStream_t s) {
    const WTensor* t = st.find(key);
    UV_REQUIRE(t && t->shape.size() >= 3, "%s: not a loaded conv weight", key.c_str());
    const int Co = (int)t->shape[0], Ci = (int)t->shape[1], CiP = (Ci + 7) / 8 * 8;
    int taps = 1;
    for (size_t d = 2; d < t->shape.size(); ++d) taps *= (int)t->shape[d];
    half_t* d;
    UV_RUN(st.derive(key + "#nhwc", {Co, taps, CiP}, &d));
    hipLaunchKernelGGL(permute_conv_weight_kernel, dim3(nb((long)Co * taps * CiP)), dim3(256), 0, s, t->ptr, d, Co, Ci, taps, CiP);
    if (taps == 9 && Ci % 64 == 0) {
        UV_RUN(st.derive(key + "#ti", {Co, Ci / 64, 9, 64}, &d));
        hipLaunchKernelGGL(permute_conv_weight_ti_kernel, dim3(nb((long)Co * Ci * 9)), dim3(256), 0, s, t->ptr, d, Co, Ci);
    }
    UV_LAUNCH_CHECK();
    return UV_OK;
}

int uv_launch_scale_f16(const half_t* in, half_t* out, long n, float f, hipStream_t s) {
    hipLaunchKernelGGL(scale_f16_kernel, dim3(nb(n)), dim3(256), 0, s, in, out, n, f);
    UV_LAUNCH_CHECK();
    return UV_OK;
}

int uv_launch_geglu_interleave(const half_t* in, half_t* out, int rows, int cols, hipStream_t s) {
    hipLaunchKernelGGL(geglu_interleave_kernel, dim3(nb((long)rows * cols)), dim3(256), 0, s, in, out, rows, cols);
    UV_LAUNCH_CHECK();
    return UV_OK;
}

int uv_launch_linear_compose(const half_t* Wp, const half_t* W2, const half_t* b2, const half_t* tb, const half_t* bp, int C, int K2, half_t* W_out,
                             half_t* bias_out, hipStream_t s) {
    UV_REQUIRE(Wp && W2 && b2 && bp && W_out && bias_out && C > 0 && K2 > 0 && C % 8 == 0 && K2 % 8 == 0 && C <= 65535,
               "linear_compose: null argument, or C=%d / K2=%d not a positive multiple of 8, or C above 65535 (one grid row per output row)", C, K2);
    hipLaunchKernelGGL(linear_compose_kernel, dim3((unsigned)((K2 + C + 1 + 255) / 256), (unsigned)C), dim3(256), 0, s, Wp, W2, b2, tb, bp, C, K2, W_out, bias_out);
    UV_LAUNCH_CHECK();
    return UV_OK;
}
