// Internal helpers shared by the libgnnmp kernels (gfx950 / CDNA4 only).
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/gnnmp.h"

#define GMP_WAVE 64
#define GMP_MAX_GROUPS 24

namespace gmp {

// thread-local last-error text, read through gmp_last_error_string()
char* err_buf();
int fail(int code, const char* fmt, ...);

// The next gmp_gemm_f32 / gmp_gemm_f32_grouped launch made by this host thread stores `value` to *flag when its first workgroup
// starts (a cross-stream gate opened by the GEMM that follows the producer anyway, instead of by a launch of its own).  A GEMM
// call that returns without launching leaves the signal pending: the caller checks signal_pending() and opens the gate itself.
void signal_on_next_gemm(int32_t* flag, int value);
bool signal_pending();

// gmp_gemm_f32 with an affine epilogue (GMP_GEMM_NT only): C = act(((alpha A B^T + bias) + resid) * scale + shift), in that order; scale and
// shift [N] (both or neither), resid [M, N] with leading dimension ldr; all three NULL = gmp_gemm_f32.  Same dispatch, same accumulation order.
int gemm_f32_epilogue(int mode, const float* A, const float* B, const float* bias, float* C, int64_t M, int64_t N, int64_t K, int64_t lda,
                      int64_t ldb, int64_t ldc, float alpha, int accumulate, int relu, const float* scale, const float* shift,
                      const float* resid, int64_t ldr, void* workspace, size_t workspace_bytes, gmp_stream_t stream);

// The step's link-prediction head may take gmp_lp_feat_gemm_bwd_fold in place of gmp_gemm_f32 (NN) + gmp_lp_edge_features_bwd: true where that
// GEMM would run on the pipelined kernel (same accumulation order, so the same bits) and every operand is 16-byte addressable.
bool lp_fold_applies(const float* gy1, const float* w0, const float* h, const float* g_hs, const float* g_hd, int64_t K, int F);

// Likewise gmp_lp_feat_gemm_fwd / gmp_lp_feat_gemm_wgrad in place of gmp_lp_edge_features_fwd + the NT GEMM and of the grouped TN GEMM over lp_feat:
// true where both materialised GEMMs would run the pipelined kernel (the weight-gradient one needs a workspace for that).
bool lp_feat_gemm_applies(const float* h, const float* w0, const float* b0, const float* y1, const float* gy1, const float* dW0,
                          const void* workspace, int64_t K, int F);

// Two-lane enqueue (step.hip): the pre-training step's launch sequence is walked by TWO host threads at once -- the caller takes the main
// stream's launches, a worker thread everything else -- because one thread needs ~4 us per launch and a step has ~250 (the launcher was the
// limiter on slower hosts; two threads launching on different streams scale 1.7x on this runtime, scripts/probe_two_threads.hip).  Both
// threads run the SAME code; a launch (kernel, async memset / copy) on a stream the thread does not take is skipped, here, below every
// gmp_* entry point.  Thread-local; 0 = take everything (every caller outside the step executor).
enum { LANE_ALL = 0, LANE_ONLY = 1, LANE_ALL_BUT = 2 };
int& lane_mode();
hipStream_t& lane_stream();
inline bool lane_takes(hipStream_t st) {
    const int m = lane_mode();
    return m == LANE_ALL || ((m == LANE_ONLY) == (st == lane_stream()));
}

inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return fail(GMP_ERR_LAUNCH, "%s: %s", what, hipGetErrorString(e));
    return GMP_OK;
}

inline int cdiv(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) belongs to the DEVICE's copy of a function: a launcher keeps one "done" bit per device
// ordinal (std::atomic<uint64_t>, function-local static) instead of a process-wide bool -- a process driving a second GPU would otherwise
// skip the call there and fail to launch its > 64 KiB tiles.  Racing threads at worst both make the (idempotent) call; ordinals >= 64 repeat it.
inline int cur_device() { int d = 0; (void)hipGetDevice(&d); return d; }
inline bool lds_attr_done(const std::atomic<uint64_t>& m) { const int d = cur_device(); return d < 64 && ((m.load(std::memory_order_acquire) >> d) & 1ull); }
inline void lds_attr_mark(std::atomic<uint64_t>& m) { const int d = cur_device(); if (d < 64) m.fetch_or(1ull << d, std::memory_order_release); }
// more than 64 KiB of dynamic LDS for `kernel`: the opt-in, made once per device
inline int reserve_lds(std::atomic<uint64_t>& done, const void* kernel, int bytes, const char* who) {
    if (lds_attr_done(done)) return GMP_OK;
    if (hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes) != hipSuccess)
        return fail(GMP_ERR_LAUNCH, "%s: cannot reserve %d bytes of LDS", who, bytes);
    lds_attr_mark(done);
    return GMP_OK;
}

// ---- Philox4x32-10 (counter-based RNG for dropout; mask is regenerated in the
// backward pass from (seed, stream, element) instead of being stored) ----------
__device__ __forceinline__ uint4 philox4x32(uint4 ctr, uint2 key) {
    const uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        // one 32 x 32 -> 64 multiply per product (v_mad_u64_u32): written as __umulhi + a 32-bit product hipcc issued TWO quarter-rate multiplies
        // each -- 308 of them per thread in the BatchNorm forward that draws a mask for eight float4 (round 3)
        const uint64_t p0 = (uint64_t)M0 * ctr.x, p1 = (uint64_t)M1 * ctr.z;
        const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0, hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
        ctr = make_uint4(hi1 ^ ctr.y ^ key.x, lo1, hi0 ^ ctr.w ^ key.y, lo0);
        key.x += W0;
        key.y += W1;
    }
    return ctr;
}

// keep-mask for 4 consecutive elements starting at element index 4*q of dropout
// stream `stream`; returns the multiplier (0 or 1/(1-p)) per element.
__device__ __forceinline__ float4 dropout_scale4(uint64_t seed, uint32_t stream, uint64_t q, float p, float inv_keep) {
    uint4 r = philox4x32(make_uint4((uint32_t)q, (uint32_t)(q >> 32), stream, 0x6d70u),
                         make_uint2((uint32_t)seed, (uint32_t)(seed >> 32)));
    // u = r * 2^-32 in [0,1); keep iff u >= p
    const float s = 2.3283064365386963e-10f;
    float4 o;
    o.x = ((float)r.x * s >= p) ? inv_keep : 0.f;
    o.y = ((float)r.y * s >= p) ? inv_keep : 0.f;
    o.z = ((float)r.z * s >= p) ? inv_keep : 0.f;
    o.w = ((float)r.w * s >= p) ? inv_keep : 0.f;
    return o;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// one wave's row: dst[0, d) = src / max(||src||, eps), zeros up to dpad (F.normalize, eps = 1e-12); the clamped norm to *norm if given
__device__ __forceinline__ void normalize_row(const float* __restrict__ src, int d, float* __restrict__ dst, int dpad, float* __restrict__ norm) {
    const int lane = threadIdx.x % 64;
    float s = 0.f;
    for (int c = lane; c < d; c += 64) s += src[c] * src[c];
    s = wave_sum(s);
    const float nr = fmaxf(sqrtf(s), 1e-12f);
    for (int c = lane; c < dpad; c += 64) dst[c] = c < d ? src[c] / nr : 0.f;
    if (norm && lane == 0) *norm = nr;
}

// out[0] = sum of v[0, n) in a fixed order, one workgroup (ntxent.hip)
void sum_rows(const float* v, int64_t n, float* out, hipStream_t st);

// out[r] = sum over e in [ptr[r], ptr[r + 1]) of src[idx[e]] in ascending e, rows of `feat` floats (a multiple of 4): aggregate.hip's
// seg_sum_kernel (one wave per output row, a fixed fp32 order).  Every workgroup first loads *gate and returns when it is 0: the
// k-means loop's early exit (kmeans.hip).
int seg_sum_gated(const float* src, const int* ptr, const int* idx, float* out, int64_t nrows, int feat, const int* gate, hipStream_t st);

// C/D layout of the 32x32 MFMAs: the lane holds column lane & 31, register r of lane half `half` (lane >> 5) holds this row of a tile
// whose first row is `row0` (summed from the left, in row0's type: the address arithmetic the kernels were tuned with)
typedef float f32x16 __attribute__((ext_vector_type(16)));
template <typename T = int>
__device__ __forceinline__ T acc_row(int r, int half, T row0 = 0) { return row0 + (r & 3) + 8 * (r >> 2) + 4 * half; }

// float bits as an unsigned that orders like the float (radix select keys), and back
__device__ __forceinline__ uint32_t orderable(float v) {
    uint32_t u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float from_orderable(uint32_t u) {
    return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}

// 64-bit selection key: the orderable score bits (high word), then `low`, which every caller passes as 0xffffffff - index: a greater key is
// a higher score, then a lower index.  And back: the index behind the low word, the score.
typedef unsigned long long u64;
__device__ __forceinline__ u64 pack_key(float v, uint32_t low) { return ((u64)orderable(v) << 32) | (u64)low; }
__device__ __forceinline__ uint32_t key_low(u64 key) { return 0xffffffffu - (uint32_t)key; }
__device__ __forceinline__ float key_score(u64 key) { return from_orderable((uint32_t)(key >> 32)); }

// the wave's earlier LDS writes are visible to its later reads: all that data private to one wave needs
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the byte ranges [a, a + a_bytes) and [b, b + b_bytes) meet (a null pointer and an empty range meet nothing)
inline bool overlap(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
    return a && b && a_bytes && b_bytes && x < y + b_bytes && y < x + a_bytes;
}

// workspace slices start on 256 bytes
inline size_t al(size_t x) { return (x + 255) & ~(size_t)255; }

// A workspace handed out slice by slice.  `align` moves the base up to the next 256 bytes and counts those 256 in total(); carving a
// null base gives the size to ask for.
class Carver {
    char *base, *q;
    bool align;
public:
    Carver(void* ws, bool align) : base(align ? (char*)(((uintptr_t)ws + 255) / 256 * 256) : (char*)ws), q(base), align(align) {}
    template <typename T>
    T* take(size_t count) {
        T* p = (T*)q;
        q += al(count * sizeof(T));
        return p;
    }
    size_t total() const { return (size_t)(q - base) + (align ? 256 : 0); }
};

}  // namespace gmp


// every launch of the library goes through the lane filter (see gmp::lane_takes)
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernelName, numBlocks, numThreads, memPerBlock, streamId, ...)                                        \
    do {                                                                                                                         \
        if (gmp::lane_takes((hipStream_t)(streamId))) hipLaunchKernelGGLInternal((kernelName), (numBlocks), (numThreads), (memPerBlock), (streamId), __VA_ARGS__); \
    } while (0)
#define hipMemsetAsync(dst, value, bytes, stream) (gmp::lane_takes((hipStream_t)(stream)) ? hipMemsetAsync((dst), (value), (bytes), (stream)) : hipSuccess)
#define hipMemcpyAsync(dst, src, bytes, kind, stream) (gmp::lane_takes((hipStream_t)(stream)) ? hipMemcpyAsync((dst), (src), (bytes), (kind), (stream)) : hipSuccess)
#define hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, kind, stream) \
    (gmp::lane_takes((hipStream_t)(stream)) ? hipMemcpy2DAsync((dst), (dpitch), (src), (spitch), (width), (height), (kind), (stream)) : hipSuccess)
