// Sparse (CSR) input for InputEncoder.linear: Y = X W^T + b with X a CSR bag-of-words matrix (Cora / CiteSeer keep
// ~1.3 % of their entries after NormalizeFeatures), and its weight gradient dW = G^T X read through the CSC form.
//
// Both products are the same gather-sum: an output row is a fixed-order sum of val * (one 1 KB row of a dense [*, H]
// operand).  One wave owns one output row; each lane holds V consecutive outputs (H = 256: one float4 per lane); the
// row's (index, value) pairs are loaded 64 at a time, one per lane, and broadcast with readlane, so every gather
// address is wave-uniform plus the lane offset and UNROLL gathers are in flight before the first FMA.  No atomics on
// any result: every output element is one sequential sum over its row's non-zeros -- bitwise reproducible.
//
//   forward:  W [H, ldw] is transposed into Wt [K, H] (workspace, one tiled launch), then Y[r,:] = sum val * Wt[col,:] + b
//   wgrad:    dW^T[k,:] = sum over column k of the CSC of val_t * G[row,:]; a block computes TK columns into LDS and
//             writes them out as TK-wide runs of the [H, ldw] rows (columns without entries and the padding get 0.0)
//   CSC:      gmp_csr_build over the (row, col) pairs: stable by non-zero id, i.e. ascending row within a column.
#include "gnnmp_internal.h"

namespace {

constexpr int SL_THREADS = 256;          // 4 waves: 4 output rows per block (forward)
constexpr int SL_UNROLL = 8;             // gathers in flight per wave
constexpr int WG_TK = 8;                 // weight gradient: columns per block, one wave each
constexpr int WG_THREADS = WG_TK * GMP_WAVE;
constexpr int SL_MAX_H = 1024;           // LDS tile of the weight gradient: WG_TK * (H + 1) * 4 B <= 33 KiB
constexpr int TP = 64;                   // transpose tile

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

template <int V> struct vec;
template <> struct vec<1> { using t = float; };
template <> struct vec<4> { using t = float4; };

__device__ __forceinline__ void fma_v(float& acc, float v, float w) { acc = fmaf(v, w, acc); }
__device__ __forceinline__ void fma_v(float4& acc, float v, float4 w) {
    acc.x = fmaf(v, w.x, acc.x); acc.y = fmaf(v, w.y, acc.y); acc.z = fmaf(v, w.z, acc.z); acc.w = fmaf(v, w.w, acc.w);
}
__device__ __forceinline__ float zero_v(float*) { return 0.f; }
__device__ __forceinline__ float4 zero_v(float4*) { return make_float4(0.f, 0.f, 0.f, 0.f); }

// acc = sum_{k in [beg, end), 0 <= idx[k] < bound} val[k] * B[idx[k] * H + c0 + lane * V .. + V), in k order.
// Returns the number of skipped (out-of-range) indices, identical on every lane.
template <int V>
__device__ __forceinline__ int gather_sum(const int* __restrict__ idx, const float* __restrict__ val, const float* __restrict__ B,
                                          int beg, int end, int bound, int H, int c0, int lane, typename vec<V>::t& acc) {
    using T = typename vec<V>::t;
    acc = zero_v((T*)nullptr);
    int bad = 0;
    for (int base = beg; base < end; base += GMP_WAVE) {
        const int n = min(GMP_WAVE, end - base);
        int my_i = -1;
        float my_v = 0.f;
        if (lane < n) { my_i = idx[base + lane]; my_v = val[base + lane]; }
        const bool my_bad = lane < n && (my_i < 0 || my_i >= bound);
        bad += __popcll(__ballot(my_bad));
        for (int i = 0; i < n; i += SL_UNROLL) {
            T w[SL_UNROLL];
            float v[SL_UNROLL];
#pragma unroll
            for (int u = 0; u < SL_UNROLL; ++u) {
                const int j = i + u, jj = j < n ? j : 0;              // wave-uniform: the pair sits in lane jj
                const int c = __builtin_amdgcn_readlane(my_i, jj);
                v[u] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(my_v), jj));
                const bool ok = j < n && c >= 0 && c < bound;
                w[u] = ok ? *reinterpret_cast<const T*>(B + (size_t)c * H + c0 + lane * V) : zero_v((T*)nullptr);
                if (!ok) v[u] = 0.f;
            }
#pragma unroll
            for (int u = 0; u < SL_UNROLL; ++u)
                if (i + u < n) fma_v(acc, v[u], w[u]);
        }
    }
    return bad;
}

__device__ __forceinline__ void store_v(float* p, float a, const float* b) { *p = a + (b ? *b : 0.f); }
__device__ __forceinline__ void store_v(float* p, float4 a, const float* b) {
    if (b) { a.x += b[0]; a.y += b[1]; a.z += b[2]; a.w += b[3]; }
    *reinterpret_cast<float4*>(p) = a;
}

// Y[r, :] = sum_k val[k] * Wt[col[k], :] (+ bias): one wave per row
template <int V>
__global__ __launch_bounds__(SL_THREADS) void sparse_rows_kernel(const int* __restrict__ rowptr, const int* __restrict__ col,
                                                               const float* __restrict__ val, const float* __restrict__ Wt,
                                                               const float* __restrict__ bias, float* __restrict__ Y, int N, int K,
                                                               int H, int64_t ldy, int* status) {
    const int lane = threadIdx.x % GMP_WAVE;
    const int r = __builtin_amdgcn_readfirstlane(blockIdx.x * (SL_THREADS / GMP_WAVE) + threadIdx.x / GMP_WAVE);
    if (r >= N) return;
    const int beg = rowptr[r], end = rowptr[r + 1];
    int bad = 0;
    for (int c0 = 0; c0 < H; c0 += GMP_WAVE * V) {
        typename vec<V>::t acc;
        bad = gather_sum<V>(col, val, Wt, beg, end, K, H, c0, lane, acc);
        store_v(Y + (size_t)r * ldy + c0 + lane * V, acc, bias ? bias + c0 + lane * V : nullptr);
    }
    if (bad && lane == 0 && status) atomicAdd(status, bad);
}

// Wt[k, h] = W[h, k] for k < K (64 x 64 tiles through LDS)
__global__ __launch_bounds__(256) void transpose_kernel(const float* __restrict__ W, float* __restrict__ Wt, int H, int K, int64_t ldw) {
    __shared__ float t[TP][TP + 1];
    const int k0 = blockIdx.x * TP, h0 = blockIdx.y * TP;
    const int tx = threadIdx.x % TP, ty = threadIdx.x / TP;         // 64 x 4
    for (int y = ty; y < TP; y += 4) {
        const int h = h0 + y, k = k0 + tx;
        t[y][tx] = (h < H && k < K) ? W[(size_t)h * ldw + k] : 0.f;
    }
    __syncthreads();
    for (int y = ty; y < TP; y += 4) {
        const int k = k0 + y, h = h0 + tx;
        if (k < K && h < H) Wt[(size_t)k * H + h] = t[tx][y];
    }
}

// dW[h, k] = sum over column k of the CSC of val_t * G[row, h]; columns [k0, k0 + WG_TK) of [0, ldw) per block
template <int V>
__global__ __launch_bounds__(WG_THREADS) void sparse_wgrad_kernel(const int* __restrict__ colptr, const int* __restrict__ row,
                                                                const float* __restrict__ val_t, const float* __restrict__ G,
                                                                float* __restrict__ dW, int N, int K, int H, int64_t ldw,
                                                                int* status) {
    extern __shared__ float tile[];                                  // [WG_TK][H + 1]
    const int lane = threadIdx.x % GMP_WAVE, w = threadIdx.x / GMP_WAVE;
    const int64_t k0 = (int64_t)blockIdx.x * WG_TK;
    const int64_t k = k0 + __builtin_amdgcn_readfirstlane(w);
    float* trow = tile + (size_t)w * (H + 1);
    int bad = 0;
    for (int c0 = 0; c0 < H; c0 += GMP_WAVE * V) {
        typename vec<V>::t acc;
        if (k < K) {
            bad = gather_sum<V>(row, val_t, G, colptr[k], colptr[k + 1], N, H, c0, lane, acc);
        } else {
            acc = zero_v((typename vec<V>::t*)nullptr);              // padding columns [K, ldw): exactly 0.0
        }
        const float* a = reinterpret_cast<const float*>(&acc);
#pragma unroll
        for (int e = 0; e < V; ++e) trow[c0 + lane * V + e] = a[e];
    }
    if (bad && lane == 0 && status) atomicAdd(status, bad);
    __syncthreads();
    // rows of dW: WG_TK consecutive floats per row, WG_TK threads per row
    for (int q = threadIdx.x; q < H * WG_TK; q += WG_THREADS) {
        const int h = q / WG_TK, t = q % WG_TK;
        if (k0 + t < ldw) dW[(size_t)h * ldw + k0 + t] = tile[(size_t)t * (H + 1) + h];
    }
}

// CSR -> (source = row, target = column) pairs for gmp_csr_build; a column outside [0, K) becomes target -1 (dropped, counted)
__global__ __launch_bounds__(256) void csc_pairs_kernel(const int* __restrict__ rowptr, const int* __restrict__ col, int N, int K,
                                                        int64_t nnz, int64_t* __restrict__ ei) {
    const int r = blockIdx.x * (256 / GMP_WAVE) + threadIdx.x / GMP_WAVE, lane = threadIdx.x % GMP_WAVE;
    if (r >= N) return;
    for (int j = rowptr[r] + lane; j < rowptr[r + 1]; j += GMP_WAVE) {
        const int c = col[j];
        ei[j] = r;
        ei[nnz + j] = (c >= 0 && c < K) ? c : -1;
    }
}

__global__ __launch_bounds__(256) void csc_finish_kernel(const int* __restrict__ colptr_full, const int* __restrict__ perm,
                                                         const float* __restrict__ val, int K, int64_t nnz, int* __restrict__ colptr,
                                                         float* __restrict__ val_t) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i <= K) colptr[i] = colptr_full[i];
    // slots past the valid count are left alone (colptr[K] = valid non-zeros)
    if (i < nnz && i < colptr_full[K]) val_t[i] = val[perm[i]];
}

int check_shape(const char* what, int64_t N, int64_t K, int H) {
    if (N < 0 || K < 0 || N > INT32_MAX - 1 || K > INT32_MAX - 1) return gmp::fail(GMP_ERR_ARG, "%s: N=%lld K=%lld", what, (long long)N, (long long)K);
    if (H <= 0 || H % GMP_WAVE || H > SL_MAX_H)
        return gmp::fail(GMP_ERR_UNSUPPORTED, "%s: out_features %d must be a positive multiple of 64 and <= %d", what, H, SL_MAX_H);
    return GMP_OK;
}

}  // namespace

extern "C" size_t gmp_sparse_linear_workspace_bytes(int64_t in_features, int out_features) {
    if (in_features < 0 || out_features <= 0) return 0;
    return align256((size_t)in_features * out_features * sizeof(float));
}

extern "C" int gmp_sparse_linear_fwd(const int32_t* rowptr, const int32_t* col, const float* val, int64_t num_rows, int64_t in_features,
                                     const float* weight, int64_t ldw, const float* bias, float* out, int out_features, int64_t ldo,
                                     int32_t* status, void* workspace, size_t workspace_bytes, gmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t N = num_rows, K = in_features;
    const int H = out_features;
    if (int rc = check_shape("sparse_linear_fwd", N, K, H)) return rc;
    if (ldw < K || ldo < H || ldo % 4) return gmp::fail(GMP_ERR_ARG, "sparse_linear_fwd: ldw=%lld (K=%lld) ldo=%lld (H=%d)", (long long)ldw,
                                                        (long long)K, (long long)ldo, H);
    if (!rowptr || !out || (K > 0 && !weight) || (N > 0 && K > 0 && (!col || !val)))
        return gmp::fail(GMP_ERR_ARG, "sparse_linear_fwd: null pointer");
    if (((uintptr_t)out | (uintptr_t)bias) % 16) return gmp::fail(GMP_ERR_ARG, "sparse_linear_fwd: out / bias not 16-byte aligned");
    if (workspace_bytes < gmp_sparse_linear_workspace_bytes(K, H) || (K > 0 && !workspace))
        return gmp::fail(GMP_ERR_WORKSPACE, "sparse_linear_fwd: workspace %zu < %zu", workspace_bytes, gmp_sparse_linear_workspace_bytes(K, H));
    if (N == 0) return GMP_OK;
    float* Wt = (float*)workspace;
    if (K > 0) hipLaunchKernelGGL(transpose_kernel, dim3(gmp::cdiv(K, TP), gmp::cdiv(H, TP)), dim3(256), 0, stream, weight, Wt, H, (int)K, ldw);
    const dim3 grid(gmp::cdiv(N, SL_THREADS / GMP_WAVE));
    if (H % (4 * GMP_WAVE) == 0)
        hipLaunchKernelGGL(sparse_rows_kernel<4>, grid, dim3(SL_THREADS), 0, stream, rowptr, col, val, Wt, bias, out, (int)N, (int)K, H, ldo, status);
    else
        hipLaunchKernelGGL(sparse_rows_kernel<1>, grid, dim3(SL_THREADS), 0, stream, rowptr, col, val, Wt, bias, out, (int)N, (int)K, H, ldo, status);
    return gmp::check_launch("sparse_linear_fwd");
}

extern "C" int gmp_sparse_linear_wgrad(const int32_t* colptr, const int32_t* row, const float* val_t, int64_t num_rows, int64_t in_features,
                                       const float* g, int out_features, float* dW, int64_t ldw, int32_t* status, gmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t N = num_rows, K = in_features;
    const int H = out_features;
    if (int rc = check_shape("sparse_linear_wgrad", N, K, H)) return rc;
    if (ldw < K) return gmp::fail(GMP_ERR_ARG, "sparse_linear_wgrad: ldw=%lld < K=%lld", (long long)ldw, (long long)K);
    if (!colptr || !dW || (N > 0 && (!g || !row || !val_t))) return gmp::fail(GMP_ERR_ARG, "sparse_linear_wgrad: null pointer");
    if ((uintptr_t)g % 16) return gmp::fail(GMP_ERR_ARG, "sparse_linear_wgrad: g not 16-byte aligned");
    if (ldw == 0) return GMP_OK;
    const dim3 grid(gmp::cdiv(ldw, WG_TK));
    const size_t lds = (size_t)WG_TK * (H + 1) * sizeof(float);
    if (H % (4 * GMP_WAVE) == 0)
        hipLaunchKernelGGL(sparse_wgrad_kernel<4>, grid, dim3(WG_THREADS), lds, stream, colptr, row, val_t, g, dW, (int)N, (int)K, H, ldw, status);
    else
        hipLaunchKernelGGL(sparse_wgrad_kernel<1>, grid, dim3(WG_THREADS), lds, stream, colptr, row, val_t, g, dW, (int)N, (int)K, H, ldw, status);
    return gmp::check_launch("sparse_linear_wgrad");
}

extern "C" size_t gmp_sparse_csc_workspace_bytes(int64_t num_rows, int64_t in_features, int64_t nnz) {
    if (num_rows < 0 || in_features < 0 || nnz < 0) return 0;
    const int64_t n = num_rows > in_features ? num_rows : in_features;
    return align256((size_t)nnz * 2 * sizeof(int64_t)) + align256((size_t)(n + 1) * 4) + align256((size_t)nnz * 4) +
           gmp_csr_build_workspace_bytes(n, nnz);
}

extern "C" int gmp_sparse_csc_build(const int32_t* rowptr, const int32_t* col, const float* val, int64_t num_rows, int64_t in_features,
                                    int64_t nnz, int32_t* colptr, int32_t* row, float* val_t, int32_t* status, void* workspace,
                                    size_t workspace_bytes, gmp_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t N = num_rows, K = in_features;
    if (N < 0 || K < 0 || nnz < 0 || N > INT32_MAX - 1 || K > INT32_MAX - 1 || nnz > INT32_MAX)
        return gmp::fail(GMP_ERR_ARG, "sparse_csc_build: N=%lld K=%lld nnz=%lld", (long long)N, (long long)K, (long long)nnz);
    if (!rowptr || !colptr || !status || (nnz > 0 && (!col || !val || !row || !val_t))) return gmp::fail(GMP_ERR_ARG, "sparse_csc_build: null pointer");
    const size_t need = gmp_sparse_csc_workspace_bytes(N, K, nnz);
    if (workspace_bytes < need || !workspace) return gmp::fail(GMP_ERR_WORKSPACE, "sparse_csc_build: workspace %zu < %zu", workspace_bytes, need);
    const int64_t n = N > K ? N : K;
    char* w = (char*)workspace;
    int64_t* ei = (int64_t*)w;
    w += align256((size_t)nnz * 2 * sizeof(int64_t));
    int* colptr_full = (int*)w;
    w += align256((size_t)(n + 1) * 4);
    int* perm = (int*)w;
    w += align256((size_t)nnz * 4);
    if (nnz > 0 && N > 0)
        hipLaunchKernelGGL(csc_pairs_kernel, dim3(gmp::cdiv(N, 256 / GMP_WAVE)), dim3(256), 0, stream, rowptr, col, (int)N, (int)K, nnz, ei);
    if (int rc = gmp::check_launch("sparse_csc_build pairs")) return rc;
    // grouped by TARGET (the column), slots in ascending non-zero id = ascending row within a column; status counts the -1 targets
    if (int rc = gmp_csr_build(ei, n, nnz, colptr_full, row, perm, nullptr, nullptr, nullptr, status, w, gmp_csr_build_workspace_bytes(n, nnz), stream_))
        return rc;
    const int64_t m = nnz > K + 1 ? nnz : K + 1;
    hipLaunchKernelGGL(csc_finish_kernel, dim3(gmp::cdiv(m, 256)), dim3(256), 0, stream, colptr_full, perm, val, (int)K, nnz, colptr, val_t);
    return gmp::check_launch("sparse_csc_build finish");
}
