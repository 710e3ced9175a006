// Integer counts behind the classification metrics of fine-tuning (finetune/metrics.py: accuracy, macro / binary F1, precision, recall and
// the one-vs-rest ROC AUC), made on the device so that one read-back of C*C + 4*C + 1 integers replaces three host copies and five
// scikit-learn calls per batch.
//   confusion[t*C + p]   rows with target t and prediction p
//   auc_counts[c*4 + k]  (n_pos, n_neg, n_greater, n_equal) of class c: over the ordered pairs (i, j) with target[i] == c != target[j],
//                        how many have prob[i, c] > prob[j, c] and how many compare equal -- AUC_c = (n_greater + n_equal / 2) / (n_pos n_neg),
//                        the Mann-Whitney form of the area under the ROC curve, ties counted half
//   status               rows left out of every count: target or prediction outside [0, C), or a non-finite probability
//
//   cls_zero_kernel   one block: the outputs set to zero (the counts are accumulated with atomics, so every call starts from zero)
//   cls_prep_kernel   256 rows per tile, tiles grid-strided: validity, the confusion histogram in LDS, the per-row class code for the pair
//                     kernel (target, or -1 for a row that is left out) into the workspace
//   cls_pair_kernel   block (x, y): thread t owns row i = 256 x + t with p_i = prob[i, y_i] in a register and walks the j rows of chunk y,
//                     256 at a time staged in LDS ([256, C] probabilities and 256 class codes).  A pair (i, j) is met once, by i's thread,
//                     and goes to class y_i only, so the whole count is n^2 compares whatever C is.
// Every lane of a wave reads the SAME staged row j at column y_i: at most C <= 32 consecutive dwords of one row, i.e. distinct banks for
// ds_read_b32 (32 banks) at any row stride, equal columns broadcast.  The gather is conflict-free by the loop order and the tile needs no
// padding (a padded stride would only add a second bank row to the staging stores).
// All sums are integers: threads count in registers, a block adds them per class in LDS and issues one 64-bit atomicAdd per class and
// count, so the result does not depend on the block order.  There is no floating-point atomic in this file.
#include <algorithm>

#include "gnnmp_internal.h"

namespace {

constexpr int MAXC = 32;            // classes
constexpr int64_t MAXN = 262144;    // rows: n^2 = 6.9e10 compares, a few milliseconds
constexpr int T = 256;              // threads per block = rows per tile, both kernels
constexpr int PREP_BLOCKS = 256;    // cap of the prep grid (tiles are grid-strided)
constexpr int PAIR_BLOCKS = 2048;   // target size of the pair grid: i-tiles x j-chunks

typedef unsigned long long u64;

__global__ __launch_bounds__(T) void cls_zero_kernel(u64* __restrict__ confusion, u64* __restrict__ auc_counts, int32_t* __restrict__ status,
                                                     int C) {
    const int t = threadIdx.x;
    for (int k = t; k < C * C; k += T) confusion[k] = 0ull;
    if (t < 4 * C) auc_counts[t] = 0ull;
    if (t == 0) status[0] = 0;
}

__global__ __launch_bounds__(T) void cls_prep_kernel(const int64_t* __restrict__ targets, const int64_t* __restrict__ predictions,
                                                     const float* __restrict__ prob, int64_t n, int C, int tiles,
                                                     u64* __restrict__ confusion, u64* __restrict__ auc_counts,
                                                     int32_t* __restrict__ status, int32_t* __restrict__ code) {
    __shared__ int hist[MAXC * MAXC];
    __shared__ int bad[T];
    __shared__ int nval;
    __shared__ int nbad;
    const int t = threadIdx.x;
    for (int k = t; k < C * C; k += T) hist[k] = 0;
    if (t == 0) {
        nval = 0;
        nbad = 0;
    }
    for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        const int64_t r0 = (int64_t)tile * T;
        const int rows = n - r0 < T ? (int)(n - r0) : T;
        __syncthreads();                                            // the previous tile is done with bad[]; the zeroes above are written
        bad[t] = 0;
        __syncthreads();
        const float* p = prob + r0 * C;
        for (int e = t; e < rows * C; e += T)                       // coalesced over the tile's rows * C probabilities
            if (!isfinite(p[e])) bad[e / C] = 1;                    // (every writer stores the same 1)
        __syncthreads();
        if (t < rows) {
            const int64_t y = targets[r0 + t], q = predictions[r0 + t];
            const bool ok = y >= 0 && y < C && q >= 0 && q < C && !bad[t];
            code[r0 + t] = ok ? (int32_t)y : -1;
            if (ok) {
                atomicAdd(&hist[(int)y * C + (int)q], 1);
                atomicAdd(&nval, 1);
            } else {
                atomicAdd(&nbad, 1);
            }
        }
    }
    __syncthreads();
    for (int k = t; k < C * C; k += T)
        if (hist[k]) atomicAdd(&confusion[k], (u64)hist[k]);
    if (t < C) {                                                    // n_pos = the class's row of the histogram, n_neg = the other valid rows
        int pos = 0;
        for (int q = 0; q < C; ++q) pos += hist[t * C + q];
        if (pos) atomicAdd(&auc_counts[t * 4 + 0], (u64)pos);
        if (nval - pos) atomicAdd(&auc_counts[t * 4 + 1], (u64)(nval - pos));
    }
    if (t == 0 && nbad) atomicAdd(&status[0], nbad);
}

__global__ __launch_bounds__(T) void cls_pair_kernel(const float* __restrict__ prob, const int32_t* __restrict__ code, int64_t n, int C,
                                                     int tiles, int tiles_per_chunk, u64* __restrict__ auc_counts) {
    extern __shared__ float4 smem4[];                               // one array: [T * C] probabilities, [T] class codes, [2 * MAXC] counts
    float* sp = reinterpret_cast<float*>(smem4);
    int* sc = reinterpret_cast<int*>(sp + T * C);
    int* cnt = sc + T;
    const int t = threadIdx.x;
    const int64_t i = (int64_t)blockIdx.x * T + t;
    const int yi = i < n ? code[i] : -1;
    const float pi = yi >= 0 ? prob[i * C + yi] : 0.f;
    if (t < 2 * MAXC) cnt[t] = 0;
    int greater = 0, equal = 0;                                     // <= n each: 32 bits are enough up to the block's sum (256 n < 2^31)
    const int t_begin = blockIdx.y * tiles_per_chunk, t_end = min(tiles, t_begin + tiles_per_chunk);
    for (int tile = t_begin; tile < t_end; ++tile) {
        const int64_t j0 = (int64_t)tile * T;
        const int rows = n - j0 < T ? (int)(n - j0) : T;
        __syncthreads();                                            // the previous tile has been read
        const float* p = prob + j0 * C;
        for (int e = t; e < rows * C; e += T) sp[e] = p[e];
        if (t < rows) sc[t] = code[j0 + t];
        __syncthreads();
        if (yi >= 0) {
            const float* col = sp + yi;
#pragma unroll 4
            for (int j = 0; j < rows; ++j) {
                const int yj = sc[j];                               // a left-out row has code -1 (and may hold a NaN: it compares false)
                const float pj = col[j * C];
                const bool neg = yj >= 0 && yj != yi;
                greater += (neg && pi > pj) ? 1 : 0;
                equal += (neg && pi == pj) ? 1 : 0;
            }
        }
    }
    __syncthreads();                                                // cnt[] zeroed (also when the chunk is empty)
    if (greater) atomicAdd(&cnt[yi], greater);
    if (equal) atomicAdd(&cnt[MAXC + yi], equal);
    __syncthreads();
    if (t < C) {
        if (cnt[t]) atomicAdd(&auc_counts[t * 4 + 2], (u64)cnt[t]);
        if (cnt[MAXC + t]) atomicAdd(&auc_counts[t * 4 + 3], (u64)cnt[MAXC + t]);
    }
}

int range_ok(const char* who, int64_t n, int classes) {
    if (n < 1 || n > MAXN) return gmp::fail(GMP_ERR_ARG, "%s: n=%lld (1 <= n <= %lld)", who, (long long)n, (long long)MAXN);
    if (classes < 2 || classes > MAXC) return gmp::fail(GMP_ERR_ARG, "%s: classes=%d (2 <= classes <= %d)", who, classes, MAXC);
    return GMP_OK;
}

}  // namespace

extern "C" size_t gmp_cls_counts_workspace_bytes(int64_t n, int classes) {
    (void)classes;
    return (size_t)(n > 0 ? n : 0) * sizeof(int32_t) + 256;        // one class code per row, behind a 256-byte alignment
}

extern "C" int gmp_cls_counts(const int64_t* targets, const int64_t* predictions, const float* probabilities, int64_t n, int classes,
                              int64_t* confusion, int64_t* auc_counts, int32_t* status, void* workspace, size_t workspace_bytes,
                              gmp_stream_t stream) {
    if (int rc = range_ok("cls_counts", n, classes)) return rc;
    if (!targets || !predictions || !probabilities || !confusion || !auc_counts || !status || !workspace)
        return gmp::fail(GMP_ERR_ARG, "cls_counts: null pointer");
    if (workspace_bytes < gmp_cls_counts_workspace_bytes(n, classes)) return gmp::fail(GMP_ERR_WORKSPACE, "cls_counts: workspace too small");
    int32_t* code = (int32_t*)(((uintptr_t)workspace + 255) / 256 * 256);
    u64* conf = reinterpret_cast<u64*>(confusion);
    u64* auc = reinterpret_cast<u64*>(auc_counts);
    const int C = classes, tiles = gmp::cdiv(n, T);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(cls_zero_kernel, dim3(1), dim3(T), 0, st, conf, auc, status, C);
    if (int rc = gmp::check_launch("cls_zero_kernel")) return rc;
    hipLaunchKernelGGL(cls_prep_kernel, dim3((unsigned)std::min(tiles, PREP_BLOCKS)), dim3(T), 0, st, targets, predictions, probabilities, n, C,
                       tiles, conf, auc, status, code);
    if (int rc = gmp::check_launch("cls_prep_kernel")) return rc;
    // i-tiles x j-chunks: every j tile its own chunk while that keeps the grid near PAIR_BLOCKS (small n: more blocks than i-tiles alone),
    // several tiles per chunk beyond that (large n: few atomics per class)
    const int chunks_wanted = std::max(1, std::min(tiles, PAIR_BLOCKS / tiles));
    const int tiles_per_chunk = gmp::cdiv(tiles, chunks_wanted), chunks = gmp::cdiv(tiles, tiles_per_chunk);
    const size_t lds = (size_t)T * C * sizeof(float) + T * sizeof(int) + 2 * MAXC * sizeof(int);
    hipLaunchKernelGGL(cls_pair_kernel, dim3((unsigned)tiles, (unsigned)chunks), dim3(T), lds, st, probabilities, (const int32_t*)code, n, C,
                       tiles, tiles_per_chunk, auc);
    return gmp::check_launch("cls_pair_kernel");
}
