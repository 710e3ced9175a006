// All-candidate link ranking on top of the fine-tuning scorer (lp_score.hip): one source against EVERY node, reduced on the fly.
//   gmp_lp_rank   for Q true pairs (src, dst): the true pair's logit and how many candidates c in [0, N) score greater than / equal to it
//                 (c == src, c == dst and the entries of src's filter row are skipped) -- the filtered rank of link-prediction evaluation
//   gmp_lp_topk   for Q sources: the k <= 64 best candidates (c != src, not in the filter row), logit descending, ties to the lower index
// Neither writes a per-candidate logit, the [Q N, 256] activation or a pair list: a candidate's logit lives in one register until it is
// compared.  The logit of (s, c) is BIT FOR BIT lp_score_fwd_kernel's with p = 0: score_tile below and that kernel run the one tile code
// of lp_tile.h (32 x 768 LDS feature tile, eight 96-deep k-slices per wave on v_mfma_f32_32x32x2_f32 added in order, 32-unit partial dots
// with w3), the eight hidden groups looped inside the block instead of over blockIdx.y, their dots added in lp_logit_kernel's order, then b3.
//
//   lp_rank_true_kernel    one block per 32 queries: logit_true, and the two counts set to zero
//   lp_rank_count_kernel   one block per (query, 32-candidate tile): compare, count in LDS, one integer atomicAdd per count and block
//   lp_topk_scan_kernel    one block per (query, part of the candidate tiles): a sorted 64-entry list in LDS, merged with each tile's 32
//                          logits by rank-by-counting over the 96 entries; the part's list goes to the workspace
//   lp_topk_merge_kernel   one block per query: the parts' lists ordered by rank-by-counting, the first k written
// Counts are integer sums and the order (logit, then index) is total, so both results are independent of the block order.
#include <algorithm>

#include "lp_filter.h"
#include "lp_tile.h"

namespace {

using namespace lpt;                // F, HID, KF, BM (candidates or queries per tile), LDA, THREADS, aligned16 and the scorer's tile code

constexpr int TILE_FLOATS = BM * LDA;
constexpr int RED_FLOATS = 8 * 32 * 32;
constexpr int LDS_BYTES = (TILE_FLOATS + RED_FLOATS) * 4;
constexpr int MAXK = 64;            // top-k list length
constexpr int UNI = MAXK + BM;      // list + one tile
constexpr int MAX_PARTS = 16;       // candidate-tile parts per query in the top-k scan

// The logits of the 32 pairs (sidx[r], didx[r]) (LDS; an index outside [0, N) reads as a zero row).  Every thread of the block calls it;
// thread t < 256 returns the logit of row t >> 3, the others return garbage.  Starts with a barrier (sidx / didx written by the caller).
__device__ __forceinline__ float score_tile(float* __restrict__ tile, float* __restrict__ red, const int64_t* sidx, const int64_t* didx,
                                            const float4* __restrict__ h4, int64_t N, const float* __restrict__ w0,
                                            const float* __restrict__ b0, const float* __restrict__ w3, const float* __restrict__ b3) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    __syncthreads();
    build(tile, h4, N, [&](int r) { return sidx[r]; }, [&](int r) { return didx[r]; });
    __syncthreads();
    float s = 0.f;
#pragma unroll 1
    for (int g = 0; g < HID / 32; ++g) {
        const int n0 = 32 * g;
        spill(red, slice(tile, w0, n0, wave, l31, half), wave, l31, half);
        __syncthreads();
        if (threadIdx.x < 256) {                                    // (waves 0-3: wave-uniform)
            const float dot = partial_dot(hidden4(red, b0, n0), w3, n0);
            s = g == 0 ? dot : s + dot;                             // lp_logit_kernel: the eight partial dots in order
        }
        __syncthreads();                                            // red is free for the next group
    }
    return s + b3[0];
}

__global__ __launch_bounds__(THREADS) void lp_rank_true_kernel(const float* __restrict__ h, const int64_t* __restrict__ src,
                                                               const int64_t* __restrict__ dst, int64_t N, int64_t Q,
                                                               const float* __restrict__ w0, const float* __restrict__ b0,
                                                               const float* __restrict__ w3, const float* __restrict__ b3,
                                                               float* __restrict__ logit_true, int32_t* __restrict__ n_greater,
                                                               int32_t* __restrict__ n_equal) {
    extern __shared__ float4 smem4[];
    __shared__ int64_t sidx[BM], didx[BM];
    float* tile = reinterpret_cast<float*>(smem4);
    const int t = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    if (t < BM) {
        const int64_t m = m0 + t;
        sidx[t] = m < Q ? src[m] : -1;
        didx[t] = m < Q ? dst[m] : -1;
    }
    const float lg = score_tile(tile, tile + TILE_FLOATS, sidx, didx, reinterpret_cast<const float4*>(h), N, w0, b0, w3, b3);
    const int64_t m = m0 + (t >> 3);
    if (t < 256 && (t & 7) == 0 && m < Q) {
        logit_true[m] = lg;
        n_greater[m] = 0;
        n_equal[m] = 0;
    }
}

__global__ __launch_bounds__(THREADS) void lp_rank_count_kernel(const float* __restrict__ h, const int64_t* __restrict__ src,
                                                                const int64_t* __restrict__ dst, int64_t N, int tiles,
                                                                const float* __restrict__ w0, const float* __restrict__ b0,
                                                                const float* __restrict__ w3, const float* __restrict__ b3,
                                                                const int32_t* __restrict__ frowptr, const int32_t* __restrict__ fcol,
                                                                int64_t fnnz, const float* __restrict__ logit_true,
                                                                int32_t* __restrict__ n_greater, int32_t* __restrict__ n_equal) {
    extern __shared__ float4 smem4[];
    __shared__ int64_t sidx[BM], didx[BM];
    __shared__ unsigned int fmask;
    __shared__ int cnt[2];
    float* tile = reinterpret_cast<float*>(smem4);
    const int t = threadIdx.x;
    const int64_t q = blockIdx.x / (unsigned)tiles, c0 = (int64_t)(blockIdx.x % (unsigned)tiles) * BM;
    const int64_t s = src[q], d = dst[q];
    if (t < BM) {
        const int64_t c = c0 + t;
        sidx[t] = c < N ? s : -1;
        didx[t] = c < N ? c : -1;
    }
    if (t == 0) {
        fmask = 0u;
        cnt[0] = 0;
        cnt[1] = 0;
    }
    __syncthreads();
    lpf::mark<1, THREADS>(frowptr, fcol, fnnz, s, N, c0, &fmask);
    const float lg = score_tile(tile, tile + TILE_FLOATS, sidx, didx, reinterpret_cast<const float4*>(h), N, w0, b0, w3, b3);
    if (t < 256 && (t & 7) == 0) {
        const int row = t >> 3;
        const int64_t c = c0 + row;
        const bool valid = c < N && c != s && c != d && !lpf::marked(&fmask, row);
        const float lt = logit_true[q];
        if (valid && lg > lt) atomicAdd(&cnt[0], 1);
        if (valid && lg == lt) atomicAdd(&cnt[1], 1);
    }
    __syncthreads();
    if (t == 0) {
        if (cnt[0]) atomicAdd(&n_greater[q], cnt[0]);
        if (cnt[1]) atomicAdd(&n_equal[q], cnt[1]);
    }
}

// a total order over list entries: real candidates (index >= 0) first, by logit descending then index ascending; padding by position
__device__ __forceinline__ bool better(float av, int ai, int apos, float bv, int bi, int bpos) {
    const bool a_ok = ai >= 0, b_ok = bi >= 0;
    if (a_ok != b_ok) return a_ok;
    if (!a_ok) return apos < bpos;
    return av > bv || (av == bv && ai < bi);
}

__global__ __launch_bounds__(THREADS) void lp_topk_scan_kernel(const float* __restrict__ h, const int64_t* __restrict__ src, int64_t N,
                                                               int tiles, int parts, const float* __restrict__ w0,
                                                               const float* __restrict__ b0, const float* __restrict__ w3,
                                                               const float* __restrict__ b3, const int32_t* __restrict__ frowptr,
                                                               const int32_t* __restrict__ fcol, int64_t fnnz,
                                                               float* __restrict__ part_v, int32_t* __restrict__ part_i) {
    extern __shared__ float4 smem4[];
    __shared__ int64_t sidx[BM], didx[BM];
    __shared__ unsigned int fmask;
    __shared__ float lv[UNI];
    __shared__ int li[UNI];
    float* tile = reinterpret_cast<float*>(smem4);
    const int t = threadIdx.x;
    const int64_t q = blockIdx.x / (unsigned)parts;
    const int part = (int)(blockIdx.x % (unsigned)parts);
    const int per = (tiles + parts - 1) / parts, t_begin = part * per, t_end = min(tiles, t_begin + per);
    const int64_t s = src[q];
    const float ninf = -__builtin_inff();
    if (t < UNI) {
        lv[t] = ninf;
        li[t] = -1;
    }
    for (int ti = t_begin; ti < t_end; ++ti) {
        const int64_t c0 = (int64_t)ti * BM;
        __syncthreads();                                            // the previous tile's merge is done with sidx / fmask / the list
        if (t < BM) {
            const int64_t c = c0 + t;
            sidx[t] = c < N ? s : -1;
            didx[t] = c < N ? c : -1;
        }
        if (t == 0) fmask = 0u;
        __syncthreads();
        lpf::mark<1, THREADS>(frowptr, fcol, fnnz, s, N, c0, &fmask);
        const float lg = score_tile(tile, tile + TILE_FLOATS, sidx, didx, reinterpret_cast<const float4*>(h), N, w0, b0, w3, b3);
        if (t < 256 && (t & 7) == 0) {
            const int row = t >> 3;
            const int64_t c = c0 + row;
            const bool valid = c < N && c != s && !lpf::marked(&fmask, row);
            lv[MAXK + row] = valid ? lg : ninf;
            li[MAXK + row] = valid ? (int)c : -1;
        }
        __syncthreads();
        float mv = 0.f;
        int mi = -1, rank = UNI;
        if (t < UNI) {
            mv = lv[t];
            mi = li[t];
            rank = 0;
            for (int j = 0; j < UNI; ++j) rank += (j != t && better(lv[j], li[j], j, mv, mi, t)) ? 1 : 0;
        }
        __syncthreads();
        if (rank < MAXK) {
            lv[rank] = mv;
            li[rank] = mi;
        }
    }
    __syncthreads();
    if (t < MAXK) {
        part_v[(int64_t)blockIdx.x * MAXK + t] = lv[t];
        part_i[(int64_t)blockIdx.x * MAXK + t] = li[t];
    }
}

__global__ __launch_bounds__(256) void lp_topk_merge_kernel(const float* __restrict__ part_v, const int32_t* __restrict__ part_i, int parts,
                                                            int k, int64_t* __restrict__ idx, float* __restrict__ logit) {
    __shared__ float lv[MAX_PARTS * MAXK];
    __shared__ int li[MAX_PARTS * MAXK];
    const int t = threadIdx.x, n = parts * MAXK;
    const int64_t q = blockIdx.x;
    for (int i = t; i < n; i += 256) {
        lv[i] = part_v[q * n + i];
        li[i] = part_i[q * n + i];
    }
    __syncthreads();
    for (int i = t; i < n; i += 256) {
        const float mv = lv[i];
        const int mi = li[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (j != i && better(lv[j], li[j], j, mv, mi, i)) ? 1 : 0;
        if (rank < k) {
            idx[q * k + rank] = mi >= 0 ? (int64_t)mi : (int64_t)-1;
            logit[q * k + rank] = mi >= 0 ? mv : -__builtin_inff();
        }
    }
}

int topk_parts(int64_t Q, int64_t N) {
    // enough blocks for the chip when there are few sources; one part per source once the sources alone fill it
    const int64_t tiles = (N + BM - 1) / BM;
    if (Q <= 0 || tiles <= 1 || Q >= 256) return 1;
    return (int)std::min<int64_t>(std::min<int64_t>(tiles, MAX_PARTS), (512 + Q - 1) / Q);
}

int common_ok(const char* who, int64_t N, int64_t Q, int feat, int hidden, const void* h, const void* w0, const void* b0, const void* w3,
              const void* b3, const int32_t*& frowptr, const int32_t* fcol, int64_t fnnz) {
    if (feat != F || hidden != HID) return gmp::fail(GMP_ERR_UNSUPPORTED, "%s: feat %d / hidden %d (this kernel is built for 256 / 256)", who, feat, hidden);
    if (N < 0 || Q < 0 || N >= ((int64_t)1 << 31) || fnnz < 0) return gmp::fail(GMP_ERR_ARG, "%s: N=%lld Q=%lld filter_nnz=%lld", who, (long long)N, (long long)Q, (long long)fnnz);
    if (int rc = lpf::filter_ok(who, frowptr, fcol, fnnz)) return rc;
    if (Q == 0) return GMP_OK;
    if ((N > 0 && !h) || !w0 || !b0 || !w3 || !b3) return gmp::fail(GMP_ERR_ARG, "%s: null pointer", who);
    if (!aligned16(h) || !aligned16(w0) || !aligned16(b0) || !aligned16(w3)) return gmp::fail(GMP_ERR_ARG, "%s: h, w0, b0 and w3 must be 16-byte aligned", who);
    return GMP_OK;
}

}  // namespace

extern "C" size_t gmp_lp_rank_workspace_bytes(int64_t Q, int64_t N) {
    (void)Q; (void)N;
    return 0;                                                       // the counts are integer atomics on the outputs: nothing is staged
}

extern "C" size_t gmp_lp_topk_workspace_bytes(int64_t Q, int64_t N) {
    const size_t n = (size_t)(Q > 0 ? Q : 0) * topk_parts(Q, N) * MAXK;     // the scan's lists: per (query, part) MAXK logits and indices
    gmp::Carver c(nullptr, true);
    c.take<float>(n);
    c.take<int32_t>(n);
    return c.total();
}

extern "C" int gmp_lp_rank(const float* h, const int64_t* src, const int64_t* dst, int64_t N, int64_t Q, int feat, int hidden,
                           const float* w0, const float* b0, const float* w3, const float* b3, const int32_t* filter_rowptr,
                           const int32_t* filter_col, int64_t filter_nnz, float* logit_true, int32_t* n_greater, int32_t* n_equal,
                           void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    (void)workspace; (void)workspace_bytes;
    if (int rc = common_ok("lp_rank", N, Q, feat, hidden, h, w0, b0, w3, b3, filter_rowptr, filter_col, filter_nnz)) return rc;
    bool done;                                                      // (common_ok has answered the front's first two checks: N and Q go together there)
    if (int rc = lpf::rank_front("lp_rank", Q, filter_rowptr, filter_col, filter_nnz, src, dst, logit_true, n_greater, n_equal, done); rc || done)
        return rc;
    const int64_t tiles = (N + BM - 1) / BM;
    if (int rc = lpf::grid_ok("lp_rank", Q, tiles)) return rc;
    static std::atomic<uint64_t> attr_true{0}, attr_count{0};
    if (int rc = gmp::reserve_lds(attr_true, (const void*)lp_rank_true_kernel, LDS_BYTES, "lp_rank")) return rc;
    if (int rc = gmp::reserve_lds(attr_count, (const void*)lp_rank_count_kernel, LDS_BYTES, "lp_rank")) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lp_rank_true_kernel, dim3((unsigned)gmp::cdiv(Q, BM)), dim3(THREADS), LDS_BYTES, st, h, src, dst, N, Q, w0, b0, w3, b3,
                       logit_true, n_greater, n_equal);
    if (int rc = gmp::check_launch("lp_rank_true_kernel")) return rc;
    if (tiles == 0) return GMP_OK;
    hipLaunchKernelGGL(lp_rank_count_kernel, dim3((unsigned)(Q * tiles)), dim3(THREADS), LDS_BYTES, st, h, src, dst, N, (int)tiles, w0, b0, w3,
                       b3, filter_rowptr, filter_col, filter_nnz, (const float*)logit_true, n_greater, n_equal);
    return gmp::check_launch("lp_rank_count_kernel");
}

extern "C" int gmp_lp_topk(const float* h, const int64_t* src, int64_t N, int64_t Q, int k, int feat, int hidden, const float* w0,
                           const float* b0, const float* w3, const float* b3, const int32_t* filter_rowptr, const int32_t* filter_col,
                           int64_t filter_nnz, int64_t* idx, float* logit, void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    if (int rc = common_ok("lp_topk", N, Q, feat, hidden, h, w0, b0, w3, b3, filter_rowptr, filter_col, filter_nnz)) return rc;
    if (k < 1 || k > MAXK) return gmp::fail(GMP_ERR_ARG, "lp_topk: k=%d (1 <= k <= %d)", k, MAXK);
    if (Q == 0) return GMP_OK;
    if (!src || !idx || !logit || !workspace) return gmp::fail(GMP_ERR_ARG, "lp_topk: null pointer");
    if (workspace_bytes < gmp_lp_topk_workspace_bytes(Q, N)) return gmp::fail(GMP_ERR_ARG, "lp_topk: workspace too small");
    const int64_t tiles = (N + BM - 1) / BM;
    const int parts = topk_parts(Q, N);
    if (Q * parts >= ((int64_t)1 << 31)) return gmp::fail(GMP_ERR_ARG, "lp_topk: Q=%lld", (long long)Q);
    static std::atomic<uint64_t> attr_scan{0};
    if (int rc = gmp::reserve_lds(attr_scan, (const void*)lp_topk_scan_kernel, LDS_BYTES, "lp_topk")) return rc;
    gmp::Carver c(workspace, true);
    float* part_v = c.take<float>((size_t)Q * parts * MAXK);
    int32_t* part_i = c.take<int32_t>((size_t)Q * parts * MAXK);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lp_topk_scan_kernel, dim3((unsigned)(Q * parts)), dim3(THREADS), LDS_BYTES, st, h, src, N, (int)tiles, parts, w0, b0, w3,
                       b3, filter_rowptr, filter_col, filter_nnz, part_v, part_i);
    if (int rc = gmp::check_launch("lp_topk_scan_kernel")) return rc;
    hipLaunchKernelGGL(lp_topk_merge_kernel, dim3((unsigned)Q), dim3(256), 0, st, (const float*)part_v, (const int32_t*)part_i, parts, k, idx, logit);
    return gmp::check_launch("lp_topk_merge_kernel");
}
