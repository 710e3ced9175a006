// The candidate filter shared by the all-candidate rankers (lp_rank.hip, lp_heuristics.hip, lp_walk.hip, emb_link.hip): a query with source s skips the entries of
// row s of an optional filter CSR (int32 rowptr / col, any order, duplicates allowed).  A block that walks the candidates
// [c0, c0 + 32 W) keeps the row as a bitmap of W words in LDS; what it counts or compares belongs to each kernel.
#pragma once
#include "gnnmp_internal.h"

namespace lpf {

// set(off) for every entry c0 + off of row s of the filter that falls into the window [c0, c0 + width); the threads that share the row call
// it with first = 0 .. step - 1.  The row is clamped to [0, nnz]; no filter (rowptr null), a source outside [0, N) and entries outside the
// window set nothing.  A kernel that lays its bitmap out itself calls this form (emb_link.hip: one bit per (query row, candidate)).
template <typename F>
__device__ __forceinline__ void mark_each(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t nnz, int64_t s, int64_t N,
                                          int64_t c0, int64_t width, int64_t first, int step, F&& set) {
    if (rowptr && s >= 0 && s < N) {
        const int64_t b = max((int64_t)rowptr[s], (int64_t)0), e = min((int64_t)rowptr[s + 1], nnz);
        for (int64_t i = b + first; i < e; i += step) {
            const uint64_t off = (uint64_t)((int64_t)col[i] - c0);
            if (off < (uint64_t)width) set(off);
        }
    }
}

// The plain bitmap of a block of `threads` that walks the candidates [c0, c0 + 32 words): ORs bit (c - c0) into bits[words] (zeroed by the
// caller, a barrier in between) for every entry c of the row; every thread of the block calls it.
__device__ __forceinline__ void mark(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t nnz, int64_t s, int64_t N,
                                     int64_t c0, unsigned int* bits, int64_t words, int threads) {
    mark_each(rowptr, col, nnz, s, N, c0, 32 * words, threadIdx.x, threads,
              [&](uint64_t off) { atomicOr(&bits[off >> 5], 1u << (unsigned)(off & 31)); });
}

// The same with both sizes known at compile time: the form the tiled kernels call.  It goes through the form above and not straight to
// mark_each, which costs lp_heuristics.hip's cn_count_kernel a different instruction order; lp_walk.hip, whose bitmap is sized at run
// time, keeps the loop written out for the same reason (walk_kernel).
template <int W, int THREADS>
__device__ __forceinline__ void mark(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t nnz, int64_t s, int64_t N,
                                     int64_t c0, unsigned int* bits) {
    mark(rowptr, col, nnz, s, N, c0, bits, W, THREADS);
}

// candidate c0 + r is in the filter row (after a barrier behind mark)
__device__ __forceinline__ bool marked(const unsigned int* bits, int r) { return (bits[r >> 5] >> (r & 31)) & 1u; }

// The filter arrays go together; a filter without a col array has no entries and is dropped here, so that the kernels test rowptr alone.
inline int filter_ok(const char* who, const int32_t*& rowptr, const int32_t* col, int64_t nnz) {
    if ((rowptr == nullptr) != (col == nullptr) && nnz != 0)
        return gmp::fail(GMP_ERR_ARG, "%s: filter_rowptr and filter_col must both be given or both be null", who);
    if (!col) rowptr = nullptr;
    return GMP_OK;
}

// one block per (query, candidate tile) in one grid
inline int grid_ok(const char* who, int64_t Q, int64_t tiles) {
    if (Q * (tiles > 0 ? tiles : 1) >= ((int64_t)1 << 31))
        return gmp::fail(GMP_ERR_ARG, "%s: Q=%lld x %lld candidate tiles exceed one grid", who, (long long)Q, (long long)tiles);
    return GMP_OK;
}

// The front of a *_rank entry point, after its scorer's own checks: the signs of Q and filter_nnz, the filter arrays, then `done` for a
// call without queries (which may pass null everything), then the pairs and the three outputs.  The caller returns on an error or on done.
inline int rank_front(const char* who, int64_t Q, const int32_t*& filter_rowptr, const int32_t* filter_col, int64_t filter_nnz, const void* src,
                      const void* dst, const void* score_true, const void* n_greater, const void* n_equal, bool& done) {
    done = Q == 0;
    if (Q < 0 || filter_nnz < 0) return gmp::fail(GMP_ERR_ARG, "%s: Q=%lld filter_nnz=%lld", who, (long long)Q, (long long)filter_nnz);
    if (int rc = filter_ok(who, filter_rowptr, filter_col, filter_nnz)) return rc;
    if (done) return GMP_OK;
    if (!src || !dst || !score_true || !n_greater || !n_equal) return gmp::fail(GMP_ERR_ARG, "%s: null pointer", who);
    return GMP_OK;
}

}  // namespace lpf
