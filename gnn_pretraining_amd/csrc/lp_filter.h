// The candidate filter shared by the all-candidate rankers (lp_rank.hip, lp_heuristics.hip, lp_walk.hip, emb_link.hip): a query with source s skips the entries of
// row s of an optional filter CSR (int32 rowptr / col, any order, duplicates allowed).  A block that walks the candidates
// [c0, c0 + 32 W) keeps the row as a bitmap of W words in LDS; what it counts or compares belongs to each kernel.
#pragma once
#include "gnnmp_internal.h"

namespace lpf {

// ORs bit (c - c0) into bits[W] (zeroed by the caller, a barrier in between) for every entry c of row s of the filter that falls into
// [c0, c0 + 32 W); every thread of a block of THREADS calls it.  The row is clamped to [0, nnz]; no filter (rowptr null), a source
// outside [0, N) and entries outside the tile mark nothing.
template <int W, int THREADS>
__device__ __forceinline__ void mark(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t nnz, int64_t s, int64_t N,
                                     int64_t c0, unsigned int* bits) {
    if (rowptr && s >= 0 && s < N) {
        const int64_t b = max((int64_t)rowptr[s], (int64_t)0), e = min((int64_t)rowptr[s + 1], nnz);
        for (int64_t i = b + threadIdx.x; i < e; i += THREADS) {
            const uint64_t off = (uint64_t)((int64_t)col[i] - c0);
            if (off < (uint64_t)(32 * W)) atomicOr(&bits[off >> 5], 1u << (unsigned)(off & 31));
        }
    }
}

// The same for a block of `threads` that keeps a bitmap of a run-time number of `words` (lp_walk.hip: one bitmap over all candidates).
__device__ __forceinline__ void mark(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t nnz, int64_t s, int64_t N,
                                     int64_t c0, unsigned int* bits, int64_t words, int threads) {
    if (rowptr && s >= 0 && s < N) {
        const int64_t b = max((int64_t)rowptr[s], (int64_t)0), e = min((int64_t)rowptr[s + 1], nnz);
        for (int64_t i = b + threadIdx.x; i < e; i += threads) {
            const uint64_t off = (uint64_t)((int64_t)col[i] - c0);
            if (off < (uint64_t)(32 * words)) atomicOr(&bits[off >> 5], 1u << (unsigned)(off & 31));
        }
    }
}

// The marking for a block that walks the candidates [c0, c0 + width) for MANY queries at once and lays its bitmap out itself (emb_link.hip:
// one bit per (query row, candidate)): set(off) for every entry c0 + off of row s that falls into the window, same clamps as above.  The
// threads that share the row call it with first = 0 .. step - 1.
template <typename F>
__device__ __forceinline__ void mark_each(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t nnz, int64_t s, int64_t N,
                                          int64_t c0, int64_t width, int first, int step, F&& set) {
    if (rowptr && s >= 0 && s < N) {
        const int64_t b = max((int64_t)rowptr[s], (int64_t)0), e = min((int64_t)rowptr[s + 1], nnz);
        for (int64_t i = b + first; i < e; i += step) {
            const uint64_t off = (uint64_t)((int64_t)col[i] - c0);
            if (off < (uint64_t)width) set((int)off);
        }
    }
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

}  // namespace lpf
