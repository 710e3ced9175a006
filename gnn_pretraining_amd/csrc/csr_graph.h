// What the baselines on a graph's own CSR share -- the link baselines (lp_heuristics.hip, lp_walk.hip) and, through csr_prop.h, the node
// baselines (label_prop.hip, feature_prop.hip): the size / null check of the int32 CSR and a row clamped to the col array, so that a CSR
// that breaks its contract gives wrong numbers, never an access outside the arrays.
#pragma once
#include "gnnmp_internal.h"

namespace csr {

struct Row { int64_t b, e; };

// row v of the CSR, clamped to the col array (v in [0, N))
__device__ __forceinline__ Row row_of(const int32_t* __restrict__ rowptr, int64_t nnz, int64_t v) {
    const int64_t b = min(max((int64_t)rowptr[v], (int64_t)0), nnz), e = min(max((int64_t)rowptr[v + 1], (int64_t)0), nnz);
    return Row{b, max(b, e)};
}

// the same for any v: empty for v outside [0, N)
__device__ __forceinline__ Row row_of(const int32_t* __restrict__ rowptr, int64_t nnz, int64_t N, int64_t v) {
    if (v < 0 || v >= N) return Row{0, 0};
    return row_of(rowptr, nnz, v);
}

inline int graph_ok(const char* who, const void* rowptr, const void* col, int64_t N, int64_t nnz) {
    if (N < 0 || N >= ((int64_t)1 << 31) || nnz < 0 || nnz >= ((int64_t)1 << 31))
        return gmp::fail(GMP_ERR_ARG, "%s: N=%lld nnz=%lld", who, (long long)N, (long long)nnz);
    if (!rowptr || (nnz > 0 && !col)) return gmp::fail(GMP_ERR_ARG, "%s: null pointer", who);
    return GMP_OK;
}

}  // namespace csr
