// What the baselines that propagate a matrix over a CSR share (label_prop.hip, feature_prop.hip; graph_feat.hip takes the row sum
// only): one row's sum as the definition above gmp_label_propagate in include/gnnmp.h fixes it, and the host loop that chains the rounds.
//
// The sum.  sum over the row's entries j, in ascending order, of right[j] * M[j], every multiply and add rounded on its own; an entry
// outside [0, n) is skipped BY A SELECT -- not added as zero, so a -0.0 survives -- and counted.  A round is a chain of dependent loads
// (rowptr -> col -> M), not a stream, so the loop takes UNROLL entries at a time: UNROLL `col` loads, then the validity tests and `right`
// loads, then UNROLL x W independent gathers, then the adds in order -- the order of the ADDS is the contract, not that of the loads.
// A row is walked by one caller (a row's sum is sequential by definition): a hub row is the accepted cost.
// The window.  With `base` the valid entries are those of [base, base + n) and load / right are indexed with j - base: one graph of a
// collated batch whose rows live in a copy of their own (graph_feat.hip).  base = 0 is the whole CSR, as label_prop.hip and
// feature_prop.hip call it.
#pragma once
#include "csr_graph.h"

namespace prop {

constexpr int UNROLL = 8;

// j - base in [0, n), for 0 <= base and base + n <= 2^31: the difference wraps, so no j outside the window passes
__device__ __forceinline__ bool inside(int j, int n, int base = 0) { return (unsigned)j - (unsigned)base < (unsigned)n; }

// right[j], NULL meaning ones
__device__ __forceinline__ float right_of(const float* __restrict__ right, int j) { return right ? right[j] : 1.0f; }

template <int W>
struct Sum {
    float acc[W];
    int bad;                                                                        // the row's entries outside [base, base + n)
};

// Row `row`'s W sums: load(j, q) is M[base + j]'s q-th value of this caller (called for j in [0, n) only), q an unrolled constant;
// right[j] likewise belongs to entry base + j.
template <int W, class Load>
__device__ __forceinline__ Sum<W> fold_row(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int n, int nnz, int64_t row,
                                           const float* __restrict__ right, Load load, int base = 0) {
    const csr::Row span = csr::row_of(rowptr, nnz, row);                            // a rowptr that is no CSR offset reads nothing outside col
    const int end = (int)span.e;
    Sum<W> s;
#pragma unroll
    for (int q = 0; q < W; ++q) s.acc[q] = 0.f;
    s.bad = 0;
    int k = (int)span.b;
    for (; k + UNROLL <= end; k += UNROLL) {
        int j[UNROLL];
        float r[UNROLL], f[UNROLL][W];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) j[u] = col[k + u];
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const bool ok = inside(j[u], n, base);
            const int js = ok ? j[u] - base : 0;                                    // a stray entry reads row 0 (there is one: row < n) and
            r[u] = right_of(right, js);                                             // is dropped below: no test around a load, so all of a
#pragma unroll                                                                      // batch's loads are in flight together
            for (int q = 0; q < W; ++q) f[u][q] = load(js, q);
        }
#pragma unroll
        for (int u = 0; u < UNROLL; ++u) {
            const bool ok = inside(j[u], n, base);
#pragma unroll
            for (int q = 0; q < W; ++q) {
                const float t = __fadd_rn(s.acc[q], __fmul_rn(r[u], f[u][q]));
                s.acc[q] = ok ? t : s.acc[q];
            }
            s.bad += ok ? 0 : 1;
        }
    }
    for (; k < end; ++k) {
        const int jj = (int)((unsigned)col[k] - (unsigned)base);                    // wraps as in inside(): no j outside the window passes
        if (inside(jj, n)) {
            const float rr = right_of(right, jj);
#pragma unroll
            for (int q = 0; q < W; ++q) s.acc[q] = __fadd_rn(s.acc[q], __fmul_rn(rr, load(jj, q)));
        } else {
            ++s.bad;
        }
    }
    return s;
}

// ---------------------------------------------------------------------------- host side
// `buffers` (0 .. 2) slices of `elems` floats off a workspace; a null base gives the bytes to ask for
inline size_t carve(void* ws, int buffers, size_t elems, float* buf[2]) {
    gmp::Carver cv(ws, true);
    for (int b = 0; b < buffers; ++b) buf[b] = cv.take<float>(elems);
    return cv.total();
}

// One launch per round, all enqueued at once: round t reads what round t - 1 wrote, the matrix ping-pongs between buf[0] and buf[1]
// (leading dimension ldb) and the last round writes `out`.  launch(t, in, ld_in, out, ld_out, first, last) returns a GMP_* code; the
// first that fails ends the loop.
template <class Launch>
int run_rounds(int rounds, const float* in, int64_t ldi, float* out, int64_t ldo, float* const buf[2], int64_t ldb, Launch launch) {
    for (int t = 0; t < rounds; ++t) {
        const bool last = t + 1 == rounds;
        float* const to = last ? out : buf[t & 1];
        const int64_t ld = last ? ldo : ldb;
        if (int rc = launch(t, in, ldi, to, ld, t == 0, last)) return rc;
        in = to;
        ldi = ld;
    }
    return GMP_OK;
}

}  // namespace prop
