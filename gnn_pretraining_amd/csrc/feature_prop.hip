// Degree-scaled propagation of a WIDE [n, d] feature matrix over a CSR, H <- diag(left) A diag(right) H for `rounds` rounds: the S^K X of
// SGC (Wu et al. 2019), 1 <= d <= 16384, dense or CSR features in.  The definition -- every multiply and add rounded on its own, a row
// summed in ascending neighbour order, no floating-point atomic -- is above gmp_feature_propagate in include/gnnmp.h; per column it is
// gmp_label_propagate with alpha = 1, beta = 0 and no clamp, with the same bits.
//
// Dense round.  One wave per (row, strip of 256 columns): lane l owns the columns strip * 256 + l + 64 q, q = 0 .. 3, so a neighbour's
// row is read as four coalesced 256-byte segments, and the row's four sums per lane are prop::fold_row<4> (csr_prop.h).  All loads and
// stores are single dwords: a leading dimension such as CiteSeer's 3,703 puts no row but the first on 16 bytes, so this scalar path is
// the only one there is (a dwordx4 form would need base and leading dimension to be multiples of 16 bytes and was not worth a second
// kernel).  The row index is wave-uniform (readfirstlane), so rowptr, col and right travel through the scalar cache, and a neighbour's
// row address is a scalar.  A hub row is walked sequentially by one wave per strip; scripts/bench_sgc.py measures it on a star graph.
//
// Sparse first round (CSR features in, dense H_1 out).  One wave owns an output row and accumulates it in an LDS strip of dpad floats,
// zeroed first; the workgroup holds as many waves (1 .. 4) as fit 64 KiB of strips, so the strip size follows d and nothing is assumed.
// Neighbours are walked in ascending order; the lanes take one neighbour's non-zeros in parallel -- distinct columns, so every column's
// sum still sees its terms in neighbour order -- and a wave's LDS operations complete in program order, so consecutive neighbours need no
// barrier.  The first 64 non-zeros of UNROLL_S neighbours are loaded together before their updates are applied in order.  Then the strip
// is scaled by left and written out.
#include "csr_prop.h"

namespace {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / GMP_WAVE;
constexpr int STRIP = 256;                     // columns per wave of the dense round
constexpr int PER_LANE = STRIP / GMP_WAVE;
constexpr int UNROLL_S = 4;
constexpr int MAX_DIM = 16384;
constexpr int MAX_ROUNDS = 64;
constexpr int LDS_BUDGET = 64 * 1024;          // the sparse round's strips per workgroup: no opt-in needed, two workgroups fit a CU
constexpr int64_t LIMIT = (int64_t)1 << 31;

// grid (cdiv(n, WAVES), cdiv(d, STRIP)).  first: count the entries outside [0, n) into status[0] (the strip-0 waves do).
__global__ __launch_bounds__(THREADS) void feature_prop_dense_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int n, int nnz,
                                                                     const float* __restrict__ left, const float* __restrict__ right,
                                                                     const float* __restrict__ hin, int64_t ldi, int d, float* __restrict__ hout,
                                                                     int64_t ldo, int32_t* __restrict__ status, int first) {
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / GMP_WAVE), lane = threadIdx.x % GMP_WAVE;
    const int64_t row = (int64_t)blockIdx.x * WAVES + wave;
    if (row >= n) return;
    const int c0 = (int)blockIdx.y * STRIP + lane;
    bool in[PER_LANE];
    int cq[PER_LANE];                                                       // a lane's column past the row's end reads the last one instead:
#pragma unroll                                                              // no test in the loop, and its sum is never stored
    for (int q = 0; q < PER_LANE; ++q) {
        in[q] = c0 + q * GMP_WAVE < d;
        cq[q] = in[q] ? c0 + q * GMP_WAVE : d - 1;
    }
    const auto sum = prop::fold_row<PER_LANE>(rowptr, col, n, nnz, row, right, [&](int j, int q) __attribute__((always_inline)) {
        return (hin + (int64_t)j * ldi)[cq[q]];                             // a uniform 64-bit row address plus the lane's column
    });
    const float l = left ? left[row] : 1.0f;
    float* dst = hout + row * ldo + c0;
#pragma unroll
    for (int q = 0; q < PER_LANE; ++q)
        if (in[q]) dst[q * GMP_WAVE] = __fmul_rn(l, sum.acc[q]);
    if (first && blockIdx.y == 0 && lane == 0 && sum.bad) atomicAdd(status, sum.bad);
}

// One neighbour's entries e = from + lane, from + lane + 64, ... < xe added into the wave's strip: an entry whose column lies outside
// [0, d) or is not greater than the stored column before it is skipped (it is counted elsewhere, once per entry).
__device__ __forceinline__ void add_entries(float* __restrict__ strip, const int32_t* __restrict__ x_col, const float* __restrict__ x_val, int xb,
                                            int from, int xe, int d, float r) {
    for (int e = from; e < xe; e += GMP_WAVE) {
        const int c = x_col[e], prev = e > xb ? x_col[e - 1] : -1;
        const float v = x_val[e];
        if ((unsigned)c < (unsigned)d && c > prev) strip[c] = __fadd_rn(strip[c], __fmul_rn(r, v));
    }
}

// grid cdiv(n, waves), `waves` waves per workgroup, waves * dpad floats of dynamic LDS.  Always the first round: counts status[0] and
// status[1] (feature row `row`'s bad entries, by the wave that owns output row `row`: every entry once).
__global__ __launch_bounds__(THREADS) void feature_prop_sparse_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int n, int nnz,
                                                                      const float* __restrict__ left, const float* __restrict__ right,
                                                                      const int32_t* __restrict__ x_rowptr, const int32_t* __restrict__ x_col,
                                                                      const float* __restrict__ x_val, int x_nnz, int d, int dpad, int waves,
                                                                      float* __restrict__ hout, int64_t ldo, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) float strips[];
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / GMP_WAVE), lane = threadIdx.x % GMP_WAVE;
    const int64_t row = (int64_t)blockIdx.x * waves + wave;
    if (row >= n) return;                                                   // no workgroup barrier below: a wave may leave alone
    float* const strip = strips + (size_t)wave * dpad;
    for (int c = lane; c < dpad; c += GMP_WAVE) strip[c] = 0.f;
    {
        const csr::Row own = csr::row_of(x_rowptr, x_nnz, row);
        const int xb = (int)own.b, xe = (int)own.e;
        int wrong = 0;
        for (int e = xb + lane; e < xe; e += GMP_WAVE) {
            const int c = x_col[e], prev = e > xb ? x_col[e - 1] : -1;
            wrong += ((unsigned)c < (unsigned)d && c > prev) ? 0 : 1;
        }
#pragma unroll
        for (int o = GMP_WAVE / 2; o > 0; o >>= 1) wrong += __shfl_xor(wrong, o, GMP_WAVE);
        if (lane == 0 && wrong) atomicAdd(status + 1, wrong);
    }
    gmp::wave_sync();
    const csr::Row adj = csr::row_of(rowptr, nnz, row);                     // a rowptr that is no CSR offset reads nothing outside col
    const int end = (int)adj.e;
    int bad = 0, k = (int)adj.b;
    for (; k + UNROLL_S <= end; k += UNROLL_S) {
        int j[UNROLL_S], xb[UNROLL_S], xe[UNROLL_S], c[UNROLL_S], prev[UNROLL_S];
        float r[UNROLL_S], v[UNROLL_S];
#pragma unroll
        for (int u = 0; u < UNROLL_S; ++u) j[u] = col[k + u];
#pragma unroll
        for (int u = 0; u < UNROLL_S; ++u) {
            const bool ok = prop::inside(j[u], n);
            const int js = ok ? j[u] : 0;                                           // a stray entry reads row 0 and takes none of it: no
            r[u] = prop::right_of(right, js);                                       // branch, so the scalar loads of all four are in flight
            const csr::Row xs = csr::row_of(x_rowptr, x_nnz, js);
            xb[u] = (int)xs.b;
            xe[u] = ok ? (int)xs.e : xb[u];
            bad += ok ? 0 : 1;
        }
#pragma unroll
        for (int u = 0; u < UNROLL_S; ++u) {
            const int e = xb[u] + lane;
            const bool has = e < xe[u];
            c[u] = has ? x_col[e] : -1;
            prev[u] = (has && e > xb[u]) ? x_col[e - 1] : -1;
            v[u] = has ? x_val[e] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < UNROLL_S; ++u) {
            if ((unsigned)c[u] < (unsigned)d && c[u] > prev[u]) strip[c[u]] = __fadd_rn(strip[c[u]], __fmul_rn(r[u], v[u]));
            add_entries(strip, x_col, x_val, xb[u], xb[u] + lane + GMP_WAVE, xe[u], d, r[u]);
            gmp::wave_sync();
        }
    }
    for (; k < end; ++k) {
        const int jj = col[k];
        if (prop::inside(jj, n)) {
            const csr::Row xs = csr::row_of(x_rowptr, x_nnz, jj);
            add_entries(strip, x_col, x_val, (int)xs.b, (int)xs.b + lane, (int)xs.e, d, prop::right_of(right, jj));
            gmp::wave_sync();
        } else {
            ++bad;
        }
    }
    const float l = left ? left[row] : 1.0f;
    float* dst = hout + row * ldo;
    for (int c = lane; c < d; c += GMP_WAVE) dst[c] = __fmul_rn(l, strip[c]);
    if (lane == 0 && bad) atomicAdd(status, bad);
}

int dpad_of(int d) { return (d + 3) & ~3; }

bool sizes_ok(int64_t n, int d, int rounds) { return n >= 0 && n < LIMIT && d >= 1 && d <= MAX_DIM && rounds >= 1 && rounds <= MAX_ROUNDS; }

int buffers_of(int rounds) { return rounds - 1 < 2 ? rounds - 1 : 2; }

// the bytes from the first to the last element of an [n, d] matrix with leading dimension ld
size_t span(int64_t n, int d, int64_t ld) { return n > 0 ? ((size_t)(n - 1) * (size_t)ld + (size_t)d) * sizeof(float) : 0; }

}  // namespace

extern "C" size_t gmp_feature_propagate_workspace_bytes(int64_t n, int32_t d, int32_t rounds) {
    float* buf[2];
    return sizes_ok(n, d, rounds) && rounds > 1 ? prop::carve(nullptr, buffers_of(rounds), (size_t)n * dpad_of(d), buf) : 0;
}

extern "C" int gmp_feature_propagate(const int32_t* rowptr, const int32_t* col, int64_t n, int64_t nnz, const float* left, const float* right,
                                     const float* x, int64_t ldx, const int32_t* x_rowptr, const int32_t* x_col, const float* x_val,
                                     int64_t x_nnz, int32_t d, int32_t rounds, float* out, int64_t ldo, int32_t* status, void* ws,
                                     size_t ws_bytes, gmp_stream_t stream) {
    const bool dense = x != nullptr, sparse = x_rowptr != nullptr || x_col != nullptr || x_val != nullptr;
    if (!sizes_ok(n, d, rounds) || nnz < 0 || nnz >= LIMIT)
        return gmp::fail(GMP_ERR_ARG, "feature_propagate: n=%lld nnz=%lld d=%d rounds=%d (0 <= n, nnz < 2^31, 1 <= d <= %d, 1 <= rounds <= %d)",
                         (long long)n, (long long)nnz, d, rounds, MAX_DIM, MAX_ROUNDS);
    if (n == 0) return GMP_OK;
    if (dense == sparse) return gmp::fail(GMP_ERR_ARG, "feature_propagate: exactly one of the dense x and the CSR x_rowptr / x_col / x_val is given");
    if (ldo < d || (dense && ldx < d)) return gmp::fail(GMP_ERR_ARG, "feature_propagate: ldx=%lld ldo=%lld for d=%d (ld >= d)", (long long)ldx, (long long)ldo, d);
    if (sparse && (x_nnz < 0 || x_nnz >= LIMIT || !x_rowptr || (x_nnz > 0 && (!x_col || !x_val))))
        return gmp::fail(GMP_ERR_ARG, "feature_propagate: x_nnz=%lld (0 <= x_nnz < 2^31) or a null x_rowptr / x_col / x_val", (long long)x_nnz);
    if (int rc = csr::graph_ok("feature_propagate", rowptr, col, n, nnz)) return rc;
    if (!out || !status) return gmp::fail(GMP_ERR_ARG, "feature_propagate: null pointer");
    const size_t out_bytes = span(n, d, ldo);
    if ((dense && gmp::overlap(out, out_bytes, x, span(n, d, ldx))) || (sparse && gmp::overlap(out, out_bytes, x_val, (size_t)x_nnz * sizeof(float))))
        return gmp::fail(GMP_ERR_ARG, "feature_propagate: out overlaps x");
    const size_t need = gmp_feature_propagate_workspace_bytes(n, d, rounds);
    if (need && (!ws || ws_bytes < need)) return gmp::fail(GMP_ERR_ARG, "feature_propagate: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, need);
    if (need && gmp::overlap(out, out_bytes, ws, ws_bytes)) return gmp::fail(GMP_ERR_ARG, "feature_propagate: out overlaps the workspace");
    hipStream_t st = (hipStream_t)stream;
    const int dpad = dpad_of(d);
    float* buf[2] = {nullptr, nullptr};
    if (need) prop::carve(ws, buffers_of(rounds), (size_t)n * dpad, buf);
    if (hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st) != hipSuccess) return gmp::fail(GMP_ERR_LAUNCH, "feature_propagate: memset");
    return prop::run_rounds(rounds, x, ldx, out, ldo, buf, dpad, [&](int t, const float* hin, int64_t ldi, float* hout, int64_t ldh, bool first, bool) {
        if (first && sparse) {
            // the strip size follows d: as many waves as fit the budget, one at least (d = 16384 is exactly 64 KiB)
            int waves = LDS_BUDGET / (dpad * (int)sizeof(float));
            waves = waves < 1 ? 1 : (waves > WAVES ? WAVES : waves);
            hipLaunchKernelGGL(feature_prop_sparse_kernel, dim3((unsigned)gmp::cdiv(n, waves)), dim3(waves * GMP_WAVE),
                               (size_t)waves * dpad * sizeof(float), st, rowptr, col, (int)n, (int)nnz, left, right, x_rowptr, x_col, x_val, (int)x_nnz, d,
                               dpad, waves, hout, ldh, status);
            return gmp::check_launch("feature_prop_sparse_kernel");
        }
        hipLaunchKernelGGL(feature_prop_dense_kernel, dim3((unsigned)gmp::cdiv(n, WAVES), (unsigned)gmp::cdiv(d, STRIP)), dim3(THREADS), 0, st, rowptr, col,
                           (int)n, (int)nnz, left, right, hin, ldi, d, hout, ldh, status, (int)first);
        return gmp::check_launch("feature_prop_dense_kernel");
    });
}
