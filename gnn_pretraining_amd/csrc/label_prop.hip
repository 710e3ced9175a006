// Degree-normalised propagation of a narrow [n, classes] matrix over a CSR, iterated with a teleport term: label spreading (Zhou et al.
// 2004), label propagation (Zhu & Ghahramani 2002), and what APPNP-style smoothing is made of.  The definition -- every multiply and add
// rounded on its own, a row summed in ascending neighbour order -- is above gmp_label_propagate in include/gnnmp.h.
//
// Mapping.  The width is 1..32, so a row gets a GROUP of CP lanes, CP = the next power of two >= classes, and a wave holds 64 / CP rows;
// lane c of the group owns class c.  A group walks its row entry by entry: `col[k]` is one address for the whole group (one request), the
// neighbour's row of F is CP consecutive floats (one 4 CP-byte segment).  At Cora size F is 76 KB, the CSR 54 KB: both live in L2, and a
// round is a chain of dependent loads (rowptr -> col -> F), not a stream.  So the loop takes UNROLL entries at a time: UNROLL independent
// `col` loads, then UNROLL independent gathers, then the adds in order -- the order of the ADDS is the contract, not that of the loads.
// A hub row is still walked by one group (a row's sum is sequential by definition); scripts/bench_label_propagation.py measures that.
// One launch per round, all enqueued at once; F ping-pongs between two workspace buffers and the last round writes `out`.
#include "gnnmp_internal.h"

namespace {

constexpr int THREADS = 256;
constexpr int UNROLL = 8;
constexpr int MAX_CLASSES = 32;
constexpr int MAX_ROUNDS = 10000;
constexpr int64_t LIMIT = (int64_t)1 << 31;

// first: count the entries outside [0, n) into status[0]; last: write pred and status[1].  residual may be NULL.
template <int CP>
__global__ __launch_bounds__(THREADS) void label_prop_round_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int n, int nnz,
                                                                   const float* __restrict__ left, const float* __restrict__ right,
                                                                   const float* __restrict__ f0, const float* __restrict__ fin,
                                                                   const uint8_t* __restrict__ clamp, int classes, float alpha, float beta,
                                                                   float* __restrict__ fout, int64_t* __restrict__ pred, uint32_t* __restrict__ residual,
                                                                   int32_t* __restrict__ status, int first, int last) {
    constexpr int ROWS = THREADS / CP;
    __shared__ uint32_t red[THREADS / GMP_WAVE];
    const int t = threadIdx.x, c = t % CP;
    const int64_t row = (int64_t)blockIdx.x * ROWS + t / CP;
    const bool live = row < n && c < classes;
    float value = 0.f;
    uint32_t diff = 0;
    if (live) {
        // a rowptr that is no CSR offset reads nothing outside col
        int beg = rowptr[row], end = rowptr[row + 1];
        beg = min(max(beg, 0), nnz);
        end = min(max(end, beg), nnz);
        float acc = 0.f;
        int bad = 0, k = beg;
        for (; k + UNROLL <= end; k += UNROLL) {
            int j[UNROLL];
            float r[UNROLL], f[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) j[u] = col[k + u];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const bool ok = (unsigned)j[u] < (unsigned)n;
                r[u] = ok ? (right ? right[j[u]] : 1.0f) : 0.f;
                f[u] = ok ? fin[(int64_t)j[u] * classes + c] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const bool ok = (unsigned)j[u] < (unsigned)n;
                const float s = __fadd_rn(acc, __fmul_rn(r[u], f[u]));
                acc = ok ? s : acc;                                     // an entry outside the graph is skipped, not added as zero
                bad += ok ? 0 : 1;
            }
        }
        for (; k < end; ++k) {
            const int jj = col[k];
            if ((unsigned)jj < (unsigned)n) acc = __fadd_rn(acc, __fmul_rn(right ? right[jj] : 1.0f, fin[(int64_t)jj * classes + c]));
            else ++bad;
        }
        const int64_t at = row * classes + c;
        const float own = f0[at];
        const float v = __fmul_rn(left ? left[row] : 1.0f, acc);
        const float o = __fadd_rn(__fmul_rn(alpha, v), __fmul_rn(beta, own));
        value = (clamp && clamp[row]) ? own : o;
        fout[at] = value;
        if (residual) diff = __float_as_uint(fabsf(__fsub_rn(value, fin[at])));    // the bits of a non-negative float order like the float
        if (first && c == 0 && bad) atomicAdd(status, bad);
    }
    if (last) {
        // argmax of the row over the group's lanes: key = (orderable score bits, ~class), integer compares only; idle lanes hold key 0
        gmp::u64 key = live ? gmp::pack_key(value, 0xffffffffu - (uint32_t)c) : 0ull;
#pragma unroll
        for (int o = CP / 2; o > 0; o >>= 1) {
            const gmp::u64 other = __shfl_xor(key, o, GMP_WAVE);
            key = other > key ? other : key;
        }
        if (live && c == 0) {
            if (pred) pred[row] = (int64_t)gmp::key_low(key);
            if (!(gmp::key_score(key) > 0.f)) atomicAdd(status + 1, 1);
        }
    }
    if (residual) {
        // integer max: by the wave's shuffle tree, the four waves through LDS, one atomic per workgroup -- independent of any order
#pragma unroll
        for (int o = GMP_WAVE / 2; o > 0; o >>= 1) diff = max(diff, (uint32_t)__shfl_xor((int)diff, o, GMP_WAVE));
        if (t % GMP_WAVE == 0) red[t / GMP_WAVE] = diff;
        __syncthreads();
        if (t == 0) {
            uint32_t m = red[0];
#pragma unroll
            for (int w = 1; w < THREADS / GMP_WAVE; ++w) m = max(m, red[w]);
            if (m) atomicMax(residual, m);
        }
    }
}

template <int CP>
int launch_round(const int32_t* rowptr, const int32_t* col, int n, int nnz, const float* left, const float* right, const float* f0, const float* fin,
                 const uint8_t* clamp, int classes, float alpha, float beta, float* fout, int64_t* pred, uint32_t* residual, int32_t* status, int first,
                 int last, hipStream_t st) {
    hipLaunchKernelGGL((label_prop_round_kernel<CP>), dim3((unsigned)gmp::cdiv(n, THREADS / CP)), dim3(THREADS), 0, st, rowptr, col, n, nnz, left, right,
                       f0, fin, clamp, classes, alpha, beta, fout, pred, residual, status, first, last);
    return gmp::check_launch("label_prop_round_kernel");
}

bool sizes_ok(int64_t n, int classes) { return n >= 0 && n < LIMIT && classes >= 1 && classes <= MAX_CLASSES; }

}  // namespace

extern "C" size_t gmp_label_propagate_workspace_bytes(int64_t n, int classes) {
    if (!sizes_ok(n, classes)) return 0;
    gmp::Carver cv(nullptr, true);
    cv.take<float>((size_t)n * classes);
    cv.take<float>((size_t)n * classes);
    return cv.total();
}

extern "C" int gmp_label_propagate(const int32_t* rowptr, const int32_t* col, int64_t n, int64_t nnz, const float* left, const float* right,
                                   const float* f0, const float* f_init, const uint8_t* clamp, int classes, int rounds, float alpha, float beta,
                                   float* out, int64_t* pred, float* residual, int32_t* status, void* workspace, size_t workspace_bytes,
                                   gmp_stream_t stream) {
    if (!sizes_ok(n, classes) || nnz < 0 || nnz >= LIMIT || rounds < 1 || rounds > MAX_ROUNDS)
        return gmp::fail(GMP_ERR_ARG, "label_propagate: n=%lld nnz=%lld classes=%d rounds=%d (0 <= n, nnz < 2^31, 1 <= classes <= %d, 1 <= rounds <= %d)",
                         (long long)n, (long long)nnz, classes, rounds, MAX_CLASSES, MAX_ROUNDS);
    if (n == 0) return GMP_OK;
    if (!rowptr || (!col && nnz > 0) || !f0 || !out || !status) return gmp::fail(GMP_ERR_ARG, "label_propagate: null pointer");
    const size_t bytes = (size_t)n * classes * sizeof(float);
    if (gmp::overlap(out, bytes, f0, bytes) || gmp::overlap(out, bytes, f_init, bytes)) return gmp::fail(GMP_ERR_ARG, "label_propagate: out aliases f0 or f_init");
    const size_t need = gmp_label_propagate_workspace_bytes(n, classes);
    if (!workspace || workspace_bytes < need)
        return gmp::fail(GMP_ERR_WORKSPACE, "label_propagate: workspace %zu < %zu", workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    gmp::Carver cv(workspace, true);
    float* const buf[2] = {cv.take<float>((size_t)n * classes), cv.take<float>((size_t)n * classes)};
    if (hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st) != hipSuccess) return gmp::fail(GMP_ERR_LAUNCH, "label_propagate: memset");
    if (residual && hipMemsetAsync(residual, 0, (size_t)rounds * sizeof(float), st) != hipSuccess)
        return gmp::fail(GMP_ERR_LAUNCH, "label_propagate: memset");
    const float* fin = f_init ? f_init : f0;
    for (int t = 0; t < rounds; ++t) {
        const int first = t == 0, last = t + 1 == rounds;
        float* const fout = last ? out : buf[t & 1];
        uint32_t* const res = residual ? (uint32_t*)residual + t : nullptr;
        int rc;
#define GMP_LP_ROUND(CP)                                                                                                                       \
    rc = launch_round<CP>(rowptr, col, (int)n, (int)nnz, left, right, f0, fin, clamp, classes, alpha, beta, fout, last ? pred : nullptr, res, status, \
                          first, last, st)
        if (classes == 1) GMP_LP_ROUND(1);
        else if (classes == 2) GMP_LP_ROUND(2);
        else if (classes <= 4) GMP_LP_ROUND(4);
        else if (classes <= 8) GMP_LP_ROUND(8);
        else if (classes <= 16) GMP_LP_ROUND(16);
        else GMP_LP_ROUND(32);
#undef GMP_LP_ROUND
        if (rc) return rc;
        fin = fout;
    }
    return GMP_OK;
}
