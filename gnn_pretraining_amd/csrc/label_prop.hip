// Degree-normalised propagation of a narrow [n, classes] matrix over a CSR, iterated with a teleport term: label spreading (Zhou et al.
// 2004), label propagation (Zhu & Ghahramani 2002), and what APPNP-style smoothing is made of.  The definition is above
// gmp_label_propagate in include/gnnmp.h; the row sum that fixes the bits and the loop over the rounds are csr_prop.h's.
//
// Mapping.  The width is 1..32, so a row gets a GROUP of CP lanes, CP = the next power of two >= classes, and a wave holds 64 / CP rows;
// lane c of the group owns class c.  A group walks its row entry by entry: `col[k]` is one address for the whole group (one request), the
// neighbour's row of F is CP consecutive floats (one 4 CP-byte segment).  At Cora size F is 76 KB, the CSR 54 KB: both live in L2.
// A hub row is still walked by one group; scripts/bench_label_propagation.py measures that.
#include "csr_prop.h"

namespace {

constexpr int THREADS = 256;
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
        const auto sum = prop::fold_row<1>(rowptr, col, n, nnz, row, right, [&](int j, int) __attribute__((always_inline)) { return fin[(int64_t)j * classes + c]; });
        const int64_t at = row * classes + c;
        const float own = f0[at];
        const float v = __fmul_rn(left ? left[row] : 1.0f, sum.acc[0]);
        const float o = __fadd_rn(__fmul_rn(alpha, v), __fmul_rn(beta, own));
        value = (clamp && clamp[row]) ? own : o;
        fout[at] = value;
        if (residual) diff = __float_as_uint(fabsf(__fsub_rn(value, fin[at])));    // the bits of a non-negative float order like the float
        if (first && c == 0 && sum.bad) atomicAdd(status, sum.bad);
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

bool sizes_ok(int64_t n, int classes) { return n >= 0 && n < LIMIT && classes >= 1 && classes <= MAX_CLASSES; }

}  // namespace

extern "C" size_t gmp_label_propagate_workspace_bytes(int64_t n, int classes) {
    float* buf[2];
    return sizes_ok(n, classes) ? prop::carve(nullptr, 2, (size_t)n * classes, buf) : 0;
}

extern "C" int gmp_label_propagate(const int32_t* rowptr, const int32_t* col, int64_t n, int64_t nnz, const float* left, const float* right,
                                   const float* f0, const float* f_init, const uint8_t* clamp, int classes, int rounds, float alpha, float beta,
                                   float* out, int64_t* pred, float* residual, int32_t* status, void* workspace, size_t workspace_bytes,
                                   gmp_stream_t stream) {
    if (!sizes_ok(n, classes) || nnz < 0 || nnz >= LIMIT || rounds < 1 || rounds > MAX_ROUNDS)
        return gmp::fail(GMP_ERR_ARG, "label_propagate: n=%lld nnz=%lld classes=%d rounds=%d (0 <= n, nnz < 2^31, 1 <= classes <= %d, 1 <= rounds <= %d)",
                         (long long)n, (long long)nnz, classes, rounds, MAX_CLASSES, MAX_ROUNDS);
    if (n == 0) return GMP_OK;
    if (int rc = csr::graph_ok("label_propagate", rowptr, col, n, nnz)) return rc;
    if (!f0 || !out || !status) return gmp::fail(GMP_ERR_ARG, "label_propagate: null pointer");
    const size_t bytes = (size_t)n * classes * sizeof(float);
    if (gmp::overlap(out, bytes, f0, bytes) || gmp::overlap(out, bytes, f_init, bytes)) return gmp::fail(GMP_ERR_ARG, "label_propagate: out aliases f0 or f_init");
    const size_t need = gmp_label_propagate_workspace_bytes(n, classes);
    if (!workspace || workspace_bytes < need)
        return gmp::fail(GMP_ERR_WORKSPACE, "label_propagate: workspace %zu < %zu", workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    float* buf[2];
    prop::carve(workspace, 2, (size_t)n * classes, buf);
    if (hipMemsetAsync(status, 0, 2 * sizeof(int32_t), st) != hipSuccess) return gmp::fail(GMP_ERR_LAUNCH, "label_propagate: memset");
    if (residual && hipMemsetAsync(residual, 0, (size_t)rounds * sizeof(float), st) != hipSuccess)
        return gmp::fail(GMP_ERR_LAUNCH, "label_propagate: memset");
    int cp = 1;
    while (cp < classes) cp *= 2;
    const auto kernel = cp == 1 ? label_prop_round_kernel<1> : cp == 2 ? label_prop_round_kernel<2> : cp == 4 ? label_prop_round_kernel<4>
                      : cp == 8 ? label_prop_round_kernel<8> : cp == 16 ? label_prop_round_kernel<16> : label_prop_round_kernel<32>;
    return prop::run_rounds(rounds, f_init ? f_init : f0, classes, out, classes, buf, classes,
                            [&](int t, const float* fin, int64_t, float* fout, int64_t, bool first, bool last) {
        hipLaunchKernelGGL(kernel, dim3((unsigned)gmp::cdiv(n, THREADS / cp)), dim3(THREADS), 0, st, rowptr, col, (int)n, (int)nnz, left, right, f0, fin,
                           clamp, classes, alpha, beta, fout, last ? pred : nullptr, residual ? (uint32_t*)residual + t : nullptr, status, (int)first,
                           (int)last);
        return gmp::check_launch("label_prop_round_kernel");
    });
}
