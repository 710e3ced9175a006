// Structural link-prediction baselines on the CSR of a simple undirected graph (rows strictly ascending, symmetric, no loops): the weighted
// common-neighbour sum S_w(s, c) = sum over z in N(s) & N(c) of w[z] (w == NULL: 1, common neighbours; 1 / ln deg: Adamic-Adar; 1 / deg:
// resource allocation) and the Jaccard coefficient CN / (deg s + deg c - CN).
//   gmp_lp_cn_score        P explicit pairs: the score of each
//   gmp_lp_cn_rank         Q true pairs: the true pair's score and how many candidates c in [0, N) score greater than / equal to it (c == src,
//                          c == dst and the entries of src's filter row are skipped) -- gmp_lp_rank's filtered rank, with these scorers
//   gmp_graph_simple_check how many entries of a CSR break the assumptions above
// A score is an fp32 sum that starts at 0.0f and adds w[z] in ascending z with plain adds, in both kernels: a pair scored explicitly and the
// same pair met as a ranking candidate have the same bits.  Jaccard is compared exactly, a / b against c / d as a d against c b in int64.
//
//   cn_pair_kernel    one wave per pair: 64 entries of the shorter row are looked up in the longer one by binary search at a time, the hits'
//                     weights are added lane by lane in ascending order; for gmp_lp_cn_rank it also sets the two counts to zero
//   cn_count_kernel   one block per (query, tile of TC consecutive candidates): an fp32 accumulator per candidate in LDS.  PUSH form: for z
//                     in N(s) ascending, the part of z's row inside the tile (two binary searches, made for 256 z at once, one per thread) gets
//                     w[z] added; a row has no duplicates, so no two lanes meet in a slot within one z, and a barrier between two z keeps the
//                     order -- no float atomic.  Then the filter row as a bitmap in LDS, compare, count in LDS, one integer atomicAdd per
//                     count and block.  No per-candidate score reaches global memory.
//   simple_check_kernel  one wave per row
// Every read of col is bounded by rowptr clamped to [0, nnz], every entry outside [0, N) is skipped and every LDS slot index is checked: a
// CSR that breaks the assumptions gives wrong numbers, never an access outside the arrays.
#include "csr_graph.h"
#include "lp_filter.h"

namespace {

constexpr int TC = 4096;            // candidates per tile: 16 KiB of accumulator
constexpr int THREADS = 256;
constexpr int WAVES = THREADS / GMP_WAVE;
constexpr int MODE_SUM = 0, MODE_JACCARD = 1;

using namespace csr;                // Row, row_of, graph_ok

// the first i in [lo, hi) with col[i] >= key (hi if none)
__device__ __forceinline__ int64_t lower_bound(const int32_t* __restrict__ col, int64_t lo, int64_t hi, int64_t key) {
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if ((int64_t)col[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// Jaccard's exact order: cn / uni against tcn / tuni, a zero union scoring 0
__device__ __forceinline__ int jaccard_cmp(int64_t cn, int64_t uni, int64_t tcn, int64_t tuni) {
    if (uni <= 0) { cn = 0; uni = 1; }
    if (tuni <= 0) { tcn = 0; tuni = 1; }
    const int64_t l = cn * tuni, r = tcn * uni;
    return l > r ? 1 : (l == r ? 0 : -1);
}

__global__ __launch_bounds__(THREADS) void cn_pair_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N,
                                                          int64_t nnz, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                          int64_t P, const float* __restrict__ weight, int mode, float* __restrict__ score,
                                                          int32_t* __restrict__ n_greater, int32_t* __restrict__ n_equal) {
    const int lane = threadIdx.x % GMP_WAVE;
    const int64_t p = (int64_t)blockIdx.x * WAVES + threadIdx.x / GMP_WAVE;
    if (p >= P) return;                                             // (wave-uniform)
    const Row rs = row_of(rowptr, nnz, N, src[p]), rd = row_of(rowptr, nnz, N, dst[p]);
    const bool s_short = rs.e - rs.b <= rd.e - rd.b;                // the same set in the same order either way
    const Row a = s_short ? rs : rd, b = s_short ? rd : rs;
    float sum = 0.f;
    int64_t cn = 0;
    for (int64_t base = a.b; base < a.e; base += GMP_WAVE) {
        const int64_t i = base + lane;
        bool hit = false;
        float w = 0.f;
        if (i < a.e) {
            const int64_t z = col[i];
            if (z >= 0 && z < N) {
                const int64_t pos = lower_bound(col, b.b, b.e, z);
                hit = pos < b.e && (int64_t)col[pos] == z;
                if (hit) w = weight ? weight[z] : 1.f;
            }
        }
        unsigned long long m = __ballot(hit);
        cn += __popcll(m);
        while (m) {                                                 // the hits in ascending z, one add each
            sum += __shfl(w, __ffsll(m) - 1, GMP_WAVE);
            m &= m - 1;
        }
    }
    if (lane == 0) {
        if (mode == MODE_JACCARD) {
            const int64_t uni = (rs.e - rs.b) + (rd.e - rd.b) - cn;
            score[p] = uni > 0 ? (float)cn / (float)uni : 0.f;
        } else {
            score[p] = sum;
        }
        if (n_greater) {
            n_greater[p] = 0;
            n_equal[p] = 0;
        }
    }
}

__global__ __launch_bounds__(THREADS) void cn_count_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N,
                                                           int64_t nnz, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                           int tiles, const float* __restrict__ weight, int mode,
                                                           const int32_t* __restrict__ frowptr, const int32_t* __restrict__ fcol, int64_t fnnz,
                                                           const float* __restrict__ score_true, int32_t* __restrict__ n_greater,
                                                           int32_t* __restrict__ n_equal) {
    __shared__ float acc[TC];
    __shared__ unsigned int fbits[TC / 32];
    __shared__ int64_t zlo[THREADS], zhi[THREADS];
    __shared__ float zw[THREADS];
    __shared__ int cnt[3];                                          // greater, equal, the true pair's common neighbours (Jaccard)
    const int t = threadIdx.x;
    const int64_t q = blockIdx.x / (unsigned)tiles, c0 = (int64_t)(blockIdx.x % (unsigned)tiles) * TC;
    const int64_t s = src[q], d = dst[q];
    const Row rs = row_of(rowptr, nnz, N, s);
    for (int r = t; r < TC; r += THREADS) acc[r] = 0.f;
    if (t < TC / 32) fbits[t] = 0u;
    if (t < 3) cnt[t] = 0;
    __syncthreads();
    for (int64_t base = rs.b; base < rs.e; base += THREADS) {
        if (base > rs.b) __syncthreads();                           // the previous chunk's zlo, zhi, zw are read
        const int64_t i = base + t;
        int64_t lo = 0, hi = 0;
        float w = 0.f;
        if (i < rs.e) {
            const int64_t z = col[i];
            if (z >= 0 && z < N) {
                const Row rz = row_of(rowptr, nnz, N, z);
                lo = lower_bound(col, rz.b, rz.e, c0);
                hi = lower_bound(col, lo, rz.e, c0 + TC);
                w = weight ? weight[z] : 1.f;
            }
        }
        zlo[t] = lo;
        zhi[t] = hi;
        zw[t] = w;
        __syncthreads();
        const int n = (int)min((int64_t)THREADS, rs.e - base);
        for (int j = 0; j < n; ++j) {                               // z ascending
            const int64_t jlo = zlo[j], jhi = zhi[j];
            if (jlo >= jhi) continue;                               // (block-uniform: nothing of this row in the tile, nothing to order)
            const float jw = zw[j];
            for (int64_t k = jlo + t; k < jhi; k += THREADS) {
                const uint64_t off = (uint64_t)((int64_t)col[k] - c0);
                if (off < (uint64_t)TC) acc[off] += jw;
            }
            __syncthreads();
        }
    }
    lpf::mark<TC / 32, THREADS>(frowptr, fcol, fnnz, s, N, c0, fbits);     // gmp_lp_rank's filter row
    const Row rd = row_of(rowptr, nnz, N, d);
    if (mode == MODE_JACCARD) {                                     // the true pair's count again, as an integer: the float quotient does not carry it
        for (int64_t i = rs.b + t; i < rs.e; i += THREADS) {
            const int64_t z = col[i];
            if (z < 0 || z >= N) continue;
            const int64_t pos = lower_bound(col, rd.b, rd.e, z);
            if (pos < rd.e && (int64_t)col[pos] == z) atomicAdd(&cnt[2], 1);
        }
    }
    __syncthreads();
    const float st = score_true[q];
    const int64_t deg_s = rs.e - rs.b, tcn = cnt[2], tuni = deg_s + (rd.e - rd.b) - tcn;
    int greater = 0, equal = 0;
    for (int r = t; r < TC; r += THREADS) {
        const int64_t c = c0 + r;
        if (c >= N || c == s || c == d || lpf::marked(fbits, r)) continue;
        int cmp;
        if (mode == MODE_JACCARD) {
            const Row rc = row_of(rowptr, nnz, N, c);
            const int64_t cn = (int64_t)acc[r];
            cmp = jaccard_cmp(cn, deg_s + (rc.e - rc.b) - cn, tcn, tuni);
        } else {
            const float v = acc[r];
            cmp = v > st ? 1 : (v == st ? 0 : -1);
        }
        greater += cmp > 0;
        equal += cmp == 0;
    }
    if (greater) atomicAdd(&cnt[0], greater);
    if (equal) atomicAdd(&cnt[1], equal);
    __syncthreads();
    if (t == 0) {
        if (cnt[0]) atomicAdd(&n_greater[q], cnt[0]);
        if (cnt[1]) atomicAdd(&n_equal[q], cnt[1]);
    }
}

__global__ __launch_bounds__(THREADS) void simple_check_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N,
                                                               int64_t nnz, int32_t* __restrict__ violations) {
    const int lane = threadIdx.x % GMP_WAVE;
    const int64_t v = (int64_t)blockIdx.x * WAVES + threadIdx.x / GMP_WAVE;
    if (v >= N) return;                                             // (wave-uniform)
    const int64_t rb = rowptr[v], re = rowptr[v + 1];
    int bad = 0;
    if (lane == 0) bad += (rb < 0 || re < rb || re > nnz) + (v == 0 && rb != 0) + (v == N - 1 && re != nnz);
    const Row r = row_of(rowptr, nnz, N, v);
    for (int64_t i = r.b + lane; i < r.e; i += GMP_WAVE) {
        const int64_t c = col[i];
        bool ok = c >= 0 && c < N && c != v && (i == r.b || (int64_t)col[i - 1] < c);
        if (ok) {                                                   // the mirror entry (c, v)
            const Row rc = row_of(rowptr, nnz, N, c);
            const int64_t pos = lower_bound(col, rc.b, rc.e, v);
            ok = pos < rc.e && (int64_t)col[pos] == v;
        }
        bad += !ok;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o, GMP_WAVE);
    if (lane == 0 && bad) atomicAdd(&violations[0], bad);
}

int scorer_ok(const char* who, const void* weight, int mode) {
    if (mode != MODE_SUM && mode != MODE_JACCARD) return gmp::fail(GMP_ERR_ARG, "%s: mode=%d (0 = weighted sum, 1 = Jaccard)", who, mode);
    if (weight && mode == MODE_JACCARD) return gmp::fail(GMP_ERR_ARG, "%s: Jaccard takes no weight array", who);
    return GMP_OK;
}

int launch_pairs(const char* who, const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int64_t* src, const int64_t* dst,
                 int64_t P, const float* weight, int mode, float* score, int32_t* n_greater, int32_t* n_equal, hipStream_t st) {
    const int64_t blocks = (P + WAVES - 1) / WAVES;
    if (blocks >= ((int64_t)1 << 31)) return gmp::fail(GMP_ERR_ARG, "%s: %lld pairs exceed one grid", who, (long long)P);
    hipLaunchKernelGGL(cn_pair_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, rowptr, col, N, nnz, src, dst, P, weight, mode, score,
                       n_greater, n_equal);
    return gmp::check_launch("cn_pair_kernel");
}

}  // namespace

extern "C" int gmp_lp_cn_tile_nodes(void) { return TC; }

extern "C" size_t gmp_lp_cn_rank_workspace_bytes(int64_t Q, int64_t N) {
    (void)Q; (void)N;
    return 0;                                                       // the counts are integer atomics on the outputs: nothing is staged
}

extern "C" int gmp_lp_cn_score(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int64_t* src, const int64_t* dst,
                               int64_t P, const float* weight, int mode, float* score, gmp_stream_t stream) {
    if (int rc = graph_ok("lp_cn_score", rowptr, col, N, nnz)) return rc;
    if (int rc = scorer_ok("lp_cn_score", weight, mode)) return rc;
    if (P < 0) return gmp::fail(GMP_ERR_ARG, "lp_cn_score: P=%lld", (long long)P);
    if (P == 0) return GMP_OK;
    if (!src || !dst || !score) return gmp::fail(GMP_ERR_ARG, "lp_cn_score: null pointer");
    return launch_pairs("lp_cn_score", rowptr, col, N, nnz, src, dst, P, weight, mode, score, nullptr, nullptr, (hipStream_t)stream);
}

extern "C" int gmp_lp_cn_rank(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int64_t* src, const int64_t* dst,
                              int64_t Q, const float* weight, int mode, const int32_t* filter_rowptr, const int32_t* filter_col,
                              int64_t filter_nnz, float* score_true, int32_t* n_greater, int32_t* n_equal, void* workspace,
                              size_t workspace_bytes, gmp_stream_t stream) {
    (void)workspace; (void)workspace_bytes;
    if (int rc = graph_ok("lp_cn_rank", rowptr, col, N, nnz)) return rc;
    if (int rc = scorer_ok("lp_cn_rank", weight, mode)) return rc;
    bool done;
    if (int rc = lpf::rank_front("lp_cn_rank", Q, filter_rowptr, filter_col, filter_nnz, src, dst, score_true, n_greater, n_equal, done); rc || done)
        return rc;
    const int64_t tiles = (N + TC - 1) / TC;
    if (int rc = lpf::grid_ok("lp_cn_rank", Q, tiles)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (int rc = launch_pairs("lp_cn_rank", rowptr, col, N, nnz, src, dst, Q, weight, mode, score_true, n_greater, n_equal, st)) return rc;
    if (tiles == 0) return GMP_OK;
    hipLaunchKernelGGL(cn_count_kernel, dim3((unsigned)(Q * tiles)), dim3(THREADS), 0, st, rowptr, col, N, nnz, src, dst, (int)tiles, weight, mode,
                       filter_rowptr, filter_col, filter_nnz, (const float*)score_true, n_greater, n_equal);
    return gmp::check_launch("cn_count_kernel");
}

extern "C" int gmp_graph_simple_check(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, int32_t* violations,
                                      gmp_stream_t stream) {
    if (int rc = graph_ok("graph_simple_check", rowptr, col, N, nnz)) return rc;
    if (!violations) return gmp::fail(GMP_ERR_ARG, "graph_simple_check: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(violations, 0, sizeof(int32_t), st) != hipSuccess) return gmp::fail(GMP_ERR_LAUNCH, "graph_simple_check: memset");
    if (N == 0) return GMP_OK;
    hipLaunchKernelGGL(simple_check_kernel, dim3((unsigned)((N + WAVES - 1) / WAVES)), dim3(THREADS), 0, st, rowptr, col, N, nnz, violations);
    return gmp::check_launch("simple_check_kernel");
}
