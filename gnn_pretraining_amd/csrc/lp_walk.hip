// Walk-based link-prediction baselines on the CSR of a simple undirected graph (the contract of lp_heuristics.hip): the damped walk sum
// acc = sum over l <= R of y_l, y_l = a A diag(w) y_{l-1}, y_0 = e_s (Katz: w = 1, a = beta; rooted PageRank: w = 1 / deg, a = 1 - alpha),
// and the hop distance cut at R.  The definition, with its order of operations, is above gmp_lp_walk_score in include/gnnmp.h.
//   gmp_lp_walk_score  P explicit pairs: the score of each; a run of equal sources is propagated once
//   gmp_lp_walk_rank   Q true pairs: the true pair's score and how many candidates c in [0, N) score greater than / equal to it (c == src,
//                      c == dst and the entries of src's filter row are skipped) -- gmp_lp_rank's filtered rank, with these scorers
//
//   walk_kernel<T, REGS>  one workgroup of T threads per source.  REGS > 0 (N <= LDS_NODES): y_prev, y_next (a float per node each) and the
//                        filter bitmap live in dynamic LDS sized by this call's N, and acc in registers -- thread t owns the rows t, t + T,
//                        ..., at most REGS of them -- until the last round is over, when it is parked in the y buffer that has fallen
//                        free.  REGS == 0: the three vectors and the bitmap live in the block's slice of the workspace, and RESIDENT
//                        blocks loop over the queries.  All instances run the same operations in the same order, so they give the same
//                        bits.  A round is a PULL pass: a thread folds w[z] y_prev[z] over each of its rows in ascending z with plain
//                        adds, writes y_next[v] and adds it to acc[v]; a barrier between two rounds.  No float atomic: a slot has one
//                        writer.  Hops: an integer distance per node in y_prev's place, a node joining the frontier of round l when a
//                        neighbour has distance l - 1.
//                        Then the same block reads acc[dst], marks the filter row in the bitmap, compares and counts all candidates and
//                        stores the three outputs: one block per query, so no output atomics and no memset.  No score reaches global memory
//                        on the LDS path.
// Every read of col is bounded by rowptr clamped to [0, nnz] and every entry outside [0, N) is skipped: a CSR that breaks the assumptions
// gives wrong numbers, never an access outside the arrays.
#include <algorithm>

#include "csr_graph.h"
#include "lp_filter.h"

namespace {

// The three instances.  Up to SMALL_NODES (Cora): 512 threads with 8 accumulators each, 59 VGPRs and at most 32.5 KiB of LDS, so three
// blocks share a CU.  Up to LDS_NODES (PubMed): 1,024 threads with 20 accumulators each, 114 VGPRs, one block a CU.  Beyond: 512 threads
// on the workspace.
constexpr int SMALL_THREADS = 512, SMALL_REGS = 8, SMALL_NODES = SMALL_THREADS * SMALL_REGS;
constexpr int LARGE_THREADS = 1024, LARGE_REGS = 20;
constexpr int LDS_NODES = 20000;                                     // 2 floats and a filter bit per node: 162,500 bytes of the 160 KiB
constexpr int WS_THREADS = 512;
constexpr int RESIDENT = 1024;                                       // blocks of the workspace path: 4 per CU
constexpr int MAX_ROUNDS = 64;
constexpr int MODE_SUM = 0, MODE_HOPS = 1;
constexpr int64_t LDS_GRID = (int64_t)1 << 16;                       // the LDS path loops too, beyond this many queries

__host__ __device__ constexpr int64_t words_of(int64_t N) { return (N + 31) / 32; }
constexpr size_t lds_bytes(int64_t N) { return (size_t)(2 * N + words_of(N)) * 4; }
static_assert(lds_bytes(LDS_NODES) + 64 <= 160 * 1024, "two vectors, the bitmap and the static counters fit one CU's LDS");
static_assert(LARGE_THREADS * LARGE_REGS >= LDS_NODES && SMALL_NODES <= LDS_NODES, "every row of an LDS instance has its accumulator");

using namespace csr;                // Row, row_of, graph_ok

// lpf::mark over all candidates, written out: as a form of lpf::mark_each it changes walk_kernel's instruction schedule
__device__ __forceinline__ void mark(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t nnz, int64_t s, int64_t N,
                                     unsigned int* bits, int64_t words, int threads) {
    if (rowptr && s >= 0 && s < N) {
        const int64_t b = max((int64_t)rowptr[s], (int64_t)0), e = min((int64_t)rowptr[s + 1], nnz);
        for (int64_t i = b + threadIdx.x; i < e; i += threads) {
            const uint64_t off = (uint64_t)col[i];
            if (off < (uint64_t)(32 * words)) atomicOr(&bits[off >> 5], 1u << (unsigned)(off & 31));
        }
    }
}

// one row of a round: a * (the fold of w[z] * prev[z] over the row in ascending z, one add each)
__device__ __forceinline__ float fold_row(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N, int64_t nnz, int64_t v,
                                          const float* __restrict__ weight, float damping, const float* prev) {
    const Row r = row_of(rowptr, nnz, v);
    float sum = 0.f;
    for (int64_t i = r.b; i < r.e; ++i) {
        const int64_t z = col[i];
        if (z < 0 || z >= N) continue;
        sum = sum + (weight ? weight[z] * prev[z] : prev[z]);
    }
    return damping * sum;
}

// The scores of source s against every node: the walk sum, or minus the hop distance cut at rounds + 1.  y holds two vectors `vs` floats
// apart; the result stands in `acc` (a third vector) or, with acc in REGS > 0 registers a thread, in one of the two, whichever the
// return value says.
template <int T, int REGS>
__device__ __forceinline__ float* propagate(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N, int64_t nnz, int64_t s,
                                            const float* __restrict__ weight, float damping, int rounds, int mode, float* y, int64_t vs,
                                            float* acc, int* grown) {
    constexpr bool IN_LDS = REGS > 0;
    const int t = threadIdx.x;
    const bool inside = s >= 0 && s < N;
    if (mode == MODE_HOPS) {
        int* dist = (int*)y;
        float* out = IN_LDS ? y + vs : acc;
        const int far = rounds + 1;
        for (int64_t v = t; v < N; v += T) dist[v] = v == s ? 0 : far;
        if (t < 3) grown[t] = 0;                                     // round l raises grown[l % 3] and clears the flag of round l + 1
        __syncthreads();
        for (int l = 1; inside && l <= rounds; ++l) {
            bool grew = false;
            if (t == 0) grown[(l + 1) % 3] = 0;
            for (int64_t v = t; v < N; v += T) {
                if (dist[v] != far) continue;
                const Row r = row_of(rowptr, nnz, v);
                for (int64_t i = r.b; i < r.e; ++i) {
                    const int64_t z = col[i];
                    // a neighbour set in this very round holds l, never l - 1: the race with its writer changes nothing
                    if (z >= 0 && z < N && dist[z] == l - 1) {
                        dist[v] = l;
                        grew = true;
                        break;
                    }
                }
            }
            if (grew) grown[l % 3] = 1;
            __syncthreads();
            if (!grown[l % 3]) break;                                // (block-uniform) the component is exhausted
        }
        for (int64_t v = t; v < N; v += T) out[v] = -(float)dist[v];
        __syncthreads();
        return out;
    }
    float a[IN_LDS ? REGS : 1];                                      // IN_LDS: acc of the rows t + k T
#pragma unroll
    for (int k = 0; k < REGS; ++k) a[k] = 0.f;
    for (int64_t v = t; v < N; v += T) {
        y[v] = v == s ? 1.f : 0.f;
        if (!IN_LDS) acc[v] = 0.f;
    }
    __syncthreads();
    for (int l = 1; inside && l <= rounds; ++l) {
        const float* prev = y + (int64_t)((l - 1) & 1) * vs;
        float* next = y + (int64_t)(l & 1) * vs;
        if (IN_LDS) {
#pragma unroll
            for (int k = 0; k < REGS; ++k) {
                const int64_t v = t + (int64_t)k * T;
                if (v < N) {
                    const float yl = fold_row(rowptr, col, N, nnz, v, weight, damping, prev);
                    next[v] = yl;
                    a[k] = a[k] + yl;
                }
            }
        } else {
            for (int64_t v = t; v < N; v += T) {
                const float yl = fold_row(rowptr, col, N, nnz, v, weight, damping, prev);
                next[v] = yl;
                acc[v] = acc[v] + yl;
            }
        }
        __syncthreads();
    }
    if (!IN_LDS) return acc;
    float* out = y + (int64_t)((rounds + 1) & 1) * vs;               // y_{R-1}'s buffer: read for the last time before the barrier above
#pragma unroll
    for (int k = 0; k < REGS; ++k) {
        const int64_t v = t + (int64_t)k * T;
        if (v < N) out[v] = a[k];
    }
    __syncthreads();
    return out;
}

template <int T, int REGS>
__global__ __launch_bounds__(T) void walk_kernel(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t N, int64_t nnz,
                                                 const int64_t* __restrict__ src, const int64_t* __restrict__ dst, int64_t items,
                                                 const float* __restrict__ weight, float damping, int rounds, int mode,
                                                 const int32_t* __restrict__ frowptr, const int32_t* __restrict__ fcol, int64_t fnnz,
                                                 float* __restrict__ score, int32_t* __restrict__ n_greater, int32_t* __restrict__ n_equal,
                                                 float* ws, int64_t vs) {
    extern __shared__ float lds[];
    __shared__ int cnt[6];                                           // greater, equal, the end of a run of equal sources, 3 frontier flags
    constexpr bool IN_LDS = REGS > 0;
    const int t = threadIdx.x;
    if (IN_LDS) vs = N;
    float* y = IN_LDS ? lds : ws + (int64_t)blockIdx.x * (4 * vs);    // y_prev | y_next | filter bits in LDS; | acc | between them in a workspace slice
    unsigned int* fbits = (unsigned int*)(y + (IN_LDS ? 2 : 3) * vs);
    const int64_t words = words_of(N);
    const float none = mode == MODE_HOPS ? -(float)(rounds + 1) : 0.f;     // an endpoint outside the graph
    const bool ranking = n_greater != nullptr;
    for (int64_t q = blockIdx.x; q < items; q += gridDim.x) {
        const int64_t s = src[q];
        if (!ranking && q > 0 && src[q - 1] == s) continue;          // (block-uniform) scored by the block that owns the head of the run
        const float* acc = propagate<T, REGS>(rowptr, col, N, nnz, s, weight, damping, rounds, mode, y, vs, y + 2 * vs, cnt + 3);
        if (!ranking) {
            for (int64_t base = q; base < items; base += T) {        // the run of pairs with this source
                if (t == 0) cnt[2] = T;
                __syncthreads();
                const int64_t p = base + t;
                if (p >= items || src[p] != s) atomicMin(&cnt[2], t);
                __syncthreads();
                const int len = cnt[2];
                if (t < len) {
                    const int64_t d = dst[p];
                    score[p] = d >= 0 && d < N ? acc[d] : none;
                }
                __syncthreads();
                if (len < T) break;
            }
            continue;
        }
        const int64_t d = dst[q];
        const float st = d >= 0 && d < N ? acc[d] : none;
        for (int64_t w = t; w < words; w += T) fbits[w] = 0u;
        if (t < 2) cnt[t] = 0;
        __syncthreads();
        mark(frowptr, fcol, fnnz, s, N, fbits, words, T);            // gmp_lp_rank's filter row
        __syncthreads();
        int greater = 0, equal = 0;
        for (int64_t c = t; c < N; c += T) {
            if (c == s || c == d || lpf::marked(fbits, (int)c)) continue;
            const float v = acc[c];
            greater += v > st;
            equal += v == st;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            greater += __shfl_xor(greater, o, GMP_WAVE);
            equal += __shfl_xor(equal, o, GMP_WAVE);
        }
        if (t % GMP_WAVE == 0) {
            if (greater) atomicAdd(&cnt[0], greater);
            if (equal) atomicAdd(&cnt[1], equal);
        }
        __syncthreads();
        if (t == 0) {
            score[q] = st;
            n_greater[q] = cnt[0];
            n_equal[q] = cnt[1];
        }
        __syncthreads();                                             // cnt and the vectors are free for the next query
    }
}

// floats between two vectors of a workspace slice: whole 256-byte lines, wide enough for the bitmap too
int64_t ws_stride(int64_t N) { return (int64_t)(gmp::al((size_t)N * 4) / 4); }

int args_ok(const char* who, const void* rowptr, const void* col, int64_t N, int64_t nnz, const void* weight, float damping, int rounds, int mode) {
    if (int rc = graph_ok(who, rowptr, col, N, nnz)) return rc;
    if (mode != MODE_SUM && mode != MODE_HOPS) return gmp::fail(GMP_ERR_ARG, "%s: mode=%d (0 = walk sum, 1 = hops)", who, mode);
    if (rounds < 1 || rounds > MAX_ROUNDS) return gmp::fail(GMP_ERR_ARG, "%s: rounds=%d (1 <= rounds <= %d)", who, rounds, MAX_ROUNDS);
    if (weight && mode == MODE_HOPS) return gmp::fail(GMP_ERR_ARG, "%s: hops take no weight array", who);
    if (mode == MODE_SUM && !(damping > 0.f && damping <= 1.f)) return gmp::fail(GMP_ERR_ARG, "%s: damping=%g (0 < damping <= 1)", who, (double)damping);
    return GMP_OK;
}

int launch(const char* who, const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int64_t* src, const int64_t* dst, int64_t items,
           const float* weight, float damping, int rounds, int mode, const int32_t* frowptr, const int32_t* fcol, int64_t fnnz, float* score,
           int32_t* n_greater, int32_t* n_equal, void* workspace, size_t workspace_bytes, hipStream_t st) {
    const dim3 lds_grid((unsigned)std::min(items, LDS_GRID));
    if (N <= SMALL_NODES) {
        hipLaunchKernelGGL((walk_kernel<SMALL_THREADS, SMALL_REGS>), lds_grid, dim3(SMALL_THREADS), lds_bytes(N), st, rowptr, col, N, nnz, src, dst,
                           items, weight, damping, rounds, mode, frowptr, fcol, fnnz, score, n_greater, n_equal, (float*)nullptr, (int64_t)0);
        return gmp::check_launch("walk_kernel<lds, small>");
    }
    if (N <= LDS_NODES) {
        static std::atomic<uint64_t> attr_set{0};                   // > 64 KiB of dynamic LDS: opt in once per device, for the largest N
        if (lds_bytes(N) > 64 * 1024)
            if (int rc = gmp::reserve_lds(attr_set, (const void*)walk_kernel<LARGE_THREADS, LARGE_REGS>, (int)lds_bytes(LDS_NODES), who)) return rc;
        hipLaunchKernelGGL((walk_kernel<LARGE_THREADS, LARGE_REGS>), lds_grid, dim3(LARGE_THREADS), lds_bytes(N), st, rowptr, col, N, nnz, src, dst,
                           items, weight, damping, rounds, mode, frowptr, fcol, fnnz, score, n_greater, n_equal, (float*)nullptr, (int64_t)0);
        return gmp::check_launch("walk_kernel<lds, large>");
    }
    const size_t need = gmp_lp_walk_workspace_bytes(items, N);
    if (!workspace || workspace_bytes < need)
        return gmp::fail(GMP_ERR_ARG, "%s: workspace %zu < %zu", who, workspace ? workspace_bytes : (size_t)0, need);
    gmp::Carver carve(workspace, true);
    const int64_t blocks = std::min(items, (int64_t)RESIDENT), vs = ws_stride(N);
    float* ws = carve.take<float>((size_t)(blocks * 4 * vs));
    hipLaunchKernelGGL((walk_kernel<WS_THREADS, 0>), dim3((unsigned)blocks), dim3(WS_THREADS), 0, st, rowptr, col, N, nnz, src, dst, items, weight,
                       damping, rounds, mode, frowptr, fcol, fnnz, score, n_greater, n_equal, ws, vs);
    return gmp::check_launch("walk_kernel<workspace>");
}

}  // namespace

extern "C" int gmp_lp_walk_lds_nodes(void) { return LDS_NODES; }

extern "C" int gmp_lp_walk_resident_blocks(void) { return RESIDENT; }

extern "C" size_t gmp_lp_walk_workspace_bytes(int64_t Q, int64_t N) {
    if (Q <= 0 || N <= LDS_NODES || N >= ((int64_t)1 << 31)) return 0;
    gmp::Carver carve(nullptr, true);
    carve.take<float>((size_t)(std::min(Q, (int64_t)RESIDENT) * 4 * ws_stride(N)));
    return carve.total();
}

extern "C" int gmp_lp_walk_score(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int64_t* src, const int64_t* dst,
                                 int64_t P, const float* weight, float damping, int rounds, int mode, float* score, void* workspace,
                                 size_t workspace_bytes, gmp_stream_t stream) {
    if (int rc = args_ok("lp_walk_score", rowptr, col, N, nnz, weight, damping, rounds, mode)) return rc;
    if (P < 0) return gmp::fail(GMP_ERR_ARG, "lp_walk_score: P=%lld", (long long)P);
    if (P == 0) return GMP_OK;
    if (!src || !dst || !score) return gmp::fail(GMP_ERR_ARG, "lp_walk_score: null pointer");
    return launch("lp_walk_score", rowptr, col, N, nnz, src, dst, P, weight, damping, rounds, mode, nullptr, nullptr, 0, score, nullptr, nullptr,
                  workspace, workspace_bytes, (hipStream_t)stream);
}

extern "C" int gmp_lp_walk_rank(const int32_t* rowptr, const int32_t* col, int64_t N, int64_t nnz, const int64_t* src, const int64_t* dst,
                                int64_t Q, const float* weight, float damping, int rounds, int mode, const int32_t* filter_rowptr,
                                const int32_t* filter_col, int64_t filter_nnz, float* score_true, int32_t* n_greater, int32_t* n_equal,
                                void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    if (int rc = args_ok("lp_walk_rank", rowptr, col, N, nnz, weight, damping, rounds, mode)) return rc;
    bool done;
    if (int rc = lpf::rank_front("lp_walk_rank", Q, filter_rowptr, filter_col, filter_nnz, src, dst, score_true, n_greater, n_equal, done); rc || done)
        return rc;
    return launch("lp_walk_rank", rowptr, col, N, nnz, src, dst, Q, weight, damping, rounds, mode, filter_rowptr, filter_col, filter_nnz,
                  score_true, n_greater, n_equal, workspace, workspace_bytes, (hipStream_t)stream);
}
