// The pooled-feature map of a batch of graphs: the sum, mean and max pools of X, S X, .. S^rounds X per graph, S = diag(left) A diag(right)
// restricted to the graph -- the structure-blind baseline of Errica et al. (ICLR 2020) at rounds = 0, SGC's features (Wu et al. 2019)
// pooled and concatenated over the scales (SIGN, Frasca et al. 2020) above it.  The definition -- every multiply and add rounded on its
// own, a row summed in ascending neighbour order, a pool summed in ascending row order, the max an integer compare -- is above
// gmp_graph_feature_map in include/gnnmp.h; H(t) has the bits of feature_prop.hip over the whole batch, the row sum is the same
// prop::fold_row (csr_prop.h) with the graph's window as its base.
//
//   graph_feat_kernel   grid (num_graphs, ceil(d / CS)), one launch per batch: a workgroup owns one graph and one strip of CS = 16
//                       columns.  Columns never interact, so no strip talks to another.  The two ping-pong copies of the graph's strip of
//                       H (cn x CS floats each) and the graph's left and right live in LDS from the first load to the last pool: global
//                       memory sees x once (a 64-byte segment per row and strip), the CSR rows once per round (rowptr and col only: L2
//                       holds them), and the [rounds + 1, 3, CS] results.
//   lanes               run along the strip's columns: lane c of a GROUP of CS lanes owns column c, a group owns a row and walks it entry
//                       by entry -- `col[k]` is one address for the whole group, the neighbour's H[j][0 .. CS) is 16 consecutive banks.  A
//                       32-lane half of a wave holds two rows, so two neighbours of equal parity share their 16 banks (2-way, one time in
//                       two on random neighbours); a strip of 32 columns would avoid it and does not fit the large instance.
//   pooling             the sequential pool of H(t) is a chain by definition and reads only H(t), as the propagation to H(t+1) does: wave 0
//                       pools (its first group the sum and the mean, its second the max, one lane per column) WHILE the other waves
//                       propagate, one workgroup barrier per round.  Only the pool of H(rounds) has the workgroup to itself.
//   skipped entries     counted by the strip-0 workgroup in the first round: an integer atomicAdd on LDS, one per row that has any.
//
// Two instances by graph size, planned by graph_block.h as for sp.hip and graph_props.hip (a batch whose max_graph_nodes is above 256 gets
// both launches, each block leaving at once when its graph belongs to the other one).  Dynamic LDS of a block = 2 cn CS 4 bytes (H) +
// 2 cn 4 bytes (left, right), cn = min(max_graph_nodes, the instance's limit), + 4 bytes static:
//   <256 threads>   n <= 256: 3 waves (12 rows at a time) propagate.  At cn = 126 (ENZYMES' largest graph) 16.7 KiB, 9 workgroups per
//                   CU by LDS and 8 by the 32 waves a CU takes at this register count; at the instance's worst (cn = 256) 34 KiB, 4 per CU.
//   <1024 threads>  256 < n <= 1024: 15 waves (60 rows at a time) propagate.  Worst (cn = 1024): 128 + 8 = 136 KiB of the 160 KiB, one
//                   workgroup per CU; at cn = 620 (PROTEINS' largest graph) 82 KiB, one per CU.
// More than 64 KiB of dynamic LDS is reserved once per device, for the large instance only.
#include "csr_prop.h"
#include "graph_block.h"

namespace {

using gmp::LARGE_N, gmp::SMALL_N;                                   // graph_block.h: the two instances and their launch plan, the status word

constexpr int CS = 16;                                              // columns per strip = lanes per row
constexpr int POOL_GROUPS = GMP_WAVE / CS;                          // the groups of wave 0, which pools
constexpr int MAX_DIM = 256, MAX_ROUNDS = 16;
constexpr int64_t LIMIT = (int64_t)1 << 31;

// dynamic LDS of one block whose graphs have at most `cn` nodes
__host__ __device__ inline size_t lds_bytes(int cn) { return ((size_t)2 * cn * CS + (size_t)2 * cn) * sizeof(float); }

template <int T>
__global__ __launch_bounds__(T) void graph_feat_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ rowptr,
                                                       const int32_t* __restrict__ col, int64_t num_nodes, int nnz,
                                                       const float* __restrict__ left, const float* __restrict__ right,
                                                       const float* __restrict__ x, int64_t ldx, int d, int rounds, int n_min, int cn,
                                                       int flag_large, float* __restrict__ out, int32_t* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ unsigned int skipped;
    constexpr int GROUPS = T / CS, PROP_GROUPS = GROUPS - POOL_GROUPS;

    const int gidx = blockIdx.x, t = threadIdx.x, c = t % CS, grp = t / CS;
    const int cc = (int)blockIdx.y * CS + c;                        // this lane's column of x and out
    const bool live = cc < d;
    const int64_t p0 = min(max(ptr[gidx], (int64_t)0), num_nodes), p1 = max(min(max(ptr[gidx + 1], (int64_t)0), num_nodes), p0);
    const int64_t nn = p1 - p0;
    float* const dst = out + (int64_t)gidx * (rounds + 1) * 3 * d + cc;      // + (t * 3 + pool) * d; dereferenced by live lanes only
    if (nn > cn) {                                                  // block-uniform: nobody reaches a barrier
        if (flag_large) {
            if (live)
                for (int k = grp; k < (rounds + 1) * 3; k += GROUPS) dst[(int64_t)k * d] = 0.f;
            if (blockIdx.y == 0 && t == 0) status[gidx] = gmp::STATUS_REFUSED;
        }
        return;
    }
    if (nn < n_min) return;                                         // the other instance's graph

    const int n = (int)nn, base = (int)p0;                          // (num_nodes < 2^31)
    float* const H0 = smem;                                         // [n, CS] of the cn * CS floats
    float* const H1 = H0 + (size_t)cn * CS;
    float* const ls = H1 + (size_t)cn * CS;                         // [n] of cn: left, ones for NULL (a multiply by 1 is exact)
    float* const rs = ls + cn;                                      // right likewise

    for (int i = grp; i < n; i += GROUPS) H0[i * CS + c] = live ? x[(p0 + i) * ldx + cc] : 0.f;     // the columns past d hold zeros
    for (int i = t; i < n; i += T) {
        ls[i] = left ? left[p0 + i] : 1.0f;
        rs[i] = right ? right[p0 + i] : 1.0f;
    }
    if (t == 0) skipped = 0u;
    __syncthreads();

    const int wave = __builtin_amdgcn_readfirstlane(t / GMP_WAVE);
    const bool counts = blockIdx.y == 0;
    for (int r = 0; r <= rounds; ++r) {
        const float* const cur = (r & 1) ? H1 : H0;
        float* const nxt = (r & 1) ? H0 : H1;
        if (wave == 0) {
            if (grp == 0) {                                         // the chain of the definition: one lane per column
                float s = 0.f;
#pragma unroll 8
                for (int i = 0; i < n; ++i) s = __fadd_rn(s, cur[i * CS + c]);
                if (live) {
                    dst[(int64_t)(r * 3) * d] = s;
                    dst[(int64_t)(r * 3 + 1) * d] = n ? __fdiv_rn(s, (float)n) : 0.f;
                }
            } else if (grp == 1) {                                  // integer compares: 0 lies below every float's orderable bits
                uint32_t m = 0u;
#pragma unroll 8
                for (int i = 0; i < n; ++i) m = max(m, gmp::orderable(cur[i * CS + c]));
                if (live) dst[(int64_t)(r * 3 + 2) * d] = n ? gmp::from_orderable(m) : 0.f;
            }
        } else if (r < rounds) {
            for (int i = grp - POOL_GROUPS; i < n; i += PROP_GROUPS) {
                const auto sum = prop::fold_row<1>(rowptr, col, n, nnz, p0 + i, rs,
                                                   [&](int j, int) __attribute__((always_inline)) { return cur[j * CS + c]; }, base);
                nxt[i * CS + c] = __fmul_rn(ls[i], sum.acc[0]);
                if (r == 0 && counts && c == 0 && sum.bad) atomicAdd(&skipped, (unsigned int)sum.bad);
            }
        }
        __syncthreads();
    }
    if (counts && t == 0) status[gidx] = (int32_t)gmp::status_word(skipped, gmp::SKIP_MAX);
}

}  // namespace

extern "C" int gmp_graph_feature_map(const int64_t* ptr, int num_graphs, const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t nnz,
                                     const float* left, const float* right, const float* x, int64_t ldx, int32_t d, int32_t rounds,
                                     int64_t max_graph_nodes, float* out, int32_t* status, gmp_stream_t stream) {
    if (num_graphs < 0 || num_nodes < 0 || num_nodes >= LIMIT || nnz < 0 || nnz >= LIMIT || max_graph_nodes < 0 || d < 1 || d > MAX_DIM ||
        rounds < 0 || rounds > MAX_ROUNDS)
        return gmp::fail(GMP_ERR_ARG, "graph_feature_map: num_graphs=%d num_nodes=%lld nnz=%lld max_graph_nodes=%lld d=%d rounds=%d "
                         "(0 <= sizes < 2^31, 1 <= d <= %d, 0 <= rounds <= %d)", num_graphs, (long long)num_nodes, (long long)nnz,
                         (long long)max_graph_nodes, d, rounds, MAX_DIM, MAX_ROUNDS);
    if (num_graphs == 0) return GMP_OK;
    if (!ptr || !rowptr || (nnz > 0 && !col) || (num_nodes > 0 && !x) || !out || !status)
        return gmp::fail(GMP_ERR_ARG, "graph_feature_map: null pointer");
    if (ldx < d) return gmp::fail(GMP_ERR_ARG, "graph_feature_map: ldx=%lld for d=%d (ld >= d)", (long long)ldx, d);
    const size_t x_bytes = num_nodes > 0 ? ((size_t)(num_nodes - 1) * (size_t)ldx + (size_t)d) * sizeof(float) : 0;
    if (gmp::overlap(out, (size_t)num_graphs * (rounds + 1) * 3 * d * sizeof(float), x, x_bytes))
        return gmp::fail(GMP_ERR_ARG, "graph_feature_map: out overlaps x");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)num_graphs, (unsigned)gmp::cdiv(d, CS));
    static std::atomic<uint64_t> done[2];                          // once per device and instance
    return gmp::launch_by_size(                                     // the large instance reserves for the largest graph
        "graph_feature_map", max_graph_nodes, done, graph_feat_kernel<SMALL_N>, 0, graph_feat_kernel<LARGE_N>, (int)lds_bytes(LARGE_N),
        [&](auto kernel, int T, const gmp::Instance& in) {
            hipLaunchKernelGGL(kernel, grid, dim3(T), lds_bytes(in.cap), st, ptr, rowptr, col, num_nodes, (int)nnz, left, right, x, ldx, d, rounds,
                               in.n_min, in.cap, in.flag_large, out, status);
            return gmp::check_launch(T == LARGE_N ? "graph_feat_kernel<1024>" : "graph_feat_kernel<256>");
        });
}
