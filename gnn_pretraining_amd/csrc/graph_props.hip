// The integer counts behind the 12 targets of the graph-property task (data/graph_properties.py: N, E, density, mean degree, degree
// variance, max degree, average clustering, transitivity, #components, diameter of the largest component, degree assortativity,
// degree centralisation), for a whole batch of graphs in one call: one workgroup per graph, the slot table of gnnmp.h per graph.
//
// The graph's simple undirected adjacency lives in LDS as an n x n bit matrix A, row stride w = ceil(n / 64) 64-bit words.  Edges are set
// with the integer LDS atomicOr (both directions; self loops skipped; an entry with an endpoint outside the graph's own node range is
// counted and skipped), so duplicates and mirrored entries merge and the matrix does not depend on the order of the edge list.
//
// Lane layout of every pass over rows: wp = the power of two >= w (1 .. 16); a wave is 64 / wp lane groups, lane `word` = lane % wp of a
// group reads word `word` of the group's row -- consecutive lanes take consecutive 64-bit words (ds_read_b64, one 256-byte bank row per 32
// lanes when the groups' rows are adjacent, as in the degree pass).  A graph of <= 64 nodes has one row per lane.
//
//   degrees      group per node: popcount of the row, added over the group's lanes with shuffles
//   triangles    group per node v: for every neighbour u (bits of row v) popcount(row_v & row_u); the same walk adds deg(u) for Sxy
//   clustering   one fp64 term per node in LDS, t2 / (deg (deg - 1)), summed by a fixed stride-halving tree over the next power of two
//                >= n (zero padded): no float atomic, the same order in every run
//   components   wave 0: bit-set BFS from the lowest unlabelled node until none is left.  One level = OR of the adjacency rows of the
//                frontier into next & ~visited; the groups of the wave split each frontier word's bits between them (bit b goes to group
//                b % groups) and an xor-shuffle ORs the groups' partial rows.  The first largest component wins (components come in
//                order of their smallest node id), its bit set goes to LDS.
//   diameter     one BFS per member of that component, members dealt round-robin to the waves; eccentricity = levels that found a new
//                node; integer LDS atomicMax over the waves.
// The BFS bit sets (frontier, visited) are one 64-bit REGISTER per lane (word `word`, replicated in every group), not LDS: a wave needs no
// slice and no barrier of its own, and the frontier word a level walks is fetched with a shuffle.
// All count sums are 64-bit integers added with LDS atomics: independent of the order.  No floating-point atomic in this file.
//
// Two instances by row width: <4 words, 256 threads> for n <= 256 (<= 11 KB of LDS: several blocks per CU) and <16 words, 1024 threads>
// for 256 < n <= 1024 (<= 140 KB: one block per CU).  A batch whose largest graph is above 256 nodes gets both launches, each block
// leaving at once when its graph belongs to the other one (graph_block.h: the plan and the status word).
#include "bit_bfs.h"

namespace {

typedef unsigned long long u64;

constexpr int SLOTS = 16;

using gmp::LARGE_N, gmp::SMALL_N;                                    // graph_block.h: the two instances and their launch plan, the status word
using gmp::Lanes;
using gmp::pow2_ceil;
using gmp::wave_bfs;                                                 // bit_bfs.h: the lane layout and the per-wave bit-set BFS

// LDS of one block whose graphs have at most `cap` nodes: the bit matrix, the clustering terms (padded to a power of two), the degrees
__host__ __device__ inline size_t lds_bytes(int cap) {
    return (size_t)cap * ((cap + 63) / 64) * 8 + (size_t)pow2_ceil(cap) * 8 + (size_t)cap * 4;
}

template <int W, int T>
__global__ __launch_bounds__(T) void graph_props_kernel(const int64_t* __restrict__ ptr, const int64_t* __restrict__ eptr,
                                                        const int64_t* __restrict__ edge_index, int64_t num_edges, int n_min, int cap,
                                                        int flag_large, int64_t* __restrict__ counts, double* __restrict__ clustering_sum) {
    extern __shared__ u64 smem[];
    __shared__ u64 sums[8];            // 0 sum deg, 1 sum deg^2, 2 sum deg^3, 3 T2, 4 Pr, 5 Sxy, 6 dropped endpoints
    __shared__ u64 best_bits[W];
    __shared__ int max_deg, num_comp, best_size, diameter;

    const int gidx = blockIdx.x, t = threadIdx.x;
    const int64_t p0 = ptr[gidx], p1 = ptr[gidx + 1];
    const int64_t nn = p1 - p0;
    int64_t* out = counts + (int64_t)gidx * SLOTS;
    if (nn < 0 || nn > cap) {                                        // block-uniform: nobody reaches a barrier (no num_nodes to hold ptr against)
        if (flag_large && t == 0) out[12] = gmp::STATUS_REFUSED;
        return;
    }
    if (nn < n_min) return;                                          // the other instance's graph

    const int n = (int)nn;
    const Lanes L = gmp::make_lanes(n, t & 63);
    const int lane = t & 63;
    const int w = L.w, wp = L.wp;
    const int P = pow2_ceil(n > 0 ? n : 1);

    u64* A = smem;                                                   // [n * w]
    double* cterm = reinterpret_cast<double*>(smem + (size_t)cap * ((cap + 63) / 64));   // [pow2_ceil(cap)]
    int* deg = reinterpret_cast<int*>(cterm + pow2_ceil(cap));       // [cap]

    for (int k = t; k < n * w; k += T) A[k] = 0ull;
    for (int k = n + t; k < P; k += T) cterm[k] = 0.0;
    if (t < 8) sums[t] = 0ull;
    if (t < W) best_bits[t] = 0ull;
    if (t == 0) {
        max_deg = 0;
        num_comp = 0;
        best_size = 0;
        diameter = 0;
    }
    __syncthreads();

    // ---- edges -> bits
    {
        int64_t e0 = eptr[gidx], e1 = eptr[gidx + 1];
        e0 = e0 < 0 ? 0 : (e0 > num_edges ? num_edges : e0);        // never read outside edge_index
        e1 = e1 < e0 ? e0 : (e1 > num_edges ? num_edges : e1);
        u64 dropped = 0ull;
        for (int64_t e = e0 + t; e < e1; e += T) {
            const int64_t s = edge_index[e] - p0, d = edge_index[num_edges + e] - p0;
            const int bad = (s < 0 || s >= nn ? 1 : 0) + (d < 0 || d >= nn ? 1 : 0);
            dropped += (u64)bad;
            if (bad == 0 && s != d) {
                const int a = (int)s, b = (int)d;
                atomicOr(&A[a * w + (b >> 6)], 1ull << (b & 63));
                atomicOr(&A[b * w + (a >> 6)], 1ull << (a & 63));
            }
        }
        if (dropped) atomicAdd(&sums[6], dropped);
    }
    __syncthreads();

    const int rows_per_pass = T / wp, row_in_pass = t / wp;

    // ---- degrees
    for (int v0 = 0; v0 < n; v0 += rows_per_pass) {                  // block-uniform trip count: every lane reaches the shuffles
        const int v = v0 + row_in_pass;
        int c = (v < n && L.word < w) ? __popcll(A[v * w + L.word]) : 0;
        for (int o = wp >> 1; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
        if (v < n && L.word == 0) deg[v] = c;
    }
    __syncthreads();

    // ---- triangles, degree sums
    {
        u64 s1 = 0ull, s2 = 0ull, s3 = 0ull, t2sum = 0ull, pr = 0ull, sxy = 0ull;
        int dmax = 0;
        for (int v0 = 0; v0 < n; v0 += rows_per_pass) {
            const int v = v0 + row_in_pass;
            const bool on = v < n && L.word < w;
            const u64 rv = on ? A[v * w + L.word] : 0ull;
            int c = 0;
            u64 nd = 0ull;                                           // sum of the neighbours' degrees
            for (int j = 0; j < w; ++j) {
                u64 m = __shfl(rv, L.g0 + j, 64);                    // word j of the group's row; 0 for a group past the last node
                while (m) {
                    const int u = j * 64 + __builtin_ctzll(m);
                    m &= m - 1ull;
                    if (on) c += __popcll(rv & A[u * w + L.word]);
                    nd += (u64)deg[u];
                }
            }
            for (int o = wp >> 1; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
            if (v < n && L.word == 0) {
                const u64 d = (u64)deg[v];
                const u64 pairs = d * (d - 1ull);                    // d == 0: 0 * (2^64 - 1) = 0
                cterm[v] = d >= 2ull ? (double)c / (double)pairs : 0.0;
                s1 += d;
                s2 += d * d;
                s3 += d * d * d;
                t2sum += (u64)c;
                pr += pairs;
                sxy += d * nd;
                dmax = max(dmax, (int)d);
            }
        }
        if (s1) {                                                    // a thread that met only isolated nodes adds nothing
            atomicAdd(&sums[0], s1);
            atomicAdd(&sums[1], s2);
            atomicAdd(&sums[2], s3);
            atomicAdd(&sums[5], sxy);
            atomicMax(&max_deg, dmax);
            if (t2sum) atomicAdd(&sums[3], t2sum);
            if (pr) atomicAdd(&sums[4], pr);
        }
    }
    __syncthreads();

    // ---- clustering sum: fixed tree over cterm[0 .. P)
    for (int s = P >> 1; s > 0; s >>= 1) {
        for (int k = t; k < s; k += T) cterm[k] += cterm[k + s];
        __syncthreads();
    }

    // ---- components (wave 0)
    if (t < 64) {
        u64 seen = 0ull, best = 0ull;
        int ncomp = 0, bsize = 0;
        const u64 group0 = (wp == 64) ? ~0ull : ((1ull << wp) - 1ull);
        for (;;) {
            const u64 open = ~seen & L.valid;
            const u64 nz = __ballot(open != 0ull) & group0;
            if (!nz) break;
            const int j = __builtin_ctzll(nz);
            const u64 ow = __shfl(open, j, 64);
            const u64 F = (L.word == j) ? (ow & (~ow + 1ull)) : 0ull;          // the lowest unlabelled node
            u64 V;
            (void)wave_bfs(A, L, F, V);
            int size = __popcll(V);
            for (int o = wp >> 1; o > 0; o >>= 1) size += __shfl_xor(size, o, 64);
            ++ncomp;
            if (size > bsize) {                                      // strictly larger: a tie stays with the earlier component
                bsize = size;
                best = V;
            }
            seen |= V;
        }
        if (lane < wp && L.word < w) best_bits[L.word] = best;
        if (lane == 0) {
            num_comp = ncomp;
            best_size = bsize;
        }
    }
    __syncthreads();

    // ---- diameter of the largest component
    if (best_size > 1) {
        const int wave = t >> 6, waves = T >> 6;
        int k = 0, ecc = 0;
        for (int j = 0; j < w; ++j) {
            u64 m = best_bits[j];
            while (m) {                                              // wave-uniform
                const u64 low = m & (~m + 1ull);
                m &= m - 1ull;
                if (k++ % waves == wave) {
                    u64 V;
                    ecc = max(ecc, wave_bfs(A, L, (L.word == j) ? low : 0ull, V));
                }
            }
        }
        if (lane == 0 && ecc) atomicMax(&diameter, ecc);
    }
    __syncthreads();

    if (t == 0) {
        out[0] = n;
        out[1] = (int64_t)(sums[0] >> 1);
        out[2] = max_deg;
        out[3] = (int64_t)sums[0];
        out[4] = (int64_t)sums[1];
        out[5] = (int64_t)sums[3];
        out[6] = (int64_t)sums[4];
        out[7] = num_comp;
        out[8] = diameter;
        out[9] = (int64_t)sums[5];
        out[10] = (int64_t)sums[1];
        out[11] = (int64_t)sums[2];
        out[12] = (int64_t)gmp::status_word(sums[6], gmp::SKIP_MAX_WIDE);      // an int64 slot: 54 bits of dropped endpoints
        out[13] = 0;
        out[14] = 0;
        out[15] = 0;
        clustering_sum[gidx] = cterm[0];
    }
}

}  // namespace

extern "C" size_t gmp_graph_props_workspace_bytes(int num_graphs, int64_t max_graph_nodes) {
    (void)num_graphs;
    (void)max_graph_nodes;
    return 0;                                                        // everything lives in LDS
}

extern "C" int gmp_graph_props(const int64_t* ptr, const int64_t* eptr, const int64_t* edge_index, int64_t num_nodes, int64_t num_edges,
                               int num_graphs, int64_t max_graph_nodes, int64_t* counts, double* clustering_sum, void* workspace,
                               size_t workspace_bytes, gmp_stream_t stream) {
    (void)workspace;
    (void)workspace_bytes;
    if (num_graphs < 0 || num_nodes < 0 || num_edges < 0 || max_graph_nodes < 0)
        return gmp::fail(GMP_ERR_ARG, "graph_props: num_graphs=%d num_nodes=%lld num_edges=%lld max_graph_nodes=%lld (all >= 0)", num_graphs,
                         (long long)num_nodes, (long long)num_edges, (long long)max_graph_nodes);
    if (num_graphs == 0) return GMP_OK;
    if (!ptr || !eptr || !counts || !clustering_sum || (num_edges > 0 && !edge_index)) return gmp::fail(GMP_ERR_ARG, "graph_props: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)num_graphs);
    static std::atomic<uint64_t> done[2];                          // once per device and instance
    return gmp::launch_by_size(                                      // the large instance reserves for the largest graph it takes
        "graph_props", max_graph_nodes, done, graph_props_kernel<SMALL_N / 64, SMALL_N>, 0, graph_props_kernel<LARGE_N / 64, LARGE_N>, (int)lds_bytes(LARGE_N),
        [&](auto kernel, int T, const gmp::Instance& in) {
            hipLaunchKernelGGL(kernel, grid, dim3(T), lds_bytes(in.cap), st, ptr, eptr, edge_index, num_edges, in.n_min, in.cap, in.flag_large, counts,
                               clustering_sum);
            return gmp::check_launch(T == LARGE_N ? "graph_props_kernel<16>" : "graph_props_kernel<4>");
        });
}
