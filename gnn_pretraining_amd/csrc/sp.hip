// The shortest-path kernel baseline of graph classification (Borgwardt & Kriegel, ICDM 2005) for a whole batch of graphs: the exact
// (label, label, hop distance) feature map defined above gmp_sp_features in include/gnnmp.h, and the kernel between two batches.
//
//   sp_features_kernel  one workgroup per graph, one launch per batch.  The graph's simple undirected adjacency lives in LDS as the n x n
//                       bit matrix of graph_props.hip (row stride w = ceil(n / 64) 64-bit words), built from the CSR rows with the integer
//                       LDS atomicOr in both directions, so the order of the entries does not matter; an entry that leaves the row's own
//                       graph is counted and skipped, never used as an index.  One wave-level bit-set BFS (bit_bfs.h) per source, sources
//                       dealt round-robin to the waves.  Every level d hands the lanes the set of nodes at distance exactly d; the lanes of
//                       ALL groups split its bits between them (the stripes of the BFS), keep those above the source's id -- every
//                       unordered pair is met once, from its lower end -- and count key = (lo << 35) | (hi << 11) | d into an open-addressing
//                       table in LDS: linear probing from mix(key + K1), a slot claimed by a 64-bit atomicCAS on the key (empty = all
//                       ones, no legal key), its count raised by a 32-bit atomicAdd.  A lane adds up a run of equal keys before it touches
//                       the table (an unlabelled graph has one key per level).  The table has 2^k >= 2 cap slots, so a graph within its
//                       `cap` fills at most half of it; a claim beyond cap, or a probe that walked the whole table, raises the overflow
//                       flag, which ends every wave at its next source.  The table is then sorted IN PLACE by a bitonic network over all
//                       slots -- the empty word is the largest, so the distinct keys end up in front, ascending -- counts moving with
//                       their keys, and written out once; the histogram is integer atomicAdd on LDS over the sorted keys.
//   sp_gram_kernel      one wave per entry K[i, j]: the lanes stride over the SHORTER of the two key rows and binary-search each key in the
//                       longer one, in global memory (staging the searched row in LDS first, as wl_gram_kernel does, was measured and
//                       bought nothing: a TU graph has ~100 keys, and the time is the waves' own, not the searches'); the products of
//                       the two counts are int64, the lanes' sums are added with shuffles; no atomic.  Both lengths are clamped to the
//                       row stride: unsorted input gives a wrong sum, never a read outside.
// Integer arithmetic only: no floating-point operation in this file, so every output is pinned bit for bit by tests/sp_ref.py.
//
// Two instances of sp_features_kernel by row width, planned by graph_block.h as for the other per-graph kernels (a batch whose
// max_graph_nodes is above 256 gets both launches, each block leaving at once when its graph belongs to the other one).  Dynamic LDS of a
// block = the bit matrix (cn ceil(cn / 64) 8 bytes, cn = min(max_graph_nodes, the instance's limit)) + 12 bytes per table slot + 4 cn
// (labels); 1 KiB of static LDS holds the histogram.
//   <256 threads>   n <= 256, cap <= 4096.  At cn = 64, cap = 1024: 0.5 + 24 + 0.25 KiB, 6 workgroups per CU; at the instance's worst
//                   (cn = 256, cap = 4096): 8 + 96 + 1 = 105 KiB, one per CU.
//   <1024 threads>  256 < n <= 1024, cap <= 1024.  Worst: 128 + 24 + 4 = 156 KiB of the 160 KiB, one workgroup per CU.
// More than 64 KiB of dynamic LDS is reserved once per device and instance.
#include "bit_bfs.h"

namespace {

typedef unsigned long long u64;
using gmp::GRAM_THREADS, gmp::GRAM_WAVES, gmp::K1, gmp::LARGE_N, gmp::SMALL_N, gmp::mix, gmp::pow2_ceil;           // graph_block.h
using gmp::Lanes;                                                   // bit_bfs.h

constexpr int SMALL_CAP = 4096, LARGE_CAP = 1024;                   // the most distinct keys per graph, by instance
constexpr int MAX_DIST = 1023, MAX_DIM = 256;
constexpr int64_t MAX_LABEL = (int64_t)1 << 24;
constexpr u64 EMPTY = ~0ull;                                        // a free table slot: above every key (keys are below 2^59)

__host__ __device__ inline int table_slots(int cap) { return pow2_ceil(2 * cap); }

// dynamic LDS of one block whose graphs have at most `cn` nodes and `cap` distinct keys
__host__ __device__ inline size_t lds_bytes(int cn, int cap) {
    return (size_t)cn * ((cn + 63) / 64) * 8 + (size_t)table_slots(cap) * 12 + (size_t)cn * 4;
}

struct Table {
    u64* key;                 // [slots]
    unsigned int* count;      // [slots]
    int slots, cap;
    int* used;                // claimed slots
    int* overflow;            // more than cap distinct keys
};

// count[key] += c
__device__ __forceinline__ void table_add(const Table& tb, u64 key, unsigned int c) {
    int h = (int)((unsigned int)(mix(key + K1) >> 32) & (unsigned int)(tb.slots - 1));
    for (int probe = 0; probe < tb.slots; ++probe) {
        u64 seen = tb.key[h];
        if (seen == EMPTY) {
            seen = atomicCAS(&tb.key[h], EMPTY, key);
            if (seen == EMPTY) {                                    // claimed
                if (atomicAdd(tb.used, 1) >= tb.cap) *tb.overflow = 1;
                seen = key;
            }
        }
        if (seen == key) {
            atomicAdd(&tb.count[h], c);
            return;
        }
        h = (h + 1) & (tb.slots - 1);
    }
    *tb.overflow = 1;                                               // every slot holds another key
}

template <int T>
__global__ __launch_bounds__(T) void sp_features_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ rowptr,
                                                        const int32_t* __restrict__ col, int64_t num_nodes, int64_t nnz,
                                                        const int64_t* __restrict__ labels, int max_dist, int dim, int n_min, int cn,
                                                        int flag_large, int cap, int64_t* __restrict__ keys, int32_t* __restrict__ counts,
                                                        int32_t* __restrict__ nuniq, int32_t* __restrict__ hist,
                                                        int32_t* __restrict__ status) {
    extern __shared__ u64 smem[];
    __shared__ unsigned int bins[MAX_DIM];
    __shared__ unsigned int skipped;
    __shared__ int used, overflow, bad_label;

    const int gidx = blockIdx.x, t = threadIdx.x;
    const int64_t p0 = ptr[gidx], p1 = ptr[gidx + 1];
    const int64_t nn = p1 - p0;
    if (nn < 0 || nn > cn || p0 < 0 || p1 > num_nodes) {            // block-uniform: nobody reaches a barrier
        if (flag_large && t == 0) {
            status[gidx] = gmp::STATUS_REFUSED;
            nuniq[gidx] = 0;
        }
        return;
    }
    if (nn < n_min) return;                                         // the other instance's graph

    const int n = (int)nn, lane = t & 63;
    const Lanes L = gmp::make_lanes(n, lane);
    const int w = L.w;
    const int slots = table_slots(cap);

    u64* A = smem;                                                  // [n * w] of the cn * ceil(cn / 64) words
    Table tb;
    tb.key = smem + (size_t)cn * ((cn + 63) / 64);                  // [slots]
    tb.count = reinterpret_cast<unsigned int*>(tb.key + slots);     // [slots]
    tb.slots = slots;
    tb.cap = cap;
    tb.used = &used;
    tb.overflow = &overflow;
    int* lab = reinterpret_cast<int*>(tb.count + slots);            // [cn]

    for (int k = t; k < n * w; k += T) A[k] = 0ull;
    for (int k = t; k < slots; k += T) {
        tb.key[k] = EMPTY;
        tb.count[k] = 0u;
    }
    for (int b = t; b < dim; b += T) bins[b] = 0u;
    if (t == 0) {
        skipped = 0u;
        used = 0;
        overflow = 0;
        bad_label = 0;
    }
    __syncthreads();

    // ---- CSR rows -> bits, degrees inside the graph, the skipped entries, the labels
    {
        unsigned int skip = 0u;
        for (int v = t; v < n; v += T) {
            const int64_t gv = p0 + v;
            int64_t deg = 0;
            skip += gmp::walk_row(rowptr, col, nnz, p0, nn, v, [&](int u) {
                ++deg;
                if (u != v) {
                    atomicOr(&A[v * w + (u >> 6)], 1ull << (u & 63));
                    atomicOr(&A[u * w + (v >> 6)], 1ull << (v & 63));
                }
            });
            const int64_t l = labels ? labels[gv] : deg;
            if (l < 0 || l >= MAX_LABEL) bad_label = 1;
            lab[v] = (int)l;
        }
        if (skip) atomicAdd(&skipped, skip);
    }
    __syncthreads();

    // ---- one BFS per source; the pairs (source, a higher node found at level d) go into the table
    if (!bad_label) {
        const int wave = t >> 6, waves = T >> 6;
        for (int s = wave; s < n - 1; s += waves) {                 // (the last node has no higher one)
            if (*(volatile int*)&overflow) break;
            const int sj = s >> 6;
            const u64 ls = (u64)lab[s];
            // the bits of this lane's word that are this lane's share (its group's stripe) and lie above the source
            const u64 above = L.word > sj ? ~0ull : (L.word == sj ? ~((2ull << (s & 63)) - 1ull) : 0ull);
            const u64 mine = L.stripe & above;
            u64 V;
            (void)gmp::wave_bfs(A, L, (L.word == sj) ? (1ull << (s & 63)) : 0ull, V, max_dist, [&](int d, u64 F) {
                u64 m = F & mine;                                   // (F is 0 in the lanes whose word lies past the row)
                u64 run_key = EMPTY;
                unsigned int run = 0u;
                while (m) {
                    const int v = L.word * 64 + __builtin_ctzll(m);
                    m &= m - 1ull;
                    const u64 lv = (u64)lab[v];
                    const u64 key = ((ls < lv ? ls : lv) << 35) | ((ls < lv ? lv : ls) << 11) | (u64)d;
                    if (key != run_key) {
                        if (run) table_add(tb, run_key, run);
                        run_key = key;
                        run = 0u;
                    }
                    ++run;
                }
                if (run) table_add(tb, run_key, run);
            });
        }
    }
    __syncthreads();

    if (bad_label || overflow) {                                    // block-uniform
        if (t == 0) {
            status[gidx] = (int32_t)gmp::status_word(skipped, gmp::SKIP_MAX, (overflow ? gmp::STATUS_OVERFLOW : 0u) | (bad_label ? gmp::STATUS_BAD_LABEL : 0u));
            nuniq[gidx] = 0;
        }
        return;
    }

    // ---- sort the table ascending by key, counts alongside: the empty word is the largest, so the used slots end up in front
    for (int k = 2; k <= slots; k <<= 1) {
        for (int s = k >> 1; s > 0; s >>= 1) {
            __syncthreads();
            for (int q = t; q < (slots >> 1); q += T) {
                const int i = (q / s) * (s << 1) + (q % s), j = i + s;
                const u64 a = tb.key[i], b = tb.key[j];
                if ((a > b) == ((i & k) == 0)) {                    // ascending blocks where bit k of i is clear, descending elsewhere
                                                                    // (two equal words are two empty slots: swapping them changes nothing)
                    tb.key[i] = b;
                    tb.key[j] = a;
                    const unsigned int c = tb.count[i];
                    tb.count[i] = tb.count[j];
                    tb.count[j] = c;
                }
            }
        }
    }
    __syncthreads();

    const int nk = used;                                            // <= cap
    for (int k = t; k < nk; k += T) {
        const u64 key = tb.key[k];
        const unsigned int c = tb.count[k];
        keys[(int64_t)gidx * cap + k] = (int64_t)key;
        counts[(int64_t)gidx * cap + k] = (int32_t)c;
        atomicAdd(&bins[gmp::hashed_bin(mix(key + K1), dim)], c);
    }
    __syncthreads();
    for (int b = t; b < dim; b += T) hist[(int64_t)gidx * dim + b] = (int32_t)bins[b];
    if (t == 0) {
        status[gidx] = (int32_t)gmp::status_word(skipped, gmp::SKIP_MAX);
        nuniq[gidx] = nk;
    }
}

// (the frame -- e -> (i, j), the shuffle sum, lane 0's write -- is written out: behind a shared helper hipcc reorders this kernel, graph_block.h)
__global__ __launch_bounds__(GRAM_THREADS) void sp_gram_kernel(const int64_t* __restrict__ ka, const int32_t* __restrict__ ca,
                                                               const int32_t* __restrict__ na, int64_t Ga, int cap_a,
                                                               const int64_t* __restrict__ kb, const int32_t* __restrict__ cb,
                                                               const int32_t* __restrict__ nb, int64_t Gb, int cap_b,
                                                               int64_t* __restrict__ K) {
    const int lane = threadIdx.x % GMP_WAVE, wave = threadIdx.x / GMP_WAVE;
    const int64_t e = (int64_t)blockIdx.x * GRAM_WAVES + wave;
    if (e >= Ga * Gb) return;                                       // (wave-uniform; no workgroup barrier below)
    const int64_t i = e / Gb, j = e - i * Gb;
    int la = min(max(na[i], 0), cap_a), lb = min(max(nb[j], 0), cap_b);
    const int64_t* __restrict__ xa = ka + i * cap_a;
    const int64_t* __restrict__ xb = kb + j * cap_b;
    const int32_t* __restrict__ ya = ca + i * cap_a;
    const int32_t* __restrict__ yb = cb + j * cap_b;
    if (la > lb) {                                                  // the sum is symmetric: walk the shorter row, search the longer
        const int l = la; la = lb; lb = l;
        const int64_t* __restrict__ x = xa; xa = xb; xb = x;
        const int32_t* __restrict__ y = ya; ya = yb; yb = y;
    }
    long long acc = 0;
    for (int k = lane; k < la; k += GMP_WAVE) {
        const int64_t x = xa[k];
        int lo = 0, hi = lb;
        while (lo < hi) {                                           // the first entry of the longer row >= x
            const int mid = (lo + hi) >> 1;
            if (xb[mid] < x) lo = mid + 1; else hi = mid;
        }
        if (lo < lb && xb[lo] == x) acc += (long long)ya[k] * (long long)yb[lo];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, GMP_WAVE);
    if (lane == 0) K[e] = acc;
}

}  // namespace

extern "C" size_t gmp_sp_workspace_bytes(int num_graphs, int64_t max_graph_nodes) {
    (void)num_graphs;
    (void)max_graph_nodes;
    return 0;                                                       // bit matrix, labels, table and histogram live in LDS
}

extern "C" int gmp_sp_max_unique(int64_t max_graph_nodes) { return gmp::two_instances(max_graph_nodes) ? LARGE_CAP : SMALL_CAP; }

extern "C" int gmp_sp_features(const int64_t* ptr, int num_graphs, const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t nnz,
                               const int64_t* labels, int max_dist, int dim, int64_t max_graph_nodes, int cap, int64_t* keys,
                               int32_t* counts, int32_t* nuniq, int32_t* hist, int32_t* status, void* workspace, size_t workspace_bytes,
                               gmp_stream_t stream) {
    (void)workspace;
    (void)workspace_bytes;
    if (num_graphs < 0 || num_nodes < 0 || num_nodes >= ((int64_t)1 << 31) || nnz < 0 || nnz >= ((int64_t)1 << 31) || max_graph_nodes < 0)
        return gmp::fail(GMP_ERR_ARG, "sp_features: num_graphs=%d num_nodes=%lld nnz=%lld max_graph_nodes=%lld", num_graphs,
                         (long long)num_nodes, (long long)nnz, (long long)max_graph_nodes);
    if (max_dist < 1 || max_dist > MAX_DIST || dim < 1 || dim > MAX_DIM || cap < 1 || cap > gmp_sp_max_unique(max_graph_nodes))
        return gmp::fail(GMP_ERR_ARG, "sp_features: max_dist=%d dim=%d cap=%d (1 <= max_dist <= %d, 1 <= dim <= %d, 1 <= cap <= %d)", max_dist,
                         dim, cap, MAX_DIST, MAX_DIM, gmp_sp_max_unique(max_graph_nodes));
    if (num_graphs == 0) return GMP_OK;
    if (!ptr || !rowptr || (nnz > 0 && !col) || !keys || !counts || !nuniq || !hist || !status)
        return gmp::fail(GMP_ERR_ARG, "sp_features: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)num_graphs);
    static std::atomic<uint64_t> done[2];                          // once per device and instance
    return gmp::launch_by_size(                                     // both reserve, for the largest graph and cap: the small one's worst is 105 KiB
        "sp_features", max_graph_nodes, done, sp_features_kernel<SMALL_N>, (int)lds_bytes(SMALL_N, SMALL_CAP), sp_features_kernel<LARGE_N>,
        (int)lds_bytes(LARGE_N, LARGE_CAP), [&](auto kernel, int T, const gmp::Instance& in) {
            hipLaunchKernelGGL(kernel, grid, dim3(T), lds_bytes(in.cap, cap), st, ptr, rowptr, col, num_nodes, nnz, labels, max_dist, dim, in.n_min,
                               in.cap, in.flag_large, cap, keys, counts, nuniq, hist, status);
            return gmp::check_launch(T == LARGE_N ? "sp_features_kernel<1024>" : "sp_features_kernel<256>");
        });
}

extern "C" int gmp_sp_gram(const int64_t* keys_a, const int32_t* counts_a, const int32_t* nuniq_a, int64_t num_graphs_a, int cap_a,
                           const int64_t* keys_b, const int32_t* counts_b, const int32_t* nuniq_b, int64_t num_graphs_b, int cap_b, int64_t* K,
                           gmp_stream_t stream) {
    if (num_graphs_a < 0 || num_graphs_b < 0 || cap_a < 1 || cap_a > SMALL_CAP || cap_b < 1 || cap_b > SMALL_CAP)
        return gmp::fail(GMP_ERR_ARG, "sp_gram: num_graphs_a=%lld num_graphs_b=%lld cap_a=%d cap_b=%d (1 <= cap <= %d)", (long long)num_graphs_a,
                         (long long)num_graphs_b, cap_a, cap_b, SMALL_CAP);
    if (num_graphs_a == 0 || num_graphs_b == 0) return GMP_OK;
    if (!keys_a || !counts_a || !nuniq_a || !keys_b || !counts_b || !nuniq_b || !K) return gmp::fail(GMP_ERR_ARG, "sp_gram: null pointer");
    int64_t blocks = 0;
    if (int rc = gmp::gram_blocks("sp_gram", num_graphs_a, num_graphs_b, &blocks)) return rc;
    hipLaunchKernelGGL(sp_gram_kernel, dim3((unsigned)blocks), dim3(GRAM_THREADS), 0, (hipStream_t)stream, keys_a, counts_a, nuniq_a, num_graphs_a,
                       cap_a, keys_b, counts_b, nuniq_b, num_graphs_b, cap_b, K);
    return gmp::check_launch("sp_gram_kernel");
}
