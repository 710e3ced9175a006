// The Weisfeiler-Lehman subtree baseline of graph classification (Shervashidze et al., JMLR 2011) for a whole batch of graphs: the hashed
// colour refinement defined above gmp_wl_refine in include/gnnmp.h, and the exact subtree kernel between two refined batches.
//
//   wl_refine_kernel  one workgroup per graph, one launch per batch, all h rounds inside it.  In LDS: the graph's two colour arrays
//                     (cur, nxt: a round reads one and writes the other, a workgroup barrier between two rounds), its list of all
//                     (h + 1) n colours and the D-bin histogram.  Round t: one thread per node walks the node's CSR row in global memory
//                     (L2-resident after the first round), adds mix(cur[u]) over the neighbours inside the graph -- a wrapping integer
//                     sum, so the order does not matter -- and hashes.  An entry outside the graph's own node range is skipped, never
//                     used as an index, and counted once (in the pass that also makes the degrees).  The list is then sorted in LDS by a
//                     bitonic network over P = the power of two >= (h + 1) n, written so that EVERY compare-exchange leaves the smaller
//                     word at the lower index (each merge starts with the mirror step i <-> block end - i, then the usual strides): the
//                     slots at and above (h + 1) n would hold "+infinity" and never move, so a pair that reaches into them is simply
//                     skipped -- padding by index bound, no sentinel value (every 64-bit word is a legal colour).  The histogram is
//                     integer atomicAdd on LDS.  Colours are compared as UNSIGNED words.
//   wl_gram_kernel    one wave per entry K[i, j]: the lanes stride over the SHORTER of segment i of A and segment j of B (the count is
//                     symmetric); a lane whose element starts a run of equal colours (its predecessor differs) finds the run's end by an
//                     upper-bound search and the equal range in the longer segment by a lower- and an upper-bound search, and adds the
//                     product of the two run lengths in int64.  Long runs (an unlabelled regular graph has one colour per round) cost
//                     one search each, not one step per element.  When the longer segment has at most 512 words (128 nodes at
//                     h = 3: every TU graph but a few) the wave first copies both segments into its 8 KiB of LDS with coalesced loads,
//                     so the ~20 dependent reads of a search chain cost LDS latency instead of a trip to L2 each; longer segments are
//                     searched in global memory.  32 KiB of static LDS per block of 4 waves: 5 blocks per CU.  The lanes' sums are
//                     added with shuffles; no atomic.  Every search is bounded by its segment, and the segments are clamped to the
//                     arrays: unsorted input gives a wrong count, never a read outside.
// Integer arithmetic only: no floating-point operation in this file, so every output is pinned bit for bit by tests/wl_ref.py.
//
// Two instances of wl_refine_kernel by graph size, planned by graph_block.h as for the other per-graph kernels (a batch whose
// max_graph_nodes is above 256 gets both launches, each block leaving at once when its graph belongs to the other one).  LDS of a block =
// 16 cap (colours) + 8 pow2((h + 1) cap) (list) + 4 D (histogram), cap = min(max_graph_nodes, the instance's limit):
//   <256 threads>   n <= 256.  At cap = 39, h = 3, D = 256 (the TU datasets): 624 + 2,048 + 1,024 = 3.6 KiB -- 8 workgroups per CU, the
//                   limit of 32 waves per CU, not LDS.  At the instance's worst (cap = 256, h = 7): 4 + 16 + 1 = 21 KiB, 7 per CU.
//   <1024 threads>  256 < n <= 1024.  Worst (cap = 1024, h = 7): 16 + 64 + 1 = 81 KiB, one workgroup per CU (160 KiB); at h = 3, 49 KiB:
//                   two by the wave limit.  More than 64 KiB of dynamic LDS is reserved once per device.
#include "graph_block.h"

namespace {

typedef unsigned long long u64;
using gmp::GRAM_THREADS, gmp::GRAM_WAVES, gmp::K1, gmp::LARGE_N, gmp::SMALL_N, gmp::mix, gmp::pow2_ceil;           // graph_block.h

constexpr int MAX_ITERS = 7, MAX_DIM = 256;
constexpr u64 K2 = 0xD1B54A32D192ED03ull;
constexpr int GRAM_STAGE = 512;                                     // words of a segment that a wave stages in LDS: 2 x 4 KiB per wave, 32 KiB per block

// LDS of one block whose graphs have at most `cap` nodes
__host__ __device__ inline size_t lds_bytes(int cap, int hp1, int dim) {
    return (size_t)cap * 16 + (size_t)pow2_ceil((int64_t)hp1 * cap) * 8 + (size_t)dim * 4;
}

template <int T>
__global__ __launch_bounds__(T) void wl_refine_kernel(const int64_t* __restrict__ ptr, const int32_t* __restrict__ rowptr,
                                                      const int32_t* __restrict__ col, int64_t num_nodes, int64_t nnz,
                                                      const int64_t* __restrict__ labels, int h, int dim, int n_min, int cap, int flag_large,
                                                      int64_t* __restrict__ colors, int64_t* __restrict__ sorted, int32_t* __restrict__ hist,
                                                      int32_t* __restrict__ status) {
    extern __shared__ u64 smem[];
    __shared__ unsigned int skipped;

    const int gidx = blockIdx.x, t = threadIdx.x;
    const int64_t p0 = ptr[gidx], p1 = ptr[gidx + 1];
    const int64_t nn = p1 - p0;
    if (nn < 0 || nn > cap || p0 < 0 || p1 > num_nodes) {           // block-uniform: nobody reaches a barrier
        if (flag_large && t == 0) status[gidx] = gmp::STATUS_REFUSED;
        return;
    }
    if (nn < n_min) return;                                         // the other instance's graph

    const int n = (int)nn, hp1 = h + 1;
    const int len = hp1 * n;                                        // <= 8 * 1024
    u64* cur = smem;                                                // [cap]
    u64* nxt = cur + cap;                                           // [cap]
    u64* list = nxt + cap;                                          // [pow2_ceil(hp1 * cap)], the first len slots are used
    unsigned int* bins = reinterpret_cast<unsigned int*>(list + pow2_ceil((int64_t)hp1 * cap));   // [dim]

    for (int b = t; b < dim; b += T) bins[b] = 0u;
    if (t == 0) skipped = 0u;
    __syncthreads();

    // ---- round 0: degrees inside the graph, the skipped entries, the start colours
    {
        unsigned int skip = 0u;
        for (int v = t; v < n; v += T) {
            const int64_t gv = p0 + v;
            int64_t deg = 0;
            skip += gmp::walk_row(rowptr, col, nnz, p0, nn, v, [&](int) { ++deg; });
            const u64 c = mix((u64)(labels ? labels[gv] : deg) + K1);
            cur[v] = c;
            list[v] = c;
            if (colors) colors[gv] = (int64_t)c;
        }
        if (skip) atomicAdd(&skipped, skip);
    }
    __syncthreads();

    // ---- rounds 1 .. h
    for (int r = 1; r <= h; ++r) {
        for (int v = t; v < n; v += T) {
            const int64_t gv = p0 + v;
            u64 sum = 0ull;
            (void)gmp::walk_row(rowptr, col, nnz, p0, nn, v, [&](int u) { sum += mix(cur[u]); });      // (round 0 counted the strays)
            const u64 c = mix(cur[v] * K1 + sum + (u64)r * K2);
            nxt[v] = c;
            list[r * n + v] = c;
            if (colors) colors[(int64_t)r * num_nodes + gv] = (int64_t)c;
        }
        __syncthreads();
        u64* s = cur;
        cur = nxt;
        nxt = s;
    }

    // ---- histogram of all (h + 1) n colours
    for (int k = t; k < len; k += T) atomicAdd(&bins[gmp::hashed_bin(list[k], dim)], 1u);

    // ---- sort list[0, len) ascending (unsigned).  Every step pairs i < j and leaves the smaller word at i; j >= len is "+infinity".
    const int P = (int)pow2_ceil(len > 0 ? len : 1);                // block-uniform trip counts: every thread reaches every barrier
    for (int k = 2; k <= P; k <<= 1) {
        const int half = k >> 1;
        __syncthreads();
        for (int q = t; q < (P >> 1); q += T) {                     // the mirror step: i <-> the block's end - i
            const int blk = q / half, off = q - blk * half;
            const int i = blk * k + off, j = blk * k + k - 1 - off;
            if (j < len) {
                const u64 a = list[i], b = list[j];
                if (a > b) {
                    list[i] = b;
                    list[j] = a;
                }
            }
        }
        for (int s = half >> 1; s > 0; s >>= 1) {
            __syncthreads();
            for (int q = t; q < (P >> 1); q += T) {
                const int i = (q / s) * (s << 1) + (q % s), j = i + s;
                if (j < len) {
                    const u64 a = list[i], b = list[j];
                    if (a > b) {
                        list[i] = b;
                        list[j] = a;
                    }
                }
            }
        }
    }
    __syncthreads();

    int64_t* out = sorted + (int64_t)hp1 * p0;
    for (int k = t; k < len; k += T) out[k] = (int64_t)list[k];
    for (int b = t; b < dim; b += T) hist[(int64_t)gidx * dim + b] = (int32_t)bins[b];
    if (t == 0) status[gidx] = (int32_t)gmp::status_word(skipped, gmp::SKIP_MAX);
}

// the first i in [lo, hi) with s[i] >= key / > key (unsigned; hi if none)
template <typename P, typename I>
__device__ __forceinline__ I lower_bound(P s, I lo, I hi, u64 key) {
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if ((u64)s[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}
template <typename P, typename I>
__device__ __forceinline__ I upper_bound(P s, I lo, I hi, u64 key) {
    while (lo < hi) {
        const I mid = (lo + hi) >> 1;
        if ((u64)s[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// The equal pairs between the sorted words sa[ab, ae) and sb[bb, be), this lane's share: the elements ab + lane, ab + lane + 64, ... that
// start a run (the predecessor differs) count the whole run, run length in a times run length in b.
template <typename P, typename I>
__device__ __forceinline__ long long equal_pairs(P sa, I ab, I ae, P sb, I bb, I be, int lane) {
    long long acc = 0;
    for (I k = ab + lane; k < ae; k += GMP_WAVE) {
        const u64 x = (u64)sa[k];
        if (k > ab && (u64)sa[k - 1] == x) continue;                // inside a run: its first element counts it
        const I lo = lower_bound(sb, bb, be, x);
        if (lo == be || (u64)sb[lo] != x) continue;
        const I run_b = upper_bound(sb, lo + 1, be, x) - lo;
        const I run_a = upper_bound(sa, k + 1, ae, x) - k;
        acc += (long long)run_a * (long long)run_b;
    }
    return acc;
}

struct Seg { int64_t b, e; };

// graph g's segment [hp1 ptr[g], hp1 ptr[g + 1]) clamped to [0, len]
__device__ __forceinline__ Seg seg_of(const int64_t* __restrict__ ptr, int64_t g, int64_t hp1, int64_t len) {
    const int64_t cap = len / hp1;                                  // the products below cannot overflow
    const int64_t b = min(max(ptr[g], (int64_t)0), cap) * hp1, e = min(max(ptr[g + 1], (int64_t)0), cap) * hp1;
    return Seg{b, max(b, e)};
}

// (the frame -- e -> (i, j), the shuffle sum, lane 0's write -- is written out: behind a shared helper hipcc reorders this kernel, graph_block.h)
__global__ __launch_bounds__(GRAM_THREADS) void wl_gram_kernel(const int64_t* __restrict__ sa, const int64_t* __restrict__ ptr_a, int64_t Ga,
                                                               int64_t len_a, const int64_t* __restrict__ sb,
                                                               const int64_t* __restrict__ ptr_b, int64_t Gb, int64_t len_b, int64_t hp1,
                                                               int64_t* __restrict__ K) {
    __shared__ u64 stage[GRAM_WAVES][2][GRAM_STAGE];                // per wave: the two segments, when the longer one fits
    const int lane = threadIdx.x % GMP_WAVE, wave = threadIdx.x / GMP_WAVE;
    const int64_t e = (int64_t)blockIdx.x * GRAM_WAVES + wave;
    if (e >= Ga * Gb) return;                                       // (wave-uniform; no workgroup barrier below)
    const int64_t i = e / Gb, j = e - i * Gb;
    Seg a = seg_of(ptr_a, i, hp1, len_a), b = seg_of(ptr_b, j, hp1, len_b);
    if (a.e - a.b > b.e - b.b) {                                     // the count is symmetric: walk the shorter segment, search the longer
        const Seg s = a;
        a = b;
        b = s;
        const int64_t* __restrict__ p = sa;
        sa = sb;
        sb = p;
    }
    const int64_t la = a.e - a.b, lb = b.e - b.b;
    long long acc = 0;
    if (la > 0 && lb <= GRAM_STAGE) {                               // (la <= lb) both into LDS with coalesced loads: the searches' dependent
        u64* ta = stage[wave][0];                                   // reads then cost LDS latency, not a trip to L2 each
        u64* tb = stage[wave][1];
        for (int k = lane; k < (int)la; k += GMP_WAVE) ta[k] = (u64)sa[a.b + k];
        for (int k = lane; k < (int)lb; k += GMP_WAVE) tb[k] = (u64)sb[b.b + k];
        gmp::wave_sync();
        acc = equal_pairs((const u64*)ta, 0, (int)la, (const u64*)tb, 0, (int)lb, lane);
    } else if (la > 0) {
        acc = equal_pairs(sa, a.b, a.e, sb, b.b, b.e, lane);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, GMP_WAVE);
    if (lane == 0) K[e] = acc;
}

}  // namespace

extern "C" size_t gmp_wl_workspace_bytes(int num_graphs, int64_t max_graph_nodes, int iters) {
    (void)num_graphs;
    (void)max_graph_nodes;
    (void)iters;
    return 0;                                                       // colours, list and histogram live in LDS
}

extern "C" int gmp_wl_refine(const int64_t* ptr, int num_graphs, const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t nnz,
                             const int64_t* labels, int iters, int dim, int64_t max_graph_nodes, int64_t* colors, int64_t* sorted,
                             int32_t* hist, int32_t* status, void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    (void)workspace;
    (void)workspace_bytes;
    if (num_graphs < 0 || num_nodes < 0 || num_nodes >= ((int64_t)1 << 31) || nnz < 0 || nnz >= ((int64_t)1 << 31) || max_graph_nodes < 0)
        return gmp::fail(GMP_ERR_ARG, "wl_refine: num_graphs=%d num_nodes=%lld nnz=%lld max_graph_nodes=%lld", num_graphs, (long long)num_nodes,
                         (long long)nnz, (long long)max_graph_nodes);
    if (iters < 0 || iters > MAX_ITERS || dim < 1 || dim > MAX_DIM)
        return gmp::fail(GMP_ERR_ARG, "wl_refine: iters=%d dim=%d (0 <= iters <= %d, 1 <= dim <= %d)", iters, dim, MAX_ITERS, MAX_DIM);
    if (num_graphs == 0) return GMP_OK;
    if (!ptr || !rowptr || (nnz > 0 && !col) || (num_nodes > 0 && !sorted) || !hist || !status)
        return gmp::fail(GMP_ERR_ARG, "wl_refine: null pointer");
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)num_graphs);
    const int hp1 = iters + 1;
    static std::atomic<uint64_t> done[2];                          // once per device and instance
    return gmp::launch_by_size(                                     // the large instance reserves for the largest graph and the most rounds
        "wl_refine", max_graph_nodes, done, wl_refine_kernel<SMALL_N>, 0, wl_refine_kernel<LARGE_N>, (int)lds_bytes(LARGE_N, MAX_ITERS + 1, MAX_DIM),
        [&](auto kernel, int T, const gmp::Instance& in) {
            hipLaunchKernelGGL(kernel, grid, dim3(T), lds_bytes(in.cap, hp1, dim), st, ptr, rowptr, col, num_nodes, nnz, labels, iters, dim, in.n_min,
                               in.cap, in.flag_large, colors, sorted, hist, status);
            return gmp::check_launch(T == LARGE_N ? "wl_refine_kernel<1024>" : "wl_refine_kernel<256>");
        });
}

extern "C" int gmp_wl_gram(const int64_t* sorted_a, const int64_t* ptr_a, int64_t num_graphs_a, int64_t len_a, const int64_t* sorted_b,
                           const int64_t* ptr_b, int64_t num_graphs_b, int64_t len_b, int iters, int64_t* K, gmp_stream_t stream) {
    if (num_graphs_a < 0 || num_graphs_b < 0 || len_a < 0 || len_b < 0 || iters < 0 || iters > MAX_ITERS)
        return gmp::fail(GMP_ERR_ARG, "wl_gram: num_graphs_a=%lld num_graphs_b=%lld len_a=%lld len_b=%lld iters=%d (0 <= iters <= %d)",
                         (long long)num_graphs_a, (long long)num_graphs_b, (long long)len_a, (long long)len_b, iters, MAX_ITERS);
    if (num_graphs_a == 0 || num_graphs_b == 0) return GMP_OK;
    if (!ptr_a || !ptr_b || !K || (len_a > 0 && !sorted_a) || (len_b > 0 && !sorted_b)) return gmp::fail(GMP_ERR_ARG, "wl_gram: null pointer");
    int64_t blocks = 0;
    if (int rc = gmp::gram_blocks("wl_gram", num_graphs_a, num_graphs_b, &blocks)) return rc;
    hipLaunchKernelGGL(wl_gram_kernel, dim3((unsigned)blocks), dim3(GRAM_THREADS), 0, (hipStream_t)stream, sorted_a, ptr_a, num_graphs_a, len_a,
                       sorted_b, ptr_b, num_graphs_b, len_b, (int64_t)(iters + 1), K);
    return gmp::check_launch("wl_gram_kernel");
}
