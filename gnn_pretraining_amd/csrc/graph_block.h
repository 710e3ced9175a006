// What the kernels that run one workgroup per graph of a collated batch share (graph_props.hip, wl.hip, sp.hip, graph_feat.hip), so that
// each file holds its own algorithm and nothing else.  Integer arithmetic only: wl.hip and sp.hip are pinned bit for bit.
//   two instances  a kernel is built for SMALL_N threads (graphs of up to SMALL_N nodes) and for LARGE_N threads (those above).
//                  launch_by_size() plans them: a batch within SMALL_N gets the small instance alone, any other both launches over one
//                  grid.  LDS above 64 KiB is reserved BEFORE the first launch, so a reservation that fails leaves nothing launched.
//   block prologue NOT here.  Every kernel opens with the same three lines -- read ptr[g] and ptr[g + 1]; refuse a graph above `cap`
//                  (status bit 0, written by the one instance that carries flag_large: the large one when there are two) and leave;
//                  leave when nn < n_min, the other instance's graph -- but each has its own rule for a ptr that is no offset table
//                  (wl, sp refuse it, graph_feat clamps it into [0, num_nodes], graph_props has no num_nodes and tests nn alone) and
//                  owes its own writes beside the status.  As a shared predicate, in any of the forms tried (an enum, two flags, a
//                  method tested in the `if`), hipcc no longer carries what the branch proved about nn into the body and reorders
//                  every kernel: 0.9 to 2.4 % slower at PROTEINS shape.  Written out, the device code is the parent's.
//   status word    bit 0 = refused (above the instance's bound, or a malformed ptr where the kernel refuses one); bit 1 = more distinct
//                  keys than the row stride, bit 2 = a label outside its range (sp.hip alone); bits 8 .. = the adjacency entries that
//                  left the graph and were skipped, saturating at SKIP_MAX (an int32 word; graph_props.hip's int64 slot: SKIP_MAX_WIDE).
//   row walk       a node's in-graph neighbours from its clamped CSR row (csr::row_of), the rest counted.  Not for graph_feat.hip (its
//                  order of float adds is prop::fold_row's contract) nor graph_props.hip (an edge list).  hash: splitmix64's
//                  finaliser, its increment K1, and the rule that takes a hash word to one of dim bins.
//   Gram launch    the block size of the two Gram kernels (one wave per entry K[i, j]) and the host's grid check.  The kernels' frame --
//                  e -> (i, j), the int64 shuffle sum, lane 0's write -- stays written out in both: behind a shared helper (a frame
//                  taking the lane's share as a callable, or an index helper plus a sum helper) wl_gram_kernel gains instructions or
//                  has them reordered, and measured 0.25 % slower at PROTEINS shape.  Written out, both are the parent's code.
#pragma once
#include <algorithm>

#include "csr_graph.h"

namespace gmp {

constexpr int SMALL_N = 256, LARGE_N = 1024;                        // the most nodes of a graph, by instance
inline bool two_instances(int64_t max_graph_nodes) { return max_graph_nodes > SMALL_N; }         // such a batch gets both
constexpr unsigned int SKIP_MAX = (1u << 23) - 1u;                  // what bits 8 .. 30 of an int32 status word hold
constexpr u64 SKIP_MAX_WIDE = (1ull << 54) - 1ull;                  // the same for an int64 slot
constexpr unsigned int STATUS_REFUSED = 1u, STATUS_OVERFLOW = 2u, STATUS_BAD_LABEL = 4u;

// the status word of a graph with `skipped` stray entries, in the width W of its counter (unsigned int or u64)
template <typename W>
__device__ __forceinline__ W status_word(W skipped, W skip_max, W flags = 0) { return (min(skipped, skip_max) << 8) | flags; }

// the power of two >= v (1 for v <= 1), in v's type
template <typename I>
__host__ __device__ inline I pow2_ceil(I v) {
    I p = 1;
    while (p < v) p <<= 1;
    return p;
}

struct Instance { int cap, n_min, flag_large; };                    // min(max_graph_nodes, the instance's limit); the kernel's two arguments

// The plan.  launch(kernel, threads, Instance) launches one instance and returns gmp::check_launch's code; small_lds / large_lds are the
// instance's worst-case dynamic LDS where that is above 64 KiB (0: nothing to reserve), reserved once per device under the name `who`;
// done[0] / done[1] are the caller's per-device "reserved" bits of its small / large kernel (a function-local static beside the call).
template <class Kernel, class Launch>
inline int launch_by_size(const char* who, int64_t max_graph_nodes, std::atomic<uint64_t> (&done)[2], Kernel small_kernel, int small_lds,
                          Kernel large_kernel, int large_lds, Launch launch) {
    const bool two = two_instances(max_graph_nodes);
    const Instance small{(int)std::max<int64_t>(1, std::min<int64_t>(max_graph_nodes, SMALL_N)), 0, two ? 0 : 1};
    const Instance large{(int)std::min<int64_t>(max_graph_nodes, LARGE_N), SMALL_N + 1, 1};
    if (small_lds)                                                  // both before anything is launched
        if (int rc = reserve_lds(done[0], (const void*)small_kernel, small_lds, who)) return rc;
    if (two && large_lds)
        if (int rc = reserve_lds(done[1], (const void*)large_kernel, large_lds, who)) return rc;
    if (int rc = launch(small_kernel, SMALL_N, small)) return rc;
    return two ? launch(large_kernel, LARGE_N, large) : GMP_OK;
}

// Row p0 + v of the batch's CSR, v a node of the graph [p0, p0 + nn): visit(u) for every entry inside the graph, u in [0, nn), in entry
// order; returns the number of entries outside it, which are never used as an index.
template <class Visit>
__device__ __forceinline__ unsigned int walk_row(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t nnz, int64_t p0,
                                                 int64_t nn, int v, Visit visit) {
    const csr::Row row = csr::row_of(rowptr, nnz, p0 + v);
    unsigned int outside = 0u;
    for (int64_t i = row.b; i < row.e; ++i) {
        const int64_t u = (int64_t)col[i] - p0;
        if (u >= 0 && u < nn) visit((int)u); else ++outside;
    }
    return outside;
}

// the splitmix64 finaliser and its increment
constexpr u64 K1 = 0x9E3779B97F4A7C15ull;
__device__ __forceinline__ u64 mix(u64 z) {
    z ^= z >> 30;
    z *= 0xBF58476D1CE4E5B9ull;
    z ^= z >> 27;
    z *= 0x94D049BB133111EBull;
    z ^= z >> 31;
    return z;
}

// the bin of a hash word among dim: (x * dim) >> 32 with x = the word's high half < 2^32, so the bin is below dim
__device__ __forceinline__ unsigned int hashed_bin(u64 word, int dim) {
    return (unsigned int)(((u64)(unsigned int)(word >> 32) * (u64)(unsigned int)dim) >> 32);
}

constexpr int GRAM_THREADS = 256, GRAM_WAVES = GRAM_THREADS / GMP_WAVE;

// *blocks = the blocks of GRAM_THREADS that cover a Ga x Gb Gram (both > 0), or GMP_ERR_ARG where they exceed one grid
inline int gram_blocks(const char* who, int64_t Ga, int64_t Gb, int64_t* blocks) {
    const int64_t limit = (int64_t)1 << 31;
    if (Ga >= limit || Gb >= limit || (Ga * Gb + GRAM_WAVES - 1) / GRAM_WAVES >= limit)
        return fail(GMP_ERR_ARG, "%s: %lld x %lld entries exceed one grid", who, (long long)Ga, (long long)Gb);
    *blocks = (Ga * Gb + GRAM_WAVES - 1) / GRAM_WAVES;
    return GMP_OK;
}

}  // namespace gmp
