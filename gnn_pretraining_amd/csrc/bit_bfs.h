// The wave-level bit-set BFS over an n x n adjacency bit matrix in LDS that graph_props.hip (components, diameter) and sp.hip (all-pairs hop
// distances) share.  The matrix A has row stride w = ceil(n / 64) 64-bit words.
//
// Lane layout: wp = the power of two >= w (1 .. 16); a wave is 64 / wp lane groups, lane `word` = lane % wp of a group holds word `word`
// of a bit set -- consecutive lanes take consecutive 64-bit words (ds_read_b64).  The BFS bit sets (frontier, visited) are one 64-bit
// REGISTER per lane (word `word`, replicated in every group), not LDS: a wave needs no slice and no barrier of its own, and the frontier
// word a level walks is fetched with a shuffle.  One level = OR of the adjacency rows of the frontier into next & ~visited; the groups of
// the wave split each frontier word's bits between them (bit b goes to group b % groups) and an xor-shuffle ORs the groups' partial rows.
#pragma once
#include "graph_block.h"

namespace gmp {

struct Lanes {
    int w, wp, word, g0;      // row words, lanes per group, this lane's word, first lane of this lane's group
    u64 stripe;               // the frontier bits this lane's group expands: b % (64 / wp) == group
    u64 valid;                // node bits of word `word` that exist (node id < n)
};

// the layout of lane `lane` for a graph of n nodes
__device__ __forceinline__ Lanes make_lanes(int n, int lane) {
    Lanes L;
    L.w = (n + 63) >> 6;
    L.wp = pow2_ceil(L.w > 0 ? L.w : 1);
    const int groups = 64 / L.wp, grp = lane / L.wp;
    L.word = lane & (L.wp - 1);
    L.g0 = lane - L.word;
    L.stripe = 0ull;
    for (int b = grp; b < 64; b += groups) L.stripe |= 1ull << b;
    const int rem = n - L.word * 64;
    L.valid = rem >= 64 ? ~0ull : (rem > 0 ? ((1ull << rem) - 1ull) : 0ull);
    return L;
}

// One BFS of a wave from the frontier F (word `word` of the bit set in every group's lane `word`); V = visited on return.
// found(d, F) is called once per level d = 1, 2, ... that found a new node, in every lane, with the lane's word of the set of nodes at
// hop distance exactly d (wave-uniform call; what it does may diverge, but it must not use a cross-lane operation).  The BFS stops after
// level max_levels.  Returns the number of levels that found a new node (unbounded: the eccentricity of a single source).
template <typename Found>
__device__ __forceinline__ int wave_bfs(const u64* __restrict__ A, const Lanes& L, u64 F, u64& V, int max_levels, Found&& found) {
    V = F;
    int levels = -1;
    const u64 group0 = (L.wp == 64) ? ~0ull : ((1ull << L.wp) - 1ull);
    for (;;) {
        u64 nz = __ballot(F != 0ull) & group0;                       // the frontier's non-empty words (wave-uniform)
        if (!nz) break;
        if (++levels > 0) found(levels, F);
        if (levels >= max_levels) break;
        u64 acc = 0ull;
        while (nz) {
            const int j = __builtin_ctzll(nz);
            nz &= nz - 1ull;
            u64 m = __shfl(F, j, 64) & L.stripe;
            while (m) {                                              // divergent between groups; no cross-lane operation inside
                const int b = __builtin_ctzll(m);
                m &= m - 1ull;
                if (L.word < L.w) acc |= A[(j * 64 + b) * L.w + L.word];
            }
        }
        for (int o = L.wp; o < 64; o <<= 1) acc |= __shfl_xor(acc, o, 64);
        F = acc & ~V;
        V |= F;
    }
    return levels < 0 ? 0 : levels;
}

// the unbounded BFS without a per-level hook
__device__ __forceinline__ int wave_bfs(const u64* __restrict__ A, const Lanes& L, u64 F, u64& V) {
    return wave_bfs(A, L, F, V, 0x7fffffff, [](int, u64) {});
}

}  // namespace gmp
