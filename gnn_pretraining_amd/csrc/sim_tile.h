// The similarity-tile walk shared by the streaming NT-Xent (ntxent_stream.hip) and the streaming hard-negative miner
// (hardneg_stream.hip): a workgroup of four waves owns BM = 128 rows of the normalised matrix zn, each wave keeps its 32 rows in
// registers, and the columns pass by in tiles of BN = 32 rows of zn staged in LDS; every 32 x 32 tile S = zn_rows zn_cols^T is one
// v_mfma_f32_32x32x2_f32 chain and lives only in accumulators.  The chain is a k-ordered fp32 fma chain, so whoever builds on this
// header sees the same bits for the same rows; the tile loop (barriers, which tiles to skip, the epilogue) belongs to each kernel.
#pragma once
#include <type_traits>

#include "gnnmp_internal.h"

namespace sim {

constexpr int THREADS = 256;
constexpr int BM = 128;         // rows per workgroup (32 per wave)
constexpr int BN = 32;          // columns per step

using gmp::acc_row;
using gmp::f32x16;
using gmp::u64;

// acc[r] for a run-time r (a chain of selects: the accumulators stay in registers)
__device__ __forceinline__ float pick(const f32x16& a, int r) {
    float v = a[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) v = r == i ? a[i] : v;
    return v;
}

// the row stride of a normalised copy: the dimension padded to a multiple of 4
constexpr int pad4(int64_t dim) { return (int)((dim + 3) / 4 * 4); }

// f(std::integral_constant<int, DP>{}) for the smallest Tile<DP> that holds rows of dpad <= 256 floats
template <typename F>
auto dispatch_dp(int dpad, F&& f) {
    if (dpad <= 32) return f(std::integral_constant<int, 32>{});
    if (dpad <= 64) return f(std::integral_constant<int, 64>{});
    if (dpad <= 128) return f(std::integral_constant<int, 128>{});
    if (dpad <= 192) return f(std::integral_constant<int, 192>{});
    return f(std::integral_constant<int, 256>{});
}

// a row difference as an int: only values within a tile are ever compared, anything further away just has to stay away.  Row / column
// tests are made on such small ints relative to the wave's first row (64-bit row numbers per accumulator would cost 64 registers):
// accumulator r of lane half `half` is row i0 + 4 half + acc_row(r, 0), the second term a compile-time constant
__device__ __forceinline__ int rel(int64_t v) { return (int)max((int64_t)-(1 << 20), min((int64_t)(1 << 20), v)); }

// One thread's share of the walk for rows of at most DP floats (t = threadIdx.x, lane = t & 63, l31 = lane & 31, half = lane >> 5).
// The kernel owns the registers: float4 q[KQ], the lane's query row for k in [half DP/2, (half + 1) DP/2), which it loads itself, and
// float4 pf[NLD], the column tile on its way to LDS.  fetch and stash take their bounds by reference, as a lambda in the kernel would
// capture them: by value hipcc merges the two tests of fetch's guard and allocates the callers' registers differently (profiles/README.md).
template <int DP>
struct Tile {
    static constexpr int LD = DP + 4;               // column-tile row stride: 16-byte slots of consecutive rows fall on consecutive bank slots
    static constexpr int KQ = DP / 8;               // float4 of the reduction range per lane (each half of the wave takes DP / 2)
    static constexpr int C4 = DP / 4;
    static constexpr int NLD = BN * C4 / THREADS;   // float4 per thread of one column tile
    static_assert(DP % 32 == 0 && BN * C4 % THREADS == 0, "tile shape");

    // rows [j0, j0 + BN) of zn into registers, zero beyond the leading dimension ld and beyond `rows`
    __device__ __forceinline__ static void fetch(float4 (&pf)[NLD], const float* zn, int64_t j0, const int64_t& rows, const int& ld, const int& t) {
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int it = t + u * THREADS, r = it / C4, c4 = it % C4;
            const int64_t j = j0 + r;
            pf[u] = (j < rows && 4 * c4 < ld) ? *reinterpret_cast<const float4*>(zn + j * ld + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }

    // the fetched rows into the LDS tile kt[BN][LD]
    __device__ __forceinline__ static void stash(const float4 (&pf)[NLD], float* const& kt, const int& t) {
#pragma unroll
        for (int u = 0; u < NLD; ++u) {
            const int it = t + u * THREADS, r = it / C4, c4 = it % C4;
            *reinterpret_cast<float4*>(kt + r * LD + 4 * c4) = pf[u];
        }
    }

    // S tile: accumulator r = <query row acc_row(r, half), row l31 of the LDS tile>
    __device__ __forceinline__ static f32x16 product(const float4 (&q)[KQ], const float* kt, int l31, int half) {
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
        const float4* b4 = reinterpret_cast<const float4*>(kt + l31 * LD + half * (DP / 2));
        // two float4 of B ahead of the MFMAs that use them and no further: left alone, the scheduler hoists every LDS read of the tile to
        // the top and spills the query rows
        constexpr int SG = KQ >= 2 ? 2 : 1;
        float4 bc[SG], bn[SG];
#pragma unroll
        for (int v = 0; v < SG; ++v) bc[v] = b4[v];
#pragma unroll
        for (int u0 = 0; u0 < KQ; u0 += SG) {
#pragma unroll
            for (int v = 0; v < SG; ++v)
                if (u0 + SG + v < KQ) bn[v] = b4[u0 + SG + v];
#pragma unroll
            for (int v = 0; v < SG; ++v) {
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(q[u0 + v].x, bc[v].x, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(q[u0 + v].y, bc[v].y, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(q[u0 + v].z, bc[v].z, acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(q[u0 + v].w, bc[v].w, acc, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int v = 0; v < SG; ++v) bc[v] = bn[v];
        }
        return acc;
    }
};

}  // namespace sim
