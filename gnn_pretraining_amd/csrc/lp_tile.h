// The scorer tile shared by the fine-tuning link scorer's forward (lp_score.hip) and the all-candidate ranking (lp_rank.hip): a
// workgroup of eight waves builds the 32 x 768 feature tile [hs+hd | hs*hd | |hs-hd|] of 32 pairs in LDS, and for one group of 32
// hidden units every wave runs a 96-deep k-slice of feat W0^T on v_mfma_f32_32x32x2_f32 (exact fp32), spills it, and the slices are
// added in wave order, then + b0, ReLU and the partial dot with w3.  Every sum here has one fixed order, so whoever builds on this
// header sees the same bits for the same pair; which pairs a tile holds, where the slices are spilled, the loop over the hidden groups
// and the barriers belong to each kernel.
#pragma once
#include "gnnmp_internal.h"

namespace lpt {

constexpr int F = 256;              // node embedding width
constexpr int HID = 256;            // hidden units of the scorer
constexpr int KF = 3 * F;           // feature width
constexpr int BM = 32;              // pairs per tile
constexpr int LDA = KF + 4;         // LDS row stride of the feature tile (16-byte skew: conflict-free ds_read_b128 down a column)
constexpr int THREADS = 512;        // 8 waves, one 96-deep k-slice each

using gmp::f32x16;

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float4 row4(const float4* __restrict__ h, int64_t i, int64_t N, int c4) {
    return (i >= 0 && i < N) ? h[i * (F / 4) + c4] : zero4();
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// The feature tile tile[BM][LDA] of the pairs (src(r), dst(r)), r in [0, BM): an index outside [0, N) reads as a zero row.  Every thread
// of the block calls it.  src and dst are taken by reference, as lambdas in the kernel would capture what they read (sim_tile.h).
template <typename Src, typename Dst>
__device__ __forceinline__ void build(float* __restrict__ tile, const float4* __restrict__ h4, int64_t N, const Src& src, const Dst& dst) {
    const int t = threadIdx.x;
    for (int it = t; it < BM * (F / 4); it += THREADS) {
        const int r = it / (F / 4), c4 = it % (F / 4);
        const float4 s = row4(h4, src(r), N, c4), d = row4(h4, dst(r), N, c4);
        float* o = tile + r * LDA + 4 * c4;
        *reinterpret_cast<float4*>(o) = make_float4(s.x + d.x, s.y + d.y, s.z + d.z, s.w + d.w);
        *reinterpret_cast<float4*>(o + F) = make_float4(s.x * d.x, s.y * d.y, s.z * d.z, s.w * d.w);
        *reinterpret_cast<float4*>(o + 2 * F) = make_float4(fabsf(s.x - d.x), fabsf(s.y - d.y), fabsf(s.z - d.z), fabsf(s.w - d.w));
    }
}

// The wave's k-slice of the 32 x 32 tile feat W0[n0, n0 + 32)^T: wave `wave` takes k in [96 wave, 96 wave + 96); lanes 0-31 take its
// first 48 k, lanes 32-63 the second (A and B agree on the pairing).  wave = t >> 6, l31 = t & 31, half = (t & 63) >> 5 come from the
// kernel, here and in spill: derived again inside, hipcc forms the spill's addresses differently and the ranking kernels take a VGPR more.
__device__ __forceinline__ f32x16 slice(const float* __restrict__ tile, const float* __restrict__ w0, int n0, int wave, int l31, int half) {
    const int kb = 96 * wave + 48 * half;
    const float4* a4 = reinterpret_cast<const float4*>(tile + l31 * LDA + kb);
    const float4* b4 = reinterpret_cast<const float4*>(w0 + (int64_t)(n0 + l31) * KF + kb);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
    float4 bv[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) bv[q] = b4[q];
#pragma unroll
    for (int q = 0; q < 12; ++q) {
        const float4 av = a4[q];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, bv[q].x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, bv[q].y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, bv[q].z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, bv[q].w, acc, 0, 0, 0);
    }
    return acc;
}

// the wave's slice into red[8][32][32] (slice, pair, hidden unit)
__device__ __forceinline__ void spill(float* __restrict__ red, const f32x16& acc, int wave, int l31, int half) {
#pragma unroll
    for (int r = 0; r < 16; ++r) red[gmp::acc_row(r, half, wave * 32) * 32 + l31] = acc[r];
}

// Threads t < 256 only, after a barrier behind spill: thread t has pair t >> 3 and the four hidden units from n0 + 4 (t & 7).
// relu(z + b0) of those, z the eight k-slices added in order
__device__ __forceinline__ float4 hidden4(const float* __restrict__ red, const float* __restrict__ b0, int n0) {
    const int t = threadIdx.x, row = t >> 3, c4 = t & 7, col = n0 + 4 * c4;
    float4 z = zero4();
#pragma unroll
    for (int w = 0; w < 8; ++w) {
        const float4 v = *reinterpret_cast<const float4*>(red + (w * 32 + row) * 32 + 4 * c4);
        z.x += v.x; z.y += v.y; z.z += v.z; z.w += v.w;
    }
    const float4 bb = *reinterpret_cast<const float4*>(b0 + col);
    return make_float4(fmaxf(z.x + bb.x, 0.f), fmaxf(z.y + bb.y, 0.f), fmaxf(z.z + bb.z, 0.f), fmaxf(z.w + bb.w, 0.f));
}

// The pair's partial dot with w3 over the 32 units of the group, on each of the pair's 8 lanes.  d is hidden4's a times the dropout
// mask; without dropout the caller passes a itself, which a mask of 1.f would give bit for bit.
__device__ __forceinline__ float partial_dot(const float4& d, const float* __restrict__ w3, int n0) {
    const int t = threadIdx.x, col = n0 + 4 * (t & 7);
    const float4 ww = *reinterpret_cast<const float4*>(w3 + col);
    float dot = d.x * ww.x;
    dot += d.y * ww.y;
    dot += d.z * ww.z;
    dot += d.w * ww.w;
    dot += __shfl_xor(dot, 1, 64);                              // the row's 8 lanes, a fixed butterfly
    dot += __shfl_xor(dot, 2, 64);
    dot += __shfl_xor(dot, 4, 64);
    return dot;
}

}  // namespace lpt
