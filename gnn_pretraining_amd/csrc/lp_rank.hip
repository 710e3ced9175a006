// All-candidate link ranking on top of the fine-tuning scorer (lp_score.hip): one source against EVERY node, reduced on the fly.
//   gmp_lp_rank   for Q true pairs (src, dst): the true pair's logit and how many candidates c in [0, N) score greater than / equal to it
//                 (c == src, c == dst and the entries of src's filter row are skipped) -- the filtered rank of link-prediction evaluation
//   gmp_lp_topk   for Q sources: the k <= 64 best candidates (c != src, not in the filter row), logit descending, ties to the lower index
// Neither writes a per-candidate logit, the [Q N, 256] activation or a pair list: a candidate's logit lives in one register until it is
// compared.  The logit of (s, c) is BIT FOR BIT lp_score_fwd_kernel's with p = 0: score_tile below is that kernel's tile code (the same
// 32 x 768 LDS feature tile, the same eight 96-deep k-slices per wave on v_mfma_f32_32x32x2_f32 added in order, the same eight 32-unit
// partial dots with w3 added in order, then b3), looped over the eight hidden groups inside the block instead of over blockIdx.y.
//
//   lp_rank_true_kernel    one block per 32 queries: logit_true, and the two counts set to zero
//   lp_rank_count_kernel   one block per (query, 32-candidate tile): compare, count in LDS, one integer atomicAdd per count and block
//   lp_topk_scan_kernel    one block per (query, part of the candidate tiles): a sorted 64-entry list in LDS, merged with each tile's 32
//                          logits by rank-by-counting over the 96 entries; the part's list goes to the workspace
//   lp_topk_merge_kernel   one block per query: the parts' lists ordered by rank-by-counting, the first k written
// Counts are integer sums and the order (logit, then index) is total, so both results are independent of the block order.
#include <algorithm>

#include "gnnmp_internal.h"

namespace {

using gmp::f32x16;

constexpr int F = 256;              // node embedding width
constexpr int HID = 256;            // hidden units of the scorer
constexpr int KF = 3 * F;           // feature width
constexpr int BM = 32;              // candidates (or queries) per tile
constexpr int LDA = KF + 4;         // LDS row stride of the feature tile, as in lp_score.hip
constexpr int THREADS = 512;        // 8 waves, one 96-deep k-slice each
constexpr int TILE_FLOATS = BM * LDA;
constexpr int RED_FLOATS = 8 * 32 * 32;
constexpr int LDS_BYTES = (TILE_FLOATS + RED_FLOATS) * 4;
constexpr int MAXK = 64;            // top-k list length
constexpr int UNI = MAXK + BM;      // list + one tile
constexpr int MAX_PARTS = 16;       // candidate-tile parts per query in the top-k scan

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float4 row4(const float4* __restrict__ h, int64_t i, int64_t N, int c4) {
    return (i >= 0 && i < N) ? h[i * (F / 4) + c4] : zero4();
}

// The logits of the 32 pairs (sidx[r], didx[r]) (LDS; an index outside [0, N) reads as a zero row).  Every thread of the block calls it;
// thread t < 256 returns the logit of row t >> 3, the others return garbage.  Starts with a barrier (sidx / didx written by the caller).
__device__ __forceinline__ float score_tile(float* __restrict__ tile, float* __restrict__ red, const int64_t* sidx, const int64_t* didx,
                                            const float4* __restrict__ h4, int64_t N, const float* __restrict__ w0,
                                            const float* __restrict__ b0, const float* __restrict__ w3, const float* __restrict__ b3) {
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    __syncthreads();
    for (int it = t; it < BM * (F / 4); it += THREADS) {
        const int r = it / (F / 4), c4 = it % (F / 4);
        const float4 s = row4(h4, sidx[r], N, c4), d = row4(h4, didx[r], N, c4);
        float* o = tile + r * LDA + 4 * c4;
        *reinterpret_cast<float4*>(o) = make_float4(s.x + d.x, s.y + d.y, s.z + d.z, s.w + d.w);
        *reinterpret_cast<float4*>(o + F) = make_float4(s.x * d.x, s.y * d.y, s.z * d.z, s.w * d.w);
        *reinterpret_cast<float4*>(o + 2 * F) = make_float4(fabsf(s.x - d.x), fabsf(s.y - d.y), fabsf(s.z - d.z), fabsf(s.w - d.w));
    }
    __syncthreads();

    const int kb = 96 * wave + 48 * half;
    const float4* a4 = reinterpret_cast<const float4*>(tile + l31 * LDA + kb);
    const int row = (t >> 3) & 31, c4 = t & 7;
    float s = 0.f;
#pragma unroll 1
    for (int g = 0; g < HID / 32; ++g) {
        const int n0 = 32 * g;
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
#pragma unroll
        for (int r = 0; r < 16; ++r) red[gmp::acc_row(r, half, wave * 32) * 32 + l31] = acc[r];
        __syncthreads();
        if (t < 256) {                                              // (waves 0-3: wave-uniform)
            const int col = n0 + 4 * c4;
            float4 z = zero4();
#pragma unroll
            for (int w = 0; w < 8; ++w) {                           // k-slices in order
                const float4 v = *reinterpret_cast<const float4*>(red + (w * 32 + row) * 32 + 4 * c4);
                z.x += v.x; z.y += v.y; z.z += v.z; z.w += v.w;
            }
            const float4 bb = *reinterpret_cast<const float4*>(b0 + col), ww = *reinterpret_cast<const float4*>(w3 + col);
            const float4 a = make_float4(fmaxf(z.x + bb.x, 0.f), fmaxf(z.y + bb.y, 0.f), fmaxf(z.z + bb.z, 0.f), fmaxf(z.w + bb.w, 0.f));
            float dot = a.x * ww.x;                                 // (the scorer's p == 0 mask is 1.f: a * 1.f is a)
            dot += a.y * ww.y;
            dot += a.z * ww.z;
            dot += a.w * ww.w;
            dot += __shfl_xor(dot, 1, 64);                          // the row's 8 lanes, the scorer's butterfly
            dot += __shfl_xor(dot, 2, 64);
            dot += __shfl_xor(dot, 4, 64);
            s = g == 0 ? dot : s + dot;                             // lp_logit_kernel: the eight partial dots in order
        }
        __syncthreads();                                            // red is free for the next group
    }
    return s + b3[0];
}

// bit (c - c0) of *fmask for every entry c of row s of the filter CSR that falls into [c0, c0 + 32); duplicates and order do not matter
__device__ __forceinline__ void filter_mark(const int32_t* __restrict__ rowptr, const int32_t* __restrict__ col, int64_t nnz, int64_t s,
                                            int64_t N, int64_t c0, unsigned int* fmask) {
    if (!rowptr || s < 0 || s >= N) return;
    const int64_t b = max((int64_t)rowptr[s], (int64_t)0), e = min((int64_t)rowptr[s + 1], nnz);
    for (int64_t i = b + threadIdx.x; i < e; i += THREADS) {
        const uint64_t off = (uint64_t)((int64_t)col[i] - c0);
        if (off < (uint64_t)BM) atomicOr(fmask, 1u << (unsigned)off);
    }
}

__global__ __launch_bounds__(THREADS) void lp_rank_true_kernel(const float* __restrict__ h, const int64_t* __restrict__ src,
                                                               const int64_t* __restrict__ dst, int64_t N, int64_t Q,
                                                               const float* __restrict__ w0, const float* __restrict__ b0,
                                                               const float* __restrict__ w3, const float* __restrict__ b3,
                                                               float* __restrict__ logit_true, int32_t* __restrict__ n_greater,
                                                               int32_t* __restrict__ n_equal) {
    extern __shared__ float4 smem4[];
    __shared__ int64_t sidx[BM], didx[BM];
    float* tile = reinterpret_cast<float*>(smem4);
    const int t = threadIdx.x;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    if (t < BM) {
        const int64_t m = m0 + t;
        sidx[t] = m < Q ? src[m] : -1;
        didx[t] = m < Q ? dst[m] : -1;
    }
    const float lg = score_tile(tile, tile + TILE_FLOATS, sidx, didx, reinterpret_cast<const float4*>(h), N, w0, b0, w3, b3);
    const int64_t m = m0 + (t >> 3);
    if (t < 256 && (t & 7) == 0 && m < Q) {
        logit_true[m] = lg;
        n_greater[m] = 0;
        n_equal[m] = 0;
    }
}

__global__ __launch_bounds__(THREADS) void lp_rank_count_kernel(const float* __restrict__ h, const int64_t* __restrict__ src,
                                                                const int64_t* __restrict__ dst, int64_t N, int tiles,
                                                                const float* __restrict__ w0, const float* __restrict__ b0,
                                                                const float* __restrict__ w3, const float* __restrict__ b3,
                                                                const int32_t* __restrict__ frowptr, const int32_t* __restrict__ fcol,
                                                                int64_t fnnz, const float* __restrict__ logit_true,
                                                                int32_t* __restrict__ n_greater, int32_t* __restrict__ n_equal) {
    extern __shared__ float4 smem4[];
    __shared__ int64_t sidx[BM], didx[BM];
    __shared__ unsigned int fmask;
    __shared__ int cnt[2];
    float* tile = reinterpret_cast<float*>(smem4);
    const int t = threadIdx.x;
    const int64_t q = blockIdx.x / (unsigned)tiles, c0 = (int64_t)(blockIdx.x % (unsigned)tiles) * BM;
    const int64_t s = src[q], d = dst[q];
    if (t < BM) {
        const int64_t c = c0 + t;
        sidx[t] = c < N ? s : -1;
        didx[t] = c < N ? c : -1;
    }
    if (t == 0) {
        fmask = 0u;
        cnt[0] = 0;
        cnt[1] = 0;
    }
    __syncthreads();
    filter_mark(frowptr, fcol, fnnz, s, N, c0, &fmask);
    const float lg = score_tile(tile, tile + TILE_FLOATS, sidx, didx, reinterpret_cast<const float4*>(h), N, w0, b0, w3, b3);
    if (t < 256 && (t & 7) == 0) {
        const int row = t >> 3;
        const int64_t c = c0 + row;
        const bool valid = c < N && c != s && c != d && !((fmask >> row) & 1u);
        const float lt = logit_true[q];
        if (valid && lg > lt) atomicAdd(&cnt[0], 1);
        if (valid && lg == lt) atomicAdd(&cnt[1], 1);
    }
    __syncthreads();
    if (t == 0) {
        if (cnt[0]) atomicAdd(&n_greater[q], cnt[0]);
        if (cnt[1]) atomicAdd(&n_equal[q], cnt[1]);
    }
}

// a total order over list entries: real candidates (index >= 0) first, by logit descending then index ascending; padding by position
__device__ __forceinline__ bool better(float av, int ai, int apos, float bv, int bi, int bpos) {
    const bool a_ok = ai >= 0, b_ok = bi >= 0;
    if (a_ok != b_ok) return a_ok;
    if (!a_ok) return apos < bpos;
    return av > bv || (av == bv && ai < bi);
}

__global__ __launch_bounds__(THREADS) void lp_topk_scan_kernel(const float* __restrict__ h, const int64_t* __restrict__ src, int64_t N,
                                                               int tiles, int parts, const float* __restrict__ w0,
                                                               const float* __restrict__ b0, const float* __restrict__ w3,
                                                               const float* __restrict__ b3, const int32_t* __restrict__ frowptr,
                                                               const int32_t* __restrict__ fcol, int64_t fnnz,
                                                               float* __restrict__ part_v, int32_t* __restrict__ part_i) {
    extern __shared__ float4 smem4[];
    __shared__ int64_t sidx[BM], didx[BM];
    __shared__ unsigned int fmask;
    __shared__ float lv[UNI];
    __shared__ int li[UNI];
    float* tile = reinterpret_cast<float*>(smem4);
    const int t = threadIdx.x;
    const int64_t q = blockIdx.x / (unsigned)parts;
    const int part = (int)(blockIdx.x % (unsigned)parts);
    const int per = (tiles + parts - 1) / parts, t_begin = part * per, t_end = min(tiles, t_begin + per);
    const int64_t s = src[q];
    const float ninf = -__builtin_inff();
    if (t < UNI) {
        lv[t] = ninf;
        li[t] = -1;
    }
    for (int ti = t_begin; ti < t_end; ++ti) {
        const int64_t c0 = (int64_t)ti * BM;
        __syncthreads();                                            // the previous tile's merge is done with sidx / fmask / the list
        if (t < BM) {
            const int64_t c = c0 + t;
            sidx[t] = c < N ? s : -1;
            didx[t] = c < N ? c : -1;
        }
        if (t == 0) fmask = 0u;
        __syncthreads();
        filter_mark(frowptr, fcol, fnnz, s, N, c0, &fmask);
        const float lg = score_tile(tile, tile + TILE_FLOATS, sidx, didx, reinterpret_cast<const float4*>(h), N, w0, b0, w3, b3);
        if (t < 256 && (t & 7) == 0) {
            const int row = t >> 3;
            const int64_t c = c0 + row;
            const bool valid = c < N && c != s && !((fmask >> row) & 1u);
            lv[MAXK + row] = valid ? lg : ninf;
            li[MAXK + row] = valid ? (int)c : -1;
        }
        __syncthreads();
        float mv = 0.f;
        int mi = -1, rank = UNI;
        if (t < UNI) {
            mv = lv[t];
            mi = li[t];
            rank = 0;
            for (int j = 0; j < UNI; ++j) rank += (j != t && better(lv[j], li[j], j, mv, mi, t)) ? 1 : 0;
        }
        __syncthreads();
        if (rank < MAXK) {
            lv[rank] = mv;
            li[rank] = mi;
        }
    }
    __syncthreads();
    if (t < MAXK) {
        part_v[(int64_t)blockIdx.x * MAXK + t] = lv[t];
        part_i[(int64_t)blockIdx.x * MAXK + t] = li[t];
    }
}

__global__ __launch_bounds__(256) void lp_topk_merge_kernel(const float* __restrict__ part_v, const int32_t* __restrict__ part_i, int parts,
                                                            int k, int64_t* __restrict__ idx, float* __restrict__ logit) {
    __shared__ float lv[MAX_PARTS * MAXK];
    __shared__ int li[MAX_PARTS * MAXK];
    const int t = threadIdx.x, n = parts * MAXK;
    const int64_t q = blockIdx.x;
    for (int i = t; i < n; i += 256) {
        lv[i] = part_v[q * n + i];
        li[i] = part_i[q * n + i];
    }
    __syncthreads();
    for (int i = t; i < n; i += 256) {
        const float mv = lv[i];
        const int mi = li[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (j != i && better(lv[j], li[j], j, mv, mi, i)) ? 1 : 0;
        if (rank < k) {
            idx[q * k + rank] = mi >= 0 ? (int64_t)mi : (int64_t)-1;
            logit[q * k + rank] = mi >= 0 ? mv : -__builtin_inff();
        }
    }
}

int topk_parts(int64_t Q, int64_t N) {
    // enough blocks for the chip when there are few sources; one part per source once the sources alone fill it
    const int64_t tiles = (N + BM - 1) / BM;
    if (Q <= 0 || tiles <= 1 || Q >= 256) return 1;
    return (int)std::min<int64_t>(std::min<int64_t>(tiles, MAX_PARTS), (512 + Q - 1) / Q);
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

int common_ok(const char* who, int64_t N, int64_t Q, int feat, int hidden, const void* h, const void* w0, const void* b0, const void* w3,
              const void* b3, const void* frowptr, const void* fcol, int64_t fnnz) {
    if (feat != F || hidden != HID) return gmp::fail(GMP_ERR_UNSUPPORTED, "%s: feat %d / hidden %d (this kernel is built for 256 / 256)", who, feat, hidden);
    if (N < 0 || Q < 0 || N >= ((int64_t)1 << 31) || fnnz < 0) return gmp::fail(GMP_ERR_ARG, "%s: N=%lld Q=%lld filter_nnz=%lld", who, (long long)N, (long long)Q, (long long)fnnz);
    if ((frowptr == nullptr) != (fcol == nullptr) && fnnz != 0)
        return gmp::fail(GMP_ERR_ARG, "%s: filter_rowptr and filter_col must both be given or both be null", who);
    if (Q == 0) return GMP_OK;
    if ((N > 0 && !h) || !w0 || !b0 || !w3 || !b3) return gmp::fail(GMP_ERR_ARG, "%s: null pointer", who);
    if (!aligned16(h) || !aligned16(w0) || !aligned16(b0) || !aligned16(w3)) return gmp::fail(GMP_ERR_ARG, "%s: h, w0, b0 and w3 must be 16-byte aligned", who);
    return GMP_OK;
}

}  // namespace

extern "C" size_t gmp_lp_rank_workspace_bytes(int64_t Q, int64_t N) {
    (void)Q; (void)N;
    return 0;                                                       // the counts are integer atomics on the outputs: nothing is staged
}

extern "C" size_t gmp_lp_topk_workspace_bytes(int64_t Q, int64_t N) {
    return (size_t)(Q > 0 ? Q : 0) * topk_parts(Q, N) * MAXK * 8 + 256;
}

extern "C" int gmp_lp_rank(const float* h, const int64_t* src, const int64_t* dst, int64_t N, int64_t Q, int feat, int hidden,
                           const float* w0, const float* b0, const float* w3, const float* b3, const int32_t* filter_rowptr,
                           const int32_t* filter_col, int64_t filter_nnz, float* logit_true, int32_t* n_greater, int32_t* n_equal,
                           void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    (void)workspace; (void)workspace_bytes;
    if (int rc = common_ok("lp_rank", N, Q, feat, hidden, h, w0, b0, w3, b3, filter_rowptr, filter_col, filter_nnz)) return rc;
    if (Q == 0) return GMP_OK;
    if (!src || !dst || !logit_true || !n_greater || !n_equal) return gmp::fail(GMP_ERR_ARG, "lp_rank: null pointer");
    const int64_t tiles = (N + BM - 1) / BM;
    if (Q * std::max<int64_t>(tiles, 1) >= ((int64_t)1 << 31)) return gmp::fail(GMP_ERR_ARG, "lp_rank: Q=%lld x %lld candidate tiles exceed one grid", (long long)Q, (long long)tiles);
    static std::atomic<uint64_t> attr_true{0}, attr_count{0};
    if (int rc = gmp::reserve_lds(attr_true, (const void*)lp_rank_true_kernel, LDS_BYTES, "lp_rank")) return rc;
    if (int rc = gmp::reserve_lds(attr_count, (const void*)lp_rank_count_kernel, LDS_BYTES, "lp_rank")) return rc;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lp_rank_true_kernel, dim3((unsigned)gmp::cdiv(Q, BM)), dim3(THREADS), LDS_BYTES, st, h, src, dst, N, Q, w0, b0, w3, b3,
                       logit_true, n_greater, n_equal);
    if (int rc = gmp::check_launch("lp_rank_true_kernel")) return rc;
    if (tiles == 0) return GMP_OK;
    if (!filter_col) filter_rowptr = nullptr;
    hipLaunchKernelGGL(lp_rank_count_kernel, dim3((unsigned)(Q * tiles)), dim3(THREADS), LDS_BYTES, st, h, src, dst, N, (int)tiles, w0, b0, w3,
                       b3, filter_rowptr, filter_col, filter_nnz, (const float*)logit_true, n_greater, n_equal);
    return gmp::check_launch("lp_rank_count_kernel");
}

extern "C" int gmp_lp_topk(const float* h, const int64_t* src, int64_t N, int64_t Q, int k, int feat, int hidden, const float* w0,
                           const float* b0, const float* w3, const float* b3, const int32_t* filter_rowptr, const int32_t* filter_col,
                           int64_t filter_nnz, int64_t* idx, float* logit, void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    if (int rc = common_ok("lp_topk", N, Q, feat, hidden, h, w0, b0, w3, b3, filter_rowptr, filter_col, filter_nnz)) return rc;
    if (k < 1 || k > MAXK) return gmp::fail(GMP_ERR_ARG, "lp_topk: k=%d (1 <= k <= %d)", k, MAXK);
    if (Q == 0) return GMP_OK;
    if (!src || !idx || !logit || !workspace) return gmp::fail(GMP_ERR_ARG, "lp_topk: null pointer");
    if (workspace_bytes < gmp_lp_topk_workspace_bytes(Q, N)) return gmp::fail(GMP_ERR_ARG, "lp_topk: workspace too small");
    const int64_t tiles = (N + BM - 1) / BM;
    const int parts = topk_parts(Q, N);
    if (Q * parts >= ((int64_t)1 << 31)) return gmp::fail(GMP_ERR_ARG, "lp_topk: Q=%lld", (long long)Q);
    static std::atomic<uint64_t> attr_scan{0};
    if (int rc = gmp::reserve_lds(attr_scan, (const void*)lp_topk_scan_kernel, LDS_BYTES, "lp_topk")) return rc;
    char* base = (char*)(((uintptr_t)workspace + 255) / 256 * 256);
    float* part_v = (float*)base;
    int32_t* part_i = (int32_t*)(base + (size_t)Q * parts * MAXK * 4);
    if (!filter_col) filter_rowptr = nullptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lp_topk_scan_kernel, dim3((unsigned)(Q * parts)), dim3(THREADS), LDS_BYTES, st, h, src, N, (int)tiles, parts, w0, b0, w3,
                       b3, filter_rowptr, filter_col, filter_nnz, part_v, part_i);
    if (int rc = gmp::check_launch("lp_topk_scan_kernel")) return rc;
    hipLaunchKernelGGL(lp_topk_merge_kernel, dim3((unsigned)Q), dim3(256), 0, st, (const float*)part_v, (const int32_t*)part_i, parts, k, idx, logit);
    return gmp::check_launch("lp_topk_merge_kernel");
}
