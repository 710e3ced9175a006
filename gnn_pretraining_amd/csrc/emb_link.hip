// The embedding link probe: pairs scored by the cosine or the inner product of their embedding rows, and every true pair ranked against
// ALL nodes under gmp_lp_rank's filtered protocol, without the Q x N score matrix.  The cross of knn.hip (queries in registers, the
// candidates streaming by in LDS tiles, sim_tile.h) and hardneg_stream.hip (an LDS bitmap of what a row must not count).
//
//   emb_link_prep_kernel        one wave per row of h: zn = h / max(||h||, 1e-12) (mode 0, gmp::normalize_row: gmp_knn_topk's copy) or h
//                               itself (mode 1), row stride padded with zeros to a multiple of 4
//   emb_link_pair_kernel<DP>    block of 128 pairs: each of the four waves keeps its 32 source rows zn[src[p]] in registers, the 32
//                               destination rows zn[dst[p]] of one wave at a time are gathered into the LDS tile, and that wave takes the
//                               DIAGONAL of its 32 x 32 tile (Tile<DP>::product): score[p].  In the ranking it also zeroes the two counts.
//   emb_link_count_kernel<DP>   block (tile of 128 queries, chunk of at most 32 candidate tiles = 1,024 nodes): the source rows in
//                               registers as above, the chunk's 32-row tiles of zn staged in LDS with the fetch / stash double step.  The
//                               exclusion mask is an LDS bitmap of 128 rows x 1,024 bits filled per query row from its source's filter row
//                               (lpf::mark_each) plus the two bits of src[q] and dst[q].  Every unmasked accumulator is compared with the
//                               row's score_true; a lane counts its 16 rows in registers (greater in the low half-word, equal in the
//                               high one), the block sums them per row in LDS and adds them to n_greater / n_equal with one integer
//                               atomicAdd per (row, block, count).
// The score of a pair (s, c) is ONE Tile<DP>::product chain of row s in registers against row c in the LDS tile, at whatever place of
// whatever tile: the pair kernel, the count kernel and matrix_out see the same bits, and in mode 0 they are gmp_knn_topk's for the query
// row h[s] (the same normalised rows, the same DP).  Integer counts only: the result does not depend on the block order.
#include <algorithm>

#include "lp_filter.h"
#include "sim_tile.h"

namespace {

using namespace sim;

constexpr int MAX_DIM = 256;
constexpr int MAX_TPC = 32;                 // candidate tiles per chunk: a mask bitmap of 128 rows x 1024 columns = 16 KiB
constexpr int64_t ROW_LIMIT = (int64_t)1 << 31;
enum { COS = 0, DOT = 1 };

struct Plan {
    int dpad, nct, tpc, chunks;
    int64_t tiles;
};

Plan make_plan(int64_t Q, int64_t N, int dim) {
    Plan p;
    p.dpad = pad4(dim);
    p.tiles = (Q + BM - 1) / BM;
    p.nct = (int)((N + BN - 1) / BN);
    // chunks of 1,024 nodes, shorter ones while the query tiles alone leave most of the 256 CUs idle: about two rounds of blocks
    int64_t c = p.tiles > 0 ? (512 + p.tiles - 1) / p.tiles : 1;
    c = std::min<int64_t>(c, p.nct);
    c = std::max<int64_t>(c, (p.nct + MAX_TPC - 1) / MAX_TPC);
    c = std::max<int64_t>(c, 1);
    p.tpc = std::max(1, (int)((p.nct + c - 1) / c));
    p.chunks = (p.nct + p.tpc - 1) / p.tpc;
    return p;
}

float* carve(void* ws, int64_t N, int dim, size_t* total) {
    gmp::Carver c(ws, true);
    float* zn = c.take<float>((size_t)N * pad4(dim));
    if (total) *total = c.total();
    return zn;
}

__global__ __launch_bounds__(THREADS) void emb_link_prep_kernel(const float* __restrict__ h, int64_t N, int d, int dpad, int mode,
                                                                float* __restrict__ zn) {
    const int64_t row = ((int64_t)blockIdx.x * THREADS + threadIdx.x) / 64;
    if (row >= N) return;
    if (mode == COS) {
        gmp::normalize_row(h + row * d, d, zn + row * dpad, dpad, nullptr);
    } else {
        for (int c = threadIdx.x % 64; c < dpad; c += 64) zn[row * dpad + c] = c < d ? h[row * d + c] : 0.f;
    }
}

// the lane's share of row `node` of zn as Tile<DP>::product takes a query row (k in [half DP/2, (half + 1) DP/2)); zeros beyond dpad and
// for a node outside [0, N)
template <int DP>
__device__ __forceinline__ void load_query(float4 (&q)[Tile<DP>::KQ], const float* __restrict__ zn, int64_t node, int64_t N, int dpad, int half) {
    const bool ok = node >= 0 && node < N;
#pragma unroll
    for (int u = 0; u < Tile<DP>::KQ; ++u) {
        const int kk = half * (DP / 2) + 4 * u;
        q[u] = (ok && kk < dpad) ? *reinterpret_cast<const float4*>(zn + node * dpad + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// Tile<DP>::fetch for rows given by index: rows[0, BN) of zn into registers, zeros for rows[r] < 0
template <int DP>
__device__ __forceinline__ void gather(float4 (&pf)[Tile<DP>::NLD], const float* __restrict__ zn, const int64_t* rows, int dpad, int t) {
#pragma unroll
    for (int u = 0; u < Tile<DP>::NLD; ++u) {
        const int it = t + u * THREADS, r = it / Tile<DP>::C4, c4 = it % Tile<DP>::C4;
        const int64_t j = rows[r];
        pf[u] = (j >= 0 && 4 * c4 < dpad) ? *reinterpret_cast<const float4*>(zn + j * dpad + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// Registers as in knn_scan_kernel (the query rows are DP / 2 floats per lane), hence the same bound: two workgroups per CU up to DP = 128.
template <int DP>
__global__ __launch_bounds__(THREADS, DP <= 128 ? 2 : 1) void emb_link_pair_kernel(const float* __restrict__ zn, int64_t N, int dpad,
                                                                                   const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                                                   int64_t P, float* __restrict__ score,
                                                                                   int32_t* __restrict__ n_greater, int32_t* __restrict__ n_equal) {
    using Tl = Tile<DP>;
    __shared__ float4 kt4[BN * Tl::LD / 4];
    __shared__ int64_t didx[BM];                                    // the block's destinations, -1 = a zero row
    float* kt = reinterpret_cast<float*>(kt4);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    const int64_t b0 = (int64_t)blockIdx.x * BM;
    const int64_t i0 = b0 + wave * 32;
    if (t < BM) {
        const int64_t p = b0 + t;
        const int64_t d = p < P ? dst[p] : -1;
        didx[t] = (d >= 0 && d < N) ? d : -1;
        if (n_greater && p < P) {
            n_greater[p] = 0;
            n_equal[p] = 0;
        }
    }
    float4 q[Tl::KQ];
    {
        const int64_t p = i0 + l31;
        load_query<DP>(q, zn, p < P ? src[p] : -1, N, dpad, half);
    }
    __syncthreads();
    const int stages = (int)min((int64_t)(BM / 32), (P - b0 + 31) / 32);        // waves with pairs
    float4 pf[Tl::NLD];
    gather<DP>(pf, zn, didx, dpad, t);
    for (int w = 0; w < stages; ++w) {
        __syncthreads();                    // the previous tile's reader is done
        Tl::stash(pf, kt, t);
        __syncthreads();
        if (w + 1 < stages) gather<DP>(pf, zn, didx + 32 * (w + 1), dpad, t);
        if (wave != w) continue;

        const f32x16 acc = Tl::product(q, kt, l31, half);

        // pair l31 of the wave is accumulator row l31, column l31: row (r & 3) + 8 (r >> 2) + 4 half of the lane with that column
        if (((l31 >> 2) & 1) == half && i0 + l31 < P) score[i0 + l31] = pick(acc, (l31 & 3) + 4 * (l31 >> 3));
    }
}

template <int DP>
__global__ __launch_bounds__(THREADS, DP <= 128 ? 2 : 1) void emb_link_count_kernel(const float* __restrict__ zn, int64_t N, int dpad, int tpc, int nct,
                                                                                    unsigned int tiles, const int64_t* __restrict__ src,
                                                                                    const int64_t* __restrict__ dst, int64_t Q,
                                                                                    const int32_t* __restrict__ frowptr, const int32_t* __restrict__ fcol,
                                                                                    int64_t fnnz, const float* __restrict__ score_true,
                                                                                    int32_t* __restrict__ n_greater, int32_t* __restrict__ n_equal,
                                                                                    float* __restrict__ matrix_out) {
    using Tl = Tile<DP>;
    __shared__ float4 kt4[BN * Tl::LD / 4];
    __shared__ unsigned int bm[MAX_TPC * BM];               // [candidate tile of the chunk][wave][column]: bit r = row r of the wave is no candidate
    __shared__ float stq[BM];                               // the rows' true scores
    __shared__ unsigned int rc[BM];                         // the rows' counts: greater | equal << 16 (at most 1,024 candidates per block)
    float* kt = reinterpret_cast<float*>(kt4);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    const int64_t b0 = (int64_t)(blockIdx.x % tiles) * BM;
    const int64_t i0 = b0 + wave * 32;
    const int cs = (int)(blockIdx.x / tiles) * tpc;         // the chunk's first candidate tile
    const int ct0 = cs, ct1 = min(cs + tpc, nct);

    for (int i = t; i < MAX_TPC * BM; i += THREADS) bm[i] = 0u;
    if (t < BM) {
        stq[t] = b0 + t < Q ? score_true[b0 + t] : 0.f;
        rc[t] = 0u;
    }
    __syncthreads();
    {                                                       // two threads per query row: its source's filter row, then src and dst themselves
        const int r = t & (BM - 1), sub = t >> 7;
        const int64_t qrow = b0 + r, c_lo = (int64_t)cs * BN, width = (int64_t)(ct1 - cs) * BN;
        if (qrow < Q) {
            const int64_t s = src[qrow], d = dst[qrow];
            auto set = [&](int off) { atomicOr(&bm[(off >> 5) * BM + (r >> 5) * 32 + (off & 31)], 1u << (r & 31)); };
            lpf::mark_each(frowptr, fcol, fnnz, s, N, c_lo, width, sub, THREADS / BM, set);
            const uint64_t off = (uint64_t)((sub ? d : s) - c_lo);
            if (off < (uint64_t)width) set((int)off);
        }
    }

    float4 q[Tl::KQ];
    {
        const int64_t qrow = i0 + l31;
        load_query<DP>(q, zn, qrow < Q ? src[qrow] : -1, N, dpad, half);
    }
    const int rlim = rel(Q - i0 - 4 * half);                // accumulator row rr exists iff rr < rlim
    float st[16];
    unsigned int cnt[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        st[r] = stq[wave * 32 + 4 * half + acc_row(r, 0)];
        cnt[r] = 0u;
    }
    float4 pf[Tl::NLD];

    Tl::fetch(pf, zn, (int64_t)ct0 * BN, N, dpad, t);
    for (int ct = ct0; ct < ct1; ++ct) {
        __syncthreads();                    // the previous tile's readers are done (first trip: the bitmap is ready)
        Tl::stash(pf, kt, t);
        __syncthreads();
        if (ct + 1 < ct1) Tl::fetch(pf, zn, (int64_t)(ct + 1) * BN, N, dpad, t);
        if (i0 >= Q) continue;              // a wave without rows

        const f32x16 acc = Tl::product(q, kt, l31, half);

        // accumulator r is row i0 + 4 half + rr(r), rr = acc_row(r, 0); column colj
        const int64_t colj = (int64_t)ct * BN + l31;
        const bool col_ok = colj < N;
        const unsigned int mw = bm[(ct - cs) * BM + wave * 32 + l31];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = acc_row(r, 0);
            const bool in = col_ok && rr < rlim;
            if (matrix_out && in) matrix_out[(i0 + 4 * half + rr) * N + colj] = acc[r];
            const bool cand = in && !((mw >> (rr + 4 * half)) & 1u);
            cnt[r] += (cand && acc[r] > st[r] ? 1u : 0u) + (cand && acc[r] == st[r] ? 0x10000u : 0u);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r)
        if (cnt[r]) atomicAdd(&rc[wave * 32 + 4 * half + acc_row(r, 0)], cnt[r]);
    __syncthreads();
    if (t < BM && b0 + t < Q) {
        const unsigned int v = rc[t];
        if (v & 0xffffu) atomicAdd(&n_greater[b0 + t], (int32_t)(v & 0xffffu));
        if (v >> 16) atomicAdd(&n_equal[b0 + t], (int32_t)(v >> 16));
    }
}

int args_ok(const char* who, int64_t N, int64_t count, int dim, int mode) {
    if (dim < 1 || dim > MAX_DIM || (mode != COS && mode != DOT) || N < 0 || N >= ROW_LIMIT || count < 0 || count >= ROW_LIMIT)
        return gmp::fail(GMP_ERR_ARG, "%s: num_nodes=%lld count=%lld dim=%d mode=%d (0 <= num_nodes, count < 2^31, 1 <= dim <= %d, mode 0 or 1)", who,
                         (long long)N, (long long)count, dim, mode, MAX_DIM);
    return GMP_OK;
}

// the padded copy of h, then the scores of the `count` pairs (and, with the counts given, their zeroes)
int prep_and_pairs(const char* who, const float* h, int64_t N, int dim, int mode, const int64_t* src, const int64_t* dst, int64_t count,
                   float* score, int32_t* n_greater, int32_t* n_equal, float* zn, hipStream_t st) {
    const int dpad = pad4(dim);
    if (N > 0) {
        hipLaunchKernelGGL(emb_link_prep_kernel, dim3((unsigned)gmp::cdiv(N * 64, THREADS)), dim3(THREADS), 0, st, h, N, dim, dpad, mode, zn);
        if (int rc = gmp::check_launch("emb_link_prep_kernel")) return rc;
    }
    dispatch_dp(dpad, [&](auto dp) {
        hipLaunchKernelGGL((emb_link_pair_kernel<dp()>), dim3((unsigned)gmp::cdiv(count, BM)), dim3(THREADS), 0, st, (const float*)zn, N, dpad, src, dst,
                           count, score, n_greater, n_equal);
    });
    return gmp::check_launch(who);
}

}  // namespace

extern "C" size_t gmp_emb_link_workspace_bytes(int64_t num_nodes, int64_t num_queries, int dim) {
    if (num_nodes < 0 || num_nodes >= ROW_LIMIT || num_queries < 0 || num_queries >= ROW_LIMIT || dim < 1 || dim > MAX_DIM) return 0;
    size_t total;
    carve(nullptr, num_nodes, dim, &total);
    return total;
}

extern "C" int gmp_emb_link_score(const float* h, int64_t num_nodes, int dim, int mode, const int64_t* src, const int64_t* dst, int64_t num_pairs,
                                  float* score, void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    if (int rc = args_ok("emb_link_score", num_nodes, num_pairs, dim, mode)) return rc;
    if (num_pairs == 0) return GMP_OK;
    if ((num_nodes && !h) || !src || !dst || !score) return gmp::fail(GMP_ERR_ARG, "emb_link_score: null pointer");
    const size_t need = gmp_emb_link_workspace_bytes(num_nodes, num_pairs, dim);
    if (!workspace || workspace_bytes < need)
        return gmp::fail(GMP_ERR_WORKSPACE, "emb_link_score: workspace %zu < %zu", workspace ? workspace_bytes : (size_t)0, need);
    return prep_and_pairs("emb_link_score", h, num_nodes, dim, mode, src, dst, num_pairs, score, nullptr, nullptr,
                          carve(workspace, num_nodes, dim, nullptr), (hipStream_t)stream);
}

extern "C" int gmp_emb_link_rank(const float* h, int64_t num_nodes, int dim, int mode, const int64_t* src, const int64_t* dst, int64_t num_queries,
                                 const int32_t* filter_rowptr, const int32_t* filter_col, int64_t filter_nnz, float* score_true,
                                 int32_t* n_greater, int32_t* n_equal, float* matrix_out, void* workspace, size_t workspace_bytes,
                                 gmp_stream_t stream) {
    if (int rc = args_ok("emb_link_rank", num_nodes, num_queries, dim, mode)) return rc;
    if (filter_nnz < 0) return gmp::fail(GMP_ERR_ARG, "emb_link_rank: filter_nnz=%lld", (long long)filter_nnz);
    bool done;                                                      // (the sign of num_queries is args_ok's)
    if (int rc = lpf::rank_front("emb_link_rank", num_queries, filter_rowptr, filter_col, filter_nnz, src, dst, score_true, n_greater, n_equal, done); rc || done)
        return rc;
    if (num_nodes && !h) return gmp::fail(GMP_ERR_ARG, "emb_link_rank: null pointer");
    const Plan p = make_plan(num_queries, num_nodes, dim);
    if (p.tiles * std::max(p.chunks, 1) >= ROW_LIMIT)
        return gmp::fail(GMP_ERR_ARG, "emb_link_rank: %lld query tiles x %d candidate chunks exceed one grid", (long long)p.tiles, p.chunks);
    const size_t need = gmp_emb_link_workspace_bytes(num_nodes, num_queries, dim);
    if (!workspace || workspace_bytes < need)
        return gmp::fail(GMP_ERR_WORKSPACE, "emb_link_rank: workspace %zu < %zu", workspace ? workspace_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    float* zn = carve(workspace, num_nodes, dim, nullptr);
    if (int rc = prep_and_pairs("emb_link_rank", h, num_nodes, dim, mode, src, dst, num_queries, score_true, n_greater, n_equal, zn, st)) return rc;
    if (p.chunks == 0) return GMP_OK;                               // no candidates
    dispatch_dp(p.dpad, [&](auto dp) {
        hipLaunchKernelGGL((emb_link_count_kernel<dp()>), dim3((unsigned)(p.tiles * p.chunks)), dim3(THREADS), 0, st, (const float*)zn, num_nodes, p.dpad,
                           p.tpc, p.nct, (unsigned)p.tiles, src, dst, num_queries, filter_rowptr, filter_col, filter_nnz, (const float*)score_true,
                           n_greater, n_equal, matrix_out);
    });
    return gmp::check_launch("emb_link_count_kernel");
}
