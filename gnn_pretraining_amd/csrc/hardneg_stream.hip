// Streaming hard-negative mining: the contract of hardneg.hip (gmp_hard_negative_topk) without the n x n similarity matrix.
// A similarity tile (sim_tile.h) lives only in MFMA accumulators; the exact radix select of hardneg.hip runs over
// RECOMPUTED tiles, so memory is O(n d + E + a fixed candidate capacity) and n is bounded by the 40 bits the flat pair index
// i * n + j gets in the key (n <= 2^20) instead of by 65535.
//
//   hns_normalize_kernel     one wave per row: zn = z / max(||z||, 1e-12), row stride padded with zeros to a multiple of 4; its first
//                            workgroup also resets the selection state
//   gmp_csr_build            existing_edges grouped by target and by source (out-of-range endpoints dropped there)
//   hns_tile_kernel<DP, M>   block (row tile of 128, column chunk of <= 1024): each of the four waves keeps its 32 rows in registers
//                            and walks the chunk's 32-column tiles of zn (staged in LDS), S tile on v_mfma_f32_32x32x2_f32 (Tile<DP>::product,
//                            __builtin_amdgcn_mfma_f32_32x32x2f32).  Only the
//                            UPPER triangle is computed: column tiles left of the row tile are skipped, elements j <= i dropped, and
//                            an unmasked pair i < j with score s stands for the two keys (s, i n + j) and (s, j n + i).  The edge mask
//                            is an LDS bitmap (one bit per element of the block's chunk) filled from the in- and out-neighbour lists
//                            of the block's 128 rows; the epilogue tests one bit per element.
//                              M = HIST    digit histogram of the keys under the decided prefix (LDS bins, 64-bit global bins)
//                              M = GATHER  every key at or above the decided prefix -> candidate buffer
//                              M = DUMP    the masked matrix to scores_out (both triangles and the diagonal)
//                            The MFMA chain is the same code in every mode: every pass sees bit-identical scores.
//   hns_pick_kernel          one block: the bucket holding the k-th key; when (keys strictly above + bucket) fit the candidate
//                            buffer it raises `done`, and the remaining histogram launches return at once
//   hns_rank_kernel          rank-by-counting among the candidates (keys are distinct) -> out_edges / out_scores, -1 / -inf tail
// Key order: orderable score bits descending (three digits 11 / 11 / 10), then flat index ascending (40 bits as ~flat, digits
// 11 / 11 / 11 / 7).  Integer atomics only; the result does not depend on the order they land in.
#include <algorithm>

#include "sim_tile.h"

namespace {

using namespace sim;

constexpr int MAX_TPC = 32;         // column tiles per chunk: a mask bitmap of 128 rows x 1024 columns = 16 KiB
constexpr int BINS = 2048;
constexpr int MAX_K = 4096;
constexpr unsigned int CAP = 65536; // candidate capacity
constexpr int64_t MAX_N = 1 << 20;
constexpr int FLAT_BITS = 40;
constexpr unsigned long long FLAT_MAX = (1ull << FLAT_BITS) - 1ull;
enum { HIST = 0, GATHER = 1, DUMP = 2 };

// first in the workspace: `passes` is readable by the caller after the call (how many histogram passes ran)
struct State {
    int passes;
    int done;
    unsigned int out_count;
    int sshift;                 // lowest decided bit of the score part (32 = none), of the flat part (40 = none)
    int fshift;
    int pad;
    u64 sprefix, fprefix;       // decided high bits of the k-th key
    u64 k_rem;                  // rank still to be resolved inside the prefix bucket
    u64 k_eff;                  // min(k, number of unmasked ordered pairs)
    u64 hist[BINS];
};

struct Plan {
    int tiles, nct, tpc, C, dpad;
};

Plan make_plan(int64_t n, int64_t d) {
    Plan p;
    p.dpad = pad4(d);
    p.tiles = (int)((n + BM - 1) / BM);
    p.nct = (int)((n + BN - 1) / BN);
    int c = (512 + p.tiles - 1) / p.tiles;              // half of the blocks lie under the diagonal and leave at once: one round of 256 CUs             // about half of the blocks lie under the diagonal and leave at once
    c = std::min(c, (p.nct + 1) / 2);
    c = std::max(c, (p.nct + MAX_TPC - 1) / MAX_TPC);
    c = std::max(c, 1);
    p.tpc = (p.nct + c - 1) / c;
    p.C = (p.nct + p.tpc - 1) / p.tpc;
    return p;
}

struct Ws {
    State* st;
    float* zn;
    unsigned int* cand_s;
    u64* cand_f;
    int *rowptr, *col, *perm, *rowptr_t, *col_t, *perm_t, *status;
    void* csr_ws;
    size_t csr_ws_bytes, total;
};

Ws carve(void* ws, int64_t n, int64_t d, int64_t E) {
    gmp::Carver c(ws, false);
    Ws w;
    w.st = c.take<State>(1);
    w.zn = c.take<float>((size_t)n * pad4(d));
    w.cand_s = c.take<unsigned int>(CAP);
    w.cand_f = c.take<u64>(CAP);
    w.rowptr = c.take<int>((size_t)n + 1);
    w.rowptr_t = c.take<int>((size_t)n + 1);
    w.col = c.take<int>((size_t)E);
    w.perm = c.take<int>((size_t)E);
    w.col_t = c.take<int>((size_t)E);
    w.perm_t = c.take<int>((size_t)E);
    w.status = c.take<int>(1);
    w.csr_ws_bytes = gmp_csr_build_workspace_bytes(n, E);
    w.csr_ws = c.take<char>(w.csr_ws_bytes);
    w.total = c.total();
    return w;
}

__device__ void init_state(State* st, u64 k) {
    for (int i = threadIdx.x; i < BINS; i += blockDim.x) st->hist[i] = 0;
    if (threadIdx.x == 0) {
        st->passes = 0;
        st->done = 0;
        st->out_count = 0;
        st->sshift = 32;
        st->fshift = FLAT_BITS;
        st->sprefix = 0;
        st->fprefix = 0;
        st->k_rem = k;
        st->k_eff = k;
    }
}

// rows; workgroup 0 also resets the selection state
__global__ __launch_bounds__(THREADS) void hns_normalize_kernel(const float* __restrict__ z, int64_t n, int d, int dpad, float* __restrict__ zn,
                                                                State* st, u64 k) {
    if (blockIdx.x == 0) init_state(st, k);
    const int64_t row = ((int64_t)blockIdx.x * THREADS + threadIdx.x) / 64;
    if (row < n) gmp::normalize_row(z + row * d, d, zn + row * dpad, dpad, nullptr);
}

// one block: walk the digit histogram from the top, find the bucket holding the k_rem-th largest key
__global__ __launch_bounds__(THREADS) void hns_pick_kernel(State* st, int is_flat, int shift, int bits) {
    __shared__ u64 part[THREADS];
    __shared__ int skip;
    if (threadIdx.x == 0) skip = st->done;
    __syncthreads();
    if (skip) return;
    const int nb = 1 << bits;
    const int per = (nb + THREADS - 1) / THREADS;
    u64 s = 0;
    for (int j = 0; j < per; ++j) {
        const int b = threadIdx.x * per + j;
        if (b < nb) s += st->hist[b];
    }
    part[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        u64 rem = st->k_rem;
        if (st->passes == 0) {                               // fewer unmasked ordered pairs than k: select them all
            u64 total = 0;
            for (int i = 0; i < THREADS; ++i) total += part[i];
            if (total < rem) {
                rem = total;
                st->k_eff = total;
            }
        }
        if (rem == 0) {
            st->k_eff = 0;
            st->done = 1;
        } else {
            int tt = THREADS - 1;
            for (; tt > 0; --tt) {
                if (part[tt] >= rem) break;
                rem -= part[tt];
            }
            int b = min(tt * per + per - 1, nb - 1);
            for (; b > tt * per; --b) {
                const u64 c = st->hist[b];
                if (c >= rem) break;
                rem -= c;
            }
            if (is_flat) {
                st->fprefix |= (u64)b << shift;
                st->fshift = shift;
            } else {
                st->sprefix |= (u64)b << shift;
                st->sshift = shift;
            }
            st->k_rem = rem;
            // keys strictly above the bucket + the bucket itself
            if (st->k_eff - rem + st->hist[b] <= (u64)CAP) st->done = 1;
        }
        st->passes += 1;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < BINS; i += THREADS) st->hist[i] = 0;
}

// HIST: digit [shift, shift + bits) of the score part (is_flat = 0) or of the flat part (is_flat = 1)
template <int DP, int MODE>
__global__ __launch_bounds__(THREADS, DP <= 128 ? 2 : 1) void hns_tile_kernel(const float* __restrict__ zn, int64_t n, int dpad, int tpc, int nct,
                                                                              const int* __restrict__ rowptr, const int* __restrict__ col,
                                                                              const int* __restrict__ rowptr_t, const int* __restrict__ col_t,
                                                                              State* __restrict__ st, int is_flat, int shift, int bits,
                                                                              unsigned int* __restrict__ cand_s, u64* __restrict__ cand_f,
                                                                              float* __restrict__ scores_out) {
    __shared__ float4 kt4[BN * Tile<DP>::LD / 4];
    __shared__ unsigned int bm[MAX_TPC * BM];               // [column tile of the chunk][wave][column]: bit r = row r of the wave is masked
    __shared__ unsigned int h[MODE == HIST ? BINS : 1];
    float* kt = reinterpret_cast<float*>(kt4);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    const int64_t b0 = (int64_t)blockIdx.x * BM;
    const int64_t i0 = b0 + wave * 32;
    const int cs = (int)blockIdx.y * tpc;                   // the chunk's first column tile
    const int ct0 = max(cs, (int)(b0 / BN)), ct1 = min(cs + tpc, nct);
    if (ct0 >= ct1) return;                                 // the chunk lies left of the row tile
    if (MODE == HIST && st->done) return;                   // the candidates fit already
    if (MODE == GATHER && st->k_eff == 0) return;

    // the decided prefix (HIST, GATHER)
    u64 sprefix = 0, fprefix = 0;
    int sshift = 0, fshift = 0;
    if (MODE != DUMP) {
        sprefix = st->sprefix; fprefix = st->fprefix;
        sshift = st->sshift; fshift = st->fshift;
    }

    // mask bitmap of the block's rows x the chunk's columns [c_lo, c_hi)
    const int64_t c_lo = (int64_t)cs * BN, c_hi = (int64_t)ct1 * BN;
    if (rowptr) {
        for (int i = t; i < MAX_TPC * BM; i += THREADS) bm[i] = 0;
    }
    if (MODE == HIST) {
        for (int i = t; i < BINS; i += THREADS) h[i] = 0;
    }
    if (rowptr) {
        __syncthreads();
        const int r = t & (BM - 1);
        const int64_t row = b0 + r;
        if (row < n) {
            const int* rp = (t >> 7) ? rowptr_t : rowptr;
            const int* cl = (t >> 7) ? col_t : col;
            const int e1 = rp[row + 1];
            for (int e = rp[row]; e < e1; ++e) {
                const int64_t c = cl[e];
                if (c >= c_lo && c < c_hi) {
                    const int off = (int)(c - c_lo);
                    atomicOr(&bm[(off >> 5) * BM + (r >> 5) * 32 + (off & 31)], 1u << (r & 31));
                }
            }
        }
    }

    using Tl = Tile<DP>;
    // the wave's 32 rows: lane (row l31, k in [half DP/2, (half + 1) DP/2)), zero beyond dpad and beyond n
    float4 q[Tl::KQ];
    {
        const int64_t qrow = i0 + l31;
#pragma unroll
        for (int u = 0; u < Tl::KQ; ++u) {
            const int k = half * (DP / 2) + 4 * u;
            q[u] = (qrow < n && k < dpad) ? *reinterpret_cast<const float4*>(zn + qrow * dpad + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const int rlim = rel(n - i0 - 4 * half);    // accumulator row rr exists iff rr < rlim
    float4 pf[Tl::NLD];

    const u64 dmask = (1ull << bits) - 1ull;
    const int hi = shift + bits;
    // HIST: one pending (bin, count) per lane, so that runs of equal digits (tie-heavy inputs) cost one LDS atomic
    unsigned int pbin = 0, pcnt = 0;
#define HNS_HIST_ADD(bin_, c_)                                  \
    do {                                                        \
        const unsigned int nb_ = (bin_);                        \
        if (nb_ != pbin) {                                      \
            if (pcnt) atomicAdd(&h[pbin], pcnt);                \
            pbin = nb_; pcnt = 0;                               \
        }                                                       \
        pcnt += (c_);                                           \
    } while (0)

    Tl::fetch(pf, zn, (int64_t)ct0 * BN, n, dpad, t);
    for (int ct = ct0; ct < ct1; ++ct) {
        __syncthreads();                    // the previous tile's readers are done (first trip: the bitmap and the bins are ready)
        Tl::stash(pf, kt, t);
        __syncthreads();
        if (ct + 1 < ct1) Tl::fetch(pf, zn, (int64_t)(ct + 1) * BN, n, dpad, t);
        const int64_t cbase = (int64_t)ct * BN;
        if (cbase + BN - 1 < i0 + (MODE == DUMP ? 0 : 1)) continue;     // this wave's rows all lie at or below the tile's columns
        const int64_t colj = cbase + l31;

        const f32x16 acc = Tl::product(q, kt, l31, half);

        // accumulator r is row i0 + 4 half + rr(r), rr = acc_row(r, 0); column colj
        const int dd = rel(colj - i0 - 4 * half);                       // column minus the lane's first row
        const bool col_ok = colj < n;
        const unsigned int mw = rowptr ? bm[(ct - cs) * BM + wave * 32 + l31] : 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = acc_row(r, 0);
            const bool upper = col_ok && rr < rlim && dd > rr;          // i < j, both inside
            const bool masked = (mw >> (rr + 4 * half)) & 1u;
            const float v = acc[r];
            if (MODE == DUMP) {
                const int64_t row = i0 + 4 * half + rr;
                if (upper) {
                    const float o = masked ? -__builtin_inff() : v;
                    scores_out[row * n + colj] = o;
                    scores_out[colj * n + row] = o;
                } else if (col_ok && dd == rr) {
                    scores_out[row * n + colj] = -__builtin_inff();
                }
                continue;
            }
            if (!upper || masked) continue;
            const u64 sb = gmp::orderable(v);
            if (MODE == HIST) {
                if (!is_flat) {
                    if ((sb >> hi) == (sprefix >> hi)) HNS_HIST_ADD((unsigned int)((sb >> shift) & dmask), 2u);
                } else if (sb == sprefix) {
                    const u64 row = (u64)(i0 + 4 * half + rr), cj = (u64)colj;
                    const u64 f1 = FLAT_MAX - (row * (u64)n + cj), f2 = FLAT_MAX - (cj * (u64)n + row);
                    if ((f1 >> hi) == (fprefix >> hi)) HNS_HIST_ADD((unsigned int)((f1 >> shift) & dmask), 1u);
                    if ((f2 >> hi) == (fprefix >> hi)) HNS_HIST_ADD((unsigned int)((f2 >> shift) & dmask), 1u);
                }
            } else {
                const u64 a = sb >> sshift, b = sprefix >> sshift;
                if (a < b) continue;
                const u64 row = (u64)(i0 + 4 * half + rr), cj = (u64)colj;
                const u64 fl[2] = {row * (u64)n + cj, cj * (u64)n + row};
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    // below the score prefix nothing, above it everything, on it (all 32 bits decided) the flat prefix decides
                    const bool take = a > b || sshift > 0 || ((FLAT_MAX - fl[e]) >> fshift) >= (fprefix >> fshift);
                    if (take) {
                        const unsigned int p = atomicAdd(&st->out_count, 1u);
                        if (p < CAP) {
                            cand_s[p] = (unsigned int)sb;
                            cand_f[p] = fl[e];
                        }
                    }
                }
            }
        }
    }
    if (MODE == HIST) {
        if (pcnt) atomicAdd(&h[pbin], pcnt);
#undef HNS_HIST_ADD
        __syncthreads();
        for (int i = t; i < BINS; i += THREADS)
            if (h[i]) atomicAdd(&st->hist[i], (u64)h[i]);
    }
}

// a before b in the output: higher score, then lower flat index
__device__ __forceinline__ bool key_before(unsigned int sa, u64 fa, unsigned int sb, u64 fb) { return sa > sb || (sa == sb && fa < fb); }

// order the candidates: rank = number of candidates before mine (all distinct); ranks below k_eff are the result.  One wave per
// candidate (waves stride over the candidates): each lane counts every 64th of the others, with several loads in flight.
constexpr int RANK_BLOCKS = 1024;
__global__ __launch_bounds__(THREADS) void hns_rank_kernel(const State* __restrict__ st, const unsigned int* __restrict__ cand_s,
                                                           const u64* __restrict__ cand_f, int k, int64_t n, int64_t* __restrict__ out_edges,
                                                           float* __restrict__ out_scores) {
    const int m = (int)min(st->out_count, CAP);
    const int keff = (int)st->k_eff;
    if (blockIdx.x == 0) {
        for (int r = keff + threadIdx.x; r < k; r += THREADS) {
            out_edges[r] = -1;
            out_edges[k + r] = -1;
            if (out_scores) out_scores[r] = -__builtin_inff();
        }
    }
    const int lane = threadIdx.x % 64;
    for (int i = (int)(blockIdx.x * (THREADS / 64) + threadIdx.x / 64); i < m; i += RANK_BLOCKS * (THREADS / 64)) {
        const unsigned int ms = cand_s[i];
        const u64 mf = cand_f[i];
        int rank = 0;
#pragma unroll 4
        for (int j = lane; j < m; j += 64) rank += key_before(cand_s[j], cand_f[j], ms, mf);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) rank += __shfl_xor(rank, o, 64);
        if (lane == 0 && rank < keff) {
            out_edges[rank] = (int64_t)(mf / (u64)n);
            out_edges[k + rank] = (int64_t)(mf % (u64)n);
            if (out_scores) out_scores[rank] = gmp::from_orderable(ms);
        }
    }
}

template <int MODE>
void launch_tiles(const Plan& p, int64_t n, const Ws& w, bool mask, int is_flat, int shift, int bits, float* scores_out, hipStream_t st) {
    const dim3 grid((unsigned)p.tiles, (unsigned)p.C), block(THREADS);
    const int* rp = mask ? w.rowptr : nullptr;
    dispatch_dp(p.dpad, [&](auto dp) {
        hipLaunchKernelGGL((hns_tile_kernel<dp(), MODE>), grid, block, 0, st, (const float*)w.zn, n, p.dpad, p.tpc, p.nct, rp, (const int*)w.col,
                           (const int*)w.rowptr_t, (const int*)w.col_t, w.st, is_flat, shift, bits, w.cand_s, w.cand_f, scores_out);
    });
}

}  // namespace

extern "C" size_t gmp_hard_negative_stream_workspace_bytes(int64_t n, int64_t d, int64_t E) {
    if (n < 1 || n > MAX_N || d < 1 || d > 256 || E < 0 || E > INT32_MAX) return 0;
    return carve(nullptr, n, d, E).total;
}

extern "C" int gmp_hard_negative_topk_stream(const float* emb, int64_t n, int64_t d, const int64_t* existing_edges, int64_t E, int64_t k,
                                             int64_t* out_edges, float* out_scores, float* scores_out, void* workspace, size_t workspace_bytes,
                                             gmp_stream_t stream) {
    if (n <= 0 || d <= 0 || E < 0 || k < 0)
        return gmp::fail(GMP_ERR_ARG, "hard_negative_topk_stream: bad sizes n=%lld d=%lld E=%lld k=%lld", (long long)n, (long long)d, (long long)E, (long long)k);
    if (n > MAX_N) return gmp::fail(GMP_ERR_ARG, "hard_negative_topk_stream: n=%lld > %lld (flat pair index must fit 40 bits)", (long long)n, (long long)MAX_N);
    if (d > 256) return gmp::fail(GMP_ERR_UNSUPPORTED, "hard_negative_topk_stream: dim=%lld > 256", (long long)d);
    if (E > INT32_MAX) return gmp::fail(GMP_ERR_ARG, "hard_negative_topk_stream: E=%lld out of int32 range", (long long)E);
    if (k > MAX_K) return gmp::fail(GMP_ERR_ARG, "hard_negative_topk_stream: k=%lld > %d", (long long)k, MAX_K);
    if (!emb || (E && !existing_edges) || (k && !out_edges) || !workspace) return gmp::fail(GMP_ERR_ARG, "hard_negative_topk_stream: null pointer");
    const Ws w = carve(workspace, n, d, E);
    if (workspace_bytes < w.total) return gmp::fail(GMP_ERR_WORKSPACE, "hard_negative_topk_stream: workspace %zu < %zu", workspace_bytes, w.total);
    hipStream_t st = (hipStream_t)stream;
    const Plan p = make_plan(n, d);

    hipLaunchKernelGGL(hns_normalize_kernel, dim3(gmp::cdiv(n * 64, THREADS)), dim3(THREADS), 0, st, emb, n, (int)d, p.dpad, w.zn, w.st, (u64)k);
    const bool mask = E > 0;
    if (mask) {
        int rc = gmp_csr_build(existing_edges, n, E, w.rowptr, w.col, w.perm, w.rowptr_t, w.col_t, w.perm_t, w.status, w.csr_ws, w.csr_ws_bytes, stream);
        if (rc != GMP_OK) return rc;
    }
    if (scores_out) launch_tiles<DUMP>(p, n, w, mask, 0, 0, 0, scores_out, st);
    if (k == 0) return gmp::check_launch("hard_negative_topk_stream");

    const int is_flat[7] = {0, 0, 0, 1, 1, 1, 1};
    const int shifts[7] = {21, 10, 0, 29, 18, 7, 0};
    const int nbits[7] = {11, 11, 10, 11, 11, 11, 7};
    for (int pass = 0; pass < 7; ++pass) {
        launch_tiles<HIST>(p, n, w, mask, is_flat[pass], shifts[pass], nbits[pass], nullptr, st);
        hipLaunchKernelGGL(hns_pick_kernel, dim3(1), dim3(THREADS), 0, st, w.st, is_flat[pass], shifts[pass], nbits[pass]);
    }
    launch_tiles<GATHER>(p, n, w, mask, 0, 0, 0, nullptr, st);
    hipLaunchKernelGGL(hns_rank_kernel, dim3(RANK_BLOCKS), dim3(THREADS), 0, st, (const State*)w.st, (const unsigned int*)w.cand_s,
                       (const u64*)w.cand_f, (int)k, n, out_edges, out_scores);
    return gmp::check_launch("hard_negative_topk_stream");
}
