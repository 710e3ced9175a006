// Streaming k-nearest neighbours in cosine similarity (the weighted k-NN probe of Wu et al. 2018): for every query row the k best rows of a
// database, without the nq x ndb similarity matrix.  A similarity tile (sim_tile.h) lives only in MFMA accumulators; memory is
// O((nq + ndb) d + nq k).
//
//   knn_normalize_kernel   one wave per row of q and of db: zn = z / max(||z||, 1e-12), row stride padded with zeros to a multiple of 4
//                          (gmp::normalize_row, the miner's)
//   knn_scan_kernel<DP>    block (row tile of 128 queries, part of the database's 32-row tiles): each of the four waves keeps its 32 query
//                          rows in registers and walks the part's tiles of the normalised database (staged in LDS), S tile on
//                          v_mfma_f32_32x32x2_f32 (Tile<DP>::product).  Every query row owns a sorted list of its best k keys in LDS and
//                          a threshold, the list's k-th key (0 while the list is short): an accumulator element is dropped with one
//                          64-bit compare.  The survivors of a row (at most 32 per tile) are merged into its list by rank-by-counting:
//                          a list entry moves down by the number of survivors before it, a survivor lands at (list entries before it) +
//                          (survivors before it); a survivor's key is read from its lane (v_readlane), the list entries sit one per lane.  A wave only ever touches the lists of its own rows, so the merge needs no block barrier.
//                          The part's lists go to the workspace.
//   knn_merge_kernel       one wave per query: the parts' lists ordered by rank-by-counting, the first k decoded to idx / sim, -1 / -inf
//                          behind them
//   knn_vote_kernel        one wave per query, lane c = class c: sum over the neighbours in order of exp(sim / T) where the label is c
// Key: orderable score bits (high word), then ~index (low word): a greater key is a better neighbour (higher score, then lower index),
// keys of one query are distinct and 0 is free for "empty".  Integer compares only and a total order: the result depends neither on
// how the database is cut into parts nor on the order the blocks run in.  The similarity of a pair is Tile<DP>::product's k-ordered
// fp32 chain whatever the grid is.
#include <algorithm>

#include "sim_tile.h"

namespace {

using namespace sim;

constexpr int MAXK = 64;                    // list length
constexpr int MAX_DIM = 256;
constexpr int MAX_PARTS = 16;               // database parts per row tile
constexpr int MAX_CLASSES = 32;
constexpr int64_t ROW_LIMIT = (int64_t)1 << 31;
constexpr int WAVES = THREADS / 64;

struct Plan {
    int dpad, tiles, nct, tpc, parts;
};

Plan make_plan(int64_t nq, int64_t ndb, int dim) {
    Plan p;
    p.dpad = pad4(dim);
    p.tiles = (int)((nq + BM - 1) / BM);
    p.nct = (int)((ndb + BN - 1) / BN);
    // the database is cut only where the row tiles alone leave most of the 256 CUs idle: about two rounds of blocks, at most 16 parts
    int parts = 1;
    if (p.tiles > 0 && p.tiles < 256) parts = std::max(1, std::min(std::min(MAX_PARTS, p.nct), (512 + p.tiles - 1) / p.tiles));
    p.tpc = std::max(1, (p.nct + parts - 1) / parts);
    p.parts = std::max(1, (p.nct + p.tpc - 1) / p.tpc);
    return p;
}

struct Ws {
    float *qn, *dbn;
    u64* lists;             // [nq][parts][k]
    size_t total;
};

Ws carve(void* ws, int64_t nq, int64_t ndb, int dim, int k) {
    gmp::Carver c(ws, true);
    const Plan p = make_plan(nq, ndb, dim);
    Ws w;
    w.qn = c.take<float>((size_t)nq * p.dpad);
    w.dbn = c.take<float>((size_t)ndb * p.dpad);
    w.lists = c.take<u64>((size_t)nq * p.parts * k);
    w.total = c.total();
    return w;
}

// v of lane `src` (wave-uniform)
__device__ __forceinline__ u64 read_lane(u64 v, int src) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
    return ((u64)hi << 32) | lo;
}

// rows [0, nq) of q into qn, rows [0, ndb) of db into dbn
__global__ __launch_bounds__(THREADS) void knn_normalize_kernel(const float* __restrict__ q, int64_t nq, const float* __restrict__ db, int64_t ndb,
                                                                int d, int dpad, float* __restrict__ qn, float* __restrict__ dbn) {
    const int64_t row = ((int64_t)blockIdx.x * THREADS + threadIdx.x) / 64;
    if (row < nq) gmp::normalize_row(q + row * d, d, qn + row * dpad, dpad, nullptr);
    else if (row - nq < ndb) gmp::normalize_row(db + (row - nq) * d, d, dbn + (row - nq) * dpad, dpad, nullptr);
}

template <int DP>
constexpr int scan_lds_bytes(int k) { return BN * Tile<DP>::LD * 4 + (BM * k + BM) * 8; }

// Registers: the query rows are DP / 2 floats per lane (128 at DP = 256) beside 16 accumulators and the tile in flight, as in
// hns_tile_kernel, hence the same bound: two workgroups per CU up to DP = 128, one above.
template <int DP>
__global__ __launch_bounds__(THREADS, DP <= 128 ? 2 : 1) void knn_scan_kernel(const float* __restrict__ qn, int64_t nq, const float* __restrict__ dbn,
                                                                              int64_t ndb, int dpad, int tpc, int nct, int k, int excl, int parts,
                                                                              u64* __restrict__ lists, float* __restrict__ matrix_out) {
    using Tl = Tile<DP>;
    extern __shared__ float4 smem4[];
    float* kt = reinterpret_cast<float*>(smem4);                    // [BN][LD]
    u64* L = reinterpret_cast<u64*>(kt + BN * Tl::LD);              // [BM][k]: a row's keys, descending, 0 = empty
    u64* thr = L + BM * k;                                          // [BM]: the row's k-th key
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    const int64_t b0 = (int64_t)blockIdx.x * BM;
    const int64_t i0 = b0 + wave * 32;
    const int part = (int)blockIdx.y;
    const int ct0 = part * tpc, ct1 = min(ct0 + tpc, nct);

    for (int i = t; i < BM * k + BM; i += THREADS) L[i] = 0ull;     // (the lists and the thresholds)

    // the wave's 32 rows: lane (row l31, k in [half DP/2, (half + 1) DP/2)), zero beyond dpad and beyond nq
    float4 q[Tl::KQ];
    {
        const int64_t qrow = i0 + l31;
#pragma unroll
        for (int u = 0; u < Tl::KQ; ++u) {
            const int kk = half * (DP / 2) + 4 * u;
            q[u] = (qrow < nq && kk < dpad) ? *reinterpret_cast<const float4*>(qn + qrow * dpad + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const int rlim = rel(nq - i0 - 4 * half);                       // accumulator row rr exists iff rr < rlim
    float4 pf[Tl::NLD];

    if (ct0 < ct1) Tl::fetch(pf, dbn, (int64_t)ct0 * BN, ndb, dpad, t);
    for (int ct = ct0; ct < ct1; ++ct) {
        __syncthreads();                    // the previous tile's readers are done (first trip: the lists are empty)
        Tl::stash(pf, kt, t);
        __syncthreads();
        if (ct + 1 < ct1) Tl::fetch(pf, dbn, (int64_t)(ct + 1) * BN, ndb, dpad, t);
        if (i0 >= nq) continue;             // a wave without rows

        const f32x16 acc = Tl::product(q, kt, l31, half);

        // accumulator r is row i0 + 4 half + rr(r), rr = acc_row(r, 0); column colj
        const int64_t colj = (int64_t)ct * BN + l31;
        const bool col_ok = colj < ndb;
        const int dd = rel(colj - i0 - 4 * half);                   // column minus the lane's first row: the diagonal is dd == rr
        const uint32_t inv_col = 0xffffffffu - (uint32_t)colj;
        unsigned int fl = 0;                                        // bit r: accumulator r beats its row's threshold
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = acc_row(r, 0);
            const bool in = col_ok && rr < rlim;
            if (matrix_out && in) matrix_out[(i0 + 4 * half + rr) * ndb + colj] = acc[r];
            const bool ok = in && !(excl && dd == rr) && gmp::pack_key(acc[r], inv_col) > thr[wave * 32 + 4 * half + rr];
            fl |= (ok ? 1u : 0u) << r;
        }
        if (__ballot(fl != 0u) == 0ull) continue;

#pragma unroll 1
        for (int r = 0; r < 16; ++r) {
            const bool mine = (fl >> r) & 1u;
            const u64 bal = __ballot(mine);
            if (bal == 0ull) continue;
            const u64 ck = gmp::pack_key(pick(acc, r), inv_col);
            const int rr = acc_row(r, 0);
#pragma unroll 1
            for (int h = 0; h < 2; ++h) {                           // the row of the lower half of the wave, then the upper half's
                const unsigned int m = (unsigned int)(bal >> (32 * h));
                if (m == 0u) continue;
                const int row = wave * 32 + 4 * h + rr;
                u64* const Lr = L + row * k;
                const bool cand = mine && half == h;
                const u64 lk = lane < k ? Lr[lane] : 0ull;          // list entry `lane`
                int cnt = 0, ccnt = 0, base = 0;
                for (unsigned int mm = m; mm; mm &= mm - 1u) {      // (wave-uniform: m comes from a ballot)
                    const int b = __builtin_ctz(mm);
                    const u64 x = read_lane(ck, 32 * h + b);        // survivor b's key, straight from its lane
                    cnt += x > lk ? 1 : 0;                          // survivors before my list entry
                    const u64 gt = __ballot(lk > x);                // list entries before survivor b (empty entries are 0: never)
                    ccnt += x > ck ? 1 : 0;                         // survivors before my survivor
                    if (l31 == b) base = __popcll(gt);
                }
                gmp::wave_sync();                                        // every list entry is in a register: the list can be rewritten
                if (lane < k) {
                    const int nr = lane + cnt;
                    if (nr < k) {
                        Lr[nr] = lk;
                        if (nr == k - 1) thr[row] = lk;
                    }
                }
                if (cand) {
                    const int nr = base + ccnt;
                    if (nr < k) {
                        Lr[nr] = ck;
                        if (nr == k - 1) thr[row] = ck;
                    }
                }
            }
        }
    }
    __syncthreads();
    for (int i = t; i < BM * k; i += THREADS) {
        const int r = i / k, p = i - r * k;
        const int64_t row = b0 + r;
        if (row < nq) lists[(row * parts + part) * k + p] = L[i];
    }
}

// n = parts * k keys per query (n == 0: nothing but the tail)
__global__ __launch_bounds__(THREADS) void knn_merge_kernel(const u64* __restrict__ lists, int64_t nq, int n, int k, int64_t* __restrict__ idx,
                                                            float* __restrict__ sim_out) {
    __shared__ u64 ks[WAVES][MAX_PARTS * MAXK];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t q = (int64_t)blockIdx.x * WAVES + wave;
    if (q >= nq) return;                                            // (only wave-level synchronisation below)
    u64* const mk = ks[wave];
    for (int i = lane; i < n; i += 64) mk[i] = lists[q * n + i];
    gmp::wave_sync();
    int real = 0;
    for (int i = lane; i < n; i += 64) {
        const u64 key = mk[i];
        if (key == 0ull) continue;
        real += 1;
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += mk[j] > key ? 1 : 0;
        if (rank < k) {
            idx[q * k + rank] = (int64_t)gmp::key_low(key);
            sim_out[q * k + rank] = gmp::key_score(key);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) real += __shfl_xor(real, o, 64);
    for (int r = min(real, k) + lane; r < k; r += 64) {
        idx[q * k + r] = -1;
        sim_out[q * k + r] = -__builtin_inff();
    }
}

__global__ __launch_bounds__(THREADS) void knn_vote_kernel(const int64_t* __restrict__ idx, const float* __restrict__ sim_in, int64_t nq, int k,
                                                           const int64_t* __restrict__ labels, int64_t ndb, int classes, float temperature,
                                                           float* __restrict__ scores, int64_t* __restrict__ pred, int32_t* __restrict__ status) {
    const int lane = threadIdx.x & 63;
    const int64_t q = ((int64_t)blockIdx.x * THREADS + threadIdx.x) / 64;
    if (q >= nq) return;
    float s = 0.f;
    int used = 0, bad = 0;
    for (int r = 0; r < k; ++r) {                                   // the neighbours in order: a fixed fp32 sum per class
        const int64_t i = idx[q * k + r];
        if (i < 0) continue;
        const int64_t lab = i < ndb ? labels[i] : -1;
        if (lab < 0 || lab >= classes) {
            bad += 1;
            continue;
        }
        used += 1;
        if (lab == lane) s += expf(sim_in[q * k + r] / temperature);
    }
    if (lane < classes) scores[q * classes + lane] = s;
    // argmax, ties to the lower class
    float bs = lane < classes ? s : -__builtin_inff();
    int bc = lane;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float os = __shfl_xor(bs, o, 64);
        const int oc = __shfl_xor(bc, o, 64);
        if (os > bs || (os == bs && oc < bc)) {
            bs = os;
            bc = oc;
        }
    }
    if (lane == 0) {
        pred[q] = used ? (int64_t)bc : (int64_t)-1;
        if (bad) atomicAdd(status, bad);
    }
}

template <int DP>
int launch_scan(const Plan& p, const Ws& w, int64_t nq, int64_t ndb, int k, int excl, float* matrix_out, hipStream_t st) {
    static std::atomic<uint64_t> attr{0};                           // up to 99,840 bytes of LDS (DP = 256, k = 64): opt in once per device
    if (int rc = gmp::reserve_lds(attr, (const void*)knn_scan_kernel<DP>, scan_lds_bytes<DP>(MAXK), "knn_topk")) return rc;
    hipLaunchKernelGGL((knn_scan_kernel<DP>), dim3((unsigned)p.tiles, (unsigned)p.parts), dim3(THREADS), (size_t)scan_lds_bytes<DP>(k), st,
                       (const float*)w.qn, nq, (const float*)w.dbn, ndb, p.dpad, p.tpc, p.nct, k, excl, p.parts, w.lists, matrix_out);
    return gmp::check_launch("knn_scan_kernel");
}

bool sizes_ok(int64_t nq, int64_t ndb, int dim, int k) {
    return nq >= 0 && ndb >= 0 && nq < ROW_LIMIT && ndb < ROW_LIMIT && dim >= 1 && dim <= MAX_DIM && k >= 1 && k <= MAXK;
}

}  // namespace

extern "C" size_t gmp_knn_workspace_bytes(int64_t nq, int64_t ndb, int dim, int k) {
    if (!sizes_ok(nq, ndb, dim, k)) return 0;
    return carve(nullptr, nq, ndb, dim, k).total;
}

extern "C" int gmp_knn_topk(const float* q, int64_t nq, const float* db, int64_t ndb, int dim, int k, int exclude_self, int64_t* idx, float* sim_out,
                            float* matrix_out, void* ws, size_t ws_bytes, gmp_stream_t stream) {
    if (!sizes_ok(nq, ndb, dim, k))
        return gmp::fail(GMP_ERR_ARG, "knn_topk: nq=%lld ndb=%lld dim=%d k=%d (0 <= nq, ndb < 2^31, 1 <= dim <= %d, 1 <= k <= %d)", (long long)nq,
                         (long long)ndb, dim, k, MAX_DIM, MAXK);
    if (exclude_self && (q != db || nq != ndb)) return gmp::fail(GMP_ERR_ARG, "knn_topk: exclude_self needs q == db and nq == ndb");
    if (nq == 0) return GMP_OK;
    if (!q || (ndb && !db) || !idx || !sim_out) return gmp::fail(GMP_ERR_ARG, "knn_topk: null pointer");
    const size_t need = gmp_knn_workspace_bytes(nq, ndb, dim, k);
    if (!ws || ws_bytes < need) return gmp::fail(GMP_ERR_WORKSPACE, "knn_topk: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    Ws w = carve(ws, nq, ndb, dim, k);
    const Plan p = make_plan(nq, ndb, dim);
    if (ndb == 0) {                                                 // no candidates: the tail alone
        hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)gmp::cdiv(nq, WAVES)), dim3(THREADS), 0, st, (const u64*)w.lists, nq, 0, k, idx, sim_out);
        return gmp::check_launch("knn_merge_kernel");
    }
    const bool shared = q == db && nq == ndb;                       // one set against itself: one normalised copy
    if (shared) w.qn = w.dbn;
    const int64_t rows = (shared ? 0 : nq) + ndb;
    hipLaunchKernelGGL(knn_normalize_kernel, dim3((unsigned)gmp::cdiv(rows * 64, THREADS)), dim3(THREADS), 0, st, q, shared ? (int64_t)0 : nq, db, ndb,
                       dim, p.dpad, w.qn, w.dbn);
    if (int rc = gmp::check_launch("knn_normalize_kernel")) return rc;
    const int excl = exclude_self ? 1 : 0;
    if (int rc = dispatch_dp(p.dpad, [&](auto dp) { return launch_scan<dp()>(p, w, nq, ndb, k, excl, matrix_out, st); })) return rc;
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)gmp::cdiv(nq, WAVES)), dim3(THREADS), 0, st, (const u64*)w.lists, nq, p.parts * k, k, idx, sim_out);
    return gmp::check_launch("knn_merge_kernel");
}

extern "C" int gmp_knn_vote(const int64_t* idx, const float* sim_in, int64_t nq, int k, const int64_t* db_labels, int64_t ndb, int classes,
                            float temperature, float* class_scores, int64_t* pred, int32_t* status, gmp_stream_t stream) {
    if (nq < 0 || nq >= ROW_LIMIT || ndb < 0 || ndb >= ROW_LIMIT || k < 1 || k > MAXK)
        return gmp::fail(GMP_ERR_ARG, "knn_vote: nq=%lld ndb=%lld k=%d (0 <= nq, ndb < 2^31, 1 <= k <= %d)", (long long)nq, (long long)ndb, k, MAXK);
    if (classes < 2 || classes > MAX_CLASSES) return gmp::fail(GMP_ERR_ARG, "knn_vote: classes=%d (2 <= classes <= %d)", classes, MAX_CLASSES);
    if (!(temperature > 0.f)) return gmp::fail(GMP_ERR_ARG, "knn_vote: temperature=%g (must be positive)", (double)temperature);
    if (!status) return gmp::fail(GMP_ERR_ARG, "knn_vote: null pointer");
    if (nq && (!idx || !sim_in || (ndb && !db_labels) || !class_scores || !pred)) return gmp::fail(GMP_ERR_ARG, "knn_vote: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return gmp::fail(GMP_ERR_LAUNCH, "knn_vote: memset");
    if (nq == 0) return GMP_OK;
    hipLaunchKernelGGL(knn_vote_kernel, dim3((unsigned)gmp::cdiv(nq * 64, THREADS)), dim3(THREADS), 0, st, idx, sim_in, nq, k, db_labels, ndb, classes,
                       temperature, class_scores, pred, status);
    return gmp::check_launch("knn_vote_kernel");
}
