// Spherical k-means on the GPU (the clustering probe: k-means in cosine similarity on L2-normalised rows, then NMI / ARI / accuracy from an
// integer contingency table).  The whole Lloyd iteration is enqueued on the caller's stream without a host round trip; memory is
// O((n + kc) d + n), never n x kc.
//
//   kmeans_normalize_kernel    one wave per row of x and of the initial centroids: zn = z / max(||z||, 1e-12), row stride padded with zeros
//                              to a multiple of 4 (gmp::normalize_row, the miner's and k-NN's); a fit also gets the caller's copy of the
//                              initial centroids and the control words
//   kmeans_assign_kernel<DP>   block = row tile of 128 rows: each of the four waves keeps its 32 rows in registers and walks the 32-row
//                              tiles of the normalised centroids (staged in LDS), S tile on v_mfma_f32_32x32x2_f32 (Tile<DP>::product).
//                              Per accumulator row ONE running best key -- no lists, no LDS beside the tile -- and after the last tile the
//                              32 lanes of a half-wave (the 32 columns of a row) reduce their keys with five shuffles.  A row writes its
//                              label and similarity, and counts itself in `moved` when its label differs from the one it replaces.
//   kmeans_book_kernel         one thread between assignment and update: iterations, changed = moved (n on the first pass), moved = 0
//   update                     centroid j = normalize(sum of the rows labelled j), the sum in ascending row order.  The rows are grouped
//                              by label with a stable counting sort over chunks of 256 rows: kmeans_count_kernel (a chunk's histogram
//                              in LDS -> counts[chunk][label]), kmeans_offsets_kernel (one wave per label: the exclusive scan over the
//                              chunks), kmeans_scatter_kernel (a row lands at rowptr[label] + the chunk's offset + its rank among the
//                              chunk's earlier rows of that label: wave by wave, ranks from ballots) -- integer work whose result, the
//                              rows of a label in ascending order, does not depend on who runs first.  Then aggregate.hip's
//                              seg_sum_kernel (gmp::seg_sum_gated) sums each centroid's rows, one wave per centroid walking them in
//                              that order.  No floating-point atomics: the bits depend on (n, kc, labels) only.
//                              (csr_build.hip's sort orders a group by rank-by-counting, quadratic in the group's size: right for a
//                              graph's degrees, 140 of 230 us per iteration at 2,708 rows in 7 clusters -- hence a sort of its own here.)
//   kmeans_finish_kernel       one wave per centroid: an empty cluster is counted and keeps its centroid, the others take normalize(sum);
//                              the working copy is the normalised stored centroid, which is also what the next call would start from,
//                              so T iterations in one call are T calls of one iteration bit for bit
//   contingency_kernel         table[a[i], b[i]] += 1 in int64 with integer atomics (small tables are counted in LDS first)
// Key, as in knn.hip: orderable score bits (high word), then ~index (low word); a greater key is a better centroid (higher score, then
// lower index); integer compares only.  The similarity of a (row, centroid) pair is Tile<DP>::product's k-ordered fp32 chain, the one
// knn_scan_kernel computes for the same two rows.
// Early exit: every kernel of an iteration begins with a plain load of the control block's `changed` word and returns when it is 0
// (the pass before moved no row: converged).  Iteration boundaries are kernel boundaries; no kernel waits for another workgroup.
#include <algorithm>

#include "sim_tile.h"

namespace {

using namespace sim;

constexpr int MAX_CLUSTERS = 1024;
constexpr int MAX_DIM = 256;
constexpr int MAX_ITER = 10000;
constexpr int MAX_TABLE = 1024;
constexpr int64_t ROW_LIMIT = (int64_t)1 << 31;
constexpr int CHUNK = 256;                  // rows per workgroup of the sort: one per thread
constexpr int LDS_TABLE = 8192;             // contingency tables up to this many cells are counted per workgroup in LDS

struct Ctrl {
    int changed;            // rows the last finished pass moved; 0 = converged, every later kernel returns at once (starts nonzero)
    unsigned int moved;     // the running pass's count
    int iters, empty;
};

struct Ws {
    float *xn, *cn, *sums;
    int *rowptr, *totals;   // [kc + 1], [kc]
    int* perm;              // [n]: the rows grouped by label, ascending within a label
    int* counts;            // [chunks][kc]: a chunk's rows per label, then their offset within the label
    Ctrl* ctrl;
    size_t total;
};

Ws carve(void* ws, int64_t n, int kc, int dim) {
    gmp::Carver c(ws, true);
    const int dpad = pad4(dim);
    const int64_t chunks = (n + CHUNK - 1) / CHUNK;
    Ws w;
    w.xn = c.take<float>((size_t)n * dpad);
    w.cn = c.take<float>((size_t)kc * dpad);
    w.sums = c.take<float>((size_t)kc * dpad);
    w.rowptr = c.take<int>((size_t)kc + 1);
    w.totals = c.take<int>((size_t)kc);
    w.perm = c.take<int>((size_t)n);
    w.counts = c.take<int>((size_t)chunks * kc);
    w.ctrl = c.take<Ctrl>(1);
    w.total = c.total();
    return w;
}

// rows [0, n) of x into xn, rows [0, kc) of c into cn; a fit (ctrl != NULL) also copies c to c_copy and opens the gate
__global__ __launch_bounds__(THREADS) void kmeans_normalize_kernel(const float* __restrict__ x, int64_t n, const float* c, int kc, int d, int dpad,
                                                                   float* __restrict__ xn, float* __restrict__ cn, float* c_copy,
                                                                   Ctrl* __restrict__ ctrl) {
    const int lane = threadIdx.x % 64;
    const int64_t row = ((int64_t)blockIdx.x * THREADS + threadIdx.x) / 64;
    if (ctrl && blockIdx.x == 0 && threadIdx.x == 0) {
        ctrl->changed = 1;
        ctrl->moved = 0u;
        ctrl->iters = 0;
        ctrl->empty = 0;
    }
    if (row < n) {
        gmp::normalize_row(x + row * d, d, xn + row * dpad, dpad, nullptr);
    } else if (row - n < kc) {
        const int64_t j = row - n;
        gmp::normalize_row(c + j * d, d, cn + j * dpad, dpad, nullptr);
        if (c_copy && c_copy != c)
            for (int k = lane; k < d; k += 64) c_copy[j * d + k] = c[j * d + k];
    }
}

template <int DP>
constexpr int assign_lds_bytes() { return BN * Tile<DP>::LD * 4; }

// Registers: the rows are DP / 2 floats per lane beside 16 accumulators, 16 keys and the tile in flight: the bound of knn_scan_kernel
template <int DP>
__global__ __launch_bounds__(THREADS, DP <= 128 ? 2 : 1) void kmeans_assign_kernel(const float* __restrict__ xn, int64_t n, const float* __restrict__ cn,
                                                                                   int kc, int dpad, int64_t* __restrict__ labels,
                                                                                   float* __restrict__ sim_out, float* __restrict__ matrix_out,
                                                                                   Ctrl* __restrict__ ctrl, int compare) {
    if (ctrl && ctrl->changed == 0) return;
    using Tl = Tile<DP>;
    extern __shared__ float4 smem4[];
    float* kt = reinterpret_cast<float*>(smem4);                    // [BN][LD]
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    const int64_t i0 = (int64_t)blockIdx.x * BM + wave * 32;
    const int64_t crows = kc;
    const int nct = (kc + BN - 1) / BN;

    // the wave's 32 rows: lane (row l31, k in [half DP/2, (half + 1) DP/2)), zero beyond dpad and beyond n
    float4 q[Tl::KQ];
    {
        const int64_t qrow = i0 + l31;
#pragma unroll
        for (int u = 0; u < Tl::KQ; ++u) {
            const int kk = half * (DP / 2) + 4 * u;
            q[u] = (qrow < n && kk < dpad) ? *reinterpret_cast<const float4*>(xn + qrow * dpad + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const int rlim = rel(n - i0 - 4 * half);                        // accumulator row rr exists iff rr < rlim
    float4 pf[Tl::NLD];
    u64 best[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) best[r] = 0ull;

    Tl::fetch(pf, cn, 0, crows, dpad, t);
    for (int ct = 0; ct < nct; ++ct) {
        __syncthreads();                    // the previous tile's readers are done
        Tl::stash(pf, kt, t);
        __syncthreads();
        if (ct + 1 < nct) Tl::fetch(pf, cn, (int64_t)(ct + 1) * BN, crows, dpad, t);
        if (i0 >= n) continue;              // a wave without rows

        const f32x16 acc = Tl::product(q, kt, l31, half);

        // accumulator r is row i0 + 4 half + rr(r), rr = acc_row(r, 0); column colj
        const int colj = ct * BN + l31;
        const bool col_ok = colj < kc;
        const uint32_t inv_col = 0xffffffffu - (uint32_t)colj;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = acc_row(r, 0);
            const bool in = col_ok && rr < rlim;
            if (matrix_out && in) matrix_out[(i0 + 4 * half + rr) * kc + colj] = acc[r];
            const u64 key = in ? gmp::pack_key(acc[r], inv_col) : 0ull;
            best[r] = key > best[r] ? key : best[r];
        }
    }
    if (i0 >= n) return;                    // (no block barrier below)

    // a row's 32 columns sit in the 32 lanes of its half-wave
#pragma unroll
    for (int r = 0; r < 16; ++r) {
#pragma unroll
        for (int o = 16; o > 0; o >>= 1) {
            const u64 other = __shfl_xor(best[r], o, 64);
            best[r] = other > best[r] ? other : best[r];
        }
    }
    // lane l31 < 16 of each half writes accumulator row l31
    u64 mine = best[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) mine = l31 == i ? best[i] : mine;
    const int rr = acc_row(l31 & 15, 0);
    const bool valid = l31 < 16 && rr < rlim;
    const int64_t row = i0 + 4 * half + rr;
    const int64_t lab = (int64_t)gmp::key_low(mine);
    const bool moved = valid && compare && labels[row] != lab;
    const u64 bal = __ballot(moved);
    if (valid) {
        labels[row] = lab;
        sim_out[row] = gmp::key_score(mine);
    }
    if (bal != 0ull && lane == 0) atomicAdd(&ctrl->moved, (unsigned int)__popcll(bal));
}

__global__ void kmeans_book_kernel(Ctrl* __restrict__ ctrl, int it, int n) {
    if (ctrl->changed == 0) return;
    ctrl->iters = it;
    ctrl->changed = it == 1 ? n : (int)ctrl->moved;
    ctrl->moved = 0u;
    if (ctrl->changed) ctrl->empty = 0;     // the update that follows counts them again
}

// counts[chunk][j] = rows of the chunk labelled j
__global__ __launch_bounds__(THREADS) void kmeans_count_kernel(const int64_t* __restrict__ labels, int64_t n, int kc, int* __restrict__ counts,
                                                               const Ctrl* __restrict__ ctrl) {
    __shared__ int hist[MAX_CLUSTERS];
    if (ctrl->changed == 0) return;
    const int t = threadIdx.x;
    for (int j = t; j < kc; j += THREADS) hist[j] = 0;
    __syncthreads();
    const int64_t row = (int64_t)blockIdx.x * CHUNK + t;
    const int64_t lab = row < n ? labels[row] : -1;
    if (lab >= 0 && lab < kc) atomicAdd(&hist[(int)lab], 1);
    __syncthreads();
    for (int j = t; j < kc; j += THREADS) counts[(int64_t)blockIdx.x * kc + j] = hist[j];
}

// one wave per label: counts[.][j] becomes its exclusive scan over the chunks, totals[j] the label's rows
__global__ __launch_bounds__(THREADS) void kmeans_offsets_kernel(int* __restrict__ counts, int64_t chunks, int kc, int* __restrict__ totals,
                                                                 const Ctrl* __restrict__ ctrl) {
    if (ctrl->changed == 0) return;
    const int lane = threadIdx.x % 64;
    const int j = (blockIdx.x * THREADS + threadIdx.x) / 64;
    if (j >= kc) return;                                            // (only wave-level work below)
    int carry = 0;
    for (int64_t b0 = 0; b0 < chunks; b0 += 64) {
        const int64_t b = b0 + lane;
        const int v = b < chunks ? counts[b * kc + j] : 0;
        int s = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(s, o, 64);
            if (lane >= o) s += u;
        }
        if (b < chunks) counts[b * kc + j] = carry + s - v;
        carry += __shfl(s, 63, 64);
    }
    if (lane == 0) totals[j] = carry;
}

// perm[rowptr[label] + the chunk's offset + the rank among the chunk's earlier rows of the label] = row; workgroup 0 also writes rowptr
__global__ __launch_bounds__(THREADS) void kmeans_scatter_kernel(const int64_t* __restrict__ labels, int64_t n, int kc, const int* __restrict__ counts,
                                                                 const int* __restrict__ totals, int* __restrict__ rowptr, int* __restrict__ perm,
                                                                 const Ctrl* __restrict__ ctrl) {
    __shared__ int cur[MAX_CLUSTERS];       // where the label's next row of this chunk goes
    __shared__ int part[THREADS];
    if (ctrl->changed == 0) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    // rowptr = the exclusive scan of totals: four labels per thread (kc <= 4 THREADS)
    static_assert(MAX_CLUSTERS <= 4 * THREADS, "scan shape");
    int v[4], s = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        v[i] = 4 * t + i < kc ? totals[4 * t + i] : 0;
        s += v[i];
    }
    part[t] = s;
    __syncthreads();
    for (int d = 1; d < THREADS; d <<= 1) {
        const int u = t >= d ? part[t - d] : 0;
        __syncthreads();
        part[t] += u;
        __syncthreads();
    }
    int run = t == 0 ? 0 : part[t - 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = 4 * t + i;
        if (j < kc) {
            if (blockIdx.x == 0) rowptr[j] = run;
            cur[j] = run + counts[(int64_t)blockIdx.x * kc + j];
        }
        run += v[i];
    }
    if (blockIdx.x == 0 && t == THREADS - 1) rowptr[kc] = part[THREADS - 1];
    __syncthreads();

    const int64_t row = (int64_t)blockIdx.x * CHUNK + t;
    const int64_t lab64 = row < n ? labels[row] : -1;
    const bool valid = lab64 >= 0 && lab64 < kc;
    const int lab = valid ? (int)lab64 : -1;
    // the lanes of this wave with my label
    u64 todo = __ballot(valid), same = 0ull;
    while (todo) {                                                  // (wave-uniform: todo comes from ballots)
        const int l = __builtin_amdgcn_readlane(lab, __builtin_ctzll(todo));
        const u64 m = __ballot(lab == l);
        if (lab == l) same = m;
        todo &= ~m;
    }
    const int rank = __popcll(same & ((1ull << lane) - 1ull)), group = __popcll(same);
    for (int w = 0; w < THREADS / 64; ++w) {                        // the waves in row order
        if (wave == w && valid) {
            perm[cur[lab] + rank] = (int)row;
            gmp::wave_sync();                                            // every lane of the label has read the cursor
            if (rank == group - 1) cur[lab] += group;
        }
        __syncthreads();
    }
}

// one wave per centroid
__global__ __launch_bounds__(THREADS) void kmeans_finish_kernel(const float* __restrict__ sums, const int* __restrict__ rowptr, int kc, int d, int dpad,
                                                                float* centroids, float* __restrict__ cn, Ctrl* __restrict__ ctrl) {
    if (ctrl->changed == 0) return;
    const int lane = threadIdx.x % 64;
    const int j = (blockIdx.x * THREADS + threadIdx.x) / 64;
    if (j >= kc) return;
    if (rowptr[j + 1] == rowptr[j]) {       // no rows: the centroid stays
        if (lane == 0) atomicAdd(&ctrl->empty, 1);
        return;
    }
    float* const cj = centroids + (int64_t)j * d;
    gmp::normalize_row(sums + (int64_t)j * dpad, d, cj, d, nullptr);
    gmp::normalize_row(cj, d, cn + (int64_t)j * dpad, dpad, nullptr);      // (a lane reads back what it wrote itself)
}

__global__ void kmeans_info_kernel(const Ctrl* __restrict__ ctrl, int64_t* __restrict__ info) {
    info[0] = ctrl->iters;
    info[1] = ctrl->changed;
    info[2] = ctrl->empty;
    info[3] = 0;
}

template <bool LDS>
__global__ __launch_bounds__(THREADS) void contingency_kernel(const int64_t* __restrict__ a, const int64_t* __restrict__ b, int64_t n, int na, int nb,
                                                              u64* __restrict__ table, int32_t* __restrict__ status) {
    __shared__ unsigned int cells[LDS ? LDS_TABLE : 1];
    const int nc = na * nb;
    if (LDS) {
        for (int i = threadIdx.x; i < nc; i += THREADS) cells[i] = 0u;
        __syncthreads();
    }
    int bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * THREADS) {
        const int64_t ai = a[i], bi = b[i];
        if (ai < 0 || ai >= na || bi < 0 || bi >= nb) {
            ++bad;
            continue;
        }
        const int cell = (int)ai * nb + (int)bi;
        if (LDS) atomicAdd(&cells[cell], 1u);
        else atomicAdd(&table[cell], 1ull);
    }
    if (bad) atomicAdd(status, bad);
    if (LDS) {
        __syncthreads();
        for (int i = threadIdx.x; i < nc; i += THREADS)
            if (cells[i]) atomicAdd(&table[i], (u64)cells[i]);
    }
}

template <int DP>
int launch_assign(const Ws& w, int64_t n, int kc, int dpad, int64_t* labels, float* sim_out, float* matrix_out, Ctrl* ctrl, int compare,
                  hipStream_t st) {
    hipLaunchKernelGGL((kmeans_assign_kernel<DP>), dim3((unsigned)((n + BM - 1) / BM)), dim3(THREADS), (size_t)assign_lds_bytes<DP>(), st,
                       (const float*)w.xn, n, (const float*)w.cn, kc, dpad, labels, sim_out, matrix_out, ctrl, compare);
    return gmp::check_launch("kmeans_assign_kernel");
}

int assign(const Ws& w, int64_t n, int kc, int dpad, int64_t* labels, float* sim_out, float* matrix_out, Ctrl* ctrl, int compare, hipStream_t st) {
    return dispatch_dp(dpad, [&](auto dp) { return launch_assign<dp()>(w, n, kc, dpad, labels, sim_out, matrix_out, ctrl, compare, st); });
}

bool sizes_ok(int64_t n, int kc, int dim) { return n >= 0 && n < ROW_LIMIT && kc >= 1 && kc <= MAX_CLUSTERS && dim >= 1 && dim <= MAX_DIM; }

}  // namespace

extern "C" size_t gmp_kmeans_workspace_bytes(int64_t n, int kc, int dim) {
    if (!sizes_ok(n, kc, dim)) return 0;
    return carve(nullptr, n, kc, dim).total;
}

extern "C" int gmp_kmeans_assign(const float* x, int64_t n, const float* centroids, int kc, int dim, int64_t* labels, float* sim_out,
                                 float* matrix_out, void* ws, size_t ws_bytes, gmp_stream_t stream) {
    if (!sizes_ok(n, kc, dim))
        return gmp::fail(GMP_ERR_ARG, "kmeans_assign: n=%lld kc=%d dim=%d (0 <= n < 2^31, 1 <= kc <= %d, 1 <= dim <= %d)", (long long)n, kc, dim,
                         MAX_CLUSTERS, MAX_DIM);
    if (n == 0) return GMP_OK;
    if (!x || !centroids || !labels || !sim_out) return gmp::fail(GMP_ERR_ARG, "kmeans_assign: null pointer");
    const size_t need = gmp_kmeans_workspace_bytes(n, kc, dim);
    if (!ws || ws_bytes < need) return gmp::fail(GMP_ERR_WORKSPACE, "kmeans_assign: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(ws, n, kc, dim);
    const int dpad = pad4(dim);
    hipLaunchKernelGGL(kmeans_normalize_kernel, dim3((unsigned)gmp::cdiv((n + kc) * 64, THREADS)), dim3(THREADS), 0, st, x, n, centroids, kc, dim, dpad,
                       w.xn, w.cn, (float*)nullptr, (Ctrl*)nullptr);
    if (int rc = gmp::check_launch("kmeans_normalize_kernel")) return rc;
    return assign(w, n, kc, dpad, labels, sim_out, matrix_out, nullptr, 0, st);
}

extern "C" int gmp_kmeans_fit(const float* x, int64_t n, const float* init, int kc, int dim, int max_iter, float* centroids, int64_t* labels,
                              float* sim_out, int64_t* info, void* ws, size_t ws_bytes, gmp_stream_t stream) {
    if (!sizes_ok(n, kc, dim) || max_iter < 1 || max_iter > MAX_ITER)
        return gmp::fail(GMP_ERR_ARG, "kmeans_fit: n=%lld kc=%d dim=%d max_iter=%d (0 <= n < 2^31, 1 <= kc <= %d, 1 <= dim <= %d, 1 <= max_iter <= %d)",
                         (long long)n, kc, dim, max_iter, MAX_CLUSTERS, MAX_DIM, MAX_ITER);
    if (n == 0) return GMP_OK;
    if (!x || !init || !centroids || !labels || !sim_out || !info) return gmp::fail(GMP_ERR_ARG, "kmeans_fit: null pointer");
    const size_t need = gmp_kmeans_workspace_bytes(n, kc, dim);
    if (!ws || ws_bytes < need) return gmp::fail(GMP_ERR_WORKSPACE, "kmeans_fit: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(ws, n, kc, dim);
    const int dpad = pad4(dim);
    const int64_t chunks = (n + CHUNK - 1) / CHUNK;
    const int* gate = &w.ctrl->changed;
    hipLaunchKernelGGL(kmeans_normalize_kernel, dim3((unsigned)gmp::cdiv((n + kc) * 64, THREADS)), dim3(THREADS), 0, st, x, n, init, kc, dim, dpad, w.xn,
                       w.cn, centroids, w.ctrl);
    if (int rc = gmp::check_launch("kmeans_normalize_kernel")) return rc;
    for (int it = 1; it <= max_iter; ++it) {
        if (int rc = assign(w, n, kc, dpad, labels, sim_out, nullptr, w.ctrl, it > 1, st)) return rc;
        hipLaunchKernelGGL(kmeans_book_kernel, dim3(1), dim3(1), 0, st, w.ctrl, it, (int)n);
        // the rows grouped by label, ascending within a label, then summed in that order
        hipLaunchKernelGGL(kmeans_count_kernel, dim3((unsigned)chunks), dim3(THREADS), 0, st, (const int64_t*)labels, n, kc, w.counts, (const Ctrl*)w.ctrl);
        hipLaunchKernelGGL(kmeans_offsets_kernel, dim3((unsigned)gmp::cdiv((int64_t)kc * 64, THREADS)), dim3(THREADS), 0, st, w.counts, chunks, kc, w.totals,
                           (const Ctrl*)w.ctrl);
        hipLaunchKernelGGL(kmeans_scatter_kernel, dim3((unsigned)chunks), dim3(THREADS), 0, st, (const int64_t*)labels, n, kc, (const int*)w.counts,
                           (const int*)w.totals, w.rowptr, w.perm, (const Ctrl*)w.ctrl);
        if (int rc = gmp::check_launch("kmeans sort")) return rc;
        if (int rc = gmp::seg_sum_gated(w.xn, w.rowptr, w.perm, w.sums, kc, dpad, gate, st)) return rc;
        hipLaunchKernelGGL(kmeans_finish_kernel, dim3((unsigned)gmp::cdiv((int64_t)kc * 64, THREADS)), dim3(THREADS), 0, st, (const float*)w.sums,
                           (const int*)w.rowptr, kc, dim, dpad, centroids, w.cn, w.ctrl);
        if (int rc = gmp::check_launch("kmeans_finish_kernel")) return rc;
    }
    hipLaunchKernelGGL(kmeans_info_kernel, dim3(1), dim3(1), 0, st, (const Ctrl*)w.ctrl, info);
    return gmp::check_launch("kmeans_info_kernel");
}

extern "C" int gmp_contingency(const int64_t* a, const int64_t* b, int64_t n, int na, int nb, int64_t* table, int32_t* status, gmp_stream_t stream) {
    if (n < 0 || n >= ROW_LIMIT || na < 1 || na > MAX_TABLE || nb < 1 || nb > MAX_TABLE)
        return gmp::fail(GMP_ERR_ARG, "contingency: n=%lld na=%d nb=%d (0 <= n < 2^31, 1 <= na, nb <= %d)", (long long)n, na, nb, MAX_TABLE);
    if (n == 0) return GMP_OK;
    if (!a || !b || !table || !status) return gmp::fail(GMP_ERR_ARG, "contingency: null pointer");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(table, 0, (size_t)na * nb * 8, st) != hipSuccess || hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess)
        return gmp::fail(GMP_ERR_LAUNCH, "contingency: memset");
    if (na * nb <= LDS_TABLE) {
        // a workgroup flushes its whole table: few of them, each with many rows
        const int blocks = (int)std::min<int64_t>(gmp::cdiv(n, THREADS * 16), 256);
        hipLaunchKernelGGL(contingency_kernel<true>, dim3(blocks), dim3(THREADS), 0, st, a, b, n, na, nb, (u64*)table, status);
    } else {
        const int blocks = (int)std::min<int64_t>(gmp::cdiv(n, THREADS), 4096);
        hipLaunchKernelGGL(contingency_kernel<false>, dim3(blocks), dim3(THREADS), 0, st, a, b, n, na, nb, (u64*)table, status);
    }
    return gmp::check_launch("contingency_kernel");
}
