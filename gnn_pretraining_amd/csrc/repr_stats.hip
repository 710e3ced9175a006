// Label-free statistics of an embedding matrix z [n, d]: the all-pairs sums behind uniformity (Wang & Isola 2020) and the mean cosine, the
// per-pair sum behind alignment, and the fp64 Gram matrix whose spectrum gives RankMe (Garrido et al. 2023).  Outputs are fp64 sums on the
// device, every reduction runs in a fixed order (no floating-point atomics): two calls on the same input are bitwise equal.
//
//   rps_normalize_kernel   one wave per row: zn = z / max(||z||, 1e-12), row stride padded with zeros to a multiple of 4 (gmp::normalize_row)
//   rps_tile_kernel<DP>    block (row tile of 128, column chunk): each of the four waves keeps its 32 rows in registers and walks the
//                          chunk's 32-column tiles of zn (staged in LDS), S tile on v_mfma_f32_32x32x2_f32 (Tile<DP>::product).  Only
//                          pairs i < j count: a row tile's chunks start at its own first column tile, a wave skips the tiles wholly left
//                          of its rows, and inside the tiles that straddle the diagonal j <= i is masked like the padding beyond n.  The
//                          16 values of a lane are summed in fp32 in register order, that sum joins the lane's fp64 running sums; lanes
//                          (butterfly), then waves (in order) fold in fp64 to one pair per (row tile, chunk).
//   rps_finish_kernel      the partials in index order: 256 contiguous runs, then the 256 run sums in order
//   align_kernel           one wave per row pair, the three dot products in fp64; a block's rows in order, per-block fp64 partials
//   gram_kernel<DP>        one wave per (row chunk, task): a task is the pair of 16-column blocks a and DT - 1 - a of the output's upper
//                          tile triangle, DT + 1 tiles of 16 x 16 in all, each a v_mfma_f64_16x16x4_f64 chain over the chunk's rows four at
//                          a time; fp32 inputs widened on load, so every product is exact.  Task 0 sees every column block and also keeps
//                          the column sums.  Partial Grams per chunk go to the workspace.
//   gram_finish_kernel     the chunks in order; element (r, c) with r <= c is written to both places, so the result is bitwise symmetric
#include <algorithm>

#include "sim_tile.h"

namespace {

using namespace sim;

constexpr int MAX_DIM = 256;
constexpr int64_t PAIR_MAX_ROWS = (int64_t)1 << 20;
constexpr int64_t GRAM_MAX_ROWS = (int64_t)1 << 24;
constexpr int MAX_CHUNKS = 32;              // column chunks of the top row tile
constexpr int FIN = 256;                    // threads of the finish kernel
constexpr int ALIGN_MAX_BLOCKS = 1024;
constexpr int GRAM_MAX_CHUNKS = 64;
constexpr int GRAM_MIN_ROWS = 128;          // rows per chunk at least (a multiple of 8: the row loop takes two MFMA steps at a time)

typedef double f64x4 __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------- pair statistics

// How the upper triangle is cut.  Row tile T meets the column tiles 4 T .. nct - 1, so the top row tiles see the most columns: every row
// tile is cut into chunks of the SAME length tpc, and a (row tile, chunk) slot whose chunk starts beyond the last column tile has no
// work (its workgroup writes zeros and leaves).  About half the slots of the tiles x C grid hold work, hence 1024 where the streaming
// NT-Xent asks for 512: two workgroups per CU while a chunk keeps >= 2 tiles.
struct PairPlan {
    int dpad, tiles, nct, tpc, C;
};

PairPlan pair_plan(int64_t n, int d) {
    PairPlan p;
    p.dpad = pad4(d);
    p.tiles = (int)((n + BM - 1) / BM);
    p.nct = (int)((n + BN - 1) / BN);
    int c = (1024 + p.tiles - 1) / p.tiles;
    c = std::min(c, MAX_CHUNKS);
    c = std::min(c, (p.nct + 1) / 2);
    c = std::max(c, 1);
    p.tpc = (p.nct + c - 1) / c;
    p.C = (p.nct + p.tpc - 1) / p.tpc;
    return p;
}

struct GramPlan {
    int chunks;
    int64_t rpc;        // rows per chunk
};

GramPlan gram_plan(int64_t n) {
    GramPlan g;
    int64_t c = std::max<int64_t>(1, std::min<int64_t>(GRAM_MAX_CHUNKS, n / GRAM_MIN_ROWS));
    g.rpc = ((n + c - 1) / c + 7) / 8 * 8;
    g.chunks = (int)((n + g.rpc - 1) / g.rpc);
    return g;
}

int align_blocks(int64_t n) { return (int)std::min<int64_t>(ALIGN_MAX_BLOCKS, (n + 3) / 4); }

// the padded dimension of the Gram partials: the Tile width that dispatch_dp picks for d
int gram_dp(int d) { return dispatch_dp(d, [](auto dp) { return (int)dp(); }); }

// One layout serves the three entry points (they never run inside each other): the normalised copy and the pair partials exist only
// where the pair statistics do (2 <= n <= 2^20).
struct Ws {
    float* zn;          // [n][dpad]
    double* ppart;      // [tiles][C][2]
    double* apart;      // [align_blocks]
    double* gpart;      // [chunks][DP][DP]
    double* cpart;      // [chunks][DP]
    size_t total;
};

Ws carve(void* ws, int64_t n, int d) {
    gmp::Carver c(ws, true);
    Ws w;
    const bool pairs = n >= 2 && n <= PAIR_MAX_ROWS;
    const PairPlan p = pair_plan(std::max<int64_t>(n, 2), d);
    const GramPlan g = gram_plan(n);
    const int DP = gram_dp(d);
    w.zn = c.take<float>(pairs ? (size_t)n * p.dpad : 0);
    w.ppart = c.take<double>(pairs ? (size_t)p.tiles * p.C * 2 : 0);
    w.apart = c.take<double>((size_t)align_blocks(n));
    w.gpart = c.take<double>((size_t)g.chunks * DP * DP);
    w.cpart = c.take<double>((size_t)g.chunks * DP);
    w.total = c.total();
    return w;
}

bool dim_ok(int d) { return d >= 1 && d <= MAX_DIM; }

// what an entry point needs of the layout (gmp_repr_alignment and gmp_repr_gram take n beyond 2^20, where it holds no normalised copy)
size_t need_bytes(int64_t n, int d) { return carve(nullptr, n, d).total; }

__global__ __launch_bounds__(THREADS) void rps_normalize_kernel(const float* __restrict__ z, int64_t n, int d, int dpad, float* __restrict__ zn) {
    const int64_t row = ((int64_t)blockIdx.x * THREADS + threadIdx.x) / 64;
    if (row < n) gmp::normalize_row(z + row * d, d, zn + row * dpad, dpad, nullptr);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// Registers: as knn_scan_kernel, the rows are DP / 2 floats per lane beside 16 accumulators and the tile in flight: two workgroups per
// CU up to DP = 128, one above.
template <int DP>
__global__ __launch_bounds__(THREADS, DP <= 128 ? 2 : 1) void rps_tile_kernel(const float* __restrict__ zn, int64_t n, int dpad, int tpc, int nct,
                                                                              int C, float c2, double* __restrict__ part) {
    using Tl = Tile<DP>;
    __shared__ float4 kt4[BN * Tl::LD / 4];
    __shared__ double wsum[THREADS / 64][2];
    float* kt = reinterpret_cast<float*>(kt4);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    const int tile = (int)blockIdx.x, chunk = (int)blockIdx.y;
    double* const out = part + ((size_t)tile * C + chunk) * 2;
    const int ct0 = 4 * tile + chunk * tpc, ct1 = min(ct0 + tpc, nct);      // (BM / BN = 4 column tiles per row tile)
    if (ct0 >= ct1) {                       // a slot without work (block-uniform: nobody waits at a barrier)
        if (t == 0) { out[0] = 0.0; out[1] = 0.0; }
        return;
    }
    const int64_t i0 = (int64_t)tile * BM + wave * 32;

    // the wave's 32 rows: lane (row l31, k in [half DP/2, (half + 1) DP/2)), zero beyond dpad and beyond n
    float4 q[Tl::KQ];
    {
        const int64_t qrow = i0 + l31;
#pragma unroll
        for (int u = 0; u < Tl::KQ; ++u) {
            const int kk = half * (DP / 2) + 4 * u;
            q[u] = (qrow < n && kk < dpad) ? *reinterpret_cast<const float4*>(zn + qrow * dpad + kk) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const int rlim = rel(n - i0 - 4 * half);                        // accumulator row rr exists iff rr < rlim
    float4 pf[Tl::NLD];
    double se = 0.0, sc = 0.0;

    Tl::fetch(pf, zn, (int64_t)ct0 * BN, n, dpad, t);
    for (int ct = ct0; ct < ct1; ++ct) {
        __syncthreads();                    // the previous tile's readers are done
        Tl::stash(pf, kt, t);
        __syncthreads();
        if (ct + 1 < ct1) Tl::fetch(pf, zn, (int64_t)(ct + 1) * BN, n, dpad, t);
        // a wave without rows, or a tile whose last column is not right of the wave's first row: no pair i < j in it
        if (i0 >= n || (int64_t)(ct + 1) * BN - 1 <= i0) continue;

        const f32x16 acc = Tl::product(q, kt, l31, half);

        // accumulator r is row i0 + 4 half + rr(r), rr = acc_row(r, 0); column colj
        const int64_t colj = (int64_t)ct * BN + l31;
        const bool col_ok = colj < n;
        const int dd = rel(colj - i0 - 4 * half);                   // column minus the lane's first row: j > i is dd > rr
        float te = 0.f, tc = 0.f;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int rr = acc_row(r, 0);
            const bool ok = col_ok && rr < rlim && dd > rr;
            const float s = acc[r];
            const float e = expf(c2 * (s - 1.f));
            te += ok ? e : 0.f;
            tc += ok ? s : 0.f;
        }
        se += (double)te;
        sc += (double)tc;
    }
    se = wave_sum_f64(se);
    sc = wave_sum_f64(sc);
    if (lane == 0) { wsum[wave][0] = se; wsum[wave][1] = sc; }
    __syncthreads();
    if (t == 0) {
        double a = wsum[0][0], b = wsum[0][1];
        for (int w = 1; w < THREADS / 64; ++w) { a += wsum[w][0]; b += wsum[w][1]; }
        out[0] = a;
        out[1] = b;
    }
}

// out[k] = sum over i in [0, count) of part[i * width + k], k < width (<= 2), in index order: thread u adds the run [u len, (u + 1) len),
// thread 0 the run sums
__global__ __launch_bounds__(FIN) void rps_finish_kernel(const double* __restrict__ part, int64_t count, int width, double* __restrict__ out) {
    __shared__ double runs[FIN][2];
    const int u = threadIdx.x;
    const int64_t len = (count + FIN - 1) / FIN, b = min(count, u * len), e = min(count, b + len);
    double s[2] = {0.0, 0.0};
    for (int64_t i = b; i < e; ++i)
        for (int k = 0; k < width; ++k) s[k] += part[i * width + k];
    runs[u][0] = s[0];
    runs[u][1] = s[1];
    __syncthreads();
    if (u == 0) {
        double a = runs[0][0], c = runs[0][1];
        for (int v = 1; v < FIN; ++v) { a += runs[v][0]; c += runs[v][1]; }
        out[0] = a;
        if (width > 1) out[1] = c;
    }
}

// ---------------------------------------------------------------- alignment

// block b owns rows [b rpb, (b + 1) rpb); wave w takes rows w, w + 4, ... of them in order
__global__ __launch_bounds__(THREADS) void align_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int64_t n, int d, int64_t rpb,
                                                        double half_alpha, double* __restrict__ part) {
    __shared__ double wsum[THREADS / 64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * rpb, r1 = min(n, r0 + rpb);
    double acc = 0.0;
    for (int64_t row = r0 + wave; row < r1; row += THREADS / 64) {
        const float *a = z1 + row * d, *b = z2 + row * d;
        double ab = 0.0, aa = 0.0, bb = 0.0;
        for (int c = lane; c < d; c += 64) {
            const double x = (double)a[c], y = (double)b[c];
            ab += x * y;
            aa += x * x;
            bb += y * y;
        }
        ab = wave_sum_f64(ab);
        aa = wave_sum_f64(aa);
        bb = wave_sum_f64(bb);
        const double s = ab / (fmax(sqrt(aa), 1e-12) * fmax(sqrt(bb), 1e-12));
        const double v = fmax(0.0, 2.0 - 2.0 * s);
        acc += half_alpha == 1.0 ? v : pow(v, half_alpha);
    }
    if (lane == 0) wsum[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = wsum[0];
        for (int w = 1; w < THREADS / 64; ++w) s += wsum[w];
        part[blockIdx.x] = s;
    }
}

// ---------------------------------------------------------------- Gram

// v_mfma_f64_16x16x4_f64: A[row l & 15][k = l >> 4], B[k = l >> 4][col l & 15], one double per lane each; C/D register g of lane l is
// (row (l >> 4) + 4 g, col l & 15) -- not the f32 16x16x4 map.  With k a row of z and A = B^T = a 16-column block of it, both operands are
// z[i0 + (l >> 4)][16 blk + (l & 15)].
//
// Task a of DT / 2 owns the tile rows a and a2 = DT - 1 - a of the upper tile triangle, DT + 1 tiles: slot j > a is tile (a, j - 1), slot
// j <= a is tile (a2, a2 + j).  Which slot is which is wave-uniform and only moves load addresses: the accumulators are indexed statically.
template <int DP>
__global__ __launch_bounds__(64) void gram_kernel(const float* __restrict__ z, int64_t n, int d, int64_t rpc, double* __restrict__ gpart,
                                                  double* __restrict__ cpart) {
    constexpr int DT = DP / 16, NS = DT + 1;
    const int lane = threadIdx.x, l15 = lane & 15, kq = lane >> 4;
    const int chunk = (int)blockIdx.x, a = (int)blockIdx.y, a2 = DT - 1 - a;
    const int64_t r0 = (int64_t)chunk * rpc, r1 = min(n, r0 + rpc);

    int col[NS];                            // the lane's column of slot j's B operand, -1 beyond d
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int c = 16 * (j > a ? j - 1 : a2 + j) + l15;
        col[j] = c < d ? c : -1;
    }
    const int ca = 16 * a + l15 < d ? 16 * a + l15 : -1, ca2 = 16 * a2 + l15 < d ? 16 * a2 + l15 : -1;

    f64x4 acc[NS];
    double cs[DT];
#pragma unroll
    for (int j = 0; j < NS; ++j) acc[j] = f64x4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < DT; ++j) cs[j] = 0.0;

    for (int64_t i = r0; i < r1; i += 8) {
        // two steps of four rows: every load of both before the first MFMA
        float bv[2][NS], av[2][2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t row = i + 4 * h + kq;
            const bool in = row < r1;
            const float* zr = z + row * d;
#pragma unroll
            for (int j = 0; j < NS; ++j) bv[h][j] = (in && col[j] >= 0) ? zr[col[j]] : 0.f;
            av[h][0] = (in && ca >= 0) ? zr[ca] : 0.f;
            av[h][1] = (in && ca2 >= 0) ? zr[ca2] : 0.f;
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
#pragma unroll
            for (int j = 0; j < NS; ++j)
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64((double)(j > a ? av[h][0] : av[h][1]), (double)bv[h][j], acc[j], 0, 0, 0);
            if (a == 0) {                   // slots 1 .. DT are the column blocks 0 .. DT - 1
#pragma unroll
                for (int j = 0; j < DT; ++j) cs[j] += (double)bv[h][j + 1];
            }
        }
    }

    double* const gp = gpart + (size_t)chunk * DP * DP;
#pragma unroll
    for (int j = 0; j < NS; ++j) {
        const int ta = j > a ? a : a2, tb = j > a ? j - 1 : a2 + j;
#pragma unroll
        for (int g = 0; g < 4; ++g) gp[(size_t)(16 * ta + kq + 4 * g) * DP + 16 * tb + l15] = acc[j][g];
    }
    if (a == 0) {
#pragma unroll
        for (int j = 0; j < DT; ++j) {
            double s = cs[j];               // the four row residues in order
            const double s1 = __shfl(s, l15 + 16, 64), s2 = __shfl(s, l15 + 32, 64), s3 = __shfl(s, l15 + 48, 64);
            s = ((s + s1) + s2) + s3;
            if (kq == 0) cpart[(size_t)chunk * DP + 16 * j + l15] = s;
        }
    }
}

// one thread per (r, c), r <= c: the chunks in order, written to (r, c) and (c, r); the threads of row 0 also finish the column sums
__global__ __launch_bounds__(THREADS) void gram_finish_kernel(const double* __restrict__ gpart, const double* __restrict__ cpart, int chunks, int d,
                                                              int DP, double* __restrict__ gram, double* __restrict__ colsum) {
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    if (idx >= d * d) return;
    const int r = idx / d, c = idx - r * d;
    if (r > c) return;
    double s = 0.0;
    for (int k = 0; k < chunks; ++k) s += gpart[((size_t)k * DP + r) * DP + c];
    gram[(size_t)r * d + c] = s;
    gram[(size_t)c * d + r] = s;
    if (r == 0) {
        double t = 0.0;
        for (int k = 0; k < chunks; ++k) t += cpart[(size_t)k * DP + c];
        colsum[c] = t;
    }
}

}  // namespace

extern "C" size_t gmp_repr_workspace_bytes(int64_t n, int d) {
    if (n < 1 || n > PAIR_MAX_ROWS || !dim_ok(d)) return 0;
    return need_bytes(n, d);
}

extern "C" int gmp_repr_pair_stats(const float* z, int64_t n, int d, float t, double* out, void* ws, size_t ws_bytes, gmp_stream_t stream) {
    if (n < 2 || n > PAIR_MAX_ROWS || !dim_ok(d) || !(t >= 0.f))
        return gmp::fail(GMP_ERR_ARG, "repr_pair_stats: n=%lld d=%d t=%g (2 <= n <= 2^20, 1 <= d <= %d, t >= 0)", (long long)n, d, (double)t, MAX_DIM);
    if (!z || !out) return gmp::fail(GMP_ERR_ARG, "repr_pair_stats: null pointer");
    const size_t need = need_bytes(n, d);
    if (!ws || ws_bytes < need) return gmp::fail(GMP_ERR_WORKSPACE, "repr_pair_stats: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(ws, n, d);
    const PairPlan p = pair_plan(n, d);
    hipLaunchKernelGGL(rps_normalize_kernel, dim3((unsigned)gmp::cdiv(n * 64, THREADS)), dim3(THREADS), 0, st, z, n, d, p.dpad, w.zn);
    if (int rc = gmp::check_launch("rps_normalize_kernel")) return rc;
    const float c2 = 2.f * t;
    dispatch_dp(p.dpad, [&](auto dp) {
        hipLaunchKernelGGL((rps_tile_kernel<dp()>), dim3((unsigned)p.tiles, (unsigned)p.C), dim3(THREADS), 0, st, (const float*)w.zn, n, p.dpad, p.tpc,
                           p.nct, p.C, c2, w.ppart);
    });
    if (int rc = gmp::check_launch("rps_tile_kernel")) return rc;
    hipLaunchKernelGGL(rps_finish_kernel, dim3(1), dim3(FIN), 0, st, (const double*)w.ppart, (int64_t)p.tiles * p.C, 2, out);
    return gmp::check_launch("rps_finish_kernel");
}

extern "C" int gmp_repr_alignment(const float* z1, const float* z2, int64_t n, int d, float alpha, double* out, void* ws, size_t ws_bytes,
                                  gmp_stream_t stream) {
    if (n < 1 || n > GRAM_MAX_ROWS || !dim_ok(d) || !(alpha > 0.f))
        return gmp::fail(GMP_ERR_ARG, "repr_alignment: n=%lld d=%d alpha=%g (1 <= n <= 2^24, 1 <= d <= %d, alpha > 0)", (long long)n, d,
                         (double)alpha, MAX_DIM);
    if (!z1 || !z2 || !out) return gmp::fail(GMP_ERR_ARG, "repr_alignment: null pointer");
    const size_t need = need_bytes(n, d);
    if (!ws || ws_bytes < need) return gmp::fail(GMP_ERR_WORKSPACE, "repr_alignment: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(ws, n, d);
    const int blocks = align_blocks(n);
    const int64_t rpb = (n + blocks - 1) / blocks;
    hipLaunchKernelGGL(align_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, z1, z2, n, d, rpb, (double)alpha * 0.5, w.apart);
    if (int rc = gmp::check_launch("align_kernel")) return rc;
    hipLaunchKernelGGL(rps_finish_kernel, dim3(1), dim3(FIN), 0, st, (const double*)w.apart, (int64_t)blocks, 1, out);
    return gmp::check_launch("rps_finish_kernel");
}

extern "C" int gmp_repr_gram(const float* z, int64_t n, int d, double* gram, double* colsum, void* ws, size_t ws_bytes, gmp_stream_t stream) {
    if (n < 1 || n > GRAM_MAX_ROWS || !dim_ok(d))
        return gmp::fail(GMP_ERR_ARG, "repr_gram: n=%lld d=%d (1 <= n <= 2^24, 1 <= d <= %d)", (long long)n, d, MAX_DIM);
    if (!z || !gram || !colsum) return gmp::fail(GMP_ERR_ARG, "repr_gram: null pointer");
    const size_t need = need_bytes(n, d);
    if (!ws || ws_bytes < need) return gmp::fail(GMP_ERR_WORKSPACE, "repr_gram: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(ws, n, d);
    const GramPlan g = gram_plan(n);
    const int DP = gram_dp(d);
    dispatch_dp(d, [&](auto dp) {
        hipLaunchKernelGGL((gram_kernel<dp()>), dim3((unsigned)g.chunks, (unsigned)(dp() / 32)), dim3(64), 0, st, z, n, d, g.rpc, w.gpart, w.cpart);
    });
    if (int rc = gmp::check_launch("gram_kernel")) return rc;
    hipLaunchKernelGGL(gram_finish_kernel, dim3((unsigned)gmp::cdiv((int64_t)d * d, THREADS)), dim3(THREADS), 0, st, (const double*)w.gpart,
                       (const double*)w.cpart, g.chunks, d, DP, gram, colsum);
    return gmp::check_launch("gram_finish_kernel");
}
