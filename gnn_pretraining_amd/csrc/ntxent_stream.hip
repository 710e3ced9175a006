// Streaming NT-Xent / InfoNCE: the loss and gradient of ntxent.hip without the [2n, 2n] similarity matrix.  The similarity tile
// (sim_tile.h) lives only in MFMA accumulators (and, for the backward's second product, in a 32 x 32 per-wave LDS patch), so memory is O(n d)
// and n is bounded by int32 row indexing of the R = 2n rows, not by 8192.  fp32 end to end, every product on
// v_mfma_f32_32x32x2_f32, every reduction in a fixed order (no float atomics): two calls on the same input are bitwise equal.
//
// With zn the R normalised rows, s_ij = <zn_i, zn_j> / T and pos(i) = i +- n:
//   forward   nts_tile_kernel<DP, false>  block (row tile of 128, column chunk): each of the four waves keeps its 32 query rows in
//                                         registers and walks the chunk's 32-column tiles of zn (staged in LDS): S tile by MFMA,
//                                         diagonal and padding skipped, per-lane running (max, sum of exp) for its 16 rows, the
//                                         positive's similarity stored when its column passes; the lanes' partials are merged by a
//                                         butterfly and written per (chunk, row)
//             nts_finish_kernel           chunks merged in chunk order -> lse[R] (kept for the backward), rowloss = lse - s_pos
//             gmp::sum_rows               the fixed-order sum of ntxent.hip
//   backward  nts_tile_kernel<DP, true>   S is symmetric and pos an involution, so (G + G^T) zn is one pass over recomputed tiles:
//                                           g_zn_i = 1/T sum_{j != i} (exp(s_ij - lse_i) + exp(s_ij - lse_j) - 2 [j = pos(i)]) zn_j
//                                         the weight tile goes through the wave's LDS patch to become the A operand of the second
//                                         product with the zn column tile that is already in LDS; per-chunk partial g_zn
//             nts_normalize_bwd_kernel    partials added in chunk order, then normalize_bwd_kernel's formula (norm <= 1e-12 rule)
// The exponentials: per S element the backward issues two v_exp_f32 next to 4 d MFMA flops (at d = 128, 32 x 8 issue cycles per
// 128 MFMAs of 64 cycles).  A wave cannot hide them under its own dependent MFMAs, so for d <= 128 the kernel is bounded to
// 256 registers and two workgroups share a CU: one wave's exponentials issue while the SIMD's other wave owns the MFMA pipe.
#include "sim_tile.h"

namespace {

using namespace sim;

constexpr int WLD = 36;         // row stride of the weight patch (floats): 144 B, 16-byte slots of 32 rows spread over the banks
constexpr int MAX_CHUNKS = 16;
constexpr int64_t MAX_N = (INT32_MAX - BM) / 2;     // 2n rows plus one tile of padding stay int32

// how the R x R problem is cut: row tiles x column chunks, enough workgroups for two per CU while a chunk keeps >= 2 column tiles
struct Plan {
    int64_t R;
    int tiles, nct, tpc, C;     // row tiles, column tiles, column tiles per chunk, chunks
};

Plan make_plan(int64_t n) {
    Plan p;
    p.R = 2 * n;
    p.tiles = (int)((p.R + BM - 1) / BM);
    p.nct = (int)((p.R + BN - 1) / BN);
    int c = (512 + p.tiles - 1) / p.tiles;
    if (c > MAX_CHUNKS) c = MAX_CHUNKS;
    if (c > (p.nct + 1) / 2) c = (p.nct + 1) / 2;
    if (c < 1) c = 1;
    p.tpc = (p.nct + c - 1) / c;
    p.C = (p.nct + p.tpc - 1) / p.tpc;
    return p;
}

struct Ws {
    float *zn, *norm, *lse, *spos, *rowloss, *pm, *ps, *gpart;
    size_t total;
};

Ws carve(void* ws, const Plan& p, int d) {
    gmp::Carver c(ws, false);
    Ws w;
    const size_t R = (size_t)p.R;
    w.zn = c.take<float>(R * d);
    w.norm = c.take<float>(R);
    w.lse = c.take<float>(R);
    w.spos = c.take<float>(R);
    w.rowloss = c.take<float>(R);
    w.pm = c.take<float>(R * p.C);
    w.ps = c.take<float>(R * p.C);
    w.gpart = c.take<float>(R * d * p.C);               // [C][R][d]
    w.total = c.total() + 256;
    return w;
}

// one wave per row of [z1; z2]
__global__ __launch_bounds__(THREADS) void nts_normalize_kernel(const float* __restrict__ z1, const float* __restrict__ z2, int64_t n, int d,
                                                                float* __restrict__ zn, float* __restrict__ norm) {
    const int64_t row = ((int64_t)blockIdx.x * THREADS + threadIdx.x) / 64;
    if (row >= 2 * n) return;
    gmp::normalize_row(row < n ? z1 + row * d : z2 + (row - n) * d, d, zn + row * d, d, norm + row);
}

// (m, s) <- (m, s) (+) (m2, s2) for sum_j exp(x_j) = s exp(m); an empty side is (-inf, 0)
__device__ __forceinline__ void lse_merge(float& m, float& s, float m2, float s2) {
    const float M = fmaxf(m, m2), Ms = M == -INFINITY ? 0.f : M;      // both empty: exp(-inf - 0) = 0 twice, not exp(nan)
    s = s * __expf(m - Ms) + s2 * __expf(m2 - Ms);
    m = M;
}

template <int DP, bool BWD>
__global__ __launch_bounds__(THREADS, DP <= 128 ? 2 : 1) void nts_tile_kernel(const float* __restrict__ zn, int64_t R, int d, float invT, int tpc,
                                                                              int nct, const float* __restrict__ lse, float* __restrict__ pm,
                                                                              float* __restrict__ ps, float* __restrict__ spos,
                                                                              float* __restrict__ gpart) {
    constexpr int LD = Tile<DP>::LD;
    constexpr int NCB = DP / 32;            // 32-column blocks of g_zn
    __shared__ float4 kt4[BN * LD / 4];
    __shared__ float4 wst4[BWD ? 4 * 32 * WLD / 4 : 1];
    float* kt = reinterpret_cast<float*>(kt4);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    const int64_t n = R / 2;
    const int64_t i0 = (int64_t)blockIdx.x * BM + wave * 32;
    const int chunk = blockIdx.y;
    const int ct0 = chunk * tpc, ct1 = min(ct0 + tpc, nct);

    using Tl = Tile<DP>;
    // the wave's 32 query rows: lane (row l31, k in [half DP/2, (half + 1) DP/2)), zero beyond d and beyond R
    float4 q[Tl::KQ];
    {
        const int64_t qrow = i0 + l31;
#pragma unroll
        for (int u = 0; u < Tl::KQ; ++u) {
            const int k = half * (DP / 2) + 4 * u;
            q[u] = (qrow < R && k < d) ? *reinterpret_cast<const float4*>(zn + qrow * d + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
    }
    const int rlim = rel(R - i0 - 4 * half);    // accumulator row rr exists iff rr < rlim
    float4 pf[Tl::NLD];

    float rm[16], rs[16];                   // forward: running max / sum of exp of this lane's columns, per accumulator row
    float li[16];                           // backward: lse of the accumulator rows
    f32x16 g[BWD ? NCB : 1];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        rm[r] = -INFINITY; rs[r] = 0.f;
        if (BWD) {
            const int64_t row = i0 + acc_row(r, half);
            li[r] = row < R ? lse[row] : 0.f;
        }
    }
    if (BWD) {
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
            for (int r = 0; r < 16; ++r) g[cb][r] = 0.f;
    }

    Tl::fetch(pf, zn, (int64_t)ct0 * BN, R, d, t);
    for (int ct = ct0; ct < ct1; ++ct) {
        __syncthreads();                    // the previous tile's readers are done
        Tl::stash(pf, kt, t);
        __syncthreads();
        if (ct + 1 < ct1) Tl::fetch(pf, zn, (int64_t)(ct + 1) * BN, R, d, t);
        const int64_t col = (int64_t)ct * BN + l31;
        float lj = 0.f;
        if (BWD) lj = col < R ? lse[col] : 0.f;

        const f32x16 acc = Tl::product(q, kt, l31, half);     // rows i0 + acc_row(r, half), column `col`

        // row / column tests relative to the wave's first row (rel, sim_tile.h)
        const int dd = rel(col - i0 - 4 * half), dpos_a = rel(col - n - i0 - 4 * half), dpos_b = rel(col + n - i0 - 4 * half);
        const bool col_ok = col < R;
        if (!BWD) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = acc_row(r, 0);
                const float x = acc[r] * invT;
                const bool ok = col_ok && dd != rr;
                // one exponential per element: of the two factors of the running-max update one is always exp(0)
                const float e = __expf(-fabsf(x - rm[r]));
                const float ns = x > rm[r] ? rs[r] * e + 1.f : rs[r] + e;
                rs[r] = ok ? ns : rs[r];
                rm[r] = ok ? fmaxf(rm[r], x) : rm[r];
            }
            // the positives of the wave's rows lie in the 32 columns from i0 + n or from i0 - n: a wave-uniform test, at most four tiles pass
            const int64_t j0 = (int64_t)ct * BN, da = j0 - (i0 + n), db = j0 - (i0 - n);
            if ((da > -32 && da < 32) || (db > -32 && db < 32)) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int rr = acc_row(r, 0);
                    if (col_ok && rr < rlim && (dpos_a == rr || dpos_b == rr)) spos[i0 + 4 * half + rr] = acc[r] * invT;
                }
            }
        } else {
            float* wp = reinterpret_cast<float*>(wst4) + wave * 32 * WLD;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int rr = acc_row(r, 0);
                const float x = acc[r] * invT;
                float w = __expf(x - li[r]) + __expf(x - lj);
                if (dpos_a == rr || dpos_b == rr) w -= 2.f;
                if (!col_ok || rr >= rlim || dd == rr) w = 0.f;
                wp[(rr + 4 * half) * WLD + l31] = w;
            }
            // the patch is private to the wave, whose LDS operations complete in order: a wave-level fence is all it needs
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            // g_zn rows += W zn_tile: A = W (row l31, column-tile rows 16 half + [0, 16)), B = the tile's row, 32 columns per block
            const float4* a4 = reinterpret_cast<const float4*>(wp + l31 * WLD + half * 16);
            const float* bt = kt + (half * 16) * LD + l31;
            // one float4 of A (four k steps) and its B values per group, fenced so that the scheduler does not hoist the whole tile's
            // reads into registers; the read latency of a group is covered by the SIMD's other wave
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const float4 a = a4[u];
                const float av[4] = {a.x, a.y, a.z, a.w};
                float b[4][NCB];
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) b[e][cb] = bt[(4 * u + e) * LD + cb * 32];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
#pragma unroll
                    for (int cb = 0; cb < NCB; ++cb) g[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[e], b[e][cb], g[cb], 0, 0, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
        }
    }

    if (!BWD) {
        // the 32 lanes of a half hold disjoint column sets of the same 16 rows: butterfly merge (a fixed order), lane 0 of the half writes
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            float m = rm[r], s = rs[r];
#pragma unroll
            for (int o = 1; o < 32; o <<= 1) {
                const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
                lse_merge(m, s, m2, s2);
            }
            const int64_t row = i0 + acc_row(r, half);
            if (l31 == 0 && row < R) {
                pm[(int64_t)chunk * R + row] = m;
                ps[(int64_t)chunk * R + row] = s;
            }
        }
    } else {
        float* out = gpart + (size_t)chunk * (size_t)R * d;
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) {
            const int c = cb * 32 + l31;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int64_t row = i0 + acc_row(r, half);
                if (row < R && c < d) out[row * d + c] = g[cb][r] * invT;
            }
        }
    }
}

// one thread per row: the chunks' (max, sum) in chunk order
__global__ __launch_bounds__(THREADS) void nts_finish_kernel(const float* __restrict__ pm, const float* __restrict__ ps,
                                                             const float* __restrict__ spos, int64_t R, int C, float* __restrict__ lse,
                                                             float* __restrict__ rowloss) {
    const int64_t row = (int64_t)blockIdx.x * THREADS + threadIdx.x;
    if (row >= R) return;
    float m = pm[row], s = ps[row];
    for (int c = 1; c < C; ++c) lse_merge(m, s, pm[(int64_t)c * R + row], ps[(int64_t)c * R + row]);
    const float l = m + logf(s);
    lse[row] = l;
    rowloss[row] = l - spos[row];
}

// one wave per row: g_zn = the chunks' partials in chunk order, then g_z = g_scale * (g_zn - zn <zn, g_zn>) / norm with
// normalize_bwd_kernel's rule for norm <= 1e-12 (d <= 256: four columns per lane)
__global__ __launch_bounds__(THREADS) void nts_normalize_bwd_kernel(const float* __restrict__ zn, const float* __restrict__ norm,
                                                                    const float* __restrict__ gpart, int C, const float* __restrict__ g_scale,
                                                                    int64_t n, int d, float* __restrict__ g1, float* __restrict__ g2) {
    const int lane = threadIdx.x % 64;
    const int64_t R = 2 * n, row = ((int64_t)blockIdx.x * THREADS + threadIdx.x) / 64;
    if (row >= R) return;
    float gv[4];
    float dot = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = lane + 64 * u;
        gv[u] = 0.f;
        if (c < d) {
            float s = gpart[row * d + c];
            for (int k = 1; k < C; ++k) s += gpart[((size_t)k * (size_t)R + row) * d + c];
            gv[u] = s;
            dot += zn[row * d + c] * s;
        }
    }
    dot = gmp::wave_sum(dot);
    const float nr = norm[row], gs = g_scale[0];
    if (nr <= 1e-12f) dot = 0.f;
    float* dst = row < n ? g1 + row * d : g2 + (row - n) * d;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int c = lane + 64 * u;
        if (c < d) dst[c] = gs * (gv[u] - zn[row * d + c] * dot) / nr;
    }
}

int args_ok(const char* who, int64_t n, int d, float T) {
    if (n < 1 || n > MAX_N) return gmp::fail(GMP_ERR_ARG, "%s: n=%lld must be in [1,%lld]", who, (long long)n, (long long)MAX_N);
    if (d < 4 || d > 256 || d % 4) return gmp::fail(GMP_ERR_ARG, "%s: dim %d must be a multiple of 4 in [4,256]", who, d);
    if (!(T > 0.f)) return gmp::fail(GMP_ERR_ARG, "%s: temperature %f", who, T);
    return GMP_OK;
}

template <bool BWD>
void launch_tiles(const Plan& p, int d, float invT, const Ws& w, hipStream_t st) {
    const dim3 grid((unsigned)p.tiles, (unsigned)p.C), block(THREADS);
    dispatch_dp(d, [&](auto dp) {
        hipLaunchKernelGGL((nts_tile_kernel<dp(), BWD>), grid, block, 0, st, (const float*)w.zn, p.R, d, invT, p.tpc, p.nct, (const float*)w.lse,
                           w.pm, w.ps, w.spos, w.gpart);
    });
}

}  // namespace

extern "C" size_t gmp_nt_xent_stream_workspace_bytes(int64_t n, int d) {
    if (n < 1 || n > MAX_N || d < 1) return 0;
    return carve(nullptr, make_plan(n), d).total;
}

extern "C" int gmp_nt_xent_stream_fwd(const float* z1, const float* z2, int64_t n, int d, float T, float* loss_sum, void* ws, size_t ws_bytes,
                                      gmp_stream_t stream) {
    if (int rc = args_ok("nt_xent_stream_fwd", n, d, T)) return rc;
    if (!z1 || !z2 || !loss_sum || !ws) return gmp::fail(GMP_ERR_ARG, "nt_xent_stream_fwd: null pointer");
    const Plan p = make_plan(n);
    const Ws w = carve(ws, p, d);
    if (ws_bytes < w.total) return gmp::fail(GMP_ERR_WORKSPACE, "nt_xent_stream_fwd: workspace");
    hipStream_t st = (hipStream_t)stream;
    const int64_t R = p.R;
    hipLaunchKernelGGL(nts_normalize_kernel, dim3((unsigned)((R * 64 + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, z1, z2, n, d, w.zn, w.norm);
    launch_tiles<false>(p, d, 1.f / T, w, st);
    hipLaunchKernelGGL(nts_finish_kernel, dim3((unsigned)((R + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, (const float*)w.pm,
                       (const float*)w.ps, (const float*)w.spos, R, p.C, w.lse, w.rowloss);
    gmp::sum_rows(w.rowloss, R, loss_sum, st);
    return gmp::check_launch("nt_xent_stream_fwd kernels");
}

extern "C" int gmp_nt_xent_stream_bwd(const float* z1, const float* z2, int64_t n, int d, float T, const float* g_scale, float* g_z1,
                                      float* g_z2, void* ws, size_t ws_bytes, gmp_stream_t stream) {
    (void)z1; (void)z2;
    if (int rc = args_ok("nt_xent_stream_bwd", n, d, T)) return rc;
    if (!g_scale || !g_z1 || !g_z2 || !ws) return gmp::fail(GMP_ERR_ARG, "nt_xent_stream_bwd: null pointer");
    const Plan p = make_plan(n);
    const Ws w = carve(ws, p, d);
    if (ws_bytes < w.total) return gmp::fail(GMP_ERR_WORKSPACE, "nt_xent_stream_bwd: workspace");
    hipStream_t st = (hipStream_t)stream;
    const int64_t R = p.R;
    launch_tiles<true>(p, d, 1.f / T, w, st);
    hipLaunchKernelGGL(nts_normalize_bwd_kernel, dim3((unsigned)((R * 64 + THREADS - 1) / THREADS)), dim3(THREADS), 0, st, (const float*)w.zn,
                       (const float*)w.norm, (const float*)w.gpart, p.C, g_scale, n, d, g_z1, g_z2);
    return gmp::check_launch("nt_xent_stream_bwd kernels");
}
