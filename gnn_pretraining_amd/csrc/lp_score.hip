// The link-prediction scorer of fine-tuning (src/models/heads.py:57-67, MLPLinkPredictor) fused over an arbitrary pair list:
//   feat[m] = [hs+hd | hs*hd | |hs-hd|]  (hs = h[src[m]], hd = h[dst[m]], F = 256 -> 768 wide)
//   z = feat W0^T + b0 (768 -> 256), act = relu(z), dropped = dropout(act), logit = <dropped, w3> + b3
// The module path writes the [K, 768] feature matrix, runs it through the GEMM path and needs ~12 launches for the MLP; here the
// features live only in LDS / registers.  Every product runs on v_mfma_f32_32x32x2_f32 (exact fp32, like the rest of the library),
// and every reduction over pairs is a fixed-order sum (slices in LDS, partials in a workspace reduced in order): no float atomics.
//
// Forward (two launches; the tile code is lp_tile.h's, which lp_rank.hip's ranking shares):
//   lp_score_fwd_kernel   one block per (32 pairs, 32 hidden units): the block builds the 32 x 768 feature tile in LDS, its eight
//                         waves each take a 96-deep k-slice (48 MFMAs), the slices are added in order through LDS, then the epilogue
//                         (bias, ReLU, the Philox mask of gmp_dropout_fwd over the [K, 256] activation) writes act = relu(z) (the kept
//                         pre-dropout activation) and the pair's partial dot with w3 over these 32 units
//   lp_logit_kernel       logit[m] = b3 + the eight partial dots in order
// Backward (four launches) from g_logit = d loss / d logit:
//   lp_gz_kernel          g_z = g_logit * w3 * mask * (act > 0) into the workspace, per 32-pair tile the column sums of g_z (db0)
//                         and of g_logit * dropped (dw3)
//   lp_dw0_kernel         dW0 = g_z^T feat: one wave per (32 x 32 output tile, 128-pair slice), the features rebuilt from h per lane
//   lp_gfeat_kernel       g_feat = g_z W0 for the three 256-wide segments of 32 columns at once (4 waves split the 256-deep
//                         reduction, added in order), turned straight into the per-pair g_hs / g_hd of gmp_lp_edge_features_bwd
//   lp_wgrad_final_kernel the slice partials of dW0, db0, dw3, db3 added in order into the gradient buffer
// An index outside [0, N) reads as a zero row (gmp_row_gather); rows of a tile beyond K are computed as zeros and never stored.
#include "lp_tile.h"

namespace {

using namespace lpt;                // F, HID, KF, BM, LDA, THREADS, zero4, row4, aligned16 and the forward's tile code

constexpr int FWD_LDS = BM * LDA * 4;
constexpr int MS = 128;             // pairs per slice of the dW0 reduction
constexpr int64_t W0N = (int64_t)HID * KF;

__device__ __forceinline__ float row1(const float* __restrict__ h, int64_t i, int64_t N, int c) {
    return (i >= 0 && i < N) ? h[i * F + c] : 0.f;
}

__device__ __forceinline__ float sgn(float v) { return (float)((v > 0.f) - (v < 0.f)); }   // torch.abs' subgradient: 0 at 0

__device__ __forceinline__ float4 mask4(int64_t m, int col, float p, uint64_t seed, uint32_t site) {
    // the mask gmp_dropout_fwd draws for element (m, col) of a contiguous [K, 256] activation
    if (p <= 0.f) return make_float4(1.f, 1.f, 1.f, 1.f);
    return gmp::dropout_scale4(seed, site, (uint64_t)(m * (HID / 4) + (col >> 2)), p, 1.f / (1.f - p));
}

__global__ __launch_bounds__(THREADS) void lp_score_fwd_kernel(const float* __restrict__ h, const int64_t* __restrict__ src,
                                                               const int64_t* __restrict__ dst, int64_t N, int64_t K,
                                                               const float* __restrict__ w0, const float* __restrict__ b0,
                                                               const float* __restrict__ w3, float* __restrict__ act,
                                                               float* __restrict__ part, float p, uint64_t seed, uint32_t site) {
    extern __shared__ float4 smem4[];
    float* tile = reinterpret_cast<float*>(smem4);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int n0 = blockIdx.y * 32;

    const auto node = [&](const int64_t* idx, int r) { return m0 + r < K ? idx[m0 + r] : (int64_t)-1; };   // beyond K: a zero row
    build(tile, reinterpret_cast<const float4*>(h), N, [&](int r) { return node(src, r); }, [&](int r) { return node(dst, r); });
    __syncthreads();
    const f32x16 acc = slice(tile, w0, n0, wave, l31, half);
    __syncthreads();                                            // every wave is done with the feature tile: it becomes red[8][32][32]
    spill(tile, acc, wave, l31, half);
    __syncthreads();
    if (t >= 256) return;                                       // (waves 4-7: wave-uniform)
    const int row = t >> 3, c4 = t & 7, col = n0 + 4 * c4;
    const float4 a = hidden4(tile, b0, n0);
    const int64_t m = m0 + row;
    const float4 mk = mask4(m, col, p, seed, site);
    const float dot = partial_dot(make_float4(a.x * mk.x, a.y * mk.y, a.z * mk.z, a.w * mk.w), w3, n0);
    if (m < K) {
        *reinterpret_cast<float4*>(act + m * HID + col) = a;
        if (c4 == 0) part[(int64_t)blockIdx.y * K + m] = dot;
    }
}

__global__ __launch_bounds__(256) void lp_logit_kernel(const float* __restrict__ part, const float* __restrict__ b3, float* __restrict__ logit, int64_t K) {
    const int64_t m = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= K) return;
    float s = part[m];
#pragma unroll
    for (int j = 1; j < HID / 32; ++j) s += part[j * K + m];
    logit[m] = s + b3[0];
}

// g_z for 32 pairs (zeros for the rows beyond K) + this tile's column sums of g_z and g_logit * dropped, and the sum of g_logit
__global__ __launch_bounds__(256) void lp_gz_kernel(const float* __restrict__ act, const float* __restrict__ g_logit, const float* __restrict__ w3,
                                                    float* __restrict__ gz, float* __restrict__ db0p, float* __restrict__ dw3p, float* __restrict__ db3p,
                                                    int64_t K, float p, uint64_t seed, uint32_t site) {
    __shared__ float4 sb[4][64], sw[4][64];
    const int t = threadIdx.x, c4 = t & 63, rs = t >> 6, col = 4 * c4;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const float4 ww = *reinterpret_cast<const float4*>(w3 + col);
    float4 cb = zero4(), cw = zero4();
    for (int i = 0; i < BM / 4; ++i) {
        const int64_t m = m0 + rs + 4 * i;
        float4 o = zero4();
        if (m < K) {
            const float4 a = *reinterpret_cast<const float4*>(act + m * HID + col), mk = mask4(m, col, p, seed, site);
            const float g = g_logit[m];
            o = make_float4(a.x > 0.f ? g * ww.x * mk.x : 0.f, a.y > 0.f ? g * ww.y * mk.y : 0.f,
                            a.z > 0.f ? g * ww.z * mk.z : 0.f, a.w > 0.f ? g * ww.w * mk.w : 0.f);
            cb.x += o.x; cb.y += o.y; cb.z += o.z; cb.w += o.w;
            cw.x += g * (a.x * mk.x); cw.y += g * (a.y * mk.y); cw.z += g * (a.z * mk.z); cw.w += g * (a.w * mk.w);
        }
        *reinterpret_cast<float4*>(gz + m * HID + col) = o;
    }
    sb[rs][c4] = cb;
    sw[rs][c4] = cw;
    __syncthreads();
    if (rs == 0) {
        float4 b = sb[0][c4], w = sw[0][c4];
#pragma unroll
        for (int j = 1; j < 4; ++j) {
            b.x += sb[j][c4].x; b.y += sb[j][c4].y; b.z += sb[j][c4].z; b.w += sb[j][c4].w;
            w.x += sw[j][c4].x; w.y += sw[j][c4].y; w.z += sw[j][c4].z; w.w += sw[j][c4].w;
        }
        *reinterpret_cast<float4*>(db0p + (int64_t)blockIdx.x * HID + col) = b;
        *reinterpret_cast<float4*>(dw3p + (int64_t)blockIdx.x * HID + col) = w;
    }
    if (t == 0) {
        float s = 0.f;
        for (int r = 0; r < BM; ++r)
            if (m0 + r < K) s += g_logit[m0 + r];
        db3p[blockIdx.x] = s;
    }
}

// dW0 partial of one 128-pair slice for one 32 (hidden) x 32 (feature) tile: lanes 0-31 reduce pairs 0-63 of the slice, 32-63 pairs 64-127
__global__ __launch_bounds__(64) void lp_dw0_kernel(const float* __restrict__ h, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                    int64_t N, int64_t K, const float* __restrict__ gz, float* __restrict__ part) {
    const int lane = threadIdx.x, l31 = lane & 31, half = lane >> 5;
    const int n0 = (blockIdx.x % (HID / 32)) * 32, k0 = (blockIdx.x / (HID / 32)) * 32;
    const int seg = k0 / F, c = (k0 % F) + l31;
    const int64_t mb = (int64_t)blockIdx.y * MS + half * (MS / 2);
    f32x16 acc;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 8
    for (int i = 0; i < MS / 2; ++i) {
        const int64_t m = mb + i;
        float a = 0.f, f = 0.f;
        if (m < K) {
            a = gz[m * HID + n0 + l31];
            const float s = row1(h, src[m], N, c), d = row1(h, dst[m], N, c);
            f = seg == 0 ? s + d : (seg == 1 ? s * d : fabsf(s - d));
        }
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, f, acc, 0, 0, 0);
    }
    float* o = part + (int64_t)blockIdx.y * W0N;
#pragma unroll
    for (int r = 0; r < 16; ++r) o[(int64_t)gmp::acc_row(r, half, n0) * KF + k0 + l31] = acc[r];
}

// g_feat = g_z W0 for 32 pairs x (the same 32 columns of all three segments); wave w reduces hidden units [64 w, 64 w + 64)
__global__ __launch_bounds__(256) void lp_gfeat_kernel(const float* __restrict__ h, const int64_t* __restrict__ src, const int64_t* __restrict__ dst,
                                                       int64_t N, int64_t K, const float* __restrict__ gz, const float* __restrict__ w0,
                                                       float* __restrict__ g_hs, float* __restrict__ g_hd) {
    __shared__ float red[4][3][32 * 32];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    const int64_t m0 = (int64_t)blockIdx.x * BM;
    const int c0 = blockIdx.y * 32;
    const int nb = 64 * wave + 32 * half;
    const float4* a4 = reinterpret_cast<const float4*>(gz + (m0 + l31) * HID + nb);     // (the g_z workspace has every row of the tile)
    f32x16 acc[3];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[s][r] = 0.f;
#pragma unroll 2
    for (int q = 0; q < 8; ++q) {
        const float4 av = a4[q];
        const float aa[4] = {av.x, av.y, av.z, av.w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* wr = w0 + (int64_t)(nb + 4 * q + j) * KF + c0 + l31;
#pragma unroll
            for (int s = 0; s < 3; ++s) acc[s] = __builtin_amdgcn_mfma_f32_32x32x2f32(aa[j], wr[s * F], acc[s], 0, 0, 0);
        }
    }
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
        for (int r = 0; r < 16; ++r) red[wave][s][gmp::acc_row(r, half) * 32 + l31] = acc[s][r];
    __syncthreads();
    for (int e = t; e < 32 * 32; e += 256) {
        const int row = e >> 5, col = e & 31;
        const int64_t m = m0 + row;
        if (m >= K) continue;
        float g[3];
#pragma unroll
        for (int s = 0; s < 3; ++s) g[s] = ((red[0][s][e] + red[1][s][e]) + red[2][s][e]) + red[3][s][e];
        const int c = c0 + col;
        const float sv = row1(h, src[m], N, c), dv = row1(h, dst[m], N, c);
        const float tt = g[2] * sgn(sv - dv);
        g_hs[m * F + c] = g[0] + g[1] * dv + tt;
        g_hd[m * F + c] = g[0] + g[1] * sv - tt;
    }
}

__global__ __launch_bounds__(256) void lp_wgrad_final_kernel(const float* __restrict__ dw0p, int S, const float* __restrict__ db0p,
                                                             const float* __restrict__ dw3p, const float* __restrict__ db3p, int T,
                                                             float* __restrict__ g_w0, float* __restrict__ g_b0, float* __restrict__ g_w3,
                                                             float* __restrict__ g_b3, int accumulate) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    float s = 0.f;
    float* out;
    if (i < W0N) {
        for (int j = 0; j < S; ++j) s += dw0p[(int64_t)j * W0N + i];
        out = g_w0 + i;
    } else if (i < W0N + HID) {
        const int n = (int)(i - W0N);
        for (int j = 0; j < T; ++j) s += db0p[(int64_t)j * HID + n];
        out = g_b0 + n;
    } else if (i < W0N + 2 * HID) {
        const int n = (int)(i - W0N - HID);
        for (int j = 0; j < T; ++j) s += dw3p[(int64_t)j * HID + n];
        out = g_w3 + n;
    } else if (i == W0N + 2 * HID) {
        for (int j = 0; j < T; ++j) s += db3p[j];
        out = g_b3;
    } else {
        return;
    }
    *out = accumulate ? *out + s : s;
}

struct BwdWs {
    float *gz, *dw0p, *db0p, *dw3p, *db3p;
    int T, S;
    size_t bytes;
};

BwdWs bwd_layout(int64_t K, void* workspace) {
    BwdWs w;
    w.T = gmp::cdiv(K, BM);
    w.S = gmp::cdiv(K, MS);
    gmp::Carver c(workspace, true);
    w.gz = c.take<float>((size_t)w.T * BM * HID);
    w.dw0p = c.take<float>((size_t)w.S * W0N);
    w.db0p = c.take<float>((size_t)w.T * HID);
    w.dw3p = c.take<float>((size_t)w.T * HID);
    w.db3p = c.take<float>((size_t)w.T);
    w.bytes = c.total();
    return w;
}

int shape_ok(const char* who, int64_t N, int64_t K, int feat, int hidden) {
    if (feat != F || hidden != HID) return gmp::fail(GMP_ERR_UNSUPPORTED, "%s: feat %d / hidden %d (this kernel is built for 256 / 256)", who, feat, hidden);
    if (N < 0 || K < 0 || K > ((int64_t)1 << 31) / HID) return gmp::fail(GMP_ERR_ARG, "%s: N=%lld K=%lld", who, (long long)N, (long long)K);
    return GMP_OK;
}

}  // namespace

extern "C" size_t gmp_lp_score_fwd_workspace_bytes(int64_t K) { return (size_t)(K > 0 ? K : 1) * (HID / 32) * 4; }

extern "C" size_t gmp_lp_score_bwd_workspace_bytes(int64_t K) { return bwd_layout(K > 0 ? K : 0, nullptr).bytes; }

extern "C" int gmp_lp_score_fwd(const float* h, const int64_t* src, const int64_t* dst, int64_t N, int64_t K, int feat, int hidden,
                                const float* w0, const float* b0, const float* w3, const float* b3, float* act, float* logit,
                                float p, uint64_t seed, uint32_t site, void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    if (int rc = shape_ok("lp_score_fwd", N, K, feat, hidden)) return rc;
    if (p < 0.f || p >= 1.f) return gmp::fail(GMP_ERR_ARG, "lp_score_fwd: p=%f", p);
    if (K == 0) return GMP_OK;
    if (!h || !src || !dst || !w0 || !b0 || !w3 || !b3 || !act || !logit || !workspace)
        return gmp::fail(GMP_ERR_ARG, "lp_score_fwd: null pointer");
    if (!aligned16(h) || !aligned16(w0) || !aligned16(b0) || !aligned16(w3) || !aligned16(act))
        return gmp::fail(GMP_ERR_ARG, "lp_score_fwd: h, w0, b0, w3 and act must be 16-byte aligned");
    if (workspace_bytes < gmp_lp_score_fwd_workspace_bytes(K)) return gmp::fail(GMP_ERR_ARG, "lp_score_fwd: workspace too small");
    static std::atomic<uint64_t> attr_set{0};               // > 64 KiB of dynamic LDS: opt in once per device (gnnmp_internal.h)
    if (int rc = gmp::reserve_lds(attr_set, (const void*)lp_score_fwd_kernel, FWD_LDS, "lp_score_fwd")) return rc;
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)workspace;
    hipLaunchKernelGGL(lp_score_fwd_kernel, dim3((unsigned)gmp::cdiv(K, BM), HID / 32), dim3(THREADS), FWD_LDS, st, h, src, dst, N, K,
                       w0, b0, w3, act, part, p, seed, site);
    if (int rc = gmp::check_launch("lp_score_fwd_kernel")) return rc;
    hipLaunchKernelGGL(lp_logit_kernel, dim3((unsigned)gmp::cdiv(K, 256)), dim3(256), 0, st, (const float*)part, b3, logit, K);
    return gmp::check_launch("lp_logit_kernel");
}

extern "C" int gmp_lp_score_bwd(const float* h, const int64_t* src, const int64_t* dst, int64_t N, int64_t K, int feat, int hidden,
                                const float* w0, const float* w3, const float* act, const float* g_logit, float p, uint64_t seed, uint32_t site,
                                float* g_w0, float* g_b0, float* g_w3, float* g_b3, int accumulate, float* g_hs, float* g_hd,
                                void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    if (int rc = shape_ok("lp_score_bwd", N, K, feat, hidden)) return rc;
    if (p < 0.f || p >= 1.f) return gmp::fail(GMP_ERR_ARG, "lp_score_bwd: p=%f", p);
    if (!g_w0 || !g_b0 || !g_w3 || !g_b3 || !workspace) return gmp::fail(GMP_ERR_ARG, "lp_score_bwd: null pointer");
    if (K > 0 && (!h || !src || !dst || !w0 || !w3 || !act || !g_logit || !g_hs || !g_hd))
        return gmp::fail(GMP_ERR_ARG, "lp_score_bwd: null pointer");
    if (!aligned16(w3) || !aligned16(act)) return gmp::fail(GMP_ERR_ARG, "lp_score_bwd: w3 and act must be 16-byte aligned");
    if (workspace_bytes < gmp_lp_score_bwd_workspace_bytes(K)) return gmp::fail(GMP_ERR_ARG, "lp_score_bwd: workspace too small");
    const BwdWs w = bwd_layout(K, workspace);
    hipStream_t st = (hipStream_t)stream;
    if (K > 0) {
        hipLaunchKernelGGL(lp_gz_kernel, dim3((unsigned)w.T), dim3(256), 0, st, act, g_logit, w3, w.gz, w.db0p, w.dw3p, w.db3p, K, p, seed, site);
        if (int rc = gmp::check_launch("lp_gz_kernel")) return rc;
        hipLaunchKernelGGL(lp_dw0_kernel, dim3((unsigned)((HID / 32) * (KF / 32)), (unsigned)w.S), dim3(64), 0, st, h, src, dst, N, K,
                           (const float*)w.gz, w.dw0p);
        if (int rc = gmp::check_launch("lp_dw0_kernel")) return rc;
        hipLaunchKernelGGL(lp_gfeat_kernel, dim3((unsigned)w.T, F / 32), dim3(256), 0, st, h, src, dst, N, K, (const float*)w.gz, w0, g_hs, g_hd);
        if (int rc = gmp::check_launch("lp_gfeat_kernel")) return rc;
    }
    hipLaunchKernelGGL(lp_wgrad_final_kernel, dim3((unsigned)gmp::cdiv(W0N + 2 * HID + 1, 256)), dim3(256), 0, st, (const float*)w.dw0p, w.S,
                       (const float*)w.db0p, (const float*)w.dw3p, (const float*)w.db3p, w.T, g_w0, g_b0, g_w3, g_b3, accumulate);
    return gmp::check_launch("lp_wgrad_final_kernel");
}
