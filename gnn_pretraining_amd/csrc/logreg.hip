// Softmax regression on the GPU (the linear-evaluation probe: a multinomial logistic regression fitted with Adam on the L2-normalised
// rows of frozen embeddings).  A whole fit is enqueued on the caller's stream without a host round trip, two launches per iteration;
// memory is O(n d) plus a bounded block of partial sums, never n x classes.
//
//   logreg_normalize_kernel    one wave per row of x: xn = x / max(||x||, 1e-12), row stride padded with zeros to a multiple of 4
//                              (gmp::normalize_row, the miner's, k-NN's and k-means'); a fit also counts the labels outside [0, classes)
//                              into `status` and copies the step count into the control block
//   logreg_rows_kernel<DP, FIT>  the row pass.  A workgroup of four waves walks 128-row tiles of xn with a grid stride (at most MAX_GROUPS
//                              workgroups).  A tile is read from memory once, into LDS.  Logits: W padded to 32 rows sits in REGISTERS as
//                              the row operand of Tile<DP>::product and a wave's 32 rows of the tile are its column tile, so a lane ends up
//                              with 16 of the 32 classes of ONE row (the other 16 in the lane 32 further on): softmax, loss and argmax are
//                              per-lane loops and one exchange with that lane.  FIT: g = p - onehot(y) goes to LDS as G [128][32 classes]
//                              and S_W += G^T X is a second chain of v_mfma_f32_32x32x2_f32 over the tile's rows in ascending order, every
//                              wave taking its 32-column blocks of X for ALL 128 rows (so no two waves ever add into the same sum);
//                              S_b += G^T 1 and the loss are summed in a fixed order beside it.  After its last tile the workgroup writes
//                              its partial sums to its own slot of the workspace.  No floating-point atomics.
//                              !FIT (predict): the argmax by integer compares on (score bits, ~class) instead, nothing else.
//   logreg_update_kernel       one thread per entry of (W | b): the slots summed in ascending order, one correctly rounded division by n,
//                              the ridge term on W, then Adam on that entry; one more thread sums the loss and writes the step count.
// The step count of the call's first update is read from the control block (copied there from `step` before the first iteration), never
// from `step` itself, which the last thread alone writes: iteration boundaries are kernel boundaries and nobody waits for another workgroup.
#include <algorithm>

#include "sim_tile.h"

namespace {

using namespace sim;

constexpr int MAX_CLASSES = 32;
constexpr int MIN_CLASSES = 2;
constexpr int MAX_DIM = 256;
constexpr int MAX_ITER = 10000;
constexpr int64_t ROW_LIMIT = (int64_t)1 << 31;
constexpr int MAX_GROUPS = 256;             // workgroups of the row pass = slots of partial sums
constexpr int GLD = 33;                     // row stride of G in LDS: the 32 lanes of a half-wave write 32 different rows

struct Ctrl {
    int64_t t0;             // the step count before this call's first update
};

struct Ws {
    float* xn;              // [n][dpad]
    float* parts;           // [groups][slot]: S_W [classes][dpad], S_b [classes], the loss sum, sum(W^2) (slot 0 only)
    Ctrl* ctrl;
    int groups, slot;
    size_t total;
};

int groups_for(int64_t n) { return (int)std::min<int64_t>((n + BM - 1) / BM, MAX_GROUPS); }

Ws carve(void* ws, int64_t n, int classes, int dim) {
    gmp::Carver c(ws, true);
    const int dpad = pad4(dim);
    Ws w;
    w.groups = groups_for(n);
    w.slot = (classes * dpad + classes + 2 + 63) / 64 * 64;
    w.xn = c.take<float>((size_t)n * dpad);
    w.parts = c.take<float>((size_t)w.groups * w.slot);
    w.ctrl = c.take<Ctrl>(1);
    w.total = c.total();
    return w;
}

__global__ __launch_bounds__(THREADS) void logreg_normalize_kernel(const float* __restrict__ x, int64_t n, int d, int dpad, float* __restrict__ xn,
                                                                   const int64_t* __restrict__ labels, int classes, int32_t* __restrict__ status,
                                                                   const int64_t* __restrict__ step, Ctrl* __restrict__ ctrl) {
    const int lane = threadIdx.x % 64;
    const int64_t row = ((int64_t)blockIdx.x * THREADS + threadIdx.x) / 64;
    if (ctrl && blockIdx.x == 0 && threadIdx.x == 0) ctrl->t0 = step[0];
    if (row >= n) return;                                           // (only wave-level work below)
    gmp::normalize_row(x + row * d, d, xn + row * dpad, dpad, nullptr);
    if (labels && lane == 0) {
        const int64_t y = labels[row];
        if (y < 0 || y >= classes) atomicAdd(status, 1);
    }
}

template <int DP>
constexpr int rows_lds_bytes(bool fit) { return (BM * Tile<DP>::LD + (fit ? BM * GLD + 8 : 0)) * 4; }

// Registers at DP = 256: W is 128 floats per lane beside 16 logits, their exponentials and (FIT) two 16-register sums: one workgroup per CU
template <int DP, bool FIT>
__global__ __launch_bounds__(THREADS) void logreg_rows_kernel(const float* __restrict__ xn, int64_t n, const float* __restrict__ W,
                                                              const float* __restrict__ b, int classes, int d, int dpad,
                                                              const int64_t* __restrict__ labels, float* __restrict__ parts, int slot,
                                                              float* __restrict__ logits_out, int64_t* __restrict__ pred) {
    using Tl = Tile<DP>;
    constexpr int LD = Tl::LD, C4 = Tl::C4;
    constexpr int NBLK = DP / 32;                                   // 32-column blocks of X
    constexpr int NBW = (NBLK + 3) / 4;                             // blocks per wave: block j belongs to wave j % 4
    constexpr int NXL = BM * C4 / THREADS;                          // float4 per thread of one tile
    static_assert(NXL % 4 == 0, "tile load shape");
    extern __shared__ float4 smem4[];
    float* xs = reinterpret_cast<float*>(smem4);                    // [BM][LD]
    float* gs = xs + BM * LD;                                       // [BM][GLD]   (FIT)
    float* red = gs + BM * GLD;                                     // [4]         (FIT)
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6, l31 = lane & 31, half = lane >> 5;
    const int64_t ntiles = (n + BM - 1) / BM;

    // W row l31 (zero beyond `classes` and beyond d), k in [half DP/2, (half + 1) DP/2): the row operand of every product of this workgroup
    float4 wq[Tl::KQ];
    {
        const bool cls_ok = l31 < classes;
        const float* wr = W + (int64_t)(cls_ok ? l31 : 0) * d;
#pragma unroll
        for (int u = 0; u < Tl::KQ; ++u) {
            const int kk = half * (DP / 2) + 4 * u;
            wq[u].x = (cls_ok && kk + 0 < d) ? wr[kk + 0] : 0.f;
            wq[u].y = (cls_ok && kk + 1 < d) ? wr[kk + 1] : 0.f;
            wq[u].z = (cls_ok && kk + 2 < d) ? wr[kk + 2] : 0.f;
            wq[u].w = (cls_ok && kk + 3 < d) ? wr[kk + 3] : 0.f;
        }
    }
    // accumulator r of this lane is class acc_row(r, half) of row l31 of the wave
    float bias[16];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int c = acc_row(r, half);
        bias[r] = c < classes ? b[c] : 0.f;
    }

    f32x16 sw[NBW];                                                 // S_W[class acc_row(r, half)][column 32 (wave + 4 u) + l31]
#pragma unroll
    for (int u = 0; u < NBW; ++u)
#pragma unroll
        for (int r = 0; r < 16; ++r) sw[u][r] = 0.f;
    float sb = 0.f, loss = 0.f;                                     // S_b[class l31] (wave 3), this lane's rows' losses (half 0)

    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t i0 = tile * BM;
        // the tile into LDS, zero beyond dpad and beyond n: the one read of these rows
#pragma unroll
        for (int u0 = 0; u0 < NXL; u0 += 4) {
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int it = t + (u0 + u) * THREADS, r = it / C4, c4 = it % C4;
                v[u] = (i0 + r < n && 4 * c4 < dpad) ? *reinterpret_cast<const float4*>(xn + (i0 + r) * dpad + 4 * c4) : make_float4(0.f, 0.f, 0.f, 0.f);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int it = t + (u0 + u) * THREADS, r = it / C4, c4 = it % C4;
                *reinterpret_cast<float4*>(xs + r * LD + 4 * c4) = v[u];
            }
        }
        __syncthreads();

        // z[row l31][class acc_row(r, half)] = <W_class, xn_row> + b_class
        const f32x16 acc = Tl::product(wq, xs + wave * 32 * LD, l31, half);
        const int64_t row = i0 + wave * 32 + l31;
        const bool row_ok = row < n;
        float z[16];
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = acc[r] + bias[r];
        if (logits_out && row_ok) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = acc_row(r, half);
                if (c < classes) logits_out[row * classes + c] = z[r];
            }
        }
        if (FIT) {
            const int64_t y64 = row_ok ? labels[row] : -1;
            const int y = (y64 >= 0 && y64 < classes) ? (int)y64 : -1;         // -1: the row contributes nothing
            float m = -INFINITY;
#pragma unroll
            for (int r = 0; r < 16; ++r) m = acc_row(r, half) < classes ? fmaxf(m, z[r]) : m;
            m = fmaxf(m, __shfl_xor(m, 32, 64));                    // (classes >= 2: class 0 is real, m is finite for finite logits)
            float e[16], s = 0.f, zy = 0.f;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = acc_row(r, half);
                e[r] = c < classes ? expf(z[r] - m) : 0.f;
                s += e[r];
                zy = c == y ? z[r] : zy;
            }
            s += __shfl_xor(s, 32, 64);                             // (a + b on one side, b + a on the other: the same bits)
            zy += __shfl_xor(zy, 32, 64);                           // (one side holds z[y], the other 0)
            if (half == 0 && y >= 0) loss += (m + logf(s)) - zy;
            float* const grow = gs + (wave * 32 + l31) * GLD;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = acc_row(r, half);
                const float p = e[r] / s;
                grow[c] = y >= 0 ? p - (c == y ? 1.f : 0.f) : 0.f;
            }
            __syncthreads();

            // S_W += G^T X: MFMA step rp contracts rows 2 rp and 2 rp + 1 of the tile (lane half `half` supplies row 2 rp + half)
#pragma unroll
            for (int u = 0; u < NBW; ++u) {
                const int jb = wave + 4 * u;
                if (jb < NBLK) {                                    // (wave-uniform)
                    const float* ga = gs + half * GLD + l31;
                    const float* xb = xs + half * LD + 32 * jb + l31;
#pragma unroll 8
                    for (int rp = 0; rp < BM / 2; ++rp)
                        sw[u] = __builtin_amdgcn_mfma_f32_32x32x2f32(ga[2 * rp * GLD], xb[2 * rp * LD], sw[u], 0, 0, 0);
                }
            }
            // S_b += G^T 1: wave 3, lane (class l31, half) over rows [64 half, 64 half + 64) in ascending order, then the two halves
            if (wave == 3) {
                float part = 0.f;
                for (int rr = 0; rr < BM / 2; ++rr) part += gs[(half * (BM / 2) + rr) * GLD + l31];
                part += __shfl_xor(part, 32, 64);
                sb += part;
            }
        } else {
            // the argmax: a greater key is a better class (higher logit, then lower class); integer compares only
            u64 best = 0ull;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int c = acc_row(r, half);
                const u64 key = c < classes ? gmp::pack_key(z[r], 0xffffffffu - (uint32_t)c) : 0ull;
                best = key > best ? key : best;
            }
            const u64 other = __shfl_xor(best, 32, 64);
            best = other > best ? other : best;
            if (half == 0 && row_ok) pred[row] = (int64_t)gmp::key_low(best);
        }
        __syncthreads();                                            // the tile's readers are done
    }

    if (FIT) {
        float* const mine = parts + (int64_t)blockIdx.x * slot;
#pragma unroll
        for (int u = 0; u < NBW; ++u) {
            const int jb = wave + 4 * u, col = 32 * jb + l31;
            if (jb < NBLK && col < dpad) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int c = acc_row(r, half);
                    if (c < classes) mine[c * dpad + col] = sw[u][r];
                }
            }
        }
        if (wave == 3 && half == 0 && l31 < classes) mine[classes * dpad + l31] = sb;
        // the loss: a wave's lanes by the fixed shuffle tree, then the four waves in order
        loss = gmp::wave_sum(loss);
        if (lane == 0) red[wave] = loss;
        // sum(W^2), workgroup 0 alone: wave 0 holds every entry of W exactly once
        float wsq = 0.f;
        if (blockIdx.x == 0 && wave == 0) {
#pragma unroll
            for (int u = 0; u < Tl::KQ; ++u) wsq += (wq[u].x * wq[u].x + wq[u].y * wq[u].y) + (wq[u].z * wq[u].z + wq[u].w * wq[u].w);
            wsq = gmp::wave_sum(wsq);
        }
        __syncthreads();
        if (t == 0) {
            mine[classes * dpad + classes] = ((red[0] + red[1]) + red[2]) + red[3];
            if (blockIdx.x == 0) mine[classes * dpad + classes + 1] = wsq;
        }
    }
}

// Adam as torch.optim.Adam: the two bias corrections in double, as torch computes them on the host, everything else in fp32
__device__ __forceinline__ void adam_entry(float g, float* __restrict__ theta, float* __restrict__ m, float* __restrict__ v, float step_size,
                                           float sqrt_bc2) {
    const float mn = 0.9f * *m + 0.1f * g;
    const float vn = 0.999f * *v + 0.001f * (g * g);
    *m = mn;
    *v = vn;
    *theta = *theta - step_size * (mn / (sqrtf(vn) / sqrt_bc2 + 1e-8f));
}

__global__ __launch_bounds__(THREADS) void logreg_update_kernel(const float* __restrict__ parts, int groups, int slot, int classes, int d, int dpad,
                                                                int64_t n, float* __restrict__ W, float* __restrict__ b, float* __restrict__ m,
                                                                float* __restrict__ v, const Ctrl* __restrict__ ctrl, int k, float lr, float l2,
                                                                int64_t* __restrict__ step, float* __restrict__ loss_out,
                                                                float* __restrict__ grad_out) {
    const int idx = blockIdx.x * THREADS + threadIdx.x;
    const int nw = classes * d, nall = classes * (d + 1);
    if (idx > nall) return;
    const float nf = (float)n;
    const int64_t tstep = ctrl->t0 + k + 1;
    if (idx == nall) {                                              // the loss at the parameters this update starts from, and the step count
        float s = 0.f;
        for (int g = 0; g < groups; ++g) s += parts[(int64_t)g * slot + classes * dpad + classes];
        loss_out[k] = __fdiv_rn(s, nf) + (0.5f * l2) * parts[classes * dpad + classes + 1];
        step[0] = tstep;
        return;
    }
    const bool is_w = idx < nw;
    const int c = is_w ? idx / d : idx - nw, kk = is_w ? idx % d : d;
    const int off = is_w ? c * dpad + kk : classes * dpad + c;
    float s = 0.f;
    for (int g = 0; g < groups; ++g) s += parts[(int64_t)g * slot + off];
    float* const theta = is_w ? W + idx : b + c;
    const float grad = is_w ? __fdiv_rn(s, nf) + l2 * *theta : __fdiv_rn(s, nf);
    if (grad_out) grad_out[c * (d + 1) + kk] = grad;
    const double bc1 = 1.0 - pow(0.9, (double)tstep), bc2 = 1.0 - pow(0.999, (double)tstep);
    adam_entry(grad, theta, m + c * (d + 1) + kk, v + c * (d + 1) + kk, (float)((double)lr / bc1), (float)sqrt(bc2));
}

template <int DP, bool FIT>
int launch_rows(const Ws& w, int64_t n, const float* W, const float* b, int classes, int d, int dpad, const int64_t* labels, float* logits_out,
                int64_t* pred, hipStream_t st) {
    static std::atomic<uint64_t> attr{0};                           // up to 150,048 bytes of LDS (DP = 256, a fit): opt in once per device
    constexpr int lds = rows_lds_bytes<DP>(FIT);
    if (int rc = gmp::reserve_lds(attr, (const void*)logreg_rows_kernel<DP, FIT>, lds, "logreg")) return rc;
    hipLaunchKernelGGL((logreg_rows_kernel<DP, FIT>), dim3((unsigned)w.groups), dim3(THREADS), (size_t)lds, st, (const float*)w.xn, n, W, b, classes, d,
                       dpad, labels, w.parts, w.slot, logits_out, pred);
    return gmp::check_launch("logreg_rows_kernel");
}

template <bool FIT>
int rows(const Ws& w, int64_t n, const float* W, const float* b, int classes, int d, int dpad, const int64_t* labels, float* logits_out, int64_t* pred,
         hipStream_t st) {
    return dispatch_dp(dpad, [&](auto dp) { return launch_rows<dp(), FIT>(w, n, W, b, classes, d, dpad, labels, logits_out, pred, st); });
}

bool sizes_ok(int64_t n, int classes, int dim) {
    return n >= 0 && n < ROW_LIMIT && classes >= MIN_CLASSES && classes <= MAX_CLASSES && dim >= 1 && dim <= MAX_DIM;
}

}  // namespace

extern "C" size_t gmp_logreg_workspace_bytes(int64_t n, int classes, int dim) {
    if (!sizes_ok(n, classes, dim)) return 0;
    return carve(nullptr, n, classes, dim).total;
}

extern "C" int gmp_logreg_fit(const float* x, const int64_t* labels, int64_t n, int classes, int dim, int iters, float lr, float l2, float* W, float* b,
                              float* exp_avg, float* exp_avg_sq, int64_t* step, float* loss_history, int32_t* status, float* grad_out,
                              float* logits_out, void* ws, size_t ws_bytes, gmp_stream_t stream) {
    if (!sizes_ok(n, classes, dim) || iters < 1 || iters > MAX_ITER)
        return gmp::fail(GMP_ERR_ARG, "logreg_fit: n=%lld classes=%d dim=%d iters=%d (0 <= n < 2^31, %d <= classes <= %d, 1 <= dim <= %d, 1 <= iters <= %d)",
                         (long long)n, classes, dim, iters, MIN_CLASSES, MAX_CLASSES, MAX_DIM, MAX_ITER);
    if (n == 0) return GMP_OK;
    if (!x || !labels || !W || !b || !exp_avg || !exp_avg_sq || !step || !loss_history || !status)
        return gmp::fail(GMP_ERR_ARG, "logreg_fit: null pointer");
    const size_t need = gmp_logreg_workspace_bytes(n, classes, dim);
    if (!ws || ws_bytes < need) return gmp::fail(GMP_ERR_WORKSPACE, "logreg_fit: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(ws, n, classes, dim);
    const int dpad = pad4(dim);
    if (hipMemsetAsync(status, 0, sizeof(int32_t), st) != hipSuccess) return gmp::fail(GMP_ERR_LAUNCH, "logreg_fit: memset");
    hipLaunchKernelGGL(logreg_normalize_kernel, dim3((unsigned)gmp::cdiv(n * 64, THREADS)), dim3(THREADS), 0, st, x, n, dim, dpad, w.xn, labels, classes,
                       status, (const int64_t*)step, w.ctrl);
    if (int rc = gmp::check_launch("logreg_normalize_kernel")) return rc;
    const int ublocks = gmp::cdiv((int64_t)classes * (dim + 1) + 1, THREADS);
    for (int k = 0; k < iters; ++k) {
        const bool last = k + 1 == iters;                           // the hooks see the call's last iteration
        if (int rc = rows<true>(w, n, W, b, classes, dim, dpad, labels, last ? logits_out : nullptr, nullptr, st)) return rc;
        hipLaunchKernelGGL(logreg_update_kernel, dim3((unsigned)ublocks), dim3(THREADS), 0, st, (const float*)w.parts, w.groups, w.slot, classes, dim, dpad,
                           n, W, b, exp_avg, exp_avg_sq, (const Ctrl*)w.ctrl, k, lr, l2, step, loss_history, last ? grad_out : nullptr);
        if (int rc = gmp::check_launch("logreg_update_kernel")) return rc;
    }
    return GMP_OK;
}

extern "C" int gmp_logreg_predict(const float* x, int64_t n, const float* W, const float* b, int classes, int dim, int64_t* pred, float* logits_out,
                                  void* ws, size_t ws_bytes, gmp_stream_t stream) {
    if (!sizes_ok(n, classes, dim))
        return gmp::fail(GMP_ERR_ARG, "logreg_predict: n=%lld classes=%d dim=%d (0 <= n < 2^31, %d <= classes <= %d, 1 <= dim <= %d)", (long long)n,
                         classes, dim, MIN_CLASSES, MAX_CLASSES, MAX_DIM);
    if (n == 0) return GMP_OK;
    if (!x || !W || !b || !pred) return gmp::fail(GMP_ERR_ARG, "logreg_predict: null pointer");
    const size_t need = gmp_logreg_workspace_bytes(n, classes, dim);
    if (!ws || ws_bytes < need) return gmp::fail(GMP_ERR_WORKSPACE, "logreg_predict: workspace %zu < %zu", ws ? ws_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    const Ws w = carve(ws, n, classes, dim);
    const int dpad = pad4(dim);
    hipLaunchKernelGGL(logreg_normalize_kernel, dim3((unsigned)gmp::cdiv(n * 64, THREADS)), dim3(THREADS), 0, st, x, n, dim, dpad, w.xn,
                       (const int64_t*)nullptr, classes, (int32_t*)nullptr, (const int64_t*)nullptr, (Ctrl*)nullptr);
    if (int rc = gmp::check_launch("logreg_normalize_kernel")) return rc;
    return rows<false>(w, n, W, b, classes, dim, dpad, nullptr, logits_out, pred, st);
}
