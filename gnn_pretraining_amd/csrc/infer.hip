// The inference path: eval-mode BatchNorm folded into the GEMM that feeds it.
//
// With running statistics BatchNorm1d is a per-channel affine map, y = scale * u + shift with scale = gamma / sqrt(running_var + eps) and
// shift = beta - scale * running_mean, so it belongs in the GEMM epilogue: no statistics pass, no segment lookup, no hand-off between
// workgroups.  gmp_bn_fold writes the (scale, shift) table of every BatchNorm of a model in one launch; gmp_linear_affine_fwd is the Linear
// forward with that map (and the GIN layer's residual, and the ReLU) applied to the accumulators -- the product itself runs through
// gmp_gemm_f32's two kernel families and dispatch rule (gemm_f32.hip, gmp::gemm_f32_epilogue).
#include "gnnmp_internal.h"

namespace {

constexpr int FOLD_MAX = 16;
constexpr int FOLD_THREADS = 256;

struct BnFoldArgs {
    float eps;
    const float* gamma[FOLD_MAX];
    const float* beta[FOLD_MAX];
    const float* mean[FOLD_MAX];
    const float* var[FOLD_MAX];
    int C[FOLD_MAX];
    int64_t off[FOLD_MAX];          // floats from the table's base to entry e's scale row; its shift row follows at + C[e]
    float* table;
};

// blockIdx.y = entry.  Correctly rounded sqrt and divide (hipcc's default for fp32) and ONE rounding for the shift (fmaf): scale is within
// 2.5 * 2^-24 relative of the exact value, shift within 3.5 * 2^-24 * |scale * mean| + 2^-24 * |beta|.
__global__ __launch_bounds__(FOLD_THREADS) void bn_fold_kernel(const BnFoldArgs a) {
    const int e = blockIdx.y, c = blockIdx.x * FOLD_THREADS + threadIdx.x, C = a.C[e];
    if (c >= C) return;
    const float g = a.gamma[e] ? a.gamma[e][c] : 1.f, b = a.beta[e] ? a.beta[e][c] : 0.f;
    const float scale = g / sqrtf(a.var[e][c] + a.eps);
    float* out = a.table + a.off[e];
    out[c] = scale;
    out[C + c] = fmaf(-scale, a.mean[e][c], b);
}

}  // namespace

extern "C" int gmp_bn_fold(int count, const float* const* gamma, const float* const* beta, const float* const* running_mean,
                           const float* const* running_var, const int32_t* channels, float eps, float* table, gmp_stream_t stream) {
    if (count < 1 || count > FOLD_MAX || !running_mean || !running_var || !channels || !table)
        return gmp::fail(GMP_ERR_ARG, "bn_fold: bad argument (count=%d, max %d)", count, FOLD_MAX);
    BnFoldArgs a{};
    a.eps = eps;
    a.table = table;
    int maxC = 0;
    int64_t off = 0;
    for (int i = 0; i < count; ++i) {
        if (!running_mean[i] || !running_var[i] || channels[i] <= 0) return gmp::fail(GMP_ERR_ARG, "bn_fold: entry %d", i);
        a.gamma[i] = gamma ? gamma[i] : nullptr;
        a.beta[i] = beta ? beta[i] : nullptr;
        a.mean[i] = running_mean[i];
        a.var[i] = running_var[i];
        a.C[i] = channels[i];
        a.off[i] = off;
        off += 2 * (int64_t)channels[i];
        if (channels[i] > maxC) maxC = channels[i];
    }
    hipLaunchKernelGGL(bn_fold_kernel, dim3((maxC + FOLD_THREADS - 1) / FOLD_THREADS, count), dim3(FOLD_THREADS), 0, (hipStream_t)stream, a);
    return gmp::check_launch("bn_fold_kernel");
}

extern "C" size_t gmp_linear_affine_workspace_bytes(int64_t M, int64_t N, int64_t K) {
    return gmp_gemm_f32_workspace_bytes(GMP_GEMM_NT, M, N, K);
}

extern "C" int gmp_linear_affine_fwd(const float* A, const float* W, const float* bias, const float* residual, const float* scale,
                                     const float* shift, float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw, int64_t ldr,
                                     int64_t ldc, int relu, void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    if (M < 0 || N < 0 || K < 1) return gmp::fail(GMP_ERR_ARG, "linear_affine: sizes M=%lld N=%lld K=%lld", (long long)M, (long long)N, (long long)K);
    if (M == 0 || N == 0) return GMP_OK;
    if (!A || !W || !C || !scale || !shift) return gmp::fail(GMP_ERR_ARG, "linear_affine: null pointer");
    if (residual && ldr < N) return gmp::fail(GMP_ERR_ARG, "linear_affine: residual leading dimension %lld < N = %lld", (long long)ldr, (long long)N);
    return gmp::gemm_f32_epilogue(GMP_GEMM_NT, A, W, bias, C, M, N, K, lda, ldw, ldc, 1.f, 0, relu, scale, shift, residual, residual ? ldr : 0,
                                  workspace, workspace_bytes, stream);
}
