// The graph-classification head of fine-tuning (src/models/finetune_model.py:68-80 + src/finetune/finetune.py:110-114) fused over one
// batch of B graphs whose rows are the contiguous segments ptr[b] .. ptr[b+1] of h:
//   pooled[b] = mean of the graph's rows (divisor max(count, 1): PyG's scatter-mean, gmp_segment_sum(mean = 1))
//   act = relu(pooled W0^T + b0) (256 -> 128), dropped = dropout(act), logits = dropped W3^T + b3 (128 -> C)
//   loss = cross-entropy sum (C > 2) or BCE-with-logits on logits[:, 1] (C == 2: logits[:, 0] gets no gradient)
// The module path runs that as about a dozen launches, forward and backward, over a 32-row matrix; here it is three.  B is a few
// hundred at most and the weights are 128 KB, so nothing here is matrix-core work: one workgroup per graph, wave-wide dot products
// against rows of the weights read as coalesced 16-byte pieces, and fixed-order loops over graphs for the weight gradients.
// Every sum is in a fixed order (no atomics): a second run is bitwise the same.
//
// Forward (two launches):
//   gc_head_fwd_kernel     one block per graph: four waves sum the graph's rows (row r to wave r % 4, the four partial rows added in
//                          order), the pooled row stays in LDS; each wave takes 32 hidden units (a 256-deep dot per unit, butterfly
//                          sum), the Philox mask of gmp_dropout_fwd over the [B, 128] activation, the C logits the same way, then the
//                          graph's loss term and d loss / d logits (scaled by the device word g_scale)
//   gc_loss_sum_kernel     loss = the B terms added in order
// Backward (one launch, blocks by role):
//   blocks [0, B)          per graph: g_z = (g_logits W3) * mask * (act > 0), g_pooled = g_z W0, every row of the graph written with
//                          g_pooled / max(count, 1) (block 0 / B - 1 also zero the rows in front of ptr[0] / behind ptr[B])
//   blocks [B, B + 32)     dW0 rows 4 j .. 4 j + 3 and db0: g_z of those four units recomputed per graph into LDS (256 graphs at a
//                          time), thread k accumulates column k over the graphs in order
//   block  B + 32          dW3 and db3 over the graphs in order, the dropped activation rebuilt from act and the mask
#include "gnnmp_internal.h"

namespace {

constexpr int F = 256;              // node embedding width
constexpr int HID = 128;            // hidden units of the head
constexpr int CMAX = 16;            // classes
constexpr int T = 256;
constexpr int JB = 4;               // hidden units per weight-gradient block (one float4 of the dropout mask)
constexpr int WG_BLOCKS = HID / JB;

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

__device__ __forceinline__ float4 mask4(int64_t b, int j4, float p, uint64_t seed, uint32_t site) {
    // the mask gmp_dropout_fwd draws for elements (b, 4 j4 .. 4 j4 + 3) of a contiguous [B, 128] activation
    if (p <= 0.f) return make_float4(1.f, 1.f, 1.f, 1.f);
    return gmp::dropout_scale4(seed, site, (uint64_t)(b * (HID / 4) + j4), p, 1.f / (1.f - p));
}

__device__ __forceinline__ float pick(const float4 v, int i) { return i == 0 ? v.x : (i == 1 ? v.y : (i == 2 ? v.z : v.w)); }

// rows [s, e) of graph b, clamped into [0, N] (a malformed ptr reads and writes nothing outside h / g_h)
__device__ __forceinline__ void graph_rows(const int32_t* __restrict__ ptr, int64_t b, int64_t N, int64_t& s, int64_t& e) {
    s = ptr[b];
    e = ptr[b + 1];
    s = s < 0 ? 0 : (s > N ? N : s);
    e = e < s ? s : (e > N ? N : e);
}

__global__ __launch_bounds__(T) void gc_head_fwd_kernel(const float* __restrict__ h, int64_t ldh, const int32_t* __restrict__ ptr, int64_t N,
                                                        int C, const float* __restrict__ w0, const float* __restrict__ b0,
                                                        const float* __restrict__ w3, const float* __restrict__ b3,
                                                        const int64_t* __restrict__ target, const float* __restrict__ g_scale,
                                                        float* __restrict__ pooled, float* __restrict__ act, float* __restrict__ logits,
                                                        float* __restrict__ g_logits, float* __restrict__ lossrow, float p, uint64_t seed,
                                                        uint32_t site) {
    __shared__ float4 part[4][F / 4];
    __shared__ float4 pool_s[F / 4];
    __shared__ float4 act_s[HID / 4];
    __shared__ float lg_s[CMAX];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int64_t b = blockIdx.x;
    int64_t s, e;
    graph_rows(ptr, b, N, s, e);

    float4 sum = zero4();
    for (int64_t r = s + wave; r < e; r += 4) {
        const float4 v = *reinterpret_cast<const float4*>(h + r * ldh + 4 * lane);
        sum.x += v.x; sum.y += v.y; sum.z += v.z; sum.w += v.w;
    }
    part[wave][lane] = sum;
    __syncthreads();
    if (wave == 0) {
        const float cnt = (float)(e - s > 1 ? e - s : 1);
        float4 a = part[0][lane];
#pragma unroll
        for (int w = 1; w < 4; ++w) { a.x += part[w][lane].x; a.y += part[w][lane].y; a.z += part[w][lane].z; a.w += part[w][lane].w; }
        a = make_float4(a.x / cnt, a.y / cnt, a.z / cnt, a.w / cnt);
        pool_s[lane] = a;
        *reinterpret_cast<float4*>(pooled + b * F + 4 * lane) = a;
    }
    __syncthreads();

    // hidden layer: wave w takes units [32 w, 32 w + 32), lane l the 16 bytes 4 l .. 4 l + 3 of the 256-deep dot
    const float4 x = pool_s[lane];
    float* act_f = reinterpret_cast<float*>(act_s);
#pragma unroll 8
    for (int i = 0; i < HID / 4; ++i) {
        const int j = wave * (HID / 4) + i;
        const float4 w = *reinterpret_cast<const float4*>(w0 + (int64_t)j * F + 4 * lane);
        const float d = gmp::wave_sum((x.x * w.x + x.y * w.y) + (x.z * w.z + x.w * w.w));
        if (lane == 0) act_f[j] = fmaxf(d + b0[j], 0.f);
    }
    __syncthreads();
    if (t < HID / 4) {
        const float4 a = act_s[t], m = mask4(b, t, p, seed, site);
        *reinterpret_cast<float4*>(act + b * HID + 4 * t) = a;                 // the kept pre-dropout activation
        act_s[t] = make_float4(a.x * m.x, a.y * m.y, a.z * m.z, a.w * m.w);
    }
    __syncthreads();

    // logits: wave w takes classes w, w + 4, ...; lane l two of the 128 products
    const float2 dv = reinterpret_cast<const float2*>(act_s)[lane];
    for (int c = wave; c < C; c += 4) {
        const float2 w = *reinterpret_cast<const float2*>(w3 + (int64_t)c * HID + 2 * lane);
        const float d = gmp::wave_sum(dv.x * w.x + dv.y * w.y);
        if (lane == 0) lg_s[c] = d + b3[c];
    }
    __syncthreads();
    if (t < C) logits[b * C + t] = lg_s[t];
    if (t == 0) {
        const float g = g_scale[0];
        const int64_t y = target[b];
        if (C == 2) {                                                           // BCE-with-logits on logits[:, 1]
            const float xx = lg_s[1], yy = (float)y;
            lossrow[b] = fmaxf(xx, 0.f) - xx * yy + log1pf(expf(-fabsf(xx)));
            g_logits[b * 2] = 0.f;
            g_logits[b * 2 + 1] = g * (1.f / (1.f + expf(-xx)) - yy);
        } else {
            float mx = lg_s[0];
            for (int c = 1; c < C; ++c) mx = fmaxf(mx, lg_s[c]);
            float se = 0.f;
            for (int c = 0; c < C; ++c) se += expf(lg_s[c] - mx);
            const float lse = mx + logf(se);
            const bool ok = y >= 0 && y < C;                                    // (an out-of-range label adds nothing: gmp_cross_entropy_sum_*)
            lossrow[b] = ok ? lse - lg_s[y] : 0.f;
            for (int c = 0; c < C; ++c) g_logits[b * C + c] = ok ? g * (expf(lg_s[c] - lse) - (c == y ? 1.f : 0.f)) : 0.f;
        }
    }
}

__global__ __launch_bounds__(T) void gc_loss_sum_kernel(const float* __restrict__ lossrow, int64_t B, float* __restrict__ loss) {
    __shared__ float sh[T];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < B; i += T) s += lossrow[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int d = T / 2; d > 0; d >>= 1) {
        if (threadIdx.x < d) sh[threadIdx.x] += sh[threadIdx.x + d];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = sh[0];
}

// g_z[b, 4 j4 .. 4 j4 + 3] = (sum_c g_logits[b, c] w3[c, j]) * mask * (act > 0), classes in order
__device__ __forceinline__ float4 gz4(const float* __restrict__ g_logits, const float* __restrict__ w3, const float* __restrict__ act, int64_t b,
                                      int j4, int C, float p, uint64_t seed, uint32_t site) {
    float4 s = zero4();
    for (int c = 0; c < C; ++c) {
        const float g = g_logits[b * C + c];
        const float4 w = *reinterpret_cast<const float4*>(w3 + (int64_t)c * HID + 4 * j4);
        s.x += g * w.x; s.y += g * w.y; s.z += g * w.z; s.w += g * w.w;
    }
    const float4 a = *reinterpret_cast<const float4*>(act + b * HID + 4 * j4), m = mask4(b, j4, p, seed, site);
    return make_float4(a.x > 0.f ? s.x * m.x : 0.f, a.y > 0.f ? s.y * m.y : 0.f, a.z > 0.f ? s.z * m.z : 0.f, a.w > 0.f ? s.w * m.w : 0.f);
}

__global__ __launch_bounds__(T) void gc_head_bwd_kernel(const int32_t* __restrict__ ptr, int64_t N, int64_t B, int C,
                                                        const float* __restrict__ w0, const float* __restrict__ w3,
                                                        const float* __restrict__ pooled, const float* __restrict__ act,
                                                        const float* __restrict__ g_logits, float p, uint64_t seed, uint32_t site,
                                                        float* __restrict__ g_w0, float* __restrict__ g_b0, float* __restrict__ g_w3,
                                                        float* __restrict__ g_b3, float* __restrict__ g_h, int64_t ldg) {
    __shared__ float4 gz_s[T];                      // role 1: g_z of one graph (32 float4); role 2: of four units for 256 graphs
    __shared__ float4 gp_s[F / 4];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;

    if ((int64_t)blockIdx.x < B) {                  // ---- one graph: g_pooled and the graph's rows of g_h
        const int64_t b = blockIdx.x;
        int64_t s, e;
        graph_rows(ptr, b, N, s, e);
        if (t < HID / 4) gz_s[t] = gz4(g_logits, w3, act, b, t, C, p, seed, site);
        __syncthreads();
        const float* gz = reinterpret_cast<const float*>(gz_s);
        const float cnt = (float)(e - s > 1 ? e - s : 1);
        float a = 0.f;
#pragma unroll 8
        for (int j = 0; j < HID; ++j) a += gz[j] * w0[(int64_t)j * F + t];
        reinterpret_cast<float*>(gp_s)[t] = a / cnt;
        __syncthreads();
        const float4 v = gp_s[lane];
        for (int64_t r = s + wave; r < e; r += 4) *reinterpret_cast<float4*>(g_h + r * ldg + 4 * lane) = v;
        if (b == 0) {                               // rows no graph owns carry no gradient
            int64_t first = ptr[0];
            first = first < 0 ? 0 : (first > N ? N : first);
            for (int64_t r = wave; r < first; r += 4) *reinterpret_cast<float4*>(g_h + r * ldg + 4 * lane) = zero4();
        }
        if (b == B - 1)
            for (int64_t r = e + wave; r < N; r += 4) *reinterpret_cast<float4*>(g_h + r * ldg + 4 * lane) = zero4();
        return;
    }
    const int role = (int)((int64_t)blockIdx.x - B);
    if (role < WG_BLOCKS) {                         // ---- dW0 rows 4 role .. 4 role + 3 (thread t: column t) and their db0
        float acc[JB] = {0.f, 0.f, 0.f, 0.f}, bias = 0.f;
        for (int64_t b0 = 0; b0 < B; b0 += T) {
            const int64_t nb = B - b0 < T ? B - b0 : T;
            __syncthreads();
            if (t < nb) gz_s[t] = gz4(g_logits, w3, act, b0 + t, role, C, p, seed, site);
            __syncthreads();
            for (int64_t i = 0; i < nb; ++i) {
                const float4 g = gz_s[i];
                const float x = pooled[(b0 + i) * F + t];
                acc[0] += g.x * x; acc[1] += g.y * x; acc[2] += g.z * x; acc[3] += g.w * x;
                if (t < JB) bias += pick(g, t);
            }
        }
#pragma unroll
        for (int jj = 0; jj < JB; ++jj) g_w0[(int64_t)(JB * role + jj) * F + t] = acc[jj];
        if (t < JB) g_b0[JB * role + t] = bias;
        return;
    }
    // ---- dW3 (thread t < 128: column t, every class) and db3 (thread 128 + c)
    if (t < HID) {
        float acc[CMAX];
#pragma unroll
        for (int c = 0; c < CMAX; ++c) acc[c] = 0.f;
        for (int64_t b = 0; b < B; ++b) {
            const float d = act[b * HID + t] * pick(mask4(b, t >> 2, p, seed, site), t & 3);
#pragma unroll
            for (int c = 0; c < CMAX; ++c)
                if (c < C) acc[c] += g_logits[b * C + c] * d;
        }
#pragma unroll
        for (int c = 0; c < CMAX; ++c)
            if (c < C) g_w3[(int64_t)c * HID + t] = acc[c];
    } else if (t - HID < C) {
        const int c = t - HID;
        float s = 0.f;
        for (int64_t b = 0; b < B; ++b) s += g_logits[b * C + c];
        g_b3[c] = s;
    }
}

int shape_ok(const char* who, int64_t N, int64_t B, int feat, int hidden, int C, int64_t ld) {
    if (feat != F || hidden != HID) return gmp::fail(GMP_ERR_UNSUPPORTED, "%s: feat %d / hidden %d (this kernel is built for 256 / 128)", who, feat, hidden);
    if (C < 2 || C > CMAX) return gmp::fail(GMP_ERR_UNSUPPORTED, "%s: %d classes (2 .. %d)", who, C, CMAX);
    if (N < 0 || B < 1 || B > (1 << 20) || N > ((int64_t)1 << 31) - 1) return gmp::fail(GMP_ERR_ARG, "%s: N=%lld B=%lld", who, (long long)N, (long long)B);
    if (ld < F || ld % 4) return gmp::fail(GMP_ERR_ARG, "%s: leading dimension %lld (>= 256, a multiple of 4)", who, (long long)ld);
    return GMP_OK;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" size_t gmp_gc_head_fwd_workspace_bytes(int64_t B) { return (size_t)(B > 0 ? B : 1) * sizeof(float) + 256; }

extern "C" int gmp_gc_head_fwd(const float* h, int64_t ldh, const int32_t* ptr, int64_t N, int64_t B, int feat, int hidden, int C,
                               const float* w0, const float* b0, const float* w3, const float* b3, const int64_t* target,
                               const float* g_scale, float* pooled, float* act, float* logits, float* loss, float* g_logits, float p,
                               uint64_t seed, uint32_t site, void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    if (int rc = shape_ok("gc_head_fwd", N, B, feat, hidden, C, ldh)) return rc;
    if (p < 0.f || p >= 1.f) return gmp::fail(GMP_ERR_ARG, "gc_head_fwd: p=%f", p);
    if (!ptr || !w0 || !b0 || !w3 || !b3 || !target || !g_scale || !pooled || !act || !logits || !loss || !g_logits || !workspace || (N > 0 && !h))
        return gmp::fail(GMP_ERR_ARG, "gc_head_fwd: null pointer");
    if (!aligned16(h) || !aligned16(w0) || !aligned16(w3) || !aligned16(pooled) || !aligned16(act))
        return gmp::fail(GMP_ERR_ARG, "gc_head_fwd: h, w0, w3, pooled and act must be 16-byte aligned");
    if (workspace_bytes < gmp_gc_head_fwd_workspace_bytes(B)) return gmp::fail(GMP_ERR_ARG, "gc_head_fwd: workspace too small");
    float* lossrow = (float*)(((uintptr_t)workspace + 255) / 256 * 256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(gc_head_fwd_kernel, dim3((unsigned)B), dim3(T), 0, st, h, ldh, ptr, N, C, w0, b0, w3, b3, target, g_scale, pooled, act,
                       logits, g_logits, lossrow, p, seed, site);
    if (int rc = gmp::check_launch("gc_head_fwd_kernel")) return rc;
    hipLaunchKernelGGL(gc_loss_sum_kernel, dim3(1), dim3(T), 0, st, (const float*)lossrow, B, loss);
    return gmp::check_launch("gc_loss_sum_kernel");
}

extern "C" int gmp_gc_head_bwd(const int32_t* ptr, int64_t N, int64_t B, int feat, int hidden, int C, const float* w0, const float* w3,
                               const float* pooled, const float* act, const float* g_logits, float p, uint64_t seed, uint32_t site,
                               float* g_w0, float* g_b0, float* g_w3, float* g_b3, float* g_h, int64_t ldg, gmp_stream_t stream) {
    if (int rc = shape_ok("gc_head_bwd", N, B, feat, hidden, C, ldg)) return rc;
    if (p < 0.f || p >= 1.f) return gmp::fail(GMP_ERR_ARG, "gc_head_bwd: p=%f", p);
    if (!ptr || !w0 || !w3 || !pooled || !act || !g_logits || !g_w0 || !g_b0 || !g_w3 || !g_b3 || (N > 0 && !g_h))
        return gmp::fail(GMP_ERR_ARG, "gc_head_bwd: null pointer");
    if (!aligned16(w3) || !aligned16(act) || !aligned16(g_h)) return gmp::fail(GMP_ERR_ARG, "gc_head_bwd: w3, act and g_h must be 16-byte aligned");
    hipLaunchKernelGGL(gc_head_bwd_kernel, dim3((unsigned)(B + WG_BLOCKS + 1)), dim3(T), 0, (hipStream_t)stream, ptr, N, B, C, w0, w3, pooled, act,
                       g_logits, p, seed, site, g_w0, g_b0, g_w3, g_b3, g_h, ldg);
    return gmp::check_launch("gc_head_bwd_kernel");
}
