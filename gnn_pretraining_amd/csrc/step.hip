// Whole-step executor: stacked forward, the five task heads (each on its own stream) and the stacked
// backward of one pre-training step, enqueued from C++ so the host crosses the FFI once.  It is a
// transcription of gnn_pretraining_amd/step_sequence.py (LaunchSequence: forward, heads, backward): same entry
// points, same order, same buffers -> bitwise the same result (tests/test_gpu_engine.py).
#include "../../include/gnnmp_step.h"
#include <stdlib.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <mutex>
#include <thread>

#include "gnnmp_internal.h"

namespace {

#define GMP_TRY(expr) do { int _rc = (expr); if (_rc != GMP_OK) return _rc; } while (0)


constexpr int H = 256;
constexpr int LAYERS = GMP_STEP_LAYERS, MAXT = GMP_STEP_MAX_TASKS;

// One cross-stream dependency of the step, with both of its carriers: a gate flag (d.sync_flags, int32[64], all compared against the step's
// epoch) when the caller vouches that the streams sit on different hardware queues, an event of the pool otherwise.  Gates are sleeping
// waves instead of barrier packets: a parked barrier packet costs every RUNNING queue ~2 us per kernel boundary (streams.hip); with the
// host several steps ahead two or three of the four queues were parked most of the time.
// The flag numbers are fixed: callers use 38 and 63 by number (dist.OverlappedGradSync, engine.check_gates).
struct Dep {
    int flag;      // index into sync_flags; -1: nothing waits for it under gates
    int ev;        // slot of the event pool; -1: it exists under gates only
    constexpr uint64_t bit() const { return 1ull << flag; }
};
namespace dep {
constexpr Dep start{0, 0};             // main -> aux (or aux -> main, upload_on_aux): the step's uploads are done
constexpr Dep fwd{1, 1};               // main -> head streams: stacked forward done
constexpr Dep main_heads{10, 2};       // main -> helper: input halves of main's own heads done
constexpr Dep l0{35, 3};               // main -> aux / exchange stream: past layer 0's eps sum
constexpr Dep bwd_done{36, 4};         // main -> exchange stream: backward done
constexpr Dep aux_done{37, 5};         // aux -> main: everything aux did for this step is done (event: its last work, the running statistics)
//            flag 38                     exchange stream -> main: set by the caller after its last unpack (dist.OverlappedGradSync)
constexpr Dep fwd_fork{39, 6};         // main -> the other forward streams: encoders done (split forward)
constexpr Dep wg1_done{42, -1};        // second weight-gradient stream -> main: everything it did for this step is done
constexpr Dep csr{43, 7};              // aux -> main: the batch's CSR / CSC are built
constexpr Dep lp_csr{44, 8};           // aux -> the link-prediction head's stream: the decoder pairs' CSR is built
constexpr Dep heads_done{-1, 9};       // main -> exchange stream: every head's input half is joined (events; under gates head_params says more)
constexpr int EV_HEAD_IN = 10, EV_HEAD_PARAMS = EV_HEAD_IN + MAXT, EV_FWD_JOIN = EV_HEAD_PARAMS + MAXT + 1, EV_LAYER = EV_FWD_JOIN + 2;
constexpr Dep head_in(int ti) { return {2 + ti, EV_HEAD_IN + ti}; }               // head stream -> main: input-gradient half done
constexpr Dep head_params(int ti) { return {26 + ti, EV_HEAD_PARAMS + ti}; }      // weight-gradient GEMMs done; ti = MAXT: the heads of the main stream
constexpr Dep fwd_join(int k) { return {40 + k, EV_FWD_JOIN + k}; }               // k = 0, 1: forward stream 1 + k -> main: its row range is done
constexpr Dep gu_ready(int l) { return {11 + 2 * l, EV_LAYER + 4 * l}; }          // main -> aux: g_u of the layer ready
constexpr Dep gz1_ready(int l) { return {12 + 2 * l, EV_LAYER + 4 * l + 2}; }     // main -> weight-gradient stream: g_z1 of the layer ready
constexpr Dep dw2_done(int l) { return {-1, EV_LAYER + 4 * l + 1}; }              // aux -> main: dW2 of the layer done (events)
constexpr Dep aux_layer(int l) { return {21 + l, EV_LAYER + 4 * l + 3}; }         // aux -> main / exchange stream: the layer's weight gradients are final
}  // namespace dep
constexpr int NEV = dep::EV_LAYER + 4 * LAYERS;
constexpr int F_ERR = 63;              // a gate timed out

struct SyncState {                     // what gmp_step_wait_grads needs from the most recent step
    int32_t* flags = nullptr;
    int epoch = 0;
    uint64_t head_params_mask = 0;
};
SyncState g_sync;

// switches read once per process: GMP_STEP_WG1=0 (no second weight-gradient stream), GMP_STEP_LANES=0 (one enqueue thread), GMP_STEP_TIMING (phase timing)
bool env_is_zero(const char* name) { return getenv(name) && atoi(getenv(name)) == 0; }
bool wg1_enabled() { static const bool on = !env_is_zero("GMP_STEP_WG1"); return on; }
bool lanes_enabled() { static const bool on = !env_is_zero("GMP_STEP_LANES"); return on; }
bool phase_timing() { static const bool on = getenv("GMP_STEP_TIMING") != nullptr; return on; }

template <int POOL, int N>
hipEvent_t* event_pool(unsigned flags) {   // one process drives one engine: small static pools of events, made at first use
    static hipEvent_t ev[N];
    static bool made = false;
    if (!made) {
        for (int i = 0; i < N; ++i) (void)hipEventCreateWithFlags(&ev[i], flags);
        made = true;
    }
    return ev;
}
hipEvent_t* events() { return event_pool<0, NEV>(hipEventDisableTiming); }      // the dependencies' (Dep::ev)
// phase timing (diagnostic, GMP_STEP_TIMING=1): events on the main stream at step start / forward done / heads joined /
// backward done, read back by gmp_step_phase_ms
hipEvent_t* phase_events() { return event_pool<1, GMP_STEP_PHASES + 1>(hipEventDefault); }
// (diagnostic) per head: its stream at the start of the head, after the input-gradient half, after the weight-gradient half; all against
// the main stream's "forward done" event
hipEvent_t* head_events() { return event_pool<2, 3 * GMP_STEP_MAX_TASKS>(hipEventDefault); }
int g_head_tasks = 0;
bool g_head_recorded[3 * GMP_STEP_MAX_TASKS] = {false};

gmp_bn_config bn_cfg(const gmp_step_desc& d, bool relu, bool dropout, uint32_t site) {
    gmp_bn_config c{};
    c.training = d.training;
    c.relu = relu;
    c.eps = 1e-5f;
    c.momentum = 0.1f;
    c.dropout_p = (dropout && d.training) ? d.dropout_p : 0.f;
    c.seed = d.seed;
    c.stream_id = site;
    c.seed_dev = nullptr;
    return c;
}

int gemm(int mode, const float* A, const float* B, const float* bias, float* C, int64_t M, int64_t N, int64_t K, int64_t lda,
         int64_t ldb, int64_t ldc, bool relu, gmp_stream_t st) {
    return gmp_gemm_f32(mode, A, B, bias, C, M, N, K, lda, ldb, ldc, 1.f, 0, relu ? 1 : 0, nullptr, 0, st);
}

// GMP_LP_FUSED (read per call: one process can interleave A/B rounds): 0 = the link-prediction head keeps its materialised K x 768 matrices
// everywhere; 1 (default) = the input gradient is folded inside its GEMM (lp_gfeat is not written: 1.335 -> 1.318 ms per step); 2 = the
// forward and weight-gradient GEMMs generate lp_feat in their loaders as well (no K x 768 matrix at all, two launches less -- and, as
// measured, SLOWER: 1.359 ms, the generated-operand GEMMs take 97 and 156 us against 66 + 14 and 88; profiles/README.md).  Same bits at every level.
int lp_fused_level() {
    const char* e = getenv("GMP_LP_FUSED");
    return e ? atoi(e) : 1;
}

// one answer for the forward (task_head_inputs) and the weight gradient (task_head_params) of a step: both generate the features or neither does
bool lp_feat_generated(const gmp_step_desc& d, const gmp_task_desc& t) {
    return lp_fused_level() >= 2 && gmp::lp_feat_gemm_applies(d.h[GMP_STEP_LAYERS], d.flat + t.one_off_w0, d.flat + t.one_off_b0, t.lp_y1, t.lp_gy1,
                                                   d.task_grads + t.one_tg_w0, t.gemm_ws, t.lp_K, H);
}

// dropout(src) -> dst, or alias src when dropout is off; returns the buffer holding the result
float* drop(const gmp_step_desc& d, float* src, float* dst, int64_t numel, uint32_t site, gmp_stream_t st, int* rc) {
    *rc = GMP_OK;
    if (!d.training || d.dropout_p <= 0.f) return src;
    *rc = gmp_dropout_fwd(src, dst, numel, d.dropout_p, d.seed, site, st);
    return dst;
}

int mlp2_fwd(const gmp_step_desc& d, const gmp_task_desc& t, float** d1_out, gmp_stream_t st) {
    const gmp_mlp2& m = t.mlp;
    const int G = d.num_domains;
    GMP_TRY(gmp_gemm_f32_grouped(GMP_GEMM_NT, m.x, d.flat, d.flat, m.y1, G, m.rows, m.off_w0, m.off_b0, nullptr, nullptr, nullptr, 0,
                                 m.k_hid, m.k_in, m.k_in, m.k_in, m.k_hid, 1.f, 0, 1, nullptr, 0, st));
    int rc;
    float* d1 = drop(d, m.y1, m.d1, (int64_t)m.rows[G] * m.k_hid, m.site, st, &rc);
    GMP_TRY(rc);
    GMP_TRY(gmp_gemm_f32_grouped(GMP_GEMM_NT, d1, d.flat, d.flat, m.y2, G, m.rows, m.off_w3, m.off_b3, nullptr, nullptr, nullptr, 0,
                                 m.k_out, m.k_hid, m.k_hid, m.k_hid, m.k_out, 1.f, 0, 0, nullptr, 0, st));
    *d1_out = d1;
    return GMP_OK;
}

// Backward of the two-layer head, in two halves: the input-gradient chain (what the stacked backward waits for) and the two
// weight-gradient GEMMs (they only feed task_grads).  mlp2_bwd_params reads g_out, d1, g_hid (after the ReLU/dropout gate) and x,
// none of which the input chain overwrites, so it may run after it.
int mlp2_bwd_inputs(const gmp_step_desc& d, const gmp_task_desc& t, gmp_stream_t st) {
    const gmp_mlp2& m = t.mlp;
    const int G = d.num_domains;
    GMP_TRY(gmp_gemm_f32_grouped(GMP_GEMM_NN, m.g_out, d.flat, nullptr, m.g_hid, G, m.rows, m.off_w3, nullptr, nullptr, nullptr, nullptr, 0,
                                 m.k_hid, m.k_out, m.k_out, m.k_hid, m.k_hid, 1.f, 0, 0, nullptr, 0, st));
    GMP_TRY(gmp_relu_dropout_bwd(m.g_hid, m.y1, m.g_hid, (int64_t)m.rows[G] * m.k_hid, d.training ? d.dropout_p : 0.f, d.seed, m.site, st));
    GMP_TRY(gmp_gemm_f32_grouped(GMP_GEMM_NN, m.g_hid, d.flat, nullptr, m.g_in, G, m.rows, m.off_w0, nullptr, nullptr, nullptr, nullptr, 0,
                                 m.k_in, m.k_hid, m.k_hid, m.k_in, m.k_in, 1.f, 0, 0, nullptr, 0, st));
    return GMP_OK;
}

int mlp2_bwd_params(const gmp_step_desc& d, const gmp_task_desc& t, float* d1, gmp_stream_t st) {
    const gmp_mlp2& m = t.mlp;
    const int G = d.num_domains;
    float* tg = d.task_grads;
    GMP_TRY(gmp_gemm_f32_grouped(GMP_GEMM_TN, m.g_out, d1, nullptr, tg, G, m.rows, nullptr, nullptr, m.tg_w3, tg, m.tg_b3, m.k_out, m.k_hid, 0,
                                 m.k_out, m.k_hid, m.k_hid, 1.f, 0, 0, t.gemm_ws, t.gemm_ws_bytes, st));
    GMP_TRY(gmp_gemm_f32_grouped(GMP_GEMM_TN, m.g_hid, m.x, nullptr, tg, G, m.rows, nullptr, nullptr, m.tg_w0, tg, m.tg_b0, m.k_hid, m.k_in, 0,
                                 m.k_hid, m.k_in, m.k_in, 1.f, 0, 0, t.gemm_ws, t.gemm_ws_bytes, st));
    return GMP_OK;
}

int nt_xent_domains(const gmp_step_desc& d, const gmp_task_desc& t, float* z, float* gz, gmp_stream_t st) {
    int64_t off[GMP_STEP_MAX_DOMAINS];
    for (int di = 0; di < d.num_domains; ++di) off[di] = t.mlp.rows[di];
    return gmp_nt_xent_grouped(z, gz, d.num_domains, t.ntx_n, off, 128, t.temperature, t.g_scale, t.ntx_sums, t.loss_sum, t.ntx_ws,
                               t.ntx_ws_bytes, st);
}

// A task head in two halves.  task_head_inputs: forward, loss, and the gradient with respect to the backbone output (added into
// gA) -- what the stacked backward waits for.  task_head_params: the head's own weight-gradient GEMMs, which only feed
// task_grads: on a stream of its own they run beside the first layers of the stacked backward instead of in front of it.
int task_head_inputs(const gmp_step_desc& d, int ti, gmp_stream_t st, float** d1_out) {
    const gmp_task_desc& t = d.task[ti];
    const gmp_mlp2& m = t.mlp;
    const int64_t N = d.N;
    float* hL = d.h[GMP_STEP_LAYERS];
    float* gH = d.gA;
    float* d1 = nullptr;
    switch (t.kind) {
        case GMP_TASK_NFM: {
            const int64_t M = t.num_idx;
            if (M == 0) return GMP_OK;
            GMP_TRY(gmp_row_gather(hL, t.idx, nullptr, m.x, M, N, H, st));
            GMP_TRY(mlp2_fwd(d, t, &d1, st));
            GMP_TRY(gmp_mse_sum_bwd(m.y2, t.nfm_target, t.g_scale, m.g_out, M * H, st));
            GMP_TRY(mlp2_bwd_inputs(d, t, st));
            *d1_out = d1;
            return gmp_row_fill(gH, t.idx, m.g_in, M, N, H, 0, st);
        }
        case GMP_TASK_LP: {
            const int64_t K = t.lp_K;
            const float *w0 = d.flat + t.one_off_w0, *b0 = d.flat + t.one_off_b0, *w3 = d.flat + t.one_off_w3, *b3 = d.flat + t.one_off_b3;
            // the K x 768 edge features are generated inside the 768 -> 256 GEMM's loader where it and the weight-gradient GEMM (task_head_params asks
            // the same question) run the pipelined kernel: same bits, lp_feat is not written; else the feature pass and the GEMM over it
            if (lp_feat_generated(d, t)) {
                GMP_TRY(gmp_lp_feat_gemm_fwd(hL, t.lp_edges, w0, b0, t.lp_y1, N, K, H, st));
            } else {
                GMP_TRY(gmp_lp_edge_features_fwd(hL, t.lp_edges, t.lp_feat, N, K, H, st));
                GMP_TRY(gemm(GMP_GEMM_NT, t.lp_feat, w0, b0, t.lp_y1, K, H, 3 * H, 3 * H, 3 * H, H, true, st));
            }
            // the 256 -> 1 layer: a dot product per row with the dropout in the same pass, and its input gradient as an outer product
            // pushed through the dropout and the ReLU (gmp_dropout_rowdot_fwd / gmp_outer_relu_dropout_bwd: no N = 1 GEMM launches)
            const float pdrop = d.training && d.dropout_p > 0.f ? d.dropout_p : 0.f;
            float* ld1 = pdrop > 0.f ? t.lp_d1 : t.lp_y1;
            if (t.lp_pos) {       // merged rows (one per unordered pair): a dropout mask, a score and a BCE term per ORDERED row (gnnmp.h gmp_lp_pair_*)
                GMP_TRY(gmp_lp_pair_rowdot_fwd(t.lp_y1, w3, b3, t.lp_pos, t.lp_y2, K, H, pdrop, d.seed, t.one_site, st));
                GMP_TRY(gmp_lp_pair_sigmoid_bce_fwd_bwd(t.lp_y2, t.lp_labels, t.lp_pos, K, t.g_scale, t.loss_sum, t.lp_p, t.lp_gy2, t.loss_ws, t.loss_ws_bytes, st));
                *d1_out = t.lp_y1;
                GMP_TRY(gmp_lp_pair_outer_bwd(t.lp_gy2, w3, t.lp_y1, t.lp_pos, t.lp_gy1, K, H, pdrop, d.seed, t.one_site, st));
            } else {
                GMP_TRY(gmp_dropout_rowdot_fwd(t.lp_y1, w3, b3, t.lp_d1, t.lp_y2, K, H, pdrop, d.seed, t.one_site, st));
                GMP_TRY(gmp_sigmoid_bce_signed_sum_fwd_bwd(t.lp_y2, t.lp_labels, K, t.g_scale, t.loss_sum, t.lp_p, t.lp_gy2, t.loss_ws, t.loss_ws_bytes, st));
                *d1_out = ld1;
                GMP_TRY(gmp_outer_relu_dropout_bwd(t.lp_gy2, w3, t.lp_y1, t.lp_gy1, K, H, pdrop, d.seed, t.one_site, st));
            }
            // g_hs / g_hd: one launch that never writes the K x 768 gradient where the pipelined GEMM applies (same bits), else the GEMM and the fold
            if (lp_fused_level() >= 1 && gmp::lp_fold_applies(t.lp_gy1, w0, hL, t.lp_ghs, t.lp_ghd, K, H)) {
                GMP_TRY(gmp_lp_feat_gemm_bwd_fold(t.lp_gy1, w0, hL, t.lp_edges, t.lp_ghs, t.lp_ghd, N, K, H, st));
            } else {
                GMP_TRY(gemm(GMP_GEMM_NN, t.lp_gy1, w0, nullptr, t.lp_gfeat, K, 3 * H, H, H, 3 * H, 3 * H, false, st));
                GMP_TRY(gmp_lp_edge_features_bwd(t.lp_gfeat, hL, t.lp_edges, t.lp_ghs, t.lp_ghd, N, K, H, st));
            }
            float* g_rows = gH + (int64_t)H * t.row0;
            GMP_TRY(gmp_segment_sum(t.lp_ghs, d.lp_csr[3] + t.row0, d.lp_csr[5], g_rows, t.row1 - t.row0, H, 0, 1, st));
            return gmp_segment_sum(t.lp_ghd, d.lp_csr[0] + t.row0, d.lp_csr[2], g_rows, t.row1 - t.row0, H, 0, 1, st);
        }
        case GMP_TASK_NC: {
            const int64_t M = t.num_idx;
            if (M == 0) return GMP_OK;
            GMP_TRY(gmp_row_gather(hL, t.idx, nullptr, m.x, M, N, H, st));
            GMP_TRY(mlp2_fwd(d, t, &d1, st));
            GMP_TRY(nt_xent_domains(d, t, m.y2, m.g_out, st));
            GMP_TRY(mlp2_bwd_inputs(d, t, st));
            *d1_out = d1;
            return gmp_row_fill(gH, t.idx, m.g_in, M, N, H, 0, st);
        }
        case GMP_TASK_GC: {
            const int B = t.pool_B;
            if (B == 0) return GMP_OK;
            GMP_TRY(gmp_segment_sum(hL, t.pool_ptr, nullptr, t.pool_mean, B, H, 1, 0, st));
            GMP_TRY(gmp_segment_max_fwd(hL, t.pool_ptr, t.pool_max, B, H, st));
            // [mean | max] -> x [B, 512]
            if (hipMemcpy2DAsync(m.x, 2 * H * sizeof(float), t.pool_mean, H * sizeof(float), H * sizeof(float), B, hipMemcpyDeviceToDevice,
                                 (hipStream_t)st) != hipSuccess ||
                hipMemcpy2DAsync(m.x + H, 2 * H * sizeof(float), t.pool_max, H * sizeof(float), H * sizeof(float), B, hipMemcpyDeviceToDevice,
                                 (hipStream_t)st) != hipSuccess)
                return gmp::fail(GMP_ERR_LAUNCH, "step: read-out concat copy failed");
            GMP_TRY(mlp2_fwd(d, t, &d1, st));
            GMP_TRY(nt_xent_domains(d, t, m.y2, m.g_out, st));
            GMP_TRY(mlp2_bwd_inputs(d, t, st));
            *d1_out = d1;
            if (hipMemcpy2DAsync(t.g_mean, H * sizeof(float), m.g_in, 2 * H * sizeof(float), H * sizeof(float), B, hipMemcpyDeviceToDevice,
                                 (hipStream_t)st) != hipSuccess ||
                hipMemcpy2DAsync(t.g_max, H * sizeof(float), m.g_in + H, 2 * H * sizeof(float), H * sizeof(float), B, hipMemcpyDeviceToDevice,
                                 (hipStream_t)st) != hipSuccess)
                return gmp::fail(GMP_ERR_LAUNCH, "step: read-out split copy failed");
            GMP_TRY(gmp_row_gather(t.g_mean, t.pool_gid, t.pool_ptr, gH + (int64_t)H * t.pool_r0, t.pool_M, B, H, st));
            return gmp_segment_max_bwd(t.g_max, hL, t.pool_max, t.pool_ptr, gH, B, H, 1, st);
        }
        case GMP_TASK_GP: {
            const int B = t.pool_B;
            GMP_TRY(gmp_segment_sum(hL, t.pool_ptr, nullptr, m.x, B, H, 1, 0, st));
            GMP_TRY(mlp2_fwd(d, t, &d1, st));
            GMP_TRY(gmp_mse_sum_bwd(m.y2, t.labels, t.g_scale, m.g_out, (int64_t)B * m.k_out, st));
            GMP_TRY(mlp2_bwd_inputs(d, t, st));
            *d1_out = d1;
            return gmp_row_gather(m.g_in, t.pool_gid, t.pool_ptr, gH + (int64_t)H * t.pool_r0, t.pool_M, B, H, st);
        }
        case GMP_TASK_DA: {
            const int B = t.pool_B, Hd = t.da_hidden, Cc = t.da_classes;
            const float *w0 = d.flat + t.one_off_w0, *b0 = d.flat + t.one_off_b0, *w3 = d.flat + t.one_off_w3, *b3 = d.flat + t.one_off_b3;
            const float pdrop = d.training ? t.da_dropout : 0.f;
            GMP_TRY(gmp_segment_sum(hL, t.pool_ptr, nullptr, m.x, B, H, 1, 0, st));
            GMP_TRY(gemm(GMP_GEMM_NT, m.x, w0, b0, m.y1, B, Hd, H, H, H, Hd, true, st));
            float* dd1 = m.y1;
            if (pdrop > 0.f) {
                GMP_TRY(gmp_dropout_fwd(m.y1, m.d1, (int64_t)B * Hd, pdrop, d.seed, t.one_site, st));
                dd1 = m.d1;
            }
            GMP_TRY(gemm(GMP_GEMM_NT, dd1, w3, b3, m.y2, B, Cc, Hd, Hd, Hd, Cc, false, st));
            GMP_TRY(gmp_cross_entropy_sum_fwd(m.y2, t.da_labels, B, Cc, t.loss_sum, t.loss_ws, t.loss_ws_bytes, st));
            GMP_TRY(gmp_cross_entropy_sum_bwd(m.y2, t.da_labels, B, Cc, t.g_scale, m.g_out, st));
            *d1_out = dd1;
            GMP_TRY(gemm(GMP_GEMM_NN, m.g_out, w3, nullptr, m.g_hid, B, Hd, Cc, Cc, Hd, Hd, false, st));
            GMP_TRY(gmp_relu_dropout_bwd(m.g_hid, m.y1, m.g_hid, (int64_t)B * Hd, pdrop, d.seed, t.one_site, st));
            // gradient reversal: d/d pooled = -lambda * (g_hid W0)
            GMP_TRY(gmp_gemm_f32(GMP_GEMM_NN, m.g_hid, w0, nullptr, m.g_in, B, H, Hd, Hd, H, H, -t.da_lambda, 0, 0, nullptr, 0, st));
            return gmp_row_gather(m.g_in, t.pool_gid, t.pool_ptr, gH + (int64_t)H * t.pool_r0, t.pool_M, B, H, st);
        }
        default:
            return gmp::fail(GMP_ERR_ARG, "step: unknown task kind %d", t.kind);
    }
}

int task_head_params(const gmp_step_desc& d, int ti, gmp_stream_t st, float* d1) {
    const gmp_task_desc& t = d.task[ti];
    const gmp_mlp2& m = t.mlp;
    float* tg = d.task_grads;
    switch (t.kind) {
        case GMP_TASK_NFM:      // the loss VALUE (two launches, reporting only) is not on the chain the backward waits for
            if (t.num_idx == 0) return GMP_OK;
            GMP_TRY(mlp2_bwd_params(d, t, d1, st));
            return gmp_mse_sum_fwd(m.y2, t.nfm_target, t.num_idx * H, t.loss_sum, t.loss_ws, t.loss_ws_bytes, st);
        case GMP_TASK_NC:
            if (t.num_idx == 0) return GMP_OK;
            return mlp2_bwd_params(d, t, d1, st);
        case GMP_TASK_GC:
            if (t.pool_B == 0) return GMP_OK;
            return mlp2_bwd_params(d, t, d1, st);
        case GMP_TASK_GP:
            GMP_TRY(mlp2_bwd_params(d, t, d1, st));
            return gmp_mse_sum_fwd(m.y2, t.labels, (int64_t)t.pool_B * m.k_out, t.loss_sum, t.loss_ws, t.loss_ws_bytes, st);
        case GMP_TASK_LP: {
            const int64_t K = t.lp_K;
            const int32_t one[2] = {0, (int32_t)K};
            const int64_t cw0[1] = {t.one_tg_w0}, cb0[1] = {t.one_tg_b0};
            // dW0 with db0 riding along (column sums of the A tile already in LDS); first: this GEMM carries the "input half done" signal
            // (with the features generated in its B loader where the forward did not write lp_feat: still "the next GEMM" of this thread for the signal)
            if (lp_feat_generated(d, t))
                GMP_TRY(gmp_lp_feat_gemm_wgrad(t.lp_gy1, d.h[GMP_STEP_LAYERS], t.lp_edges, tg + t.one_tg_w0, tg + t.one_tg_b0, d.N, K, H, t.gemm_ws, t.gemm_ws_bytes, st));
            else
                GMP_TRY(gmp_gemm_f32_grouped(GMP_GEMM_TN, t.lp_gy1, t.lp_feat, nullptr, tg, 1, one, nullptr, nullptr, cw0, tg, cb0, H, 3 * H, 0, H, 3 * H, 3 * H,
                                             1.f, 0, 0, t.gemm_ws, t.gemm_ws_bytes, st));
            // dW3 [1, 256] and db3: a weighted column sum (the grouped GEMM path took 54 us for these 257 numbers)
            if (t.lp_pos)
                return gmp_lp_pair_weighted_colsum(t.lp_gy2, t.lp_y1, t.lp_pos, tg + t.one_tg_w3, tg + t.one_tg_b3, K, H,
                                                   d.training && d.dropout_p > 0.f ? d.dropout_p : 0.f, d.seed, t.one_site, t.gemm_ws, t.gemm_ws_bytes, st);
            return gmp_weighted_colsum(t.lp_gy2, d1, tg + t.one_tg_w3, tg + t.one_tg_b3, K, H, t.gemm_ws, t.gemm_ws_bytes, st);
        }
        case GMP_TASK_DA: {
            const int B = t.pool_B, Hd = t.da_hidden, Cc = t.da_classes;
            const int32_t one[2] = {0, B};
            const int64_t cw3[1] = {t.one_tg_w3}, cb3[1] = {t.one_tg_b3}, cw0[1] = {t.one_tg_w0}, cb0[1] = {t.one_tg_b0};
            GMP_TRY(gmp_gemm_f32_grouped(GMP_GEMM_TN, m.g_out, d1, nullptr, tg, 1, one, nullptr, nullptr, cw3, tg, cb3, Cc, Hd, 0, Cc, Hd, Hd, 1.f, 0, 0,
                                         nullptr, 0, st));
            return gmp_gemm_f32_grouped(GMP_GEMM_TN, m.g_hid, m.x, nullptr, tg, 1, one, nullptr, nullptr, cw0, tg, cb0, Hd, H, 0, Hd, H, H, 1.f, 0, 0,
                                        nullptr, 0, st);
        }
        default:
            return gmp::fail(GMP_ERR_ARG, "step: unknown task kind %d", t.kind);
    }
}

}  // namespace

extern "C" size_t gmp_step_desc_size(void) { return sizeof(gmp_step_desc); }

namespace {

struct Range { int s0, s1; int64_t r0, r1; hipStream_t st; void* ws; };      // segments, rows, stream and BatchNorm scratch of one forward range

// One walk of the step's launch sequence: what every phase reads, and what the phases hand to each other.
// `lanes`: the sequence is being walked by two host threads at once (gnnmp_internal.h lane filter: each skips the launches on streams it does
// not take).
struct StepCtx {
    const gmp_step_desc& d;
    const hipStream_t main, aux;
    const gmp_stream_t* const task_streams;
    const bool gates;                  // cross-stream dependencies by gates (the caller passed flags: streams on different hardware queues), else events
    const bool lanes, timing;
    const bool defer;                  // training: the running statistics are brought up to date at the end of the step on the aux stream
    hipEvent_t* const ev = events();
    const size_t bn_slice;             // one BatchNorm's scratch; d.bn_ws holds 2 * LAYERS + 1 of them (check_desc)
    SyncState sync;
    // ---- what the phases hand to each other
    Range ranges[3];                   // forward
    int nranges = 1;
    float* head_d1[MAXT] = {nullptr};  // heads: the hidden activation (after dropout) each head's weight-gradient half reads
    hipStream_t helper;                //   the stream that runs the weight-gradient halves of main's own heads
    bool main_heads = false;
    hipStream_t wg1;                   // backward: the stream of the dW1 GEMMs (aux, or a head stream: plan_weight_gradients)
    void *wg1_ws, *enc_ws;             //   gemm_ws in parts: aux | wg1, if there are two | encoder backward on main (no join between them)
    size_t wg_ws_bytes, enc_ws_bytes;
    float* gcur;                       //   gradient w.r.t. the output of the layer the backward has reached

    StepCtx(const gmp_step_desc& d_, gmp_stream_t main_, const gmp_stream_t* ts, gmp_stream_t aux_, bool lanes_)
        : d(d_), main((hipStream_t)main_), aux((hipStream_t)aux_), task_streams(ts), gates(d_.sync_flags != nullptr), lanes(lanes_),
          timing(phase_timing()), defer(d_.training != 0), bn_slice(gmp_bn_workspace_bytes(d_.N, 2 * H, d_.S, d_.max_seg)),
          helper(main), wg1(aux), gcur(d_.gA) {
        sync.flags = gates ? d.sync_flags : nullptr;
        sync.epoch = d.epoch;
    }
    hipStream_t head_stream(int ti) const { return (hipStream_t)task_streams[ti]; }
    void* slice(int i) const { return (char*)d.bn_ws + bn_slice * (size_t)i; }        // 0: encoder BatchNorm, 1 + 2 l / 2 + 2 l: layer l's second / first
    bool two_wg() const { return wg1 != aux; }
    // Training with gates: the eps gradient of layer l (a 5 us sum over rowdot that only feeds task_grads) runs on aux at the start of aux's
    // layer l-1 work -- the flag aux waits for there is set after main's aggregation backward of layer l -- from a rowdot slice per layer;
    // layer 0's goes to aux's tail.
    bool eps_on_aux() const { return gates && defer && aux != main; }

    int open(Dep x, hipStream_t s) const { return gmp_gate_open(d.sync_flags + x.flag, d.epoch, s); }
    int record(Dep x, hipStream_t s) const { (void)hipEventRecord(ev[x.ev], s); return GMP_OK; }
    int wait_event(Dep x, hipStream_t s) const { (void)hipStreamWaitEvent(s, ev[x.ev], 0); return GMP_OK; }
    int await_flags(uint64_t mask, hipStream_t s) const { return gmp_gate_wait(d.sync_flags, mask, d.epoch, d.sync_flags + F_ERR, s); }   // one sleeping wave
    int signal(Dep x, hipStream_t s) const { return gates ? (x.flag < 0 ? GMP_OK : open(x, s)) : (x.ev < 0 ? GMP_OK : record(x, s)); }
    int await(Dep x, hipStream_t s) const { return gates ? await_flags(x.bit(), s) : wait_event(x, s); }
    // signal carried by the NEXT GEMM launched from this thread (it must be on stream s and follow immediately in host order):
    // saves the one-thread launch on a critical chain; signal_flush opens the gate itself if that GEMM turned out to be empty
    void signal_by_gemm(Dep x, hipStream_t s) const {
        if (!gates) (void)record(x, s);
        else if (gmp::lane_takes(s)) gmp::signal_on_next_gemm(d.sync_flags + x.flag, d.epoch);      // (the GEMM that carries it is this thread's to launch)
    }
    int signal_flush(Dep x, hipStream_t s) const {
        if (!gates || !gmp::lane_takes(s) || !gmp::signal_pending()) return GMP_OK;
        gmp::signal_on_next_gemm(nullptr, 0);
        return open(x, s);
    }
    // The two CSR dependencies stay events even under gates -- unless two host threads walk the step: an event recorded by one host thread
    // cannot be waited on by the other
    int signal_csr(Dep x) const { return lanes ? open(x, aux) : record(x, aux); }
    int await_csr(Dep x, hipStream_t s) const { return lanes ? await_flags(x.bit(), s) : wait_event(x, s); }
};

// What the engine always passes and the executor relies on; checked before any event or stream is touched.
int check_desc(const gmp_step_desc& d) {
    if (d.hidden != H || d.num_tasks < 1 || d.num_tasks > MAXT || d.num_domains < 1 || d.num_domains > GMP_STEP_MAX_DOMAINS || d.N <= 0 || d.S <= 0 ||
        d.enc_groups < 0 || d.enc_groups > GMP_STEP_MAX_ENC_GROUPS)
        return gmp::fail(GMP_ERR_ARG, "step: bad sizes (N=%d S=%d tasks=%d domains=%d hidden=%d)", d.N, d.S, d.num_tasks, d.num_domains, d.hidden);
    for (int l = 0; l < LAYERS; ++l)
        if (!d.gu_l[l] || !d.gz1_l[l]) return gmp::fail(GMP_ERR_ARG, "step: gu_l[%d] / gz1_l[%d] is NULL (the per-layer gradient buffers are required)", l, l);
    if (!d.rowdot) return gmp::fail(GMP_ERR_ARG, "step: rowdot is NULL (%d slices of N floats are required)", LAYERS);
    // (gmp_bn_workspace_bytes grows with S and max_seg: a workspace sized for the largest step holds every step)
    const size_t need = (2 * LAYERS + 1) * gmp_bn_workspace_bytes(d.N, 2 * H, d.S, d.max_seg);
    if (!d.bn_ws || d.bn_ws_bytes < need)
        return gmp::fail(GMP_ERR_WORKSPACE, "step: bn_ws holds %zu bytes, a slice per BatchNorm (%d) takes %zu", d.bn_ws_bytes, 2 * LAYERS + 1, need);
    return GMP_OK;
}

// ---- graph structure: the two CSR builds on aux, beside the encoders (they only need the uploaded indices)
int graph_structure(StepCtx& c) {
    const gmp_step_desc& d = c.d;
    const bool up_aux = d.upload_on_aux && c.aux != c.main;      // the uploads came up on aux (in order there): main is the one that waits
    GMP_TRY(c.signal(dep::start, up_aux ? c.aux : c.main));
    GMP_TRY(c.await(dep::start, up_aux ? c.main : c.aux));
    if (d.max_seg <= 8192 && d.max_seg_edges <= 24576)      // block diagonal: one workgroup per (segment, orientation)
        GMP_TRY(gmp_csr_build_segmented(d.edge_index, d.N, d.E, d.seg_ptr, d.seg_eptr, d.S, d.max_seg, d.max_seg_edges, d.csr[0], d.csr[1], d.csr[2], d.csr[3],
                                        d.csr[4], d.csr[5], d.csr_status, c.aux));
    else
        GMP_TRY(gmp_csr_build(d.edge_index, d.N, d.E, d.csr[0], d.csr[1], d.csr[2], d.csr[3], d.csr[4], d.csr[5], d.csr_status, d.csr_ws, d.csr_ws_bytes, c.aux));
    GMP_TRY(c.signal_csr(dep::csr));
    int lp_task = -1;
    for (int ti = 0; ti < d.num_tasks; ++ti)
        if (d.task[ti].kind == GMP_TASK_LP) lp_task = ti;
    if (lp_task >= 0) {
        const gmp_task_desc& t = d.task[lp_task];
        if (d.lp_S > 0)
            GMP_TRY(gmp_csr_build_segmented(t.lp_edges, d.lp_rows_end, t.lp_K, d.lp_seg_ptr, d.lp_seg_eptr, d.lp_S, d.lp_max_seg_rows, d.lp_max_seg_edges,
                                            d.lp_csr[0], d.lp_csr[1], d.lp_csr[2], d.lp_csr[3], d.lp_csr[4], d.lp_csr[5], d.lp_csr_status, c.aux));
        else
            GMP_TRY(gmp_csr_build(t.lp_edges, d.N, t.lp_K, d.lp_csr[0], d.lp_csr[1], d.lp_csr[2], d.lp_csr[3], d.lp_csr[4], d.lp_csr[5], d.lp_csr_status,
                                  d.lp_csr_ws, d.lp_csr_ws_bytes, c.aux));
    }
    return c.signal_csr(dep::lp_csr);
}

// ---- input encoders, their BatchNorm, the NFM mask; main then waits for the CSR
int encoders(StepCtx& c) {
    const gmp_step_desc& d = c.d;
    GMP_TRY(gmp_encoder_fwd(d.x_all, d.x_rows, d.N, d.S, d.src_row, d.seg_ptr, d.seg_dom, (const uint64_t*)d.rowmask, d.tiles, d.num_tiles, d.flat,
                            d.num_domains, d.enc_off_w, d.enc_off_b, d.enc_d_in, d.dpad, d.z0, c.main));
    gmp_bn_config bc = bn_cfg(d, true, true, 1);
    GMP_TRY(gmp_bn_fwd(d.z0, nullptr, d.seg_ptr, d.seg_dom, d.S, d.max_seg, d.N, H, d.flat + d.enc_off_gamma0, d.flat + d.enc_off_beta0,
                       c.defer ? nullptr : d.enc_rm, c.defer ? nullptr : d.enc_rv, d.enc_mean, d.enc_rstd, d.h[0], &bc, c.slice(0), c.bn_slice, c.main));
    if (d.nfm_task >= 0 && d.task[d.nfm_task].num_idx > 0) {
        const gmp_task_desc& t = d.task[d.nfm_task];
        GMP_TRY(gmp_row_gather(d.h[0], t.idx, nullptr, t.nfm_target, t.num_idx, d.N, H, c.main));
        GMP_TRY(gmp_row_fill(d.h[0], t.idx, d.flat + d.off_mask_token, t.num_idx, d.N, H, 1, c.main));
    }
    GMP_TRY(c.await_csr(dep::csr, c.main));
    if (c.timing) (void)hipEventRecord(phase_events()[1], c.main);
    return GMP_OK;
}

// ---- stacked backbone forward: one pass on main, or up to three row ranges on as many streams (gnnmp_step.h fwd_cut_*)
void select_forward_ranges(StepCtx& c) {
    const gmp_step_desc& d = c.d;
    hipStream_t fwd_streams[3] = {c.main, c.main, c.main};
    int extra = 0;
    for (int ti = 0; ti < d.num_tasks && extra < 2; ++ti) {
        hipStream_t ts = c.head_stream(ti);
        if (ts != c.main && ts != c.aux && ts != fwd_streams[1]) fwd_streams[++extra] = ts;
    }
    c.ranges[0] = Range{0, d.S, 0, d.N, c.main, d.bn_ws};
    // (every range at least 1,024 rows: below that gmp_gemm_f32 runs its first kernel, whose K order differs from the pipelined one the
    // single pass uses -- the split must not change a bit -- and a step that small has nothing to hide behind anyway)
    int cuts = 0, prev_seg = 0;
    int64_t prev_row = 0;
    bool ok = d.N < 65536;
    for (int k = 0; k < 2 && ok; ++k) {
        if (d.fwd_cut_seg[k] <= 0) break;
        ok = d.fwd_cut_seg[k] > prev_seg && d.fwd_cut_seg[k] < d.S && d.fwd_cut_row[k] - prev_row >= 1024 && d.N - d.fwd_cut_row[k] >= 1024;
        prev_seg = d.fwd_cut_seg[k]; prev_row = d.fwd_cut_row[k];
        ++cuts;
    }
    if (!ok || cuts == 0 || cuts > extra) return;
    c.nranges = cuts + 1;
    for (int k = 0; k < c.nranges; ++k)       // (a BatchNorm slice each: bn_ws holds 11)
        c.ranges[k] = Range{k ? d.fwd_cut_seg[k - 1] : 0, k + 1 < c.nranges ? d.fwd_cut_seg[k] : d.S,
                            k ? d.fwd_cut_row[k - 1] : 0, k + 1 < c.nranges ? d.fwd_cut_row[k] : d.N, fwd_streams[k], c.slice(k)};
}

int stacked_forward(StepCtx& c) {
    const gmp_step_desc& d = c.d;
    const bool split = c.nranges > 1;
    if (split) {
        GMP_TRY(c.signal(dep::fwd_fork, c.main));
        for (int k = 1; k < c.nranges; ++k) GMP_TRY(c.await(dep::fwd_fork, c.ranges[k].st));
    }
    for (int l = 0; l < LAYERS; ++l) {
        const gmp_layer_desc& L = d.layer[l];
        for (int k = 0; k < c.nranges; ++k) {
            const Range& R = c.ranges[k];
            const hipStream_t st = R.st;
            const int64_t M = R.r1 - R.r0;
            const int Sk = R.s1 - R.s0;
            const int32_t* sp = d.seg_ptr + R.s0;
            if (split) GMP_TRY(gmp_gin_aggregate_fwd_rows(d.h[l], d.csr[0], d.csr[1], d.flat + L.off_eps, L.a, R.r0, R.r1, H, st));
            else GMP_TRY(gmp_gin_aggregate_fwd(d.h[l], d.csr[0], d.csr[1], d.flat + L.off_eps, L.a, d.N, H, st));
            GMP_TRY(gemm(GMP_GEMM_NT, L.a + R.r0 * H, d.flat + L.off_w1, d.flat + L.off_b1, L.z1 + R.r0 * 2 * H, M, 2 * H, H, H, H, 2 * H, false, st));
            gmp_bn_config bc = bn_cfg(d, true, false, 0);
            // (absolute row numbers in seg_ptr: the BatchNorm takes whole-batch base pointers and this range's segments)
            GMP_TRY(gmp_bn_fwd(L.z1, nullptr, sp, nullptr, Sk, d.max_seg, d.N, 2 * H, d.flat + L.off_g1, d.flat + L.off_be1, c.defer ? nullptr : L.rm1,
                               c.defer ? nullptr : L.rv1, L.m1 + (size_t)R.s0 * 2 * H, L.s1 + (size_t)R.s0 * 2 * H, L.r1, &bc, R.ws, c.bn_slice, st));
            GMP_TRY(gemm(GMP_GEMM_NT, L.r1 + R.r0 * 2 * H, d.flat + L.off_w2, d.flat + L.off_b2, L.z2 + R.r0 * H, M, H, 2 * H, 2 * H, 2 * H, H, false, st));
            bc = bn_cfg(d, true, true, 10 + l);
            GMP_TRY(gmp_bn_fwd(L.z2, d.h[l], sp, nullptr, Sk, d.max_seg, d.N, H, d.flat + L.off_g2, d.flat + L.off_be2, c.defer ? nullptr : L.rm2,
                               c.defer ? nullptr : L.rv2, L.m2 + (size_t)R.s0 * H, L.s2 + (size_t)R.s0 * H, d.h[l + 1], &bc, R.ws, c.bn_slice, st));
        }
        if (c.timing && l + 1 < LAYERS) (void)hipEventRecord(phase_events()[2 + l], c.main);
    }
    if (split) {
        for (int k = 1; k < c.nranges; ++k) GMP_TRY(c.signal(dep::fwd_join(k - 1), c.ranges[k].st));
        if (c.gates) GMP_TRY(c.await_flags(dep::fwd_join(0).bit() | (c.nranges > 2 ? dep::fwd_join(1).bit() : 0), c.main));
        else for (int k = 1; k < c.nranges; ++k) GMP_TRY(c.wait_event(dep::fwd_join(k - 1), c.main));
    }
    return GMP_OK;
}

// ---- task heads, each on its own stream, in two halves (task_head_inputs / task_head_params): main waits for the first only
int run_head(StepCtx& c, int ti) {
    const gmp_step_desc& d = c.d;
    const hipStream_t ts = c.head_stream(ti);
    if (ts != c.main) GMP_TRY(c.await(dep::fwd, ts));
    if (d.task[ti].kind == GMP_TASK_LP) GMP_TRY(c.await_csr(dep::lp_csr, ts));
    if (c.timing) { (void)hipEventRecord(head_events()[3 * ti], ts); g_head_recorded[3 * ti] = true; g_head_recorded[3 * ti + 2] = false; }
    GMP_TRY(task_head_inputs(d, ti, c.task_streams[ti], &c.head_d1[ti]));
    if (c.timing) { (void)hipEventRecord(head_events()[3 * ti + 1], ts); g_head_recorded[3 * ti + 1] = true; }
    if (ts == c.main) return c.main_heads = true, GMP_OK;      // (its weight-gradient half goes to `helper`, behind all of main's heads)
    c.signal_by_gemm(dep::head_in(ti), ts);          // the head's first weight-gradient GEMM opens main's gate
    GMP_TRY(task_head_params(d, ti, c.task_streams[ti], c.head_d1[ti]));
    GMP_TRY(c.signal_flush(dep::head_in(ti), ts));
    if (c.timing) { (void)hipEventRecord(head_events()[3 * ti + 2], ts); g_head_recorded[3 * ti + 2] = true; }
    GMP_TRY(c.signal(dep::head_params(ti), ts));     // (events: main joins these before the tail: long complete by then)
    if (c.gates) c.sync.head_params_mask |= dep::head_params(ti).bit();
    return GMP_OK;
}

int heads(StepCtx& c) {
    const gmp_step_desc& d = c.d;
    const int T = d.num_tasks;
    if (hipMemsetAsync(d.gA, 0, (size_t)d.N * H * sizeof(float), c.main) != hipSuccess) return gmp::fail(GMP_ERR_LAUNCH, "step: memset");
    GMP_TRY(c.signal(dep::fwd, c.main));
    if (c.timing) (void)hipEventRecord(phase_events()[1 + LAYERS], c.main);
    g_head_tasks = T;
    for (int ti = 0; ti < T; ++ti) {
        hipStream_t ts = c.head_stream(ti);
        if (ts != c.main && (c.helper == c.main || ts != c.aux)) c.helper = ts;     // prefer a stream the backward does not use
    }
    // heads on other streams first (their chains are the long ones: they start while main is still being fed), the ones packed onto main
    // last; main joins the other streams only after everything is enqueued.
    // (round 3: enqueueing the main stream's heads first moves THEIR start from ~100 us to 8 us after the forward and the others'
    // back by as much -- the step takes the same 1.413 ms either way)
    for (int pass = 0; pass < 2; ++pass)
        for (int ti = 0; ti < T; ++ti)
            if ((c.head_stream(ti) == c.main) == (pass == 1)) GMP_TRY(run_head(c, ti));
    if (c.main_heads) {
        if (c.helper != c.main) {
            GMP_TRY(c.signal(dep::main_heads, c.main));
            GMP_TRY(c.await(dep::main_heads, c.helper));
        }
        for (int ti = 0; ti < T; ++ti)
            if (c.head_stream(ti) == c.main) GMP_TRY(task_head_params(d, ti, c.helper, c.head_d1[ti]));
        if (c.helper != c.main) {
            GMP_TRY(c.signal(dep::head_params(MAXT), c.helper));
            if (c.gates) c.sync.head_params_mask |= dep::head_params(MAXT).bit();
        }
    }
    uint64_t mask = 0;      // gates: one sleeping wave on main for all the heads' flags
    for (int ti = 0; ti < T; ++ti) {
        if (c.head_stream(ti) == c.main) continue;
        if (c.gates) mask |= dep::head_in(ti).bit();
        else GMP_TRY(c.wait_event(dep::head_in(ti), c.main));
    }
    // (events: the decoder CSR too -- with an LP head its join implies it; without one the CSR's does)
    GMP_TRY(c.gates ? c.await_flags(mask, c.main) : c.wait_event(dep::lp_csr, c.main));
    if (d.dp_exchange) GMP_TRY(c.signal(dep::heads_done, c.main));   // (events; gmp_step_wait_grads adds the params events)
    if (c.timing) (void)hipEventRecord(phase_events()[2 + LAYERS], c.main);
    return GMP_OK;
}

// ---- stacked backbone backward: per-task parameter gradients from ONE pass.
// The input-gradient chain (BN bwd -> dgrad GEMM -> BN bwd -> dgrad GEMM -> aggregation bwd) is the critical path; the weight-gradient
// GEMMs only feed task_grads, so they run beside it on the aux stream.  g_u / g_z1 of every layer have a buffer of their own (gu_l / gz1_l):
// aux may lag main by any number of layers and main never waits for it inside the backward.  (A wait on an event that was not complete when
// it was ENQUEUED costs the waiting stream 3-4 us even when the event has long fired by the time the packet is reached --
// scripts/diag_blocked_queues.py -- and the host runs ahead.)
// BatchNorm gamma/beta gradients also only feed task_grads: each BN backward leaves its per-segment sums in its own slice of bn_ws and the
// reduction per task runs next to the weight-gradient GEMM.
//
// Two weight-gradient streams: per layer aux carries dW2 (+ the BatchNorm-2 sums, the eps sum), and a head stream -- idle once its head's
// weight gradients are out -- carries dW1 (+ the BatchNorm-1 sums).  On ONE stream the two GEMMs, their slice reductions and the sums
// add up to ~105 us per layer, as long as main's input-gradient chain (110 us).  Worth 0.8 % (1.409 -> 1.397, 1.417 -> 1.401 ms in two
// A/B pairs): the backward is bound by the chip's throughput, not by either chain ("two row ranges").
// Needs gates and a third of gemm_ws that still holds the slices (GMP_STEP_WG1=0: everything on aux).  Not in data-parallel runs: the
// exchange lives on a head stream too (engine.py comm_stream) and follows the backward layer by layer through aux's flags; behind a whole
// weight-gradient chain in the same in-order queue it would start when the backward ends.
void plan_weight_gradients(StepCtx& c) {
    const gmp_step_desc& d = c.d;
    if (c.gates && c.aux != c.main && !d.dp_exchange && d.gemm_ws_bytes >= ((size_t)36 << 20) && wg1_enabled())
        for (int pass = 0; pass < 2 && c.wg1 == c.aux; ++pass)       // not the link-prediction head's stream if there is another: its weight gradients take longest
            for (int ti = 0; ti < d.num_tasks && c.wg1 == c.aux; ++ti) {
                hipStream_t ts = c.head_stream(ti);
                if (ts != c.main && ts != c.aux && (pass == 1 || d.task[ti].kind != GMP_TASK_LP)) c.wg1 = ts;
            }
    const int parts = c.two_wg() ? 2 : 1;            // weight-gradient parts in front of the encoder backward's
    c.wg_ws_bytes = (d.gemm_ws_bytes / (parts + 1)) & ~(size_t)255;
    c.wg1_ws = (char*)d.gemm_ws + (parts - 1) * c.wg_ws_bytes;
    c.enc_ws = (char*)d.gemm_ws + parts * c.wg_ws_bytes;
    c.enc_ws_bytes = d.gemm_ws_bytes - parts * c.wg_ws_bytes;
}

int backward_layer(StepCtx& c, int l) {
    const gmp_step_desc& d = c.d;
    const gmp_layer_desc& L = d.layer[l];
    const int64_t N = d.N;
    const int T = d.num_tasks;
    float *tg = d.task_grads, *gu = d.gu_l[l], *gz1 = d.gz1_l[l];
    const bool eps_on_aux = c.eps_on_aux();
    // second half of the layer (Linear 512 -> 256, BatchNorm): g_u on main, dW2 and the BatchNorm sums on aux
    gmp_bn_config bc = bn_cfg(d, true, true, 10 + l);
    GMP_TRY(gmp_bn_bwd(c.gcur, L.z2, d.h[l], d.seg_ptr, nullptr, d.S, d.max_seg, N, H, d.flat + L.off_g2, d.flat + L.off_be2, L.rm2, L.rv2, L.m2, L.s2, gu,
                       tg, tg, d.task_seg, L.tg_g2, L.tg_be2, 0, &bc, c.slice(1 + 2 * l), c.bn_slice, c.main));
    c.signal_by_gemm(dep::gu_ready(l), c.main);              // the input-gradient GEMM below tells aux as it starts
    GMP_TRY(gemm(GMP_GEMM_NN, gu, d.flat + L.off_w2, nullptr, d.gW, N, 2 * H, H, H, 2 * H, 2 * H, false, c.main));
    GMP_TRY(c.signal_flush(dep::gu_ready(l), c.main));
    GMP_TRY(c.await(dep::gu_ready(l), c.aux));
    if (eps_on_aux && l + 1 < LAYERS) {
        GMP_TRY(gmp_group_sum_1d(d.rowdot + (size_t)(l + 1) * N, T, d.task_row, d.layer[l + 1].tg_eps, tg, c.aux));
        if (d.dp_exchange) GMP_TRY(c.signal(dep::aux_layer(l + 1), c.aux));     // layer l+1 is final now
    }
    GMP_TRY(gmp_bn_param_grads(c.slice(1 + 2 * l), d.S, H, tg, tg, d.task_seg, L.tg_g2, L.tg_be2, T, c.aux));
    GMP_TRY(gmp_gemm_f32_grouped(GMP_GEMM_TN, gu, L.r1, nullptr, tg, T, d.task_row, nullptr, nullptr, L.tg_w2, tg, L.tg_b2, H, 2 * H, 0, H, 2 * H, 2 * H,
                                 1.f, 0, 0, d.gemm_ws, c.wg_ws_bytes, c.aux));
    if (!c.gates) GMP_TRY(c.signal(dep::dw2_done(l), c.aux));      // (a record costs its stream ~3 us: only where somebody waits for it)
    // first half (Linear 256 -> 512, BatchNorm): g_z1 on main, dW1 and the BatchNorm sums on the weight-gradient stream
    bc = bn_cfg(d, true, false, 0);
    GMP_TRY(gmp_bn_bwd(d.gW, L.z1, nullptr, d.seg_ptr, nullptr, d.S, d.max_seg, N, 2 * H, d.flat + L.off_g1, d.flat + L.off_be1, L.rm1, L.rv1, L.m1,
                       L.s1, gz1, tg, tg, d.task_seg, L.tg_g1, L.tg_be1, 0, &bc, c.slice(2 + 2 * l), c.bn_slice, c.main));
    c.signal_by_gemm(dep::gz1_ready(l), c.main);
    GMP_TRY(gemm(GMP_GEMM_NN, gz1, d.flat + L.off_w1, nullptr, d.ga, N, H, 2 * H, 2 * H, H, H, false, c.main));
    GMP_TRY(c.signal_flush(dep::gz1_ready(l), c.main));
    GMP_TRY(c.await(dep::gz1_ready(l), c.wg1));
    GMP_TRY(gmp_bn_param_grads(c.slice(2 + 2 * l), d.S, 2 * H, tg, tg, d.task_seg, L.tg_g1, L.tg_be1, T, c.wg1));
    GMP_TRY(gmp_gemm_f32_grouped(GMP_GEMM_TN, gz1, L.a, nullptr, tg, T, d.task_row, nullptr, nullptr, L.tg_w1, tg, L.tg_b1, 2 * H, H, 0, 2 * H, H, H,
                                 1.f, 0, 0, c.wg1_ws, c.wg_ws_bytes, c.wg1));
    if (!c.gates || (d.dp_exchange && !eps_on_aux)) GMP_TRY(c.signal(dep::aux_layer(l), c.aux));
    // aggregation backward; the eps sum on main where aux does not take it
    float* rowdot = eps_on_aux ? d.rowdot + (size_t)l * N : d.rowdot;
    GMP_TRY(gmp_gin_aggregate_bwd_ex(d.ga, d.csr[3], d.csr[4], d.flat + L.off_eps, d.h[l], gu, c.gcur, rowdot, N, H, c.main));
    if (!eps_on_aux) GMP_TRY(gmp_group_sum_1d(rowdot, T, d.task_row, L.tg_eps, tg, c.main));
    if (c.timing) (void)hipEventRecord(phase_events()[3 + LAYERS + (LAYERS - 1 - l)], c.main);
    return GMP_OK;
}

// running statistics of the 11 BatchNorms (training never reads them): one launch on aux behind its last weight-gradient GEMM, beside the
// encoder backward and PCGrad (in front of the aux stream's head it delayed that head by 45 us)
int running_statistics(StepCtx& c) {
    const gmp_step_desc& d = c.d;
    gmp_bn_config bc = bn_cfg(d, true, false, 0);
    constexpr int NB = 2 * LAYERS + 1;
    const int32_t* sg[NB];
    int32_t ch[NB];
    float *rm[NB], *rv[NB];
    const float *sm[NB], *sr[NB];
    sg[0] = d.seg_dom; ch[0] = H; rm[0] = d.enc_rm; rv[0] = d.enc_rv; sm[0] = d.enc_mean; sr[0] = d.enc_rstd;
    for (int l = 0; l < LAYERS; ++l) {
        const gmp_layer_desc& L = d.layer[l];
        const int a = 1 + 2 * l, b = 2 + 2 * l;
        sg[a] = nullptr; ch[a] = 2 * H; rm[a] = L.rm1; rv[a] = L.rv1; sm[a] = L.m1; sr[a] = L.s1;
        sg[b] = nullptr; ch[b] = H; rm[b] = L.rm2; rv[b] = L.rv2; sm[b] = L.m2; sr[b] = L.s2;
    }
    return gmp_bn_running_update_batch(NB, d.seg_ptr, d.S, sg, ch, rm, rv, sm, sr, &bc, c.aux);
}

// ---- below the backbone: layer 0's eps sum, the mask token (NFM), the running statistics, the encoders (every task but NFM), the final join.
// Training: the mask-token sum (3 launches that only feed task_grads) goes to aux, in front of the running statistics, beside the encoder
// backward on main.
int tail(StepCtx& c) {
    const gmp_step_desc& d = c.d;
    const int T = d.num_tasks;
    float* tg = d.task_grads;
    if (!c.gates) {
        for (int l = 0; l < LAYERS && l < 2; ++l) {
            GMP_TRY(c.await(dep::dw2_done(l), c.main));
            GMP_TRY(c.await(dep::aux_layer(l), c.main));
        }
        // join the heads' weight-gradient GEMMs, which ran beside the backward (long done; the mask-token sum below reuses the
        // NFM head's input buffer, which its dW0 GEMM reads)
        for (int ti = 0; ti < T; ++ti)
            if (c.head_stream(ti) != c.main) GMP_TRY(c.await(dep::head_params(ti), c.main));
        if (c.main_heads && c.helper != c.main) GMP_TRY(c.await(dep::head_params(MAXT), c.main));
    }
    const bool nfm_tail = d.nfm_task >= 0 && d.task[d.nfm_task].num_idx > 0;
    const bool tail_on_aux = c.defer && c.aux != c.main;
    const bool eps_on_aux = c.eps_on_aux();
    if (d.dp_exchange || (tail_on_aux && nfm_tail) || eps_on_aux) GMP_TRY(c.signal(dep::l0, c.main));   // main is past layer 0
    const hipStream_t tail_st = tail_on_aux ? c.aux : c.main;
    if (c.gates) {            // one gate in front of the tail work: main past layer 0 (when the work is on aux), and the NFM head's
                              // dW0 GEMM done (it reads the buffer the mask-token sum reuses)
        uint64_t mask = 0;
        if (nfm_tail) mask = dep::head_params(c.head_stream(d.nfm_task) == c.main ? MAXT : d.nfm_task).bit() & c.sync.head_params_mask;
        if (tail_on_aux && (nfm_tail || eps_on_aux)) mask |= dep::l0.bit();
        GMP_TRY(c.await_flags(mask, tail_st));
    } else if (tail_on_aux && nfm_tail) GMP_TRY(c.await(dep::l0, c.aux));
    if (eps_on_aux) {
        GMP_TRY(gmp_group_sum_1d(d.rowdot, T, d.task_row, d.layer[0].tg_eps, tg, c.aux));
        if (d.dp_exchange) GMP_TRY(c.signal(dep::aux_layer(0), c.aux));
    }
    if (nfm_tail) {
        const gmp_task_desc& t = d.task[d.nfm_task];
        GMP_TRY(gmp_row_gather(c.gcur, t.idx, nullptr, t.mlp.x, t.num_idx, d.N, H, tail_st));
        GMP_TRY(gmp_colsum(t.mlp.x, tg + d.tg_mask_token, t.num_idx, H, H, 0, t.loss_ws, t.loss_ws_bytes, tail_st));
    }
    if (c.defer) {
        GMP_TRY(running_statistics(c));
        if (!c.gates) GMP_TRY(c.signal(dep::aux_done, c.aux));
    }
    if (c.gates && c.aux != c.main) GMP_TRY(c.signal(dep::aux_done, c.aux));
    if (c.two_wg()) GMP_TRY(c.signal(dep::wg1_done, c.wg1));
    if (d.enc_groups > 0) {
        gmp_bn_config bc = bn_cfg(d, true, true, 1);
        float* gz0 = d.gB;       // gradient w.r.t. the encoders' pre-BatchNorm output
        // (its own slice of the BatchNorm scratch: aux may still be reducing layer 0's slices)
        GMP_TRY(gmp_bn_bwd(c.gcur, d.z0, nullptr, d.seg_ptr, d.seg_dom, d.S, d.max_seg, d.N, H, d.flat + d.enc_off_gamma0, d.flat + d.enc_off_beta0, d.enc_rm,
                           d.enc_rv, d.enc_mean, d.enc_rstd, gz0, tg, tg, d.enc_gseg, d.enc_tg_gamma, d.enc_tg_beta, d.enc_groups, &bc,
                           c.slice(0), c.bn_slice, c.main));
        GMP_TRY(gmp_encoder_bwd(d.x_all, d.x_rows, d.N, d.S, d.src_row, d.seg_ptr, d.seg_dom, (const uint64_t*)d.rowmask, gz0, d.num_domains, d.enc_d_in,
                                d.dpad, d.enc_groups, d.enc_gseg, d.enc_tg_w, d.enc_tg_b, tg, c.enc_ws, c.enc_ws_bytes, c.main));
    }
    if (c.gates) {        // ONE sleeping wave joins everything that ran beside main: aux (weight gradients, mask token, running
                          // statistics) and the heads' weight-gradient GEMMs -- instead of ten event waits at 3-4 us each
        uint64_t mask = c.sync.head_params_mask;
        if (c.aux != c.main) mask |= dep::aux_done.bit();
        if (c.two_wg()) mask |= dep::wg1_done.bit();
        GMP_TRY(c.await_flags(mask, c.main));
    } else if (c.defer) GMP_TRY(c.await(dep::aux_done, c.main));   // the next step's forward overwrites the saved batch statistics they read
    if (d.dp_exchange) GMP_TRY(c.signal(dep::bwd_done, c.main));
    if (c.timing) (void)hipEventRecord(phase_events()[GMP_STEP_PHASES], c.main);
    return GMP_OK;
}

// The launch sequence of one step (the descriptor has passed check_desc).  `primary`: this thread also leaves the step's flag state behind
// for gmp_step_wait_grads.
int step_body(const gmp_step_desc* dp, gmp_stream_t main_, const gmp_stream_t* task_streams, gmp_stream_t aux_, bool lanes, bool primary) {
    StepCtx c(*dp, main_, task_streams, aux_, lanes);
    if (c.timing) (void)hipEventRecord(phase_events()[0], c.main);
    gmp::signal_on_next_gemm(nullptr, 0);           // nothing left pending by an earlier call that failed half-way
    GMP_TRY(graph_structure(c));
    GMP_TRY(encoders(c));
    select_forward_ranges(c);
    GMP_TRY(stacked_forward(c));
    GMP_TRY(heads(c));
    plan_weight_gradients(c);
    for (int l = LAYERS - 1; l >= 0; --l) GMP_TRY(backward_layer(c, l));
    GMP_TRY(tail(c));
    if (primary) g_sync = c.sync;
    return GMP_OK;
}

// ---- the second enqueue thread ---------------------------------------------------------------------------------------------------
// One worker per process, started at the first two-lane step and never joined (it sleeps on a condition variable between jobs after a short
// spin: a step arrives every ~1.4 ms).  A job is one walk of step_body with the lane filter "everything but the main stream".
struct LaneJob {
    const gmp_step_desc* d;
    gmp_stream_t main_, aux_;
    const gmp_stream_t* task_streams;
    int device;
};
class LaneWorker {
  public:
    void post(const LaneJob& j) {
        job_ = j;
        done_.store(false, std::memory_order_relaxed);
        {
            std::lock_guard<std::mutex> lk(m_);
            seq_.fetch_add(1, std::memory_order_release);
        }
        cv_.notify_one();
    }
    int wait(char* err, size_t n) {          // spin: the worker finishes within tens of microseconds of the caller's own walk
        while (!done_.load(std::memory_order_acquire)) std::this_thread::yield();
        if (rc_ && err) snprintf(err, n, "%s", err_);
        return rc_;
    }
    static LaneWorker& get() {
        static LaneWorker* w = new LaneWorker();     // leaked on purpose: the thread may outlive static destruction
        return *w;
    }

  private:
    LaneWorker() { std::thread([this] { run(); }).detach(); }
    void run() {
        unsigned seen = 0;
        for (;;) {
            // a step every ~1.4 ms: spin for a while, then sleep
            const auto t0 = std::chrono::steady_clock::now();
            while (seq_.load(std::memory_order_acquire) == seen) {
                if (std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(400)) {
                    std::unique_lock<std::mutex> lk(m_);
                    cv_.wait(lk, [&] { return seq_.load(std::memory_order_acquire) != seen; });
                    break;
                }
            }
            seen = seq_.load(std::memory_order_acquire);
            (void)hipSetDevice(job_.device);
            gmp::lane_mode() = gmp::LANE_ALL_BUT;
            gmp::lane_stream() = (hipStream_t)job_.main_;
            rc_ = step_body(job_.d, job_.main_, job_.task_streams, job_.aux_, true, false);
            if (rc_) snprintf(err_, sizeof(err_), "%s", gmp::err_buf());
            gmp::lane_mode() = gmp::LANE_ALL;
            done_.store(true, std::memory_order_release);
        }
    }
    std::mutex m_;
    std::condition_variable cv_;
    std::atomic<unsigned> seq_{0};
    std::atomic<bool> done_{true};
    LaneJob job_{};
    int rc_ = 0;
    char err_[512] = "";
};

}  // namespace
extern "C" int gmp_pretrain_step_fwd_bwd(const gmp_step_desc* dp, gmp_stream_t main_, const gmp_stream_t* task_streams, gmp_stream_t aux_) {
    if (!dp || !task_streams) return gmp::fail(GMP_ERR_ARG, "step: null descriptor");
    const gmp_step_desc& d = *dp;
    GMP_TRY(check_desc(d));        // (before anything is created or enqueued)
    // Two enqueue threads when every cross-stream dependency of the step is a gate (nothing a host thread records for the other to wait on),
    // no phase timing, and there is a stream besides main to hand over.  GMP_STEP_LANES=0: one thread.
    bool other = false;
    for (int ti = 0; ti < d.num_tasks; ++ti) other = other || task_streams[ti] != main_;
    const bool two = lanes_enabled() && d.sync_flags != nullptr && !phase_timing() && aux_ != main_ && other && gmp::lane_mode() == gmp::LANE_ALL;
    (void)events();                // (the static event pool: made before two threads could race for it)
    if (!two) return step_body(dp, main_, task_streams, aux_, false, true);
    LaneWorker& w = LaneWorker::get();
    w.post(LaneJob{dp, main_, aux_, task_streams, gmp::cur_device()});
    gmp::lane_mode() = gmp::LANE_ONLY;
    gmp::lane_stream() = (hipStream_t)main_;
    const int rc0 = step_body(dp, main_, task_streams, aux_, true, true);
    gmp::lane_mode() = gmp::LANE_ALL;
    char err[512];
    const int rc1 = w.wait(err, sizeof(err));
    if (!rc0 && rc1) return gmp::fail(rc1, "%s", err);
    return rc0;
}

// Data-parallel exchange beside the backward: `st` waits until the per-task gradients of one part of the model are final in
// task_grads -- part 0: the task heads (written before the stacked backward starts), part 1 + k: backbone layer L-1-k (its
// weight-gradient GEMMs and BatchNorm parameter sums on aux, its eps sum on main), last part: the mask token and the encoders
// (end of the backward).  Uses the flags or events of the most recent gmp_pretrain_step_fwd_bwd of this process (dp_exchange set).
extern "C" int gmp_step_wait_grads(int part, gmp_stream_t st_) {
    if (part < 0 || part > LAYERS + 1) return gmp::fail(GMP_ERR_ARG, "step_wait_grads: part %d not in [0, %d]", part, LAYERS + 1);
    // what a backbone layer's part waits for: aux's weight gradients and BatchNorm parameter sums of layer l, and main past layer l's eps sum
    const int l = LAYERS - part;                             // 4 .. 0 for the layer parts
    const Dep layer_deps[2] = {dep::aux_layer(l > 0 ? l : 0), l > 0 ? dep::gu_ready(l - 1) : dep::l0};
    if (g_sync.flags) {       // the step ran with gates: one sleeping wave on `st` for the flags of this part
        uint64_t mask;
        if (part == 0) mask = g_sync.head_params_mask;
        else if (part == LAYERS + 1) mask = dep::bwd_done.bit();
        else mask = layer_deps[0].bit() | layer_deps[1].bit();
        return gmp_gate_wait(g_sync.flags, mask, g_sync.epoch, g_sync.flags + F_ERR, st_);
    }
    hipStream_t st = (hipStream_t)st_;
    hipEvent_t* ev = events();
    hipError_t e = hipSuccess;
    if (part == 0) {      // input halves joined on main + every head's weight-gradient GEMMs (events of absent tasks: never recorded = no wait)
        e = hipStreamWaitEvent(st, ev[dep::heads_done.ev], 0);
        for (int i = 0; i <= MAXT && e == hipSuccess; ++i) e = hipStreamWaitEvent(st, ev[dep::head_params(i).ev], 0);
    } else if (part == LAYERS + 1) {
        e = hipStreamWaitEvent(st, ev[dep::bwd_done.ev], 0);
    } else {
        for (int i = 0; i < 2 && e == hipSuccess; ++i) e = hipStreamWaitEvent(st, ev[layer_deps[i].ev], 0);
    }
    return e == hipSuccess ? GMP_OK : gmp::fail(GMP_ERR_LAUNCH, "step_wait_grads: hipStreamWaitEvent failed");
}

extern "C" int gmp_step_phase_ms(float* out3) {
    if (!out3) return gmp::fail(GMP_ERR_ARG, "step_phase_ms: null pointer");
    float all[GMP_STEP_PHASES];
    if (int rc = gmp_step_phase_detail_ms(all)) return rc;
    out3[0] = out3[1] = out3[2] = 0.f;
    for (int i = 0; i < GMP_STEP_PHASES; ++i) out3[i <= GMP_STEP_LAYERS ? 0 : (i == GMP_STEP_LAYERS + 1 ? 1 : 2)] += all[i];
    return GMP_OK;
}

extern "C" int gmp_step_phase_detail_ms(float* out) {
    if (!out) return gmp::fail(GMP_ERR_ARG, "step_phase_detail_ms: null pointer");
    if (!phase_timing()) return gmp::fail(GMP_ERR_UNSUPPORTED, "step_phase_detail_ms: set GMP_STEP_TIMING=1 before the first step");
    hipEvent_t* e = phase_events();
    if (hipEventSynchronize(e[GMP_STEP_PHASES]) != hipSuccess) return gmp::fail(GMP_ERR_LAUNCH, "step_phase_detail_ms: no step recorded");
    for (int i = 0; i < GMP_STEP_PHASES; ++i)
        if (hipEventElapsedTime(&out[i], e[i], e[i + 1]) != hipSuccess) return gmp::fail(GMP_ERR_LAUNCH, "step_phase_detail_ms: elapsed");
    return GMP_OK;
}

// (diagnostic, GMP_STEP_TIMING=1) per task: ms from "stacked forward done" to the head's start, to the end of its input-gradient half and
// to the end of its weight-gradient half (0 where the head runs on the main stream and has no separate second half) -- out[3 * task + k]
extern "C" int gmp_step_head_ms(float* out, int max_tasks) {
    if (!out || max_tasks < g_head_tasks) return gmp::fail(GMP_ERR_ARG, "step_head_ms: bad argument");
    if (!phase_timing()) return gmp::fail(GMP_ERR_UNSUPPORTED, "step_head_ms: set GMP_STEP_TIMING=1 before the first step");
    hipEvent_t fwd_done = phase_events()[1 + GMP_STEP_LAYERS];
    (void)hipEventSynchronize(phase_events()[GMP_STEP_PHASES]);
    for (int i = 0; i < 3 * g_head_tasks; ++i) {
        out[i] = 0.f;
        if (g_head_recorded[i] && hipEventSynchronize(head_events()[i]) == hipSuccess) (void)hipEventElapsedTime(&out[i], fwd_done, head_events()[i]);
    }
    return GMP_OK;
}
