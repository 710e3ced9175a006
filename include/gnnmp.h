/*
 * libgnnmp -- MI355X (gfx950) message-passing kernels behind a flat C ABI.
 *
 * This is the drop-in boundary of the build.  The reference
 * (alonbebchuk/GNN-Pretraining) has no FFI of its own: its hot path calls
 * torch-geometric / torch operators from Python.  Each entry point below names the
 * reference call site (file:line under /root/reference) whose operator it serves.
 *
 * Conventions
 *   - every function returns GMP_OK (0) or a negative GMP_ERR_* code; the text of
 *     the last error on the calling thread is at gmp_last_error_string();
 *   - no exceptions cross the boundary, nothing here allocates or frees device
 *     memory: the caller owns every buffer and passes a workspace where one is
 *     needed (size from the matching *_workspace_bytes function);
 *   - all pointers are DEVICE pointers unless a parameter says "host";
 *   - all work is enqueued asynchronously on `stream` (a hipStream_t passed as
 *     void*); no call synchronises;
 *   - feature matrices are row-major fp32 -- except the sparse input of
 *     gmp_sparse_linear_*, which is CSR (int32 rowptr / col, fp32 values); graph
 *     indices handed over by the caller are int64 (the reference's dtype), CSR
 *     arrays produced here are int32;
 *   - F (feature width) must be a multiple of 4 and rows must be 16-byte aligned.
 */
#ifndef GNNMP_H
#define GNNMP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMP_OK 0
#define GMP_ERR_ARG (-1)       /* bad argument (null pointer, negative size, bad alignment) */
#define GMP_ERR_LAUNCH (-2)    /* HIP reported a launch/runtime error */
#define GMP_ERR_WORKSPACE (-3) /* workspace too small */
#define GMP_ERR_UNSUPPORTED (-4)

typedef void* gmp_stream_t; /* hipStream_t */

int gmp_version(void);
const char* gmp_last_error_string(void);

/* ------------------------------------------------------------------------- *
 * Index build: COO int64 -> CSR int32, both orientations.
 * Serves PyG MessagePassing.propagate's gather/scatter indexing for
 * GINConv(h, edge_index) (src/models/gnn.py:41) and its backward.
 *   edge_index  [2,E] int64, row 0 = source j, row 1 = target i (PyG flow).
 *   rowptr/col/perm      grouped by TARGET: row i lists the sources of edges j->i
 *   rowptr_t/col_t/perm_t grouped by SOURCE (transposed graph, for the backward);
 *                         the three *_t pointers may all be NULL.
 *   perm[k] = COO edge id stored at CSR slot k; within a row slots are in ascending
 *   edge id (stable counting sort) -- bit-exact against oracle.graph_ops.coo_to_csr.
 *   status      device int32[1]: number of endpoints outside [0,N) (those edges are
 *               dropped instead of faulting); 0 on well-formed input.
 * ------------------------------------------------------------------------- */
size_t gmp_csr_build_workspace_bytes(int64_t num_nodes, int64_t num_edges);
int gmp_csr_build(const int64_t* edge_index, int64_t num_nodes, int64_t num_edges,
                  int32_t* rowptr, int32_t* col, int32_t* perm,
                  int32_t* rowptr_t, int32_t* col_t, int32_t* perm_t,
                  int32_t* status, void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* The same arrays for a BLOCK-DIAGONAL batch whose blocks ("segments": one forward() call's graphs) own contiguous row ranges
 * seg_row_ptr[s]..[s+1] and contiguous edge ranges seg_edge_ptr[s]..[s+1] (device int32 [S+1]; no edge leaves its segment):
 * one workgroup per (segment, orientation) instead of one per orientation -- the stacked batch of a pre-training step.
 * max_seg_rows / max_seg_edges: host-side maxima (LDS sizing; GMP_ERR_UNSUPPORTED when a segment does not fit).  An edge with
 * an endpoint outside its segment is dropped and counted in status. */
int gmp_csr_build_segmented(const int64_t* edge_index, int64_t num_nodes, int64_t num_edges, const int32_t* seg_row_ptr,
                            const int32_t* seg_edge_ptr, int num_segments, int64_t max_seg_rows, int64_t max_seg_edges,
                            int32_t* rowptr, int32_t* col, int32_t* perm, int32_t* rowptr_t, int32_t* col_t, int32_t* perm_t,
                            int32_t* status, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * GIN neighbourhood aggregation (the SpMM-style kernel of BASELINE.json).
 *   fwd: out[i,:] = (1 + eps) * x[i,:] + sum_{k in rowptr[i]..rowptr[i+1]} x[col[k],:]
 *        == PyG GINConv before its nn (src/models/gnn.py:29-41).
 *   bwd: g_x[i,:] = (1 + eps) * g_out[i,:] + sum over the TRANSPOSED CSR of g_out;
 *        g_eps[0] = sum_i <g_out[i,:], x[i,:]>  (deterministic two-stage reduction).
 *   eps is a device float[1] (the learnable GINConv.eps, shape [1]).
 * Algorithmic bytes per launch: 2*4*F*N + 4*(N+1) + 4*E.
 * ------------------------------------------------------------------------- */
int gmp_gin_aggregate_fwd(const float* x, const int32_t* rowptr, const int32_t* col, const float* eps,
                          float* out, int64_t num_nodes, int feat, gmp_stream_t stream);
/* rows [row0, row1) of gmp_gin_aggregate_fwd (x, rowptr, col in the whole batch's numbering; cache-resident sizes) */
int gmp_gin_aggregate_fwd_rows(const float* x, const int32_t* rowptr, const int32_t* col, const float* eps, float* out,
                               int64_t row0, int64_t row1, int feat, gmp_stream_t stream);
size_t gmp_gin_aggregate_bwd_workspace_bytes(int64_t num_nodes, int feat);
int gmp_gin_aggregate_bwd(const float* g_out, const int32_t* rowptr_t, const int32_t* col_t, const float* eps,
                          const float* x, float* g_x, float* g_eps, int64_t num_nodes, int feat,
                          void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* Stacked-pass backward: g_x = (1+eps) g + sum over the transposed CSR of g (+ addend: the residual
 * branch's gradient), rowdot[r] = <g[r,:], x[r,:]> (nullable) so that the eps gradient can be reduced
 * per task with gmp_group_sum_1d: out[out_off_host[g]] = sum vals[rows[g] .. rows[g+1]). */
int gmp_gin_aggregate_bwd_ex(const float* g_out, const int32_t* rowptr_t, const int32_t* col_t, const float* eps,
                             const float* x, const float* addend, float* g_x, float* rowdot, int64_t num_nodes,
                             int feat, gmp_stream_t stream);
int gmp_group_sum_1d(const float* vals, int groups, const int32_t* group_rows_host, const int64_t* out_off_host,
                     float* out, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Generic segmented row sum:  out[r,:] (+)= scale_r * sum_{k in ptr[r]..ptr[r+1]} src[idx ? idx[k] : k, :]
 *   mean != 0  -> scale_r = 1 / max(ptr[r+1]-ptr[r], 1)   (PyG scatter 'mean')
 * Serves global_mean_pool (src/pretrain/tasks.py:241,244,299,331; finetune_model.py:75)
 * and the scatter-add backward of row gathers h[idx] (tasks.py:80, heads.py:59-60).
 * ------------------------------------------------------------------------- */
int gmp_segment_sum(const float* src, const int32_t* ptr, const int32_t* idx, float* out,
                    int64_t num_segments, int feat, int mean, int accumulate, gmp_stream_t stream);

/* out[m,:] = scale_m * src[idx[m],:];  scale_m = 1, or 1/max(count[idx[m]],1) when
 * seg_ptr != NULL (backward of global_mean_pool: idx = batch vector). idx int64. */
int gmp_row_gather(const float* src, const int64_t* idx, const int32_t* seg_ptr, float* out,
                   int64_t num_out_rows, int64_t num_src_rows, int feat, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * global_max_pool (tasks.py:242,245): out[b,f] = max over rows ptr[b]..ptr[b+1];
 * empty segment -> 0 (PyG: new_zeros + scatter_reduce amax, include_self=False).
 * bwd splits g evenly between tied maxima, as torch's scatter_reduce('amax') does
 * (including its count of the zero-initialised output as one more tie when max == 0).
 * ------------------------------------------------------------------------- */
int gmp_segment_max_fwd(const float* x, const int32_t* ptr, float* out, int64_t num_segments, int feat,
                        gmp_stream_t stream);
int gmp_segment_max_bwd(const float* g_out, const float* x, const float* out, const int32_t* ptr,
                        float* g_x, int64_t num_segments, int feat, int accumulate, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Dense fp32 GEMM on the f32 MFMA (v_mfma_f32_32x32x2_f32), C = alpha * op(A) op(B) (+ bias)(+ C).
 * nn.Linear forward / input-grad / weight-grad of the GIN MLP and the heads
 * (gnn.py:14,31,34; heads.py:42).
 *   GMP_GEMM_NT: C[M,N] = A[M,K] * B[N,K]^T      (Linear forward: x W^T)
 *   GMP_GEMM_NN: C[M,N] = A[M,K] * B[K,N]        (input grad: g W)
 *   GMP_GEMM_TN: C[M,N] = A[K,M]^T * B[K,N]      (weight grad: g^T x), reduction over rows
 *   bias: NULL or [N], added to every row.  accumulate != 0 -> C += result.
 *   relu != 0 -> C = max(C, 0) after bias (MLPHead hidden layers).
 * ------------------------------------------------------------------------- */
#define GMP_GEMM_NT 0
#define GMP_GEMM_NN 1
#define GMP_GEMM_TN 2
/* workspace: optional; when the output tile count cannot fill the chip and K is long
 * (weight gradients) the kernel splits K over blockIdx.z into this buffer and sums the
 * slices in order (deterministic).  0 bytes / NULL -> no split-K. */
size_t gmp_gemm_f32_workspace_bytes(int mode, int64_t M, int64_t N, int64_t K);
int gmp_gemm_f32(int mode, const float* A, const float* B, const float* bias, float* C,
                 int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc,
                 float alpha, int accumulate, int relu, void* workspace, size_t workspace_bytes,
                 gmp_stream_t stream);
/* Grouped form: `groups` (<= 24) independent problems in ONE launch (blockIdx.z = group), row ranges
 * group_rows_host[g] .. group_rows_host[g+1] (HOST int32, ascending):
 *   NT / NN: group g multiplies ITS rows of A by ITS OWN weight matrix B + b_off_host[g] (+ bias +
 *            bias_off_host[g]) into the same rows of C  -- the per-domain heads of one task
 *            (pretrain_model.py:41-63) in one launch;
 *   TN:      group g reduces over ITS rows of A [rows, M_tn] and B [rows, N] into C + c_off_host[g]
 *            -- per-task weight gradients of the stacked backbone pass (one group per task, the
 *            offsets point into the per-task gradient buffer PCGrad reads).
 *            a_colsum (nullable): a_colsum + a_colsum_off_host[g] + m receives sum over the group's rows of
 *            A[:, m] -- the bias gradient rides along with the weight gradient for free.
 *            workspace (nullable): lets TN slice each group's rows over several workgroups (partials summed
 *            in slice order by a second kernel) when the output alone cannot fill the chip.
 * Offsets are in floats; NULL offset arrays mean 0 (a_colsum_off_host: g * M_tn).
 * Epilogue, every mode and every path (with or without a workspace): C = alpha * product (+ bias, NT / NN only: a bias with TN is refused);
 *   accumulate != 0 -> that value is ADDED to what C held; relu != 0 -> max(., 0) last.  An empty group of the TN form therefore leaves
 *   zeros, or C as it was under accumulate; an empty group of NT / NN owns no rows and writes nothing.  a_colsum is always stored, never
 *   accumulated.  Rows of C beyond group_rows_host[groups] and columns beyond N (ldc > N) are never written.
 * Leading dimensions follow gmp_gemm_f32: NT lda, ldb >= K; NN lda >= K, ldb >= N; TN lda >= M_tn, ldb >= N; always ldc >= N -- anything
 *   smaller is GMP_ERR_ARG and nothing is launched.  groups outside 1 .. 24, a NULL or descending row list, N <= 0 likewise.
 * Alignment is never required: bases, leading dimensions and offsets (b_off, bias_off, c_off) that are not multiples of 4 floats / 16 bytes
 *   only select the guarded loads and scalar stores (and with them possibly the other kernel family: the same products, summed in that
 *   kernel's order).  A call whose groups are all empty (TN: M_tn == 0)
 *   launches nothing, returns GMP_OK and leaves a pending gmp_gate_open_by_next_gemm signal pending. */
int gmp_gemm_f32_grouped(int mode, const float* A, const float* B, const float* bias, float* C, int groups,
                         const int32_t* group_rows_host, const int64_t* b_off_host, const int64_t* bias_off_host,
                         const int64_t* c_off_host, float* a_colsum, const int64_t* a_colsum_off_host,
                         int64_t M_tn, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, float alpha,
                         int accumulate, int relu, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
/* column sums: out[n] (+)= sum_m A[m,n]  (bias gradient), rows [0,M) */
size_t gmp_colsum_workspace_bytes(int64_t M, int64_t N);
int gmp_colsum(const float* A, float* out, int64_t M, int64_t N, int64_t lda, int accumulate,
               void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Segment-wise BatchNorm1d (+ residual, ReLU, dropout) -- gnn.py:15,19-22,32,38,42-43.
 * A "segment" is one reference forward() call's worth of rows: statistics are
 * taken per segment so several independent forwards can share one launch.
 *   seg_ptr     device int32 [S+1] row offsets; max_seg_rows = host-side max length.
 *   training:   mean/biased var over the segment (eps 1e-5), saved to save_mean /
 *               save_rstd [S,C]; running_mean/var (nullable) are updated segment by
 *               segment in order with momentum 0.1 and the unbiased variance,
 *               num_batches_tracked is the caller's business.
 *   eval:       uses running_mean / running_var.
 *   y = dropout(relu?( gamma * (x [+ residual] - mean) * rstd + beta ))
 *   dropout keep-mask comes from Philox(seed, stream_id, element) and is NOT stored:
 *   the backward regenerates it.  p = 0 disables dropout.
 * ------------------------------------------------------------------------- */
typedef struct {
    int training;        /* batch statistics vs running statistics */
    int relu;            /* apply ReLU after the affine transform */
    float eps;           /* 1e-5 */
    float momentum;      /* 0.1 */
    float dropout_p;     /* 0 = none */
    uint64_t seed;       /* dropout seed */
    uint32_t stream_id;  /* distinct per dropout site */
    const uint64_t* seed_dev;  /* NULL, or a DEVICE word added to `seed` when the kernel runs: a launch captured in a hipGraph draws fresh
                                  masks on every replay (the caller bumps the word between replays, gmp_counter_add) */
    int32_t* sync;       /* NULL, or a DEVICE buffer of gmp_bn_sync_bytes, zero-filled by the caller ONCE and private to the stream the
                            call runs on: segments of 1,025..4,096 rows (the Cora graph) are then cut into 128-row slabs over the whole chip
                            that exchange their partial statistics through this buffer inside ONE launch, instead of one workgroup per
                            (segment, column strip).  sync[0] != 0 afterwards = a wait timed out (buffer not zeroed, or shared by streams) */
    uint32_t sync_words; /* int32 words behind `sync`; fewer than gmp_bn_sync_bytes asks for = the slab form is not used */
} gmp_bn_config;

size_t gmp_bn_workspace_bytes(int64_t rows, int channels, int num_segments, int64_t max_seg_rows);
size_t gmp_bn_sync_bytes(int channels, int num_segments);
/* seg_group: NULL, or device int32 [S] giving each segment's PARAMETER GROUP: gamma, beta and the running
 * statistics are then [groups][C] arrays (the four per-domain input encoders stacked in one launch). */
int gmp_bn_fwd(const float* x, const float* residual, const int32_t* seg_ptr, const int32_t* seg_group,
               int num_segments, int64_t max_seg_rows, int64_t rows, int channels,
               const float* gamma, const float* beta, float* running_mean, float* running_var,
               float* save_mean, float* save_rstd, float* y,
               const gmp_bn_config* cfg, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
/* Training-mode gmp_bn_fwd with running_mean == NULL leaves the running statistics alone; this applies that update later
 * from the saved batch statistics (segments in order, as S successive forward() calls would: bit-identical). */
int gmp_bn_running_update(const int32_t* seg_ptr, const int32_t* seg_group, int num_segments, int channels,
                          float* running_mean, float* running_var, const float* save_mean, const float* save_rstd,
                          const gmp_bn_config* cfg, gmp_stream_t stream);
/* The same for `count` (<= 16) BatchNorms that share seg_ptr, in one launch: HOST arrays of device pointers / channel counts
 * (seg_group: NULL, or per entry NULL / device int32 [S]). */
int gmp_bn_running_update_batch(int count, const int32_t* seg_ptr, int num_segments, const int32_t* const* seg_group,
                                const int32_t* channels, float* const* running_mean, float* const* running_var,
                                const float* const* save_mean, const float* const* save_rstd, const gmp_bn_config* cfg,
                                gmp_stream_t stream);
/* backward: given g_y, the BN input u = x (+ residual, recomputed on the fly), saved stats.
 *   g_u [rows,C]   gradient w.r.t. the BN input (also the residual's gradient)
 *   g_gamma/g_beta: per GRADIENT group sums (<= 24 groups, one launch); group g covers segments
 *   grp_seg_ptr_host[g]..[g+1] (host int32 [G+1]) and is written at g_gamma + grp_off_gamma_host[g]
 *   (float offsets, host int64 [G]; NULL -> g*C).  G=1 -> ordinary gradients; G=#tasks with offsets
 *   into the per-task gradient buffer -> the per-task gradients PCGrad needs, from ONE backward. */
int gmp_bn_bwd(const float* g_y, const float* x, const float* residual, const int32_t* seg_ptr,
               const int32_t* seg_group, int num_segments, int64_t max_seg_rows, int64_t rows, int channels,
               const float* gamma, const float* beta, const float* running_mean, const float* running_var,
               const float* save_mean, const float* save_rstd,
               float* g_u, float* g_gamma, float* g_beta, const int32_t* grp_seg_ptr_host,
               const int64_t* grp_off_gamma_host, const int64_t* grp_off_beta_host, int num_groups,
               const gmp_bn_config* cfg, void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* gmp_bn_bwd with num_groups = 0 leaves the per-segment sums at the start of its workspace; this turns them into the per-group
 * g_gamma / g_beta later, on any stream (bit-identical to passing the groups to gmp_bn_bwd). */
int gmp_bn_param_grads(const void* bwd_workspace, int num_segments, int channels, float* g_gamma, float* g_beta,
                       const int32_t* grp_seg_ptr_host, const int64_t* grp_off_gamma_host, const int64_t* grp_off_beta_host,
                       int num_groups, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Inference: eval-mode BatchNorm1d folded into the Linear that feeds it.  With running statistics the norm is the per-channel
 * affine map y = scale * u + shift, scale = gamma / sqrt(running_var + eps), shift = beta - scale * running_mean.
 *
 * gmp_bn_fold: the (scale, shift) rows of `count` (<= 16) BatchNorms in ONE launch.  gamma / beta / running_mean / running_var are HOST
 *   arrays of `count` device pointers, channels a HOST int32 array (gamma / beta, or single entries of them, may be NULL: 1 / 0).
 *   `table` is the caller's: entry e's scale row starts at float offset 2 * (channels[0] + .. + channels[e-1]), its shift row follows
 *   at + channels[e]; 2 * sum(channels) floats in all.  Asynchronous on `stream`, allocates nothing.
 *
 * gmp_linear_affine_fwd: C[M,N] = act(((A W^T + bias) + residual) * scale + shift), evaluated in exactly that order (fp32, no fused
 *   multiply-add).  A [M,K] (lda), W [N,K] as nn.Linear stores it (ldw), bias [N] or NULL, residual [M,N] (ldr) or NULL, scale and
 *   shift [N] (rows of gmp_bn_fold's table), relu != 0 -> max(., 0).  Any M >= 1, K >= 1.  The product runs on gmp_gemm_f32's kernels
 *   under its dispatch rule (GMP_GEMM_NT, alpha 1): with scale = 1, shift = 0 and no residual the result equals gmp_gemm_f32's given
 *   the same workspace -- the same accumulation order, so the same bits, except that an element gmp_gemm_f32 leaves at -0.0 becomes +0.0.  Rows beyond M are never written.  No atomics: bitwise reproducible.  The workspace is optional, as for
 *   gmp_gemm_f32 (K-slices when the output alone cannot fill the chip).
 * ------------------------------------------------------------------------- */
int gmp_bn_fold(int count, const float* const* gamma, const float* const* beta, const float* const* running_mean,
                const float* const* running_var, const int32_t* channels, float eps, float* table, gmp_stream_t stream);
size_t gmp_linear_affine_workspace_bytes(int64_t M, int64_t N, int64_t K);
int gmp_linear_affine_fwd(const float* A, const float* W, const float* bias, const float* residual, const float* scale,
                          const float* shift, float* C, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldw, int64_t ldr,
                          int64_t ldc, int relu, void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Link-prediction edge features (the per-edge MLP input, heads.py:58-66):
 *   feat[k,:] = [ hs+hd | hs*hd | |hs-hd| ],  hs = h[edges[0,k]], hd = h[edges[1,k]]
 * bwd produces per-edge gradients g_hs, g_hd [K,F]; the caller reduces them onto
 * nodes with gmp_segment_sum over a CSR of the decoder edges.
 * ------------------------------------------------------------------------- */
int gmp_lp_edge_features_fwd(const float* h, const int64_t* edges, float* feat, int64_t num_nodes,
                             int64_t num_edges, int feat_dim, gmp_stream_t stream);
int gmp_lp_edge_features_bwd(const float* g_feat, const float* h, const int64_t* edges, float* g_hs,
                             float* g_hd, int64_t num_nodes, int64_t num_edges, int feat_dim,
                             gmp_stream_t stream);
/* The input-gradient GEMM of the first head layer with gmp_lp_edge_features_bwd in its epilogue:
 *   g_feat = gy1 w0 ([K, 3 feat], never written), folded per pair into g_hs, g_hd [K, feat] as gmp_lp_edge_features_bwd does.
 * gy1 [K, 256], w0 [256, 768] row-major, h [num_nodes, 256], edges int64 [2, K].  Bit for bit what gmp_gemm_f32(GMP_GEMM_NN, gy1, w0,
 * NULL, g_feat, K, 768, 256, ...) without a workspace followed by gmp_lp_edge_features_bwd gives where that GEMM runs on the pipelined
 * kernel, hence: feat_dim == 256 (GMP_ERR_UNSUPPORTED otherwise), K >= 1024 and every float operand 16-byte aligned (GMP_ERR_ARG;
 * nothing is launched).  Carries a pending gmp_gate_open_by_next_gemm signal like the GEMM it replaces. */
int gmp_lp_feat_gemm_bwd_fold(const float* gy1, const float* w0, const float* h, const int64_t* edges, float* g_hs,
                              float* g_hd, int64_t num_nodes, int64_t num_edges, int feat_dim, gmp_stream_t stream);
/* The two GEMMs that read feat, with feat generated inside their operand loaders (never written):
 *   fwd:   y1 = relu(feat w0^T + b0) [K, 256]       -- gmp_lp_edge_features_fwd + gmp_gemm_f32(GMP_GEMM_NT, feat, w0, b0, y1, ..., relu)
 *   wgrad: dW0 = gy1^T feat [256, 768], db0 = column sums of gy1 [256] (NULL: skipped)
 *                                                    -- gmp_gemm_f32_grouped(GMP_GEMM_TN, gy1, feat, ..., one group, WITH this workspace)
 * bit for bit, where those GEMMs run on the pipelined kernel: feat_dim == 256 (GMP_ERR_UNSUPPORTED otherwise), K >= 1024, float operands
 * 16-byte aligned (GMP_ERR_ARG); wgrad needs a workspace (GMP_ERR_WORKSPACE without: the materialised GEMM would not take the pipelined
 * kernel) and slices the rows exactly as the materialised call with the same workspace size does.  Nothing is launched on an error.
 * Both carry a pending gmp_gate_open_by_next_gemm signal. */
int gmp_lp_feat_gemm_fwd(const float* h, const int64_t* edges, const float* w0, const float* b0, float* y1, int64_t num_nodes,
                         int64_t num_edges, int feat_dim, gmp_stream_t stream);
int gmp_lp_feat_gemm_wgrad(const float* gy1, const float* h, const int64_t* edges, float* dW0, float* db0, int64_t num_nodes,
                           int64_t num_edges, int feat_dim, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
/* DIAGNOSTIC: how many gmp_lp_feat_gemm_fwd / _wgrad / _bwd_fold calls of this process have launched so far (the pre-training step counts here too); lets a
 * test tell whether a step took the fused launches or its fallback. */
uint64_t gmp_lp_feat_gemm_launch_count(void);

/* ------------------------------------------------------------------------- *
 * The fused link-prediction scorer (MLPLinkPredictor, heads.py:57-67) over a pair list src[k], dst[k] (int64, k < K):
 *   feat = [hs+hd | hs*hd | |hs-hd|] (never written to memory), z = feat w0^T + b0 (w0 [hidden, 3 feat] row-major),
 *   act = relu(z) [K, hidden] (the pre-dropout activation, kept for the backward), logit = <dropout(act), w3> + b3.
 * Dropout is the mask gmp_dropout_fwd(act, p, seed, site) draws over the contiguous [K, hidden] activation; p == 0: no mask.
 * The sigmoid / BCE / d loss / d logit that follow are gmp_sigmoid_bce_sum_fwd_bwd.
 * bwd from g_logit [K]: g_w0 [hidden, 3 feat], g_b0 [hidden], g_w3 [hidden], g_b3 [1] written (accumulate = 0) or added to,
 * per-pair g_hs / g_hd [K, feat] (torch.abs' subgradient: 0 at hs == hd; reduce them onto nodes with gmp_segment_sum).
 * feat == hidden == 256 (GMP_ERR_UNSUPPORTED otherwise).  Every sum over pairs is in a fixed order (no atomics): bitwise
 * reproducible.  An index outside [0, num_nodes) reads as a zero row.  h, w0, b0, w3, act 16-byte aligned.
 * ------------------------------------------------------------------------- */
size_t gmp_lp_score_fwd_workspace_bytes(int64_t num_pairs);
size_t gmp_lp_score_bwd_workspace_bytes(int64_t num_pairs);
int gmp_lp_score_fwd(const float* h, const int64_t* src, const int64_t* dst, int64_t num_nodes, int64_t num_pairs, int feat_dim,
                     int hidden, const float* w0, const float* b0, const float* w3, const float* b3, float* act, float* logit,
                     float p, uint64_t seed, uint32_t site, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_lp_score_bwd(const float* h, const int64_t* src, const int64_t* dst, int64_t num_nodes, int64_t num_pairs, int feat_dim,
                     int hidden, const float* w0, const float* w3, const float* act, const float* g_logit, float p, uint64_t seed,
                     uint32_t site, float* g_w0, float* g_b0, float* g_w3, float* g_b3, int accumulate, float* g_hs, float* g_hd,
                     void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * All-candidate link ranking with the scorer above (p = 0): one source against every node of h [num_nodes, feat], reduced on the fly.
 * The logit of a pair (s, c) is bit for bit the one gmp_lp_score_fwd gives it with p = 0 (the same MFMA products, k-slices and partial
 * dots in the same order), so ranks are exact integers that agree with scoring the explicit pair list.  No per-candidate logit, no
 * [Q num_nodes, hidden] activation and no pair list is written to memory.
 * The optional filter is a CSR of known edges, row = source: filter_rowptr int32 [num_nodes + 1], filter_col int32 [filter_nnz]
 * (both NULL: no filter).  Rows need not be sorted and may hold duplicates; entries outside [0, num_nodes) are ignored.
 * gmp_lp_rank, for Q true pairs (src[q], dst[q]): logit_true [Q], and over the candidates c in [0, num_nodes) except c == src[q],
 *   c == dst[q] and the entries of src[q]'s filter row: n_greater [Q] = how many score greater than the true pair, n_equal [Q] = how
 *   many score equal to it (int32; the filtered rank is 1 + n_greater + n_equal / 2).  Integer sums: independent of the block order.
 *   Needs no workspace (gmp_lp_rank_workspace_bytes is 0; workspace may be NULL).
 * gmp_lp_topk, for Q sources and 1 <= k <= 64: idx [Q, k] int64 and logit [Q, k], the k best candidates c != src[q] outside the
 *   filter row, logit descending, ties to the lower node index; a row with fewer than k candidates is padded with -1 / -inf.
 *   workspace >= gmp_lp_topk_workspace_bytes(Q, num_nodes): at most 16 partial lists of 64 entries per source, O(Q).
 * src / dst outside [0, num_nodes) read as a zero row (and have an empty filter row).  feat == hidden == 256; num_nodes < 2^31;
 * h, w0, b0, w3 16-byte aligned.
 * ------------------------------------------------------------------------- */
size_t gmp_lp_rank_workspace_bytes(int64_t num_queries, int64_t num_nodes);
size_t gmp_lp_topk_workspace_bytes(int64_t num_queries, int64_t num_nodes);
int gmp_lp_rank(const float* h, const int64_t* src, const int64_t* dst, int64_t num_nodes, int64_t num_queries, int feat_dim, int hidden,
                const float* w0, const float* b0, const float* w3, const float* b3, const int32_t* filter_rowptr,
                const int32_t* filter_col, int64_t filter_nnz, float* logit_true, int32_t* n_greater, int32_t* n_equal,
                void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_lp_topk(const float* h, const int64_t* src, int64_t num_nodes, int64_t num_queries, int k, int feat_dim, int hidden,
                const float* w0, const float* b0, const float* w3, const float* b3, const int32_t* filter_rowptr,
                const int32_t* filter_col, int64_t filter_nnz, int64_t* idx, float* logit, void* workspace, size_t workspace_bytes,
                gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Structural link-prediction baselines: common neighbours, Adamic-Adar, resource allocation and Jaccard on a simple undirected graph,
 * scored for explicit pairs or ranked under gmp_lp_rank's protocol (csrc/lp_heuristics.hip).
 * The graph is a CSR, rowptr int32 [num_nodes + 1] and col int32 [nnz]: symmetric, no self-loops, every row strictly ascending.
 * gmp_graph_simple_check counts the entries that break this; on such a graph the two scorers give wrong numbers but read nothing outside
 * the arrays (rowptr is clamped to [0, nnz], entries outside [0, num_nodes) are skipped).
 * mode 0, the weighted sum: S_w(s, c) = the sum over z in N(s) & N(c) of weight[z], weight fp32 [num_nodes], NULL = 1.0f everywhere
 *   (common neighbours: exact integers below 2^24).  fp32, started at 0.0f, one plain add per z in ASCENDING z -- part of the contract: a
 *   score is bitwise reproducible, and the same pair has the same bits from gmp_lp_cn_score and as a candidate of gmp_lp_cn_rank.
 *   Adamic-Adar is weight[z] = 1 / ln(deg z) for deg z >= 2 else 0, resource allocation 1 / deg z for deg z >= 1 else 0; the caller
 *   computes them (the Python layer: float64 on the host, rounded once) -- the kernels see an array only.
 * mode 1, Jaccard: CN / (deg s + deg c - CN), 0 for an empty union, deg from rowptr; weight must be NULL.  The float quotient is what
 *   is written; ranking compares a / b with c / d exactly, as a d against c b in int64.
 * gmp_lp_cn_score: score [num_pairs]; a pair with an endpoint outside [0, num_nodes) scores 0.
 * gmp_lp_cn_rank, for Q true pairs (src[q], dst[q]): score_true [Q] (gmp_lp_cn_score's), and over the candidates c in [0, num_nodes)
 *   except c == src[q], c == dst[q] and the entries of src[q]'s filter row (gmp_lp_rank's filter CSR: unsorted rows, duplicates and
 *   out-of-range entries allowed; both NULL = none): n_greater [Q] and n_equal [Q], int32, the filtered rank being 1 + n_greater +
 *   n_equal / 2.  Integer sums: independent of the block order.  No per-candidate score is written to memory and no workspace is needed
 *   (gmp_lp_cn_rank_workspace_bytes is 0; workspace may be NULL).  Candidates are taken in tiles of gmp_lp_cn_tile_nodes().
 * gmp_graph_simple_check: *violations (int32, zeroed inside the call) = the number of entries that lie outside [0, num_nodes), equal
 *   their row, are not greater than their predecessor in the row, or lack the mirror entry, plus the rows whose rowptr bounds are not
 *   0 <= rowptr[v] <= rowptr[v + 1] <= nnz, rowptr[0] == 0, rowptr[num_nodes] == nnz.
 * GMP_ERR_ARG: num_nodes or nnz outside [0, 2^31), Q x tiles >= 2^31, a null pointer, mode outside {0, 1}, a weight array with mode 1.
 * num_pairs == 0 / num_queries == 0 return GMP_OK without a launch.  Asynchronous on `stream`, no host read-back, no allocation.
 * ------------------------------------------------------------------------- */
int gmp_lp_cn_tile_nodes(void);
size_t gmp_lp_cn_rank_workspace_bytes(int64_t num_queries, int64_t num_nodes);
int gmp_lp_cn_score(const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t nnz, const int64_t* src, const int64_t* dst,
                    int64_t num_pairs, const float* weight, int mode, float* score, gmp_stream_t stream);
int gmp_lp_cn_rank(const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t nnz, const int64_t* src, const int64_t* dst,
                   int64_t num_queries, const float* weight, int mode, const int32_t* filter_rowptr, const int32_t* filter_col,
                   int64_t filter_nnz, float* score_true, int32_t* n_greater, int32_t* n_equal, void* workspace, size_t workspace_bytes,
                   gmp_stream_t stream);
int gmp_graph_simple_check(const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t nnz, int32_t* violations,
                           gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Walk-based link-prediction baselines: the damped walk sum (Katz, rooted PageRank) and the hop distance, scored for explicit pairs or
 * ranked under gmp_lp_rank's protocol (csrc/lp_walk.hip).  The graph is the CSR of a simple undirected graph, the contract of
 * gmp_lp_cn_score above: a CSR that breaks it gives wrong numbers but nothing outside the arrays is read (rowptr is clamped to [0, nnz],
 * entries outside [0, num_nodes) are skipped).
 * Inputs: a source s, `rounds` R with 1 <= R <= 64, `damping` a (fp32, finite, 0 < a <= 1), an optional fp32 weight per node w (NULL = 1).
 * mode 0, the walk sum:
 *   y_0 = e_s and acc = 0.0f everywhere.
 *   for l = 1 .. R and every node v:  t = 0.0f;  for z in N(v) in ASCENDING z: t = t + w[z] * y_{l-1}[z]  (a plain add of y_{l-1}[z] when
 *   w is NULL);  y_l[v] = a * t;  acc[v] = acc[v] + y_l[v].
 *   score(s, c) = acc[c].
 *   Every multiply and add is rounded on its own (no fused multiply-add), subnormals are kept, there are no float atomics: a score is
 *   bitwise reproducible, and the same pair has the same bits from gmp_lp_walk_score and as a candidate of gmp_lp_walk_rank.  All terms
 *   are non-negative, so skipping zero terms or unreached rows changes no bit.  A source outside [0, num_nodes) has an all-zero acc.
 *   With w = NULL and a = beta this is the truncated Katz index, the sum over l <= R of beta^l (A^l)[s, c]; with w[z] = 1 / deg z and
 *   a = 1 - alpha it is the R-term rooted PageRank of s at c divided by alpha (the same order).  The caller computes w (the Python
 *   layer: float64 on the host, rounded once) -- the kernel sees an array only.
 * mode 1, hops: dist(s, c) the BFS distance in integers; score = -(float)dist if dist <= R, else -(float)(R + 1) (unreachable nodes and a
 *   source or destination outside the graph included).  weight must be NULL and damping is ignored.  Not derived from acc > 0: an
 *   underflow must not move a node.
 * gmp_lp_walk_score: score [num_pairs]; a destination outside [0, num_nodes) scores 0 (mode 0) / -(R + 1) (mode 1).  Runs of equal
 *   sources share one propagation.
 * gmp_lp_walk_rank, for Q true pairs (src[q], dst[q]): score_true [Q] (gmp_lp_walk_score's), and over the candidates c in [0, num_nodes)
 *   except c == src[q], c == dst[q] and the entries of src[q]'s filter row (gmp_lp_rank's filter CSR: unsorted rows, duplicates and
 *   out-of-range entries allowed; both NULL = none): n_greater [Q] and n_equal [Q], int32, the filtered rank being 1 + n_greater +
 *   n_equal / 2.  One workgroup per query stores its three outputs itself: no [Q, num_nodes] array, no output atomics, no memset.
 * Storage: for num_nodes <= gmp_lp_walk_lds_nodes() the per-query vectors live in LDS and no workspace is needed (NULL is fine).  Beyond
 *   it they live in `workspace`, gmp_lp_walk_workspace_bytes(Q, num_nodes) bytes, shared by at most gmp_lp_walk_resident_blocks()
 *   workgroups that loop over the queries: the size does not grow with Q beyond that many and is at most resident_blocks *
 *   (16 num_nodes + 4096).  Both paths run the same code and give the same bits.
 * GMP_ERR_ARG: rounds outside [1, 64]; in mode 0 a damping that is NaN, <= 0 or > 1; a weight array with mode 1; mode outside {0, 1};
 *   num_nodes or nnz outside [0, 2^31); a negative count; a null pointer; filter_rowptr without filter_col (or the reverse) with
 *   filter_nnz != 0; a workspace that is too small.  num_pairs == 0 / num_queries == 0 return GMP_OK without a launch.  Asynchronous on
 *   `stream`, no host read-back, no allocation.
 * ------------------------------------------------------------------------- */
int gmp_lp_walk_lds_nodes(void);
int gmp_lp_walk_resident_blocks(void);
size_t gmp_lp_walk_workspace_bytes(int64_t num_queries, int64_t num_nodes);
int gmp_lp_walk_score(const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t nnz, const int64_t* src, const int64_t* dst,
                      int64_t num_pairs, const float* weight, float damping, int rounds, int mode, float* score, void* workspace,
                      size_t workspace_bytes, gmp_stream_t stream);
int gmp_lp_walk_rank(const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t nnz, const int64_t* src, const int64_t* dst,
                     int64_t num_queries, const float* weight, float damping, int rounds, int mode, const int32_t* filter_rowptr,
                     const int32_t* filter_col, int64_t filter_nnz, float* score_true, int32_t* n_greater, int32_t* n_equal, void* workspace,
                     size_t workspace_bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Streaming k-nearest neighbours in cosine similarity and the weighted k-NN vote on top of them (the k-NN probe of Wu et al. 2018 for
 * self-supervised embeddings): q [nq, dim] queries against db [ndb, dim] database rows, both contiguous fp32.  Rows are normalised as the
 * hard-negative miner does, z / max(||z||, 1e-12) with the stride padded with zeros, so a zero row scores 0 against everything and never
 * gives NaN.  The similarity of a (query, database row) pair is one k-ordered fp32 MFMA chain (csrc/sim_tile.h): its bits depend on
 * neither the grid nor the other rows.  No [nq, ndb] array exists unless matrix_out is given.
 * gmp_knn_topk, for 1 <= k <= 64: idx [nq, k] int64 and sim [nq, k], per query the k best database rows, similarity descending, ties to
 *   the lower database index (a total order); a query with fewer than k candidates is padded with -1 / -inf.
 *   exclude_self != 0 leaves out j == i (leave-one-out over one set) and requires q == db and nq == ndb, GMP_ERR_ARG otherwise.
 *   matrix_out: NULL or [nq, ndb], every similarity exactly as the selection saw it (the diagonal included) -- test / diagnostic hook.
 *   1 <= dim <= 256, 1 <= nq, ndb < 2^31; nq == 0 is a no-op and ndb == 0 writes the -1 / -inf tail alone, both GMP_OK.  GMP_ERR_ARG
 *   outside those ranges, GMP_ERR_WORKSPACE when workspace_bytes < gmp_knn_workspace_bytes(nq, ndb, dim, k); nothing is launched then.
 *   gmp_knn_workspace_bytes = 4 (nq + ndb) dpad + 8 nq parts k + a constant below 1 KiB, dpad = dim rounded up to 4: the two normalised
 *   copies and per query `parts` lists of k 64-bit keys; the database is cut into parts (at most 16) only while nq <= 32,640, so beyond
 *   that it is 4 (nq + ndb) dpad + 8 nq k (2.5 GiB at nq = ndb = 2^20, dim = 256, k = 64).  0 for sizes outside the ranges.
 *   Asynchronous on `stream`, no host read-back, no allocation, integer compares only: the output is a pure function of the input.
 * gmp_knn_vote, on idx / sim [nq, k] as gmp_knn_topk returns them and db_labels [ndb] int64: class_scores [nq, classes] with
 *   class_scores[q, c] = the sum over r = 0 .. k-1, in that order and in fp32, of exp(sim[q, r] / temperature) where idx[q, r] >= 0 and
 *   db_labels[idx[q, r]] == c; pred [nq] int64 = the argmax, ties to the lower class, -1 for a query without a valid neighbour.
 *   status int32 [1] (zeroed inside the call) counts the neighbours whose label lies outside [0, classes) or whose index lies outside
 *   [0, ndb); those are skipped.  1 <= k <= 64, 2 <= classes <= 32, temperature > 0 (GMP_ERR_ARG otherwise).
 * ------------------------------------------------------------------------- */
size_t gmp_knn_workspace_bytes(int64_t nq, int64_t ndb, int dim, int k);
int gmp_knn_topk(const float* q, int64_t nq, const float* db, int64_t ndb, int dim, int k, int exclude_self, int64_t* idx, float* sim,
                 float* matrix_out, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_knn_vote(const int64_t* idx, const float* sim, int64_t nq, int k, const int64_t* db_labels, int64_t ndb, int classes,
                 float temperature, float* class_scores, int64_t* pred, int32_t* status, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * The embedding link probe: a pair of nodes scored from the rows of an embedding matrix alone, for explicit pairs or ranked against all
 * nodes under gmp_lp_rank's protocol (csrc/emb_link.hip).  No parameters, no fitting, no random state.
 * Inputs: h [num_nodes, dim] contiguous fp32, 1 <= dim <= 256.
 * mode 0, cosine: rows normalised exactly as gmp_knn_topk normalises, z / max(||z||, 1e-12) with the stride padded with zeros to a
 *   multiple of 4; a zero row scores 0 against everything.
 * mode 1, inner product: the raw rows in the same padded copy, without the division.
 * The score of a pair (s, c) is one k-ordered fp32 MFMA chain of row s against row c (csrc/sim_tile.h): its bits depend on neither the
 *   grid nor the other pairs, so the same pair has the same bits from gmp_emb_link_score, as score_true, as a candidate inside
 *   gmp_emb_link_rank and in matrix_out; in mode 0 they are the bits gmp_knn_topk's matrix_out has for the query row h[s] against the
 *   database row c.  A src or dst outside [0, num_nodes) reads as a zero row (score +0.0f); such a source has an empty filter row.
 * gmp_emb_link_score: score [num_pairs].
 * gmp_emb_link_rank, for Q true pairs (src[q], dst[q]): score_true [Q], and over the candidates c in [0, num_nodes) except c == src[q],
 *   c == dst[q] and the entries of src[q]'s filter row (gmp_lp_rank's filter CSR: unsorted rows, duplicates and out-of-range entries
 *   allowed; both NULL = none): n_greater [Q] and n_equal [Q], int32, zeroed inside the call, scores compared as IEEE floats (>, ==); the
 *   filtered rank is 1 + n_greater + n_equal / 2.  Counts are integer sums: they do not depend on the block order.
 *   matrix_out: NULL or [Q, num_nodes], every score exactly as the compare saw it (the filtered and the self columns included) -- test /
 *   diagnostic hook that changes no other output bit.  No [Q, num_nodes] array exists unless it is given.
 * GMP_ERR_ARG: dim outside [1, 256]; mode outside {0, 1}; num_nodes or a count outside [0, 2^31); a negative filter_nnz; a null required
 *   pointer; filter_rowptr without filter_col (or the reverse) with filter_nnz != 0; (query tiles of 128) x (candidate chunks) beyond one
 *   grid of 2^31 - 1 blocks.  GMP_ERR_WORKSPACE when workspace_bytes < gmp_emb_link_workspace_bytes(num_nodes, count, dim) =
 *   256 + 4 num_nodes dpad rounded up to 256 bytes, dpad = dim rounded up to 4: the padded copy of h (it does not grow with the count);
 *   0 for sizes outside the ranges.  Nothing is launched in an error case.  num_pairs == 0 / num_queries == 0 return GMP_OK without a
 *   launch.  Asynchronous on `stream`, no host read-back, no allocation, no global state, no float atomics.
 * ------------------------------------------------------------------------- */
size_t gmp_emb_link_workspace_bytes(int64_t num_nodes, int64_t num_queries, int dim);
int gmp_emb_link_score(const float* h, int64_t num_nodes, int dim, int mode, const int64_t* src, const int64_t* dst, int64_t num_pairs,
                       float* score, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_emb_link_rank(const float* h, int64_t num_nodes, int dim, int mode, const int64_t* src, const int64_t* dst, int64_t num_queries,
                      const int32_t* filter_rowptr, const int32_t* filter_col, int64_t filter_nnz, float* score_true, int32_t* n_greater,
                      int32_t* n_equal, float* matrix_out, void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Spherical k-means (k-means in cosine similarity on L2-normalised rows, the clustering probe for self-supervised embeddings) and the
 * integer contingency table its scores are computed from: x [n, dim] rows against kc centroids [kc, dim], contiguous fp32.  Rows and
 * centroids are normalised as gmp_knn_topk does, z / max(||z||, 1e-12) with the stride padded with zeros (a zero row scores 0 against every
 * centroid and lands on centroid 0), and the similarity of a (row, centroid) pair is the same k-ordered fp32 MFMA chain (csrc/sim_tile.h)
 * gmp_knn_topk computes for those two rows.  No [n, kc] array exists unless matrix_out is given.
 * gmp_kmeans_assign: labels [n] int64 = the centroid of greatest similarity, ties to the lower centroid index (integer compares on
 *   (score bits, ~index), a total order), sim [n] = that similarity.  matrix_out: NULL or [n, kc], every similarity exactly as the
 *   selection saw it -- test / diagnostic hook.
 * gmp_kmeans_fit enqueues max_iter Lloyd iterations on `stream` with no host synchronisation:
 *       c = normalize(init);  for it = 1 .. max_iter:  labels_new, sim = assign(xn, c);  changed = (it == 1) ? n : count(labels_new != labels);
 *       labels = labels_new;  if changed == 0: stop (converged);  c = update(xn, labels, c)
 *   update: centroid j = normalize(sum of xn[i] over labels[i] == j), the sum in ascending i (a stable counting sort by label and a
 *   segmented sum, no floating-point atomics: bitwise repeatable, whatever order the workgroups run in); a cluster without rows keeps its
 *   centroid.
 *   After convergence every remaining kernel reads the device-side `changed` word, finds 0 and returns at once.  Outputs: labels and sim of
 *   the last assignment pass; centroids [kc, dim], unit rows from the last update -- a cluster that never had a row keeps its row of
 *   `init` as given (init may be `centroids` itself); info int64 [4] = {iterations run, changed of the last pass, clusters the last update
 *   found empty, 0}.  Every iteration normalises the stored centroids again, so T iterations in one call equal T calls of one iteration,
 *   each started from the centroids of the one before, bit for bit.  One wave sums a cluster's rows, so the update's time grows with the
 *   largest cluster.
 * gmp_contingency: table int64 [na, nb] with table[a[i], b[i]] += 1 over i < n, a and b int64 [n], integer atomics; status int32 [1] counts
 *   the rows with a[i] outside [0, na) or b[i] outside [0, nb), which are left out.  Both are zeroed inside the call.
 * 0 <= n < 2^31, 1 <= kc <= 1024, 1 <= dim <= 256, 1 <= max_iter <= 10000, 1 <= na, nb <= 1024: GMP_ERR_ARG outside those ranges or on a
 * NULL pointer, GMP_ERR_WORKSPACE when workspace_bytes < gmp_kmeans_workspace_bytes(n, kc, dim); nothing is launched then.  n == 0 is a
 * no-op (no output is touched), GMP_OK.  gmp_kmeans_workspace_bytes = 4 (n + 2 kc) dpad + 4 n + 4 kc ceil(n / 256) + 8 kc + a constant below
 * 4 KiB, dpad = dim rounded up to 4 (the normalised rows and centroids, the sums, the sorted row list and the sort's counts per chunk of
 * 256 rows: at most 20 bytes per row beside the normalised copy), 0 for sizes outside the ranges.
 * Asynchronous on `stream`, no allocation, no global state.
 * ------------------------------------------------------------------------- */
size_t gmp_kmeans_workspace_bytes(int64_t n, int kc, int dim);
int gmp_kmeans_assign(const float* x, int64_t n, const float* centroids, int kc, int dim, int64_t* labels, float* sim, float* matrix_out,
                      void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_kmeans_fit(const float* x, int64_t n, const float* init, int kc, int dim, int max_iter, float* centroids, int64_t* labels, float* sim,
                   int64_t* info, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_contingency(const int64_t* a, const int64_t* b, int64_t n, int na, int nb, int64_t* table, int32_t* status, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Softmax regression (the linear-evaluation probe for self-supervised embeddings: a multinomial logistic regression fitted with Adam on
 * frozen rows): x [n, dim] contiguous fp32, labels [n] int64, W [classes, dim], b [classes].  Rows are normalised as gmp_knn_topk and
 * gmp_kmeans_* do, xn_i = x_i / max(||x_i||, 1e-12) with the stride padded with zeros (a zero row scores b alone); the copy is made once
 * per call and lives in the workspace.  All in fp32 unless said otherwise:
 *   logits   z[i, c] = <xn_i, W_c> + b_c, the k-ordered fp32 MFMA chain of csrc/sim_tile.h;  p_i = softmax(z_i) with the row maximum
 *            subtracted;  row loss = logsumexp(z_i) - z[i, y_i]
 *   loss     L = S_L / n + (l2 / 2) sum(W^2), S_L the sum of the row losses
 *   gradient gW = S_W / n + l2 W, gb = S_b / n; S_W[c, :] = the unscaled sum over rows of (p[i, c] - [y_i == c]) xn_i, S_b[c] the sum of
 *            (p[i, c] - [y_i == c]); each entry is divided by n once, a correctly rounded fp32 division.  The ridge term acts on W only.
 *   update   Adam as torch.optim.Adam (no amsgrad) on the [classes, dim + 1] block (W | b): t += 1; m = b1 m + (1 - b1) g;
 *            v = b2 v + (1 - b2) g g; theta -= lr / (1 - b1^t) m / (sqrt(v) / sqrt(1 - b2^t) + eps); b1 = 0.9, b2 = 0.999, eps = 1e-8 (the
 *            two bias corrections in double, as torch computes them)
 * gmp_logreg_fit enqueues `iters` iterations on `stream`, two launches each (the row pass: logits, softmax, loss and the S_W / S_b
 *   partial sums of a workgroup from ONE read of each normalised row; then reduce + ridge + Adam + loss + step count), with no host
 *   synchronisation.  W, b, exp_avg and exp_avg_sq [classes, dim + 1] and step int64 [1] (a device word) are read and written in place;
 *   loss_history [iters]: entry k = L at the parameters before update k of this call.  The row pass runs min(ceil(n / 128), 256) workgroups
 *   that walk the 128-row tiles with a grid stride; each writes its sums to its own workspace slot and the slots are added in ascending
 *   order: no floating-point atomics, so one call of T iterations leaves the same bits as T calls of one, and two runs on the same input
 *   leave the same bits.  A row whose label lies outside [0, classes) contributes nothing and is counted in status int32 [1] (zeroed
 *   inside the call); n in the divisions stays n.  No [n, classes] array exists unless logits_out is given.
 *   Hooks for tests and diagnostics, NULL otherwise: grad_out [classes, dim + 1] = (gW | gb) of the call's LAST iteration exactly as the
 *   update saw it, logits_out [n, classes] = the logits of that iteration.  They change no other output bit.
 * gmp_logreg_predict: the same normalisation and logits; pred [n] int64 = the argmax, ties to the lower class (integer compares on
 *   (score bits, ~class), as gmp_kmeans_assign); logits_out NULL or [n, classes].
 * 0 <= n < 2^31, 2 <= classes <= 32, 1 <= dim <= 256, 1 <= iters <= 10000: GMP_ERR_ARG outside those ranges or on a NULL pointer,
 * GMP_ERR_WORKSPACE when workspace_bytes < gmp_logreg_workspace_bytes(n, classes, dim); nothing is launched then.  n == 0 is a no-op (no
 * output is touched), GMP_OK.  gmp_logreg_workspace_bytes = 4 n dpad + 4 min(ceil(n / 128), 256) slot + a constant below 1 KiB, dpad = dim
 * rounded up to 4, slot = classes dpad + classes + 2 rounded up to 64 (the normalised rows and one slot of partial sums per workgroup of
 * the row pass: at most 8.1 MiB beside the normalised copy), 0 for sizes outside the ranges.  Asynchronous on `stream`, no allocation, no
 * global state.
 * ------------------------------------------------------------------------- */
size_t gmp_logreg_workspace_bytes(int64_t n, int classes, int dim);
int gmp_logreg_fit(const float* x, const int64_t* labels, int64_t n, int classes, int dim, int iters, float lr, float l2, float* W, float* b,
                   float* exp_avg, float* exp_avg_sq, int64_t* step, float* loss_history, int32_t* status, float* grad_out, float* logits_out,
                   void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_logreg_predict(const float* x, int64_t n, const float* W, const float* b, int classes, int dim, int64_t* pred, float* logits_out,
                       void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Label-free statistics of an embedding matrix (csrc/repr_stats.hip): the sums behind uniformity and alignment (Wang & Isola 2020) and the
 * fp64 Gram matrix whose spectrum gives RankMe (Garrido et al. 2023).  z [n, dim] contiguous fp32, 1 <= dim <= 256.  Where rows are
 * normalised it is as gmp_knn_topk does, zn = z / max(||z||, 1e-12): a zero row stays zero and its similarities are 0.  s_ij = <zn_i, zn_j>.
 * Outputs are fp64 sums on the device (the caller divides); every reduction runs in a fixed order without floating-point atomics, so two
 * calls on the same input give equal bits.  Asynchronous on `stream`, no host read-back, no allocation.
 * gmp_repr_pair_stats, 2 <= n <= 2^20, t >= 0: out[0] = the sum over i < j of exp(-2 t (1 - s_ij)) (= exp(-t ||zn_i - zn_j||^2) on unit
 *   rows), out[1] = the sum over i < j of s_ij.  s_ij is the k-ordered fp32 MFMA chain of csrc/sim_tile.h and lives only in accumulators:
 *   no n x n array exists, every unordered pair is computed once.  The 16 values a lane holds of a tile are summed in fp32, everything
 *   above that in fp64.
 * gmp_repr_alignment, 1 <= n <= 2^24, alpha > 0: out[0] = the sum over i of max(0, 2 - 2 s_ii)^(alpha / 2), s_ii = <zn1_i, zn2_i> of the
 *   rows of z1 and z2 [n, dim]; the dot products and norms are accumulated in fp64.
 * gmp_repr_gram, 1 <= n <= 2^24: gram [dim, dim] = Z^T Z and colsum [dim] = the sum of the rows, both fp64, on the raw (not normalised)
 *   rows.  Products and accumulation are fp64 (v_mfma_f64_16x16x4_f64) from fp32 inputs widened on load, so every product is exact; gram
 *   is bitwise symmetric.
 * GMP_ERR_ARG outside those ranges, GMP_ERR_WORKSPACE when the workspace is short; nothing is launched then.
 * gmp_repr_workspace_bytes(n, dim), 1 <= n <= 2^20, serves all three: 4 n dpad (the normalised copy, dpad = dim rounded up to 4) + at most
 *   64 partial Grams of 8 DP^2 bytes (DP = dim rounded up to 32, 64, 128, 192 or 256) + under 1 MiB of partial sums.  0 outside that
 *   range; gmp_repr_alignment and gmp_repr_gram beyond 2^20 rows need no more than gmp_repr_workspace_bytes(2^20, dim).
 * ------------------------------------------------------------------------- */
size_t gmp_repr_workspace_bytes(int64_t n, int dim);
int gmp_repr_pair_stats(const float* z, int64_t n, int dim, float t, double* out, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_repr_alignment(const float* z1, const float* z2, int64_t n, int dim, float alpha, double* out, void* workspace, size_t workspace_bytes,
                       gmp_stream_t stream);
int gmp_repr_gram(const float* z, int64_t n, int dim, double* gram, double* colsum, void* workspace, size_t workspace_bytes,
                  gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Integer counts for the classification metrics of fine-tuning (src/finetune/metrics.py:39-82: accuracy, F1, precision, recall and the
 * one-vs-rest ROC AUC of scikit-learn), from targets [n] int64, predictions [n] int64 and probabilities [n, classes] fp32 contiguous:
 *   confusion  int64 [classes * classes]  entry [t * classes + p] = rows with target t and prediction p
 *   auc_counts int64 [classes * 4]        per class c: n_pos (rows with target c), n_neg (rows with another target), and over the pairs
 *                                         (i, j) with target[i] == c != target[j]: n_greater = how many have prob[i, c] > prob[j, c],
 *                                         n_equal = how many compare equal (AUC_c = (n_greater + n_equal / 2) / (n_pos n_neg))
 *   status     int32 [1]                  rows with a target or prediction outside [0, classes) or a non-finite probability; such rows
 *                                         are left out of every count
 * The outputs are zeroed inside the call.  All sums are integer: the result does not depend on the block order.  The pair count is
 * exhaustive, n^2 compares whatever `classes` is, hence 1 <= n <= 262144; 2 <= classes <= 32.  GMP_ERR_ARG outside those ranges,
 * GMP_ERR_WORKSPACE when workspace_bytes < gmp_cls_counts_workspace_bytes(n, classes) (one int32 per row); nothing is launched then.
 * ------------------------------------------------------------------------- */
size_t gmp_cls_counts_workspace_bytes(int64_t n, int classes);
int gmp_cls_counts(const int64_t* targets, const int64_t* predictions, const float* probabilities, int64_t n, int classes,
                   int64_t* confusion, int64_t* auc_counts, int32_t* status, void* workspace, size_t workspace_bytes,
                   gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Integer counts behind the 12 structural targets of the graph-property task (src/data/graph_properties.py:17-96) for a batch of
 * num_graphs graphs, one workgroup per graph.  The batch is described as for gmp_aug_two_views: ptr int64 [num_graphs + 1] node
 * offsets, eptr int64 [num_graphs + 1] edge offsets, edge_index int64 [2, num_edges] with batch-global ids, grouped by graph.  The
 * targets are those of the SIMPLE UNDIRECTED graph: self loops are dropped, duplicate and mirrored entries merge, in any order.
 * An entry with an endpoint outside its own graph's [ptr[g], ptr[g+1]) is dropped and never dereferenced; every such endpoint is
 * counted in the graph's status word.  eptr is clamped into [0, num_edges].  num_nodes is checked for its sign only (node ids are
 * held against ptr, which lives on the device; a caller that does not know the total may pass 0).
 * counts int64 [num_graphs, 16], per graph:
 *    0  n
 *    1  E, simple undirected edges = (sum of deg) / 2
 *    2  max degree
 *    3  sum of deg
 *    4  sum of deg^2
 *    5  T2 = sum over v of t2[v], t2[v] = sum over u in N(v) of |N(v) & N(u)| (= 2 x triangles through v)
 *    6  Pr = sum of deg (deg - 1)
 *    7  number of connected components
 *    8  diameter of the largest component (ties in size: the component holding the smallest node id); 0 if its size <= 1
 *    9  Sxy = sum over directed adjacency entries (u, v) of deg(u) deg(v)
 *   10  Sx  = sum over directed entries of deg(u)   (= sum of deg^2)
 *   11  Sxx = sum over directed entries of deg(u)^2 (= sum of deg^3)
 *   12  status: bit 0 = the graph is too large for the kernel (n > min(max_graph_nodes, 1024), or ptr decreasing); bits 8.. = the
 *       number of dropped endpoints (saturating at 2^54 - 1)
 *   13-15  reserved, written as 0
 * clustering_sum double [num_graphs]: sum over the nodes with deg >= 2 of t2[v] / (deg(v) (deg(v) - 1)), each term one fp64 division
 * of integers, added in ascending node order by a fixed tree (no float atomic): bitwise reproducible.
 * A graph with status bit 0 set gets ONLY slot 12 written (= 1): its other slots and its clustering_sum keep what the caller left
 * there.  n = 0 and n = 1 are valid (all sums 0, components = n).  max_graph_nodes is the caller's bound on ptr[g+1] - ptr[g]; it
 * selects the launch (n <= 256: an 8 KB bit matrix; n <= 1024: 128 KB, one workgroup per CU) and sizes the LDS.  Needs no workspace
 * (gmp_graph_props_workspace_bytes is 0; workspace may be NULL).  num_graphs == 0 is a no-op; GMP_ERR_ARG on a negative size or a
 * null pointer, before any launch.  All integer sums are order-independent.
 * ------------------------------------------------------------------------- */
size_t gmp_graph_props_workspace_bytes(int num_graphs, int64_t max_graph_nodes);
int gmp_graph_props(const int64_t* ptr, const int64_t* eptr, const int64_t* edge_index, int64_t num_nodes, int64_t num_edges,
                    int num_graphs, int64_t max_graph_nodes, int64_t* counts /* [B,16] */, double* clustering_sum /* [B] */,
                    void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * The Weisfeiler-Lehman subtree baseline of graph classification (Shervashidze et al., JMLR 2011; csrc/wl.hip): hashed colour refinement
 * of a batch of graphs, one workgroup per graph, and the exact subtree kernel between two refined batches.  Integer arithmetic only.
 * All arithmetic is on unsigned 64-bit words modulo 2^64.  mix is the splitmix64 finaliser,
 *   z ^= z >> 30; z *= 0xBF58476D1CE4E5B9; z ^= z >> 27; z *= 0x94D049BB133111EB; z ^= z >> 31,
 * and K1 = 0x9E3779B97F4A7C15, K2 = 0xD1B54A32D192ED03.
 * The batch: ptr int64 [num_graphs + 1] node offsets (as for gmp_graph_props), a simple undirected CSR over the batch's nodes, rowptr int32
 * [num_nodes + 1] and col int32 [nnz] under the contract of gmp_lp_cn_score / gmp_graph_simple_check (rowptr is clamped to [0, nnz]),
 * and labels int64 [num_nodes] or NULL: with NULL a node's label is its degree in the CSR counted inside its own graph.  An entry of col
 * outside its row's own graph [ptr[g], ptr[g+1]) is skipped, never dereferenced, and counted in the graph's status word.
 *   c_0[v]     = mix(label[v] + K1)
 *   c_{t+1}[v] = mix(c_t[v] * K1 + (the sum over u in N(v) of mix(c_t[u])) + (t + 1) * K2),   t = 0 .. iters - 1.
 * The neighbour sum is commutative and exact, so the result does not depend on neighbour order, node numbering or scheduling.
 * gmp_wl_refine writes, for 0 <= iters <= 7 and 1 <= dim <= 256:
 *   colors int64 [iters + 1, num_nodes]  the colour bits c_t[v] (optional, NULL to skip: a diagnostic and test hook);
 *   sorted int64 [(iters + 1) * num_nodes]  graph g owns [(iters + 1) ptr[g], (iters + 1) ptr[g+1]): all its (iters + 1) n_g colours in
 *     ascending UNSIGNED order -- the exact feature map in sparse form;
 *   hist int32 [num_graphs, dim]  hist[g, b] = the number of (node, iteration) colours c of g with b = (uint32(c >> 32) * dim) >> 32 --
 *     the hashed feature map;
 *   status int32 [num_graphs]  bit 0 = the graph is refused: n_g > min(max_graph_nodes, 1024), ptr decreasing, or its node range leaves
 *     [0, num_nodes]; bits 8.. = the number of skipped entries (saturating at 2^23 - 1).  A graph with bit 0 set gets ONLY its status
 *     written: its parts of colors, sorted and hist keep what the caller left there.
 * n_g = 0 and 1 are valid.  max_graph_nodes is the caller's bound on ptr[g+1] - ptr[g]; it selects the launch (n <= 256: 256 threads, at
 * most 21 KiB of LDS; n <= 1024: 1024 threads, at most 81 KiB) and sizes the LDS.  No workspace (gmp_wl_workspace_bytes is 0; workspace may
 * be NULL).
 * gmp_wl_gram: K int64 [num_graphs_a, num_graphs_b], K[i, j] = the number of pairs (x in segment i of sorted_a, y in segment j of
 * sorted_b) with x == y -- the WL subtree kernel, the sum over iterations and colours of count_i * count_j -- between two `sorted` arrays
 * of gmp_wl_refine made with the same iters (they may be the same array); len_a / len_b = the int64 words in each array, to which the
 * segments are clamped.  One wave per entry, equal runs counted by binary searches, int64 products, no atomics.  On unsorted input the
 * result is wrong, but nothing outside the arrays is read.
 * Both: asynchronous on `stream`, no allocation, no global state, no host read-back.  GMP_ERR_ARG before any launch on a null pointer
 * (labels and colors may be NULL), iters outside [0, 7], dim outside [1, 256], a negative size, num_nodes or nnz >= 2^31, or a Gram of
 * more than 2^33 entries.  num_graphs == 0, num_graphs_a == 0 and num_graphs_b == 0 are no-ops.
 * ------------------------------------------------------------------------- */
size_t gmp_wl_workspace_bytes(int num_graphs, int64_t max_graph_nodes, int iters);
int gmp_wl_refine(const int64_t* ptr, int num_graphs, const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t nnz,
                  const int64_t* labels, int iters, int dim, int64_t max_graph_nodes, int64_t* colors, int64_t* sorted, int32_t* hist,
                  int32_t* status, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_wl_gram(const int64_t* sorted_a, const int64_t* ptr_a, int64_t num_graphs_a, int64_t len_a, const int64_t* sorted_b,
                const int64_t* ptr_b, int64_t num_graphs_b, int64_t len_b, int iters, int64_t* K, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * The shortest-path kernel baseline of graph classification (Borgwardt & Kriegel, ICDM 2005; csrc/sp.hip): the exact feature map of
 * (label, label, hop distance) triples of a batch of graphs, one workgroup per graph, and the kernel between two batches -- a delta kernel
 * on the two labels and on the distance.  Integer arithmetic only; mix and K1 are those of the Weisfeiler-Lehman block above.
 * The batch is described as for gmp_wl_refine: ptr int64 [num_graphs + 1] node offsets, a simple undirected CSR over the batch's nodes,
 * rowptr int32 [num_nodes + 1] and col int32 [nnz] (rowptr is clamped to [0, nnz]), and labels int64 [num_nodes] or NULL: with NULL a
 * node's label is its degree in the CSR counted inside its own graph.  An entry of col outside its row's own graph [ptr[g], ptr[g+1]) is
 * skipped, never dereferenced, and counted in the graph's status word.  The adjacency is the entries' symmetric closure without self
 * loops, whatever their order and multiplicity.
 * For every unordered pair {u, v} of nodes of one graph with hop distance 1 <= d <= max_dist (1 <= max_dist <= 1023; the search stops
 * after max_dist levels, unreachable pairs count nowhere), with lo <= hi the two labels, both in [0, 2^24):
 *   key = (lo << 35) | (hi << 11) | d          (exact: nothing is hashed)
 * gmp_sp_features writes, with the caller's row stride cap (1 <= cap <= gmp_sp_max_unique(max_graph_nodes)) and 1 <= dim <= 256:
 *   keys   int64 [num_graphs, cap]  the graph's distinct keys in ascending order;
 *   counts int32 [num_graphs, cap]  the number of pairs per key;
 *   nuniq  int32 [num_graphs]       the number of distinct keys;
 *   hist   int32 [num_graphs, dim]  hist[g, b] = the sum of counts over the keys with b = (uint32(mix(key + K1) >> 32) * dim) >> 32 -- the
 *     hashed feature map;
 *   status int32 [num_graphs]  bit 0 = the graph is refused for its size: n_g > min(max_graph_nodes, 1024), ptr decreasing, or its node
 *     range leaves [0, num_nodes]; bit 1 = it has more than cap distinct keys; bit 2 = a label lies outside [0, 2^24); bits 8.. = the
 *     number of skipped entries (saturating at 2^23 - 1).
 * A graph with any of bits 0 - 2 set gets its status and nuniq[g] = 0 written and nothing else: its rows of keys, counts and hist keep what
 * the caller left there, as do the entries of every row at and beyond nuniq[g].  n_g = 0 and 1 are valid and have no pairs.  The result
 * does not depend on node numbering, neighbour order or scheduling.
 * max_graph_nodes is the caller's bound on ptr[g+1] - ptr[g]; it selects the launch (n <= 256: 256 threads; n <= 1024: 1024 threads, one
 * workgroup per CU) and, with cap, sizes the LDS: the n x n bit matrix, the labels and a table of 2^k >= 2 cap slots of 12 bytes.
 * gmp_sp_max_unique(max_graph_nodes) is the largest cap the launch accepts: 4096 up to 256 nodes, 1024 above.  No workspace
 * (gmp_sp_workspace_bytes is 0; workspace may be NULL).
 * gmp_sp_gram: K int64 [num_graphs_a, num_graphs_b], K[i, j] = the sum over the keys present in row i of a and in row j of b of
 * count_a * count_b, between two outputs of gmp_sp_features with row strides cap_a and cap_b in [1, 4096] (they may be the same arrays).
 * One wave per entry, the shorter row binary-searched in the longer, int64 products, no atomics.  nuniq is clamped to [0, cap]: on unsorted
 * input the result is wrong, but nothing outside the rows is read.
 * Both: asynchronous on `stream`, no allocation, no global state, no host read-back.  GMP_ERR_ARG before any launch on a null pointer
 * (labels may be NULL), max_dist outside [1, 1023], dim outside [1, 256], cap outside its range, a negative size, num_nodes or nnz >= 2^31,
 * or a Gram of more than 2^33 entries.  num_graphs == 0, num_graphs_a == 0 and num_graphs_b == 0 are no-ops.
 * ------------------------------------------------------------------------- */
size_t gmp_sp_workspace_bytes(int num_graphs, int64_t max_graph_nodes);
int gmp_sp_max_unique(int64_t max_graph_nodes);
int gmp_sp_features(const int64_t* ptr, int num_graphs, const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t nnz,
                    const int64_t* labels, int max_dist, int dim, int64_t max_graph_nodes, int cap, int64_t* keys, int32_t* counts,
                    int32_t* nuniq, int32_t* hist, int32_t* status, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_sp_gram(const int64_t* keys_a, const int32_t* counts_a, const int32_t* nuniq_a, int64_t num_graphs_a, int cap_a,
                const int64_t* keys_b, const int32_t* counts_b, const int32_t* nuniq_b, int64_t num_graphs_b, int cap_b, int64_t* K,
                gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Degree-normalised propagation of a narrow matrix over a graph, iterated with a teleport term (csrc/label_prop.hip): label spreading
 * (Zhou et al. 2004), label propagation (Zhu & Ghahramani 2002), and the smoothing step of APPNP and Correct-and-Smooth.
 * The graph is a CSR, rowptr int32 [n + 1] and col int32 [nnz]; left and right are fp32 [n] scales, NULL = all ones; f0 and f_init are
 * contiguous fp32 [n, classes], f_init NULL = f0; clamp is uint8 [n] or NULL.  All arithmetic is IEEE fp32, every multiply and every add
 * rounded on its own (no fused multiply-add), subnormals kept.  F(0) = f_init.  For round t = 0 .. rounds - 1, row i, class c:
 *   acc = 0;  for k = rowptr[i] .. rowptr[i+1] - 1, ASCENDING:  j = col[k];  acc = acc + (right[j] * F(t)[j, c])
 *   v   = left[i] * acc
 *   o   = (alpha * v) + (beta * f0[i, c])
 *   F(t+1)[i, c] = clamp && clamp[i] ? f0[i, c] : o
 *   residual[t]  = max over i, c of |F(t+1)[i, c] - F(t)[i, c]|
 * out [n, classes] = F(rounds).  pred int64 [n] (or NULL) = the argmax of each row of out, ties to the lower class, by integer compares on
 * (score bits made orderable, ~class) as gmp_kmeans_assign compares.  residual fp32 [rounds] or NULL.  status int32 [2], zeroed inside the
 * call: status[0] = the number of CSR entries whose col lies outside [0, n) -- counted once, skipped (not added as zero) in every round;
 * status[1] = the number of rows of out whose maximum is not > 0: the nodes no label reached.  rowptr is clamped to [0, nnz], so a
 * malformed CSR gives wrong numbers but reads nothing outside col.
 * Determinism: a row's sum is sequential in ascending k, there is no floating-point atomic, and the residual is an integer atomic max on
 * the bit pattern of a non-negative float.  So two calls leave the same bits, and one call of T rounds leaves the bits of T calls of one
 * round, each fed the previous out as f_init.
 * One launch per round (round t + 1 reads all of round t; there is no in-kernel grid barrier), all enqueued on `stream` without a host
 * synchronisation; F ping-pongs between two [n, classes] buffers in the workspace and the last round writes out, pred and status[1].
 * 0 <= n < 2^31, 0 <= nnz < 2^31, 1 <= classes <= 32, 1 <= rounds <= 10000: GMP_ERR_ARG outside those ranges, on a null required pointer
 * (rowptr, f0, out, status; col when nnz > 0) and when out overlaps f0 or f_init; GMP_ERR_WORKSPACE when the workspace is smaller than
 * gmp_label_propagate_workspace_bytes(n, classes) (0 for sizes out of range).  Nothing is launched in an error case.  n == 0 returns
 * GMP_OK and writes nothing.  Asynchronous, no allocation, no global state.
 * ------------------------------------------------------------------------- */
size_t gmp_label_propagate_workspace_bytes(int64_t n, int classes);
int gmp_label_propagate(const int32_t* rowptr, const int32_t* col, int64_t n, int64_t nnz, const float* left, const float* right,
                        const float* f0, const float* f_init, const uint8_t* clamp, int classes, int rounds, float alpha, float beta,
                        float* out, int64_t* pred, float* residual, int32_t* status, void* workspace, size_t workspace_bytes,
                        gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Degree-scaled propagation of a WIDE feature matrix over a graph (csrc/feature_prop.hip): H <- diag(left) A diag(right) H, `rounds`
 * times -- with A = adjacency + I and left = right = 1 / sqrt(deg + 1) the S^K X of SGC (Wu et al. 2019).
 * The graph is a CSR, rowptr int32 [n + 1] and col int32 [nnz]; left and right are fp32 [n] scales, NULL = all ones.  The features come
 * in exactly one of two forms: dense, x fp32 [n, d] with leading dimension ldx (x_rowptr, x_col, x_val NULL), or CSR, x_rowptr int32
 * [n + 1], x_col int32 [x_nnz], x_val fp32 [x_nnz] (x NULL; ldx is ignored).  All arithmetic is IEEE fp32, every multiply and every add
 * rounded on its own (no fused multiply-add), subnormals kept.  H(0) = X.  For round t = 0 .. rounds - 1, row i, column c:
 *   acc = +0;  for k = rowptr[i] .. rowptr[i+1] - 1, ASCENDING:  j = col[k];  acc = acc + (right[j] * H(t)[j, c])
 *   H(t+1)[i, c] = left[i] * acc
 * out [n, d] (leading dimension ldo) = H(rounds).  Per column this is gmp_label_propagate with alpha = 1, beta = 0 and no clamp, with
 * the same bits.  Self-loops are the caller's business: ordinary CSR entries at their sorted position.
 * status int32 [2], zeroed inside the call.  status[0] = the number of adjacency entries whose col lies outside [0, n): counted once
 * (in round 1), skipped -- not added as zero -- in every round.  status[1] = the number of stored feature entries that break the CSR
 * form's contract (0 with dense features): a feature row's columns must be strictly ascending, and an entry x_col[e] outside [0, d) or
 * not greater than the stored x_col[e - 1] of the same row is skipped and counted, once per entry.  (A row that holds one column twice
 * AROUND a skipped entry -- 5, 3, 5 -- keeps both and is outside the contract: status[1] is non-zero, and which term that column sees is
 * unspecified.)  rowptr and x_rowptr are clamped to [0, nnz] and [0, x_nnz], so a malformed CSR gives wrong numbers but reads nothing
 * outside col, x_col and x_val.
 * CSR features and dense features agree bit for bit: for finite inputs the CSR form leaves the bits the dense form leaves on the
 * densified matrix.  The first round with CSR features visits a neighbour's stored entries only; the terms it leaves out are
 * right[j] * 0 = +-0, the accumulator starts at +0 and can never become -0 (x + (-x) rounds to +0), and acc + (+-0) = acc, so a skipped
 * r * 0 term changes nothing.  A stored explicit zero is added as the dense form adds it.
 * Determinism: a row's sum is sequential in ascending k and there is no floating-point atomic.  Two calls leave the same bits, and one
 * call of T rounds leaves the bits of T chained calls of one round.
 * One launch per round (there is no in-kernel grid barrier), all enqueued on `stream` without a host synchronisation.  H ping-pongs
 * between min(rounds - 1, 2) buffers of n x dpad floats (dpad = d rounded up to 4) in the workspace and the last round writes out, so
 * rounds == 1 needs no workspace (ws may be NULL); x is never written.  Loads and stores are single dwords: ldx and ldo may be any value
 * >= d, multiples of 4 or not (CiteSeer's rows are 3,703 floats), bases need 4-byte alignment only, row offsets j * ld are 64-bit, and
 * the columns [d, ldo) of out are not touched.
 * 0 <= n < 2^31, 0 <= nnz, x_nnz < 2^31, 1 <= d <= 16384, 1 <= rounds <= 64.  GMP_ERR_ARG, with nothing launched: a size outside those
 * ranges, both feature forms or neither, ldx < d (dense) or ldo < d, a null required pointer (rowptr, out, status; col when nnz > 0;
 * x_col and x_val when x_nnz > 0), out overlapping x (x_val) or the workspace, or a workspace smaller than
 * gmp_feature_propagate_workspace_bytes(n, d, rounds) (0 for sizes out of range and for rounds == 1).  n == 0 returns GMP_OK and writes
 * nothing.  Asynchronous, no allocation, no global state.
 * ------------------------------------------------------------------------- */
size_t gmp_feature_propagate_workspace_bytes(int64_t n, int32_t d, int32_t rounds);
int gmp_feature_propagate(const int32_t* rowptr, const int32_t* col, int64_t n, int64_t nnz, const float* left, const float* right,
                          const float* x, int64_t ldx, const int32_t* x_rowptr, const int32_t* x_col, const float* x_val, int64_t x_nnz,
                          int32_t d, int32_t rounds, float* out, int64_t ldo, int32_t* status, void* ws, size_t ws_bytes,
                          gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * The pooled-feature map of a batch of graphs (csrc/graph_feat.hip): the sum, mean and max pools of X, S X, .. S^rounds X per graph --
 * what the structure-blind baseline of Errica et al. (ICLR 2020) reads at rounds = 0, and SGC's features (Wu et al. 2019) pooled and
 * concatenated over the scales as in SIGN (Frasca et al. 2020) above it.  One launch per batch, one workgroup per (graph, strip of 16
 * columns).
 * The batch: ptr int64 [num_graphs + 1] node offsets (clamped to [0, num_nodes]); ONE CSR over all num_nodes nodes, rowptr int32
 * [num_nodes + 1] (clamped to [0, nnz]) and col int32 [nnz]; left and right fp32 [num_nodes] scales, NULL = all ones; x fp32
 * [num_nodes, d] with leading dimension ldx.  Self-loops are the caller's business, as for gmp_feature_propagate.
 * All arithmetic is IEEE fp32, every multiply and every add rounded on its own (no fused multiply-add), subnormals kept.  H(0) = X.
 * For round t = 0 .. rounds - 1, graph g with the window [b, e) = [ptr[g], ptr[g+1]), row i in the window, column c:
 *   acc = +0;  for k = rowptr[i] .. rowptr[i+1] - 1, ASCENDING:  j = col[k]
 *              if b <= j < e:  acc = acc + (right[j] * H(t)[j, c])      else: skipped by a select (not added as zero) and counted
 *   H(t+1)[i, c] = left[i] * acc
 * and for every t = 0 .. rounds the three pools over the graph's n_g = e - b rows:
 *   sum [g, t, c]:  s = +0;  for i = b .. e - 1, ASCENDING:  s = s + H(t)[i, c]
 *   mean[g, t, c]:  sum / (float)n_g      (one correctly rounded division; n_g = 0 gives +0)
 *   max [g, t, c]:  the largest H(t)[i, c] under the integer order on the orderable bit pattern that gmp_label_propagate's argmax uses
 *                   (so -0 < +0; n_g = 0 gives +0)
 * out fp32, contiguous, [num_graphs, rounds + 1, 3, d], pool order sum, mean, max.
 * On a well-formed batch no entry leaves its graph; H(t) then has the bits gmp_feature_propagate leaves over the whole batch.  Inputs are
 * finite by contract: non-finite values give unspecified numbers, never an access out of range.
 * status int32 [num_graphs], written inside the call.  Bit 0 = the graph has more nodes than the call takes -- more than 1024 or more
 * than max_graph_nodes, the caller's bound on ptr[g+1] - ptr[g]: all its outputs are +0.  Bits 8 .. 30 = the number of skipped adjacency
 * entries of the graph, each counted once (in round 1, by the workgroup of the first strip), saturating at 2^23 - 1; rounds == 0 reads no
 * adjacency entry and counts none.  A malformed rowptr or ptr gives wrong numbers and reads nothing outside the arrays.
 * max_graph_nodes selects the launch: graphs up to 256 nodes take a workgroup of 256 threads, graphs up to 1024 nodes one of 1024; a
 * bound above 256 launches both and each workgroup leaves at once when its graph belongs to the other.  It also sizes the LDS, which holds
 * the two ping-pong copies of the graph's strip of H and its left and right from the first load to the last pool: global memory sees x
 * once, the CSR rows once per round, and the [rounds + 1, 3, 16] results.
 * Determinism: every sum is sequential, there is no floating-point atomic (the skipped entries are counted by an integer atomic in LDS),
 * so two calls leave the same bits.
 * 0 <= num_graphs, 0 <= num_nodes, nnz < 2^31, 1 <= d <= 256, 0 <= rounds <= 16, 0 <= max_graph_nodes.  GMP_ERR_ARG, with nothing launched:
 * a size outside those ranges, a null required pointer (ptr, rowptr, out, status; col when nnz > 0; x when num_nodes > 0), ldx < d, or out
 * overlapping x.  num_graphs == 0 returns GMP_OK and writes nothing.  Asynchronous, no allocation, no global state, no workspace.
 * ------------------------------------------------------------------------- */
int gmp_graph_feature_map(const int64_t* ptr, int num_graphs, const int32_t* rowptr, const int32_t* col, int64_t num_nodes, int64_t nnz,
                          const float* left, const float* right, const float* x, int64_t ldx, int32_t d, int32_t rounds,
                          int64_t max_graph_nodes, float* out, int32_t* status, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * The fused graph-classification head of fine-tuning (finetune_model.py:68-80, finetune.py:110-114) over one batch of
 * num_graphs graphs; graph b owns the rows ptr[b] .. ptr[b+1] of h (ptr: device int32 [num_graphs + 1]):
 *   pooled[b] = mean of the graph's rows, divisor max(count, 1) (gmp_segment_sum(mean = 1); an empty graph pools to zero),
 *   act = relu(pooled w0^T + b0) [B, hidden] (the pre-dropout activation, kept for the backward; w0 [hidden, feat] row-major),
 *   logits = dropout(act) w3^T + b3 [B, classes] (w3 [classes, hidden]),
 *   loss (device float[1]) = cross-entropy sum over the batch (classes > 2; target int64 [B], a label outside [0, classes) adds
 *   nothing) or the BCE-with-logits sum on logits[:, 1] (classes == 2: target 0 / 1, logits[:, 0] gets a zero gradient),
 *   g_logits [B, classes] = d loss / d logits scaled by the device word g_scale (1 / B for the mean).
 * Dropout is the mask gmp_dropout_fwd(act, p, seed, site) draws over the contiguous [B, hidden] activation; p == 0: no mask.
 * bwd (the mask is regenerated) writes g_w0 [hidden, feat], g_b0 [hidden], g_w3 [classes, hidden], g_b3 [classes] (pointers into
 * the caller's gradient buffer) and EVERY row of g_h [num_nodes, feat] (leading dimension ldg): g_pooled[graph(i)] / max(count, 1),
 * zero for a row no graph owns -- no zero-fill, no scatter.
 * feat == 256, hidden == 128, 2 <= classes <= 16 (GMP_ERR_UNSUPPORTED otherwise), num_graphs >= 1.  fp32; every sum in a fixed
 * order (no atomics): bitwise reproducible.  Three launches in all (fwd two, bwd one), nothing read back.  ptr entries are
 * clamped into [0, num_nodes].  h, w0, w3, pooled, act, g_h 16-byte aligned, ldh / ldg multiples of 4.
 * ------------------------------------------------------------------------- */
size_t gmp_gc_head_fwd_workspace_bytes(int64_t num_graphs);
int gmp_gc_head_fwd(const float* h, int64_t ldh, const int32_t* ptr, int64_t num_nodes, int64_t num_graphs, int feat_dim, int hidden,
                    int classes, const float* w0, const float* b0, const float* w3, const float* b3, const int64_t* target,
                    const float* g_scale, float* pooled, float* act, float* logits, float* loss, float* g_logits, float p,
                    uint64_t seed, uint32_t site, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_gc_head_bwd(const int32_t* ptr, int64_t num_nodes, int64_t num_graphs, int feat_dim, int hidden, int classes, const float* w0,
                    const float* w3, const float* pooled, const float* act, const float* g_logits, float p, uint64_t seed,
                    uint32_t site, float* g_w0, float* g_b0, float* g_w3, float* g_b3, float* g_h, int64_t ldg, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * NT-Xent / InfoNCE (tasks.py:192-213, 265-287).
 *   z = [normalize(z1); normalize(z2)]  (eps 1e-12), sim = z z^T / T, diag = -inf,
 *   loss_sum = sum_i CE(sim[i,:], pos_i),  pos_i = (i + n) mod 2n.
 * fwd writes loss_sum (device float[1]); bwd returns d loss_sum / d z1, d z2 scaled
 * by `g_scale` (device float[1], the upstream gradient).  n <= 8192.
 * An index outside [0, num_src_rows) in gmp_row_gather / gmp_lp_edge_features_* reads
 * as a zero row instead of faulting.
 * ------------------------------------------------------------------------- */
size_t gmp_nt_xent_workspace_bytes(int64_t n, int dim);
int gmp_nt_xent_fwd(const float* z1, const float* z2, int64_t n, int dim, float temperature,
                    float* loss_sum, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_nt_xent_bwd(const float* z1, const float* z2, int64_t n, int dim, float temperature,
                    const float* g_scale, float* g_z1, float* g_z2,
                    void* workspace /* the one fwd filled */, size_t workspace_bytes, gmp_stream_t stream);

/* The same loss and gradient without the [2n, 2n] similarity matrix (flash-attention style: similarity tiles live in registers /
 * LDS only, the workspace is O(n * dim)).  Arguments and conventions are those of gmp_nt_xent_fwd / _bwd; the backward reads the
 * normalised rows and the per-row log-sum-exp the forward left in the workspace.  dim: a multiple of 4 in [4, 256];
 * 1 <= n <= (INT32_MAX - 128) / 2 (int32 row indexing of the 2n rows).  Bad arguments and a short workspace are refused before
 * any launch.  Fixed-order reductions: bitwise reproducible.  Results agree with the matrix form to fp32 rounding, not bit for bit. */
size_t gmp_nt_xent_stream_workspace_bytes(int64_t n, int dim);
int gmp_nt_xent_stream_fwd(const float* z1, const float* z2, int64_t n, int dim, float temperature,
                           float* loss_sum, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_nt_xent_stream_bwd(const float* z1, const float* z2, int64_t n, int dim, float temperature,
                           const float* g_scale, float* g_z1, float* g_z2,
                           void* workspace /* the one fwd filled */, size_t workspace_bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * MLPHead pieces (heads.py:42-45): Linear -> ReLU -> Dropout.  The ReLU rides in the
 * GEMM epilogue; these two handle the dropout and the fused backward
 *   out = g * dropmask * (act > 0),  act = the ReLU output.  numel % 4 == 0.
 * ------------------------------------------------------------------------- */
int gmp_dropout_fwd(const float* x, float* y, int64_t numel, float p, uint64_t seed, uint32_t stream_id,
                    gmp_stream_t stream);
int gmp_relu_dropout_bwd(const float* g, const float* act, float* out, int64_t numel, float p, uint64_t seed,
                         uint32_t stream_id, gmp_stream_t stream);
/* The Linear(hidden, 1) that ends the link-prediction scorer (src/models/heads.py:45-52, behind ReLU + dropout) as what it is -- a dot
 * product per row, an outer product, a weighted column sum -- instead of three GEMM-path launches with N = 1:
 *   gmp_dropout_rowdot_fwd:      dropped = dropout(x) (written when p > 0; may be NULL otherwise), y[m] = <dropped[m, :], w> + bias[0]
 *   gmp_outer_relu_dropout_bwd:  out[m, c] = g[m] * w[c] * dropout_mask * (act[m, c] > 0)   (same site / seed as the forward)
 *   gmp_weighted_colsum:         out_w[c] = sum_m g[m] * x[m, c], out_b[0] = sum_m g[m] (nullable); two ordered stages, deterministic */
int gmp_dropout_rowdot_fwd(const float* x, const float* w, const float* bias, float* dropped, float* y, int64_t rows, int feat, float p,
                           uint64_t seed, uint32_t stream_id, gmp_stream_t stream);
int gmp_outer_relu_dropout_bwd(const float* g, const float* w, const float* act, float* out, int64_t rows, int feat, float p,
                               uint64_t seed, uint32_t stream_id, gmp_stream_t stream);
size_t gmp_weighted_colsum_workspace_bytes(int64_t rows, int feat);
int gmp_weighted_colsum(const float* g, const float* x, float* out_w, float* out_b, int64_t rows, int feat, void* workspace,
                        size_t workspace_bytes, gmp_stream_t stream);

/* The same layer over MERGED link-prediction rows.  The scorer's features [hs + hd, hs * hd, |hs - hd|] (src/models/heads.py:57-61) are
 * symmetric in (src, dst), so the engine sends one row per unordered pair through Linear(768, 256) + ReLU; but the reference scores an
 * ORDERED list (src/pretrain/tasks.py:111-120: positives in both directions, then the negatives) and its Dropout(0.2) (heads.py:44-52) draws
 * an independent mask for every row of that list.  A merged row therefore carries the one or two ordered rows it stands for:
 * pos[m] = position of its first occurrence in the reference's list, pos[rows + m] = of its second, or -1.  Masks are keyed by
 * (seed, stream_id, ordered position * feat / 4 + column quad) -- the key gmp_dropout_rowdot_fwd uses when it is run over the ordered list --
 * so every ordered row gets the mask, the score and the loss term the unmerged path gives it (scores bit for bit).
 *   gmp_lp_pair_rowdot_fwd:       y2[m] / y2[rows + m] = <dropout_{first / second}(x[m, :]), w> + bias[0]   (second = first when p == 0)
 *   gmp_lp_pair_sigmoid_bce_fwd_bwd (losses): loss = sum over ordered rows of BCE(sigmoid(y2), sign[m] > 0) with torch's -100 clamp,
 *                                 g_y2 = d (g_scale * loss) / d y2 (zero where there is no second occurrence), p_out nullable [2 rows]
 *   gmp_lp_pair_outer_bwd:        out[m, c] = (act[m, c] > 0) * w[c] * (g_y2[m] * mask_first + g_y2[rows + m] * mask_second)
 *   gmp_lp_pair_weighted_colsum:  out_w[c] = sum_m act[m, c] * (g_y2[m] * mask_first + g_y2[rows + m] * mask_second),
 *                                 out_b[0] = sum_m g_y2[m] + g_y2[rows + m]  (nullable); two ordered stages, deterministic
 * feat % 4 == 0, feat <= 256.  workspace >= gmp_lp_pair_colsum_workspace_bytes(rows, feat). */
int gmp_lp_pair_rowdot_fwd(const float* x, const float* w, const float* bias, const int32_t* pos, float* y2, int64_t rows, int feat, float p,
                           uint64_t seed, uint32_t stream_id, gmp_stream_t stream);
int gmp_lp_pair_sigmoid_bce_fwd_bwd(const float* y2, const float* sign, const int32_t* pos, int64_t rows, const float* g_scale, float* loss,
                                    float* p_out, float* g_y2, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_lp_pair_outer_bwd(const float* g_y2, const float* w, const float* act, const int32_t* pos, float* out, int64_t rows, int feat, float p,
                          uint64_t seed, uint32_t stream_id, gmp_stream_t stream);
size_t gmp_lp_pair_colsum_workspace_bytes(int64_t rows, int feat);
int gmp_lp_pair_weighted_colsum(const float* g_y2, const float* act, const int32_t* pos, float* out_w, float* out_b, int64_t rows, int feat,
                                float p, uint64_t seed, uint32_t stream_id, void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* Grouped form: the per-domain problems of one contrastive task (tasks.py:192-213, 265-287 loop over domains) in 7 launches
 * instead of 7 per domain; forward and backward in one call.  Group g's 2*n_host[g] rows [z1; z2] start at row
 * row_off_host[g] of z [*, dim] and its gradient goes to the same rows of g_z; loss_sums[g] (nullable) receives the group's
 * loss sum, loss_total (nullable) their sum in group order.  groups <= 8; n may be 0 for a group.  Per group the gradients
 * are bit for bit those of gmp_nt_xent_fwd / _bwd (zero padding adds nothing); the loss sums add the same row losses in another order. */
size_t gmp_nt_xent_grouped_workspace_bytes(int groups, int64_t max_n, int dim);
int gmp_nt_xent_grouped(const float* z, float* g_z, int groups, const int32_t* n_host, const int64_t* row_off_host, int dim,
                        float temperature, const float* g_scale, float* loss_sums, float* loss_total, void* workspace,
                        size_t workspace_bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Task losses (sum reductions; the caller divides by the pooled size, tasks.py:84-93).
 *   mse_sum          F.mse_loss(a, b, reduction='sum')               tasks.py:83,305
 *   sigmoid          torch.sigmoid of the edge scores                heads.py:67
 *   bce_sum          F.binary_cross_entropy(p, y, 'sum'), log terms clamped at -100,
 *                    backward g*(p-y)/max(p(1-p),1e-12) as torch does  tasks.py:120
 *   cross_entropy_sum F.cross_entropy(logits, target, 'sum')         tasks.py:336, finetune.py:158,177
 *   *_bwd take the upstream scalar gradient as device float[1] g_scale.
 *   workspace >= gmp_loss_workspace_bytes(numel or rows).
 * gmp_row_fill: dst[idx[m],:] = broadcast ? src[0,:] : src[m,:]  (mask-token rows,
 *   pretrain_model.py:82-85); out-of-range idx entries are skipped.
 * ------------------------------------------------------------------------- */
size_t gmp_loss_workspace_bytes(int64_t numel);
int gmp_mse_sum_fwd(const float* a, const float* b, int64_t numel, float* loss, void* workspace,
                    size_t workspace_bytes, gmp_stream_t stream);
int gmp_mse_sum_bwd(const float* a, const float* b, const float* g_scale, float* g_a, int64_t numel,
                    gmp_stream_t stream);
int gmp_sigmoid_fwd(const float* x, float* y, int64_t numel, gmp_stream_t stream);
int gmp_sigmoid_bwd(const float* g, const float* y, float* out, int64_t numel, gmp_stream_t stream);
int gmp_bce_sum_fwd(const float* p, const float* labels, int64_t numel, float* loss, void* workspace,
                    size_t workspace_bytes, gmp_stream_t stream);
int gmp_bce_sum_bwd(const float* p, const float* labels, const float* g_scale, float* g_p, int64_t numel,
                    gmp_stream_t stream);
/* sigmoid_fwd + bce_sum_fwd + bce_sum_bwd + sigmoid_bwd in one pass over the scores x (same arithmetic, element by element):
 * loss = BCE(sigmoid(x), labels) summed, g_x = d (g_scale * loss) / d x; p_out (nullable) receives sigmoid(x). */
int gmp_sigmoid_bce_sum_fwd_bwd(const float* x, const float* labels, int64_t numel, const float* g_scale, float* loss,
                                float* p_out, float* g_x, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
/* The same pass over pairs that carry a multiplicity: signed_weight[i] = +w for a positive pair, -w for a negative pair, w >= 1 the
 * number of times the pair stands in the reference's list (the scorer of src/models/heads.py:57-67 is symmetric in (src, dst), so
 * (i, j) and (j, i) need scoring once); loss term and g_x[i] are scaled by w.  With w = 1 everywhere: the call above, bit for bit. */
int gmp_sigmoid_bce_signed_sum_fwd_bwd(const float* x, const float* signed_weight, int64_t numel, const float* g_scale, float* loss,
                                       float* p_out, float* g_x, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_cross_entropy_sum_fwd(const float* logits, const int64_t* target, int64_t rows, int classes,
                              float* loss, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_cross_entropy_sum_bwd(const float* logits, const int64_t* target, int64_t rows, int classes,
                              const float* g_scale, float* g_logits, gmp_stream_t stream);
int gmp_row_fill(float* dst, const int64_t* idx, const float* src, int64_t num_idx, int64_t num_dst_rows,
                 int feat, int broadcast, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Hard-negative mining for link-prediction fine-tuning
 * (finetune.py:45-75, LinkPredictionHardNegativeMiner.mine_hard_negatives_for_edges; called per
 * training batch from finetune.py:190-196).
 *   zn = F.normalize(emb, dim=1) (eps 1e-12); S = zn zn^T; pairs (s,d) and (d,s) of
 *   existing_edges ([2,E] int64, row 0 = sources) and the diagonal are excluded;
 *   out_edges [2,k] int64 = the k highest-scoring remaining ordered pairs (i,j), sorted by score
 *   descending -- what torch.topk(potential_scores, k) + potential_indices gives.  Ties (S is
 *   symmetric, so every score appears twice) are broken by the LOWER flat index i*n+j; torch.topk
 *   leaves that order unspecified.
 *   out_scores: NULL or [k] float, the selected scores.  scores_out: NULL or [n,n] float, receives the
 *   masked similarity matrix (masked entries = -inf) -- test / diagnostic hook.
 *   The caller guarantees k <= number of unmasked pairs (finetune.py:66-67 clamps it); n <= 65535,
 *   k <= 4096.  workspace >= gmp_hard_negative_workspace_bytes(n, dim).
 * ------------------------------------------------------------------------- */
size_t gmp_hard_negative_workspace_bytes(int64_t n, int64_t dim);
int gmp_hard_negative_topk(const float* emb, int64_t n, int64_t dim, const int64_t* existing_edges, int64_t E,
                           int64_t k, int64_t* out_edges, float* out_scores, float* scores_out,
                           void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* The same contract without the n x n matrix (csrc/hardneg_stream.hip): similarity tiles are recomputed in MFMA
 * accumulators (upper triangle only; a pair i < j stands for the ordered pairs (i,j) and (j,i)) for every pass of the
 * same exact radix select, over the key (score descending, flat index i*n+j ascending, 40 bits).  Once the keys at or above
 * the decided prefix fit a fixed candidate buffer (65,536 keys) the remaining histogram passes return at once, one more tile
 * pass gathers the candidates and the k winners are ranked among them.
 *   1 <= dim <= 256 (any value; GMP_ERR_UNSUPPORTED above), 1 <= n <= 2^20, 0 <= k <= 4096, E >= 0 (GMP_ERR_ARG otherwise).
 *   workspace >= gmp_hard_negative_stream_workspace_bytes(n, dim, E) = O(n dim + E) + a constant below 1 MiB: the normalised
 *   rows, both CSR orientations of existing_edges (gmp_csr_build; endpoints outside [0,n) are ignored) and the candidates.
 *   scores_out: NULL or [n,n], the masked matrix exactly as the selection saw it, written by the same tile code -- the only
 *   n^2 object, and only on request.
 *   If fewer than k unmasked ordered pairs exist, the tail of out_edges is -1 and the tail of out_scores -inf.
 *   Asynchronous on `stream`, no host read-back, no allocation; integer atomics only, and the output is a pure function of
 *   the input.  Scores equal the dense form's bit for bit where the arithmetic is exact; elsewhere the two forms sum the
 *   dim products in different orders.
 *   Diagnostic: after the call has run, the first int32 of the workspace holds the number of histogram passes (tile passes
 *   before the gather) that did work.
 */
size_t gmp_hard_negative_stream_workspace_bytes(int64_t n, int64_t dim, int64_t E);
int gmp_hard_negative_topk_stream(const float* emb, int64_t n, int64_t dim, const int64_t* existing_edges, int64_t E,
                                  int64_t k, int64_t* out_edges, float* out_scores, float* scores_out,
                                  void* workspace, size_t workspace_bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Pack / unpack a fixed list of slices of one buffer into one contiguous message (the data-parallel exchange of per-task
 * gradients: only the (task, tensor) pairs that carry a gradient travel).  table_dev: device int64 [2n+1] = n source offsets
 * (floats into base) followed by the n+1 exclusive prefix sums of the slice lengths; offsets and lengths are multiples of 4;
 * n <= 256; total = prefix[n].  unpack multiplies by `scale` (1 / world size).
 * ------------------------------------------------------------------------- */
int gmp_segments_pack(const float* base, float* packed, const int64_t* table_dev, int n, int64_t total, gmp_stream_t stream);
int gmp_segments_unpack(float* base, const float* packed, const int64_t* table_dev, int n, int64_t total, float scale,
                        gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Host -> device upload of up to 4 small arrays by one kernel (the per-step index arrays: the reference builds them on the
 * CPU, masks / negatives / views at pretrain_model.py:72-80, tasks.py:107-111, augmentations.py:17-111, and moves them with
 * .to(device)).  src_pinned_host[i]: PINNED host memory (hipHostMalloc / torch pin_memory: mapped into the device's address
 * space), dst[i]: device memory, bytes[i]: multiples of 16, all pointers 16-byte aligned; the three arrays are host arrays.
 * The caller keeps a source buffer untouched until the stream has passed the call.
 * ------------------------------------------------------------------------- */
int gmp_upload(int n, const void* const* src_pinned_host, void* const* dst, const int64_t* bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Streams and hardware queues (no reference counterpart: the reference runs everything on one stream).  The runtime maps a
 * process's HIP streams onto a few hardware queues (4 by default) and packets of one queue run in order, so two streams on
 * the same queue never overlap.  gmp_streams_share_queue MEASURES it: a 400 us spin kernel on `a`, an empty kernel on `b`;
 * *share_host = 1 when b's kernel only finished with a's (same queue, or a == b), 0 when it ran beside it.  Synchronises both
 * streams (start-up calibration, not a per-step call).  gmp_spin_us enqueues the busy-wait kernel (diagnostics).
 * ------------------------------------------------------------------------- */
int gmp_streams_share_queue(gmp_stream_t a, gmp_stream_t b, int* share_host);
int gmp_spin_us(int microseconds, gmp_stream_t stream);
/* Device-side gates: cross-stream dependencies without barrier packets.  Measured (scripts/diag_blocked_queues.py): every
 * hardware queue parked on a hipStreamWaitEvent adds ~2 us to every kernel boundary of the queues that are running; a gate --
 * one wave sleeping on flag words -- costs them nothing.  gmp_gate_wait parks one wave on `stream` until flags[i] >= want for
 * every bit i of mask (flags: device int32[64]); after two minutes it gives up and ORs 1 into *err (may be NULL).
 * gmp_gate_open stores `value` to *flag from a kernel on its stream (after everything enqueued there before).  ONLY between
 * streams on different hardware queues (gmp_streams_share_queue): in one in-order queue a gate ahead of its opener never opens. */
int gmp_gate_wait(const int32_t* flags, uint64_t mask, int want, int32_t* err, gmp_stream_t stream);
int gmp_gate_open(int32_t* flag, int value, gmp_stream_t stream);
/* The same signal without a launch of its own: the NEXT gmp_gemm_f32 / gmp_gemm_f32_grouped call made by this host thread stores `value` to
 * *flag when its first workgroup starts -- stream order has then retired everything enqueued on that GEMM's stream before it -- which takes
 * the one-thread launch (4 us + a kernel boundary) off a critical chain (flag NULL: cancel).  gmp_gate_open_pending: 1 while a signal waits
 * for its GEMM (a GEMM call that launched nothing leaves it pending: open the gate with gmp_gate_open then). */
int gmp_gate_open_by_next_gemm(int32_t* flag, int value);
int gmp_gate_open_pending(void);
/* Time-out of the gates enqueued from now on (default: GMP_GATE_TIMEOUT_S seconds, else 120; fractions allowed).  A gate that
 * times out sets *err and lets its stream go on; the engine's data-parallel start-up check (StepEngine.verify_gates) runs
 * its probe steps with a short one so that a stream layout that cannot carry gates shows within seconds. */
int gmp_gate_set_timeout(double seconds);
/* *word += inc on the device, in stream order (one thread).  With gmp_bn_config.seed_dev: a step captured in a hipGraph ends with this
 * launch, so every replay draws the dropout masks of the next step number -- the masks an eager run of that step would draw. */
int gmp_counter_add(uint64_t* word, uint64_t inc, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Stacked input encoders (InputEncoder.linear, gnn.py:14,19) for every segment of a step in one
 * launch.  Features of all domains sit padded to `dpad` (<= 64) columns in x_all [R, dpad]; stacked row
 * r reads x_all[src_row[r]]; segment s belongs to domain seg_dom[s] (weights at params + w_off_host[d],
 * shape [256, d_in_host[d]], bias at params + b_off_host[d]); row_colmask[r] (nullable) bit k = feature k of stacked row r zeroed
 * (attribute-mask augmentation, augmentations.py:17-29).  tiles [num_tiles][2] = (segment, first row),
 * 32 rows each; indices outside [0,num_x_rows) / [0,num_rows) / [0,num_segments) read as zero rows.
 * bwd: one gradient group per (task, domain) pair covering segments
 * group_seg_host[g]..[g+1]; dW lands at grad_out + off_w_host[g] ([256, d_in]), db at + off_b_host[g].
 * An empty group (group_seg_host[g] == [g+1]) writes nothing; a group whose segments have no rows writes zeros.
 * workspace (nullable): groups * 16 * 256 * (DP + 1) floats, DP = dpad rounded up to 8 / 24 / 40 / 64, splits each
 * group's rows over 16 workgroups; without it (or with fewer bytes) one workgroup per group stores directly.
 * Both entry points return GMP_ERR_ARG, before anything is launched, when a d_in_host[d] lies outside [1, dpad];
 * gmp_encoder_bwd also when group_seg_host descends or leaves [0, num_segments].
 * ------------------------------------------------------------------------- */
int gmp_encoder_fwd(const float* x_all, int64_t num_x_rows, int64_t num_rows, int num_segments, const int32_t* src_row, const int32_t* seg_ptr, const int32_t* seg_dom,
                    const uint64_t* row_colmask, const int32_t* tiles, int num_tiles, const float* params,
                    int num_domains, const int64_t* w_off_host, const int64_t* b_off_host,
                    const int32_t* d_in_host, int dpad, float* z, gmp_stream_t stream);
int gmp_encoder_bwd(const float* x_all, int64_t num_x_rows, int64_t num_rows, int num_segments, const int32_t* src_row, const int32_t* seg_ptr, const int32_t* seg_dom,
                    const uint64_t* row_colmask, const float* g_z, int num_domains, const int32_t* d_in_host,
                    int dpad, int groups, const int32_t* group_seg_host, const int64_t* off_w_host,
                    const int64_t* off_b_host, float* grad_out, void* workspace, size_t workspace_bytes,
                    gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Sparse (CSR) input for InputEncoder.linear (gnn.py:17-22) on the Planetoid domains, whose bag-of-words
 * features keep ~1 % of their entries after NormalizeFeatures (data_setup.py:154).  Opt-in; the dense GEMM
 * path is untouched.
 *   X [N, K]: CSR rowptr int32 [N+1], col int32 [nnz], val fp32 [nnz] (columns need not be sorted).
 *   W [H, ldw] row-major (nn.Linear layout), ldw >= K: the fine-tune engine's K-padded slot works as is.
 *   H (out_features) must be a multiple of 64 and <= 1024, else GMP_ERR_UNSUPPORTED (256 is the model's).
 *   status: device int32[1], nullable; the forward and the weight gradient ADD the number of indices they
 *   skipped (column outside [0,K), resp. CSC row outside [0,N)) -- the caller zeroes it.
 *
 * fwd:   out[r, :] = sum_{k in rowptr[r]..rowptr[r+1]} val[k] * W[:, col[k]] + bias   (empty row -> bias)
 *        out [N, ldo] fp32, ldo >= H and a multiple of 4; bias [H] nullable.  Two launches: W transposed into
 *        the workspace (gmp_sparse_linear_workspace_bytes(K, H) bytes), then one wave per row gathering rows
 *        of W^T.  Each output is one sum in non-zero order: bitwise reproducible.
 * wgrad: dW[h, k] = sum over column k of val_t * g[row, h]   (G^T X; g [N, H] contiguous, 16-byte aligned)
 *        from the CSC form (colptr int32 [K+1], row int32, val_t fp32) of gmp_sparse_csc_build.  OVERWRITES
 *        every column of [0, ldw): columns without entries and the padding [K, ldw) get exactly 0.0.  No
 *        atomics: each element is one fixed-order sum.  The bias gradient is gmp_colsum(g).
 * csc:   the CSC form of X, stable (ascending row within a column; gmp_csr_build over the (row, col)
 *        pairs).  status is ZEROED, then counts the non-zeros whose column lies outside [0,K): those are
 *        left out, colptr[K] = the non-zeros kept.  row / val_t need nnz slots.  Once per feature matrix.
 * ------------------------------------------------------------------------- */
size_t gmp_sparse_linear_workspace_bytes(int64_t in_features, int out_features);
int gmp_sparse_linear_fwd(const int32_t* rowptr, const int32_t* col, const float* val, int64_t num_rows, int64_t in_features,
                          const float* weight, int64_t ldw, const float* bias, float* out, int out_features, int64_t ldo,
                          int32_t* status, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
int gmp_sparse_linear_wgrad(const int32_t* colptr, const int32_t* row, const float* val_t, int64_t num_rows, int64_t in_features,
                            const float* g, int out_features, float* dW, int64_t ldw, int32_t* status, gmp_stream_t stream);
size_t gmp_sparse_csc_workspace_bytes(int64_t num_rows, int64_t in_features, int64_t nnz);
int gmp_sparse_csc_build(const int32_t* rowptr, const int32_t* col, const float* val, int64_t num_rows, int64_t in_features,
                         int64_t nnz, int32_t* colptr, int32_t* row, float* val_t, int32_t* status, void* workspace,
                         size_t workspace_bytes, gmp_stream_t stream);

/* ------------------------------------------------------------------------- *
 * Multi-tensor PCGrad + clip_grad_norm_ + AdamW over flat buffers (gradient_surgery.py:41-103,
 * pretrain.py:152-153, optimizers.py:8-75), five launches, deterministic.
 *   task_grads [T][task_stride]: per-task gradients laid out like `params`; tensor k occupies
 *   [tensor_off[k], +tensor_len[k]) (device arrays); has[k*8 + t] != 0 iff task t's backward produced a
 *   gradient for tensor k (device uint8, row stride 8).
 *   order_host[0..n_order): the shuffled task order of PCGrad (gradient_surgery.py:43).
 *   last_task: last task in dict order -- where PCGrad emits nothing (tensor absent from the FIRST
 *   shuffled task) the reference leaves that task's raw .grad in place (gradient_surgery.py:61 quirk);
 *   extra_task: -1 or a task whose gradient is added on top (domain_adv, pretrain.py:149-150).
 *   Tensors that end up without a gradient (flags_out[k] == 0) are skipped by AdamW entirely, including
 *   their step count, as torch.optim does for grad=None.
 *   apply_update == 0: stop after final_grad / normsq_out (unclipped) -- used by parity tests.
 *   Layout contract (the sweeps move float4): every buffer 16-byte aligned, task_stride and every tensor_off multiples of 4,
 *   and each tensor's slot padded to a multiple of 4 floats with zeros in params, task_grads and the optimizer state (the
 *   padding is swept along and stays zero).
 * ------------------------------------------------------------------------- */
size_t gmp_mt_workspace_bytes(int num_tensors);
int gmp_mt_pcgrad_clip_adamw(const float* task_grads, int64_t task_stride, int num_tasks, int num_tensors,
                             const int64_t* tensor_off, const int32_t* tensor_len, const uint8_t* has,
                             const int32_t* order_host, int n_order, int last_task, int extra_task,
                             float* params, float* exp_avg, float* exp_avg_sq, float* steps,
                             const float* lr, const float* wd, float beta1, float beta2, float eps,
                             float max_norm, float* final_grad, float* normsq_out, int32_t* metrics_out,
                             int32_t* flags_out, void* workspace, size_t workspace_bytes, int apply_update,
                             gmp_stream_t stream);
/* The same in pieces, so PCGrad can follow the backward part by part: phases bit 0 = Gram / solve / combine for the tensors
 * [k_begin, k_end) only (their final_grad, flags, step counts, norm partials), bit 1 = total norm + clip + AdamW over ALL tensors
 * (call it once, after bit 0 has covered every tensor; same stream order or an explicit dependency in between).  Results are
 * bitwise those of the one-shot call: every tensor's arithmetic is independent of the others up to the norm.
 * bit 2 (value 4), for data-parallel runs that shard PCGrad over the ranks: the tensors [k_begin, k_end) are FOREIGN -- their combined
 * gradient was computed by another rank and already stands in final_grad (all-gathered); this leaves their flag, step count and norm
 * partials as the owner's bit 0 pass left them there, without touching task_grads (gnn_pretraining_amd/dist.py ShardedGradSync). */
int gmp_mt_pcgrad_clip_adamw_ex(const float* task_grads, int64_t task_stride, int num_tasks, int num_tensors,
                                const int64_t* tensor_off, const int32_t* tensor_len, const uint8_t* has,
                                const int32_t* order_host, int n_order, int last_task, int extra_task,
                                float* params, float* exp_avg, float* exp_avg_sq, float* steps,
                                const float* lr, const float* wd, float beta1, float beta2, float eps,
                                float max_norm, float* final_grad, float* normsq_out, int32_t* metrics_out,
                                int32_t* flags_out, void* ws, size_t ws_bytes, int apply_update,
                                int k_begin, int k_end, int phases, const int32_t* abort_flag, gmp_stream_t stream);
/* abort_flag (nullable, device): when *abort_flag != 0 at run time neither parameters, moments nor step counters are touched -- the
 * engine passes the error word of its cross-stream gates (sync_flags[63]), so a gate that timed out cannot turn into an update
 * computed from incomplete gradients; the host sees the flag at its next check_gates(). */

/* The same tail under another gradient-surgery RULE.  The Gram pass, combine, norm, clip and AdamW are the ones above; a rule is another
 * small solve in Gram space and another answer to "which tensors get a gradient".  P = the tasks of order_host, H_k = those of P that
 * hold tensor k.
 *   GMP_SURGERY_REFERENCE  the reference's rule, bit for bit gmp_mt_pcgrad_clip_adamw_ex (scope and perm_host are not read; the only
 *                          rule that reads last_task).
 *   GMP_SURGERY_PCGRAD     PCGrad as published (Yu et al. 2020, Alg. 1).  Every i in H_k starts from v = g_i[k] and walks the other
 *                          tasks in the order perm_host[i] (tasks outside H_k are skipped): a pair with ||v||^2 <= 0 or ||g_j||^2 <= 0
 *                          is skipped, every other pair counts one projection, and where <v, g_j> < 0 one conflict and
 *                          v -= <v, g_j> / ||g_j||^2 g_j (g_j as the task produced it).  final[k] = mean over H_k of the v_i; a tensor with
 *                          one holder gets that gradient as it is, so every head is trained in every step.  flag[k] = |H_k| > 0.
 *       GMP_SURGERY_SCOPE_TENSOR  one such walk per tensor, on the tensor's own Gram matrix.
 *       GMP_SURGERY_SCOPE_MODEL   ONE walk on G^ = the sum of the Gram matrices of the tensors with |H_k| >= 2 (ascending k, double),
 *                          i.e. on the tasks' whole shared vectors, over the tasks that hold any such tensor; with v_i = sum_b
 *                          alpha[i][b] g_b, tensor k of that set takes g_b[k] with weight (sum_i alpha[i][b]) / |H_k|.  The other
 *                          tensors behave as in tensor scope.  Conflicts and projections are those of the one walk.
 *   GMP_SURGERY_MEAN       final[k] = mean over H_k of g_i[k]; no projections (metrics 0, 0); scope is not read.
 *   extra_task is added on top under every rule and sets the flag.
 * perm_host [n_order][n_order - 1] (host, read during the call; pcgrad only, may be null when n_order == 1): row i lists the ORDER
 * POSITIONS task order_host[i] walks, a permutation of the positions other than i.
 * phases: tensor scope (and mean) -- bits 0 and 1 as above.  Model scope -- bit value 8 = the Gram matrices of [k_begin, k_end) only,
 * bit value 16 = fold, solve and combine over ALL tensors (once every tensor's Gram matrix stands), bit 1 as above; the one-shot call is
 * 8 | 16 | 2 over all tensors.  Bit 0 with model scope, bits 8 / 16 without it and the foreign pass (bit 2, which encodes the
 * reference's emission rule) with any other rule than the reference's are GMP_ERR_ARG, as are an unknown rule or scope and a perm_host
 * row that is no permutation; nothing is launched then. */
#define GMP_SURGERY_REFERENCE 0
#define GMP_SURGERY_PCGRAD 1
#define GMP_SURGERY_MEAN 2
#define GMP_SURGERY_SCOPE_TENSOR 0
#define GMP_SURGERY_SCOPE_MODEL 1
int gmp_mt_surgery_clip_adamw(int rule, int scope, const int32_t* perm_host,
                              const float* task_grads, int64_t task_stride, int num_tasks, int num_tensors,
                              const int64_t* tensor_off, const int32_t* tensor_len, const uint8_t* has,
                              const int32_t* order_host, int n_order, int last_task, int extra_task,
                              float* params, float* exp_avg, float* exp_avg_sq, float* steps,
                              const float* lr, const float* wd, float beta1, float beta2, float eps,
                              float max_norm, float* final_grad, float* normsq_out, int32_t* metrics_out,
                              int32_t* flags_out, void* ws, size_t ws_bytes, int apply_update,
                              int k_begin, int k_end, int phases, const int32_t* abort_flag, gmp_stream_t stream);


/* ---- device-side augmentation and masking ------------------------------------------------------------
 * The per-graph loops of src/pretrain/augmentations.py:17-111 (GraphAugmentor.create_two_views: node drop, subgraph relabel,
 * edge drop, attribute mask, common-node masks) and of src/models/pretrain_model.py:71-80 (mask indices) over a whole domain batch.
 * Random subsets are "the k smallest Philox keys of the graph" (seed, stream_id, element id): the reference's distributions, not its
 * mt19937 stream -- the bit-exact replay of that stream stays on the host (csrc_host/hostdraw.cpp).  All index arrays are int64
 * like the reference's; graphs are given as offset arrays (ptr / eptr: [G + 1]) over a batch in batch-local numbering.
 *
 * gmp_aug_node_masks: out_idx[out_ptr[g] ...] = the max(1, int(.15 n_g)) masked nodes of graph g (n_g >= 3), ascending; out_ptr is the
 *   caller's exclusive scan of those counts (they depend on the graph sizes only).
 * gmp_aug_two_views: both views of every graph.  view_ptr = exclusive scan of the kept-node counts n_g - max(1, int(.2 n_g)) (n_g >= 3,
 *   else n_g), the same for both views.  Outputs per view: rows [view_ptr[G]] (kept nodes, batch numbering, ascending), rowmask
 *   (bit c = column c zeroed, per row), edges [2, edge_capacity] (view numbering; PyG subgraph(relabel_nodes=True) order, minus the
 *   dropped ones), common (view-local ids of nodes kept in BOTH views); counts [5 G] = edges of view 1 / view 2 / common nodes /
 *   "drew an attribute mask" in view 1 / view 2, per graph; totals_and_flags [5] = total edges of view 1, of view 2, total common nodes, "some graph of view 1 / 2 drew an attribute
 *   mask".  Limits: 4,096 nodes and 8,192 edges per graph, 64 feature columns. */
size_t gmp_aug_workspace_bytes(int64_t num_nodes, int64_t num_edges, int num_graphs);
int gmp_aug_node_masks(const int64_t* ptr, const int64_t* out_ptr, int num_graphs, int64_t max_graph_nodes, uint64_t seed,
                       uint32_t stream_id, int64_t* out_idx, gmp_stream_t stream);
int gmp_aug_two_views(const int64_t* ptr, const int64_t* eptr, const int64_t* edge_index, int64_t num_nodes, int64_t num_edges,
                      const int64_t* view_ptr, int num_graphs, int64_t max_graph_nodes, int64_t max_graph_edges, int num_features,
                      uint64_t seed, uint32_t stream_id, int64_t* rows1, int64_t* rows2, uint64_t* rowmask1, uint64_t* rowmask2,
                      int64_t* edges1, int64_t* edges2, int64_t edge_capacity, int64_t* common1, int64_t* common2, int32_t* counts,
                      int32_t* totals_and_flags, void* workspace, size_t workspace_bytes, gmp_stream_t stream);
/* The same for all the jobs of a step -- one per (task, domain) pair -- in one launch (masks) / two launches (views): host arrays of
 * plain-data jobs whose fields are the arguments of the calls above (seed shared, stream_id per job); results identical to them. */
typedef struct {
    const int64_t *ptr, *out_ptr;
    int32_t num_graphs;
    uint32_t stream_id;
    int64_t* out_idx;
} gmp_aug_masks_job;
typedef struct {
    const int64_t *ptr, *eptr, *edge_index;
    int64_t num_nodes, num_edges;
    const int64_t* view_ptr;
    int32_t num_graphs, num_features;
    uint32_t stream_id;
    int64_t *rows1, *rows2;
    uint64_t *rowmask1, *rowmask2;
    int64_t *edges1, *edges2;
    int64_t edge_capacity;
    int64_t *common1, *common2;
    int32_t *counts, *totals_and_flags;
    void* workspace;
    size_t workspace_bytes;
} gmp_aug_views_job;
int gmp_aug_node_masks_batch(const gmp_aug_masks_job* jobs, int count, int64_t max_graph_nodes, uint64_t seed, gmp_stream_t stream);
int gmp_aug_two_views_batch(const gmp_aug_views_job* jobs, int count, int64_t max_graph_nodes, int64_t max_graph_edges, uint64_t seed,
                            gmp_stream_t stream);

/* Link-prediction negatives of a domain batch: batched_negative_sampling(to_undirected(edge_index), batch, num_neg) per graph, in
 * batch-local numbering.  Per graph of n nodes: the undirected adjacency (both directions, duplicates coalesced, self loops ignored)
 * has cnt entries; pop = n (n - 1); M = pop - cnt non-edges (ordered pairs i != j, not adjacent in either direction).  n < 2 or
 * cnt >= pop give nothing.  When pop <= int(1.1 * num_neg / (1.0 - cnt / pop)) (the sampler's own fp64 expression) no draw happens: the
 * graph gives its first min(M, num_neg) non-edges in ascending code i * n + j, bit for bit what the host sampler returns.  Otherwise
 * every non-edge gets a Philox key (seed, stream_id, the ordered pair) and the num_neg smallest keys are the sample (ties to the
 * lower code): a uniform num_neg-subset without replacement.  Two departures from PyG in that case: a graph always gives exactly
 * min(M, num_neg) pairs (PyG can come back short after its three tries), and they are listed in ascending code order, not in random
 * order.  neg_out [2, capacity] int64 holds the pairs compacted, graphs in batch order (row 1 at neg_out + capacity); counts [G] the
 * pairs per graph; total [1] their sum.  capacity >= sum_g min(num_neg, n_g (n_g - 1)) (a host-known bound).  The workspace holds the
 * bitmaps and per-graph slots: gmp_aug_negative_edges_workspace_bytes(num_nodes, max_graph_nodes, capacity), with the SAME
 * max_graph_nodes as the call.  Limit: 1,024 nodes per graph (GMP_ERR_ARG above it, nothing is launched).  num_graphs == 0 is a no-op.
 * gmp_aug_negative_edges_batch: all the jobs of a step in two launches (build, emit); results identical to the per-job calls. */
size_t gmp_aug_negative_edges_workspace_bytes(int64_t num_nodes, int64_t max_graph_nodes, int64_t capacity);
int gmp_aug_negative_edges(const int64_t* ptr, const int64_t* eptr, const int64_t* edge_index, int64_t num_nodes, int64_t num_edges,
                           int num_graphs, int64_t max_graph_nodes, int64_t num_neg, uint64_t seed, uint32_t stream_id,
                           int64_t* neg_out, int64_t capacity, int32_t* counts, int32_t* total, void* workspace, size_t workspace_bytes,
                           gmp_stream_t stream);
typedef struct {
    const int64_t *ptr, *eptr, *edge_index;
    int64_t num_nodes, num_edges;
    int32_t num_graphs;
    uint32_t stream_id;
    int64_t num_neg;
    int64_t* neg_out;
    int64_t capacity;
    int32_t *counts, *total;
    void* workspace;
    size_t workspace_bytes;
} gmp_aug_neg_job;
int gmp_aug_negative_edges_batch(const gmp_aug_neg_job* jobs, int count, int64_t max_graph_nodes, uint64_t seed, gmp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GNNMP_H */
