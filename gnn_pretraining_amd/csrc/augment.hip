// Device-side augmentation and masking: the per-graph Python loops of
// src/pretrain/augmentations.py:17-111 (node drop -> subgraph relabel -> edge drop -> attribute mask, two views per graph,
// common-node masks) and src/models/pretrain_model.py:67-88 (node-feature-masking indices) as kernels over a whole domain batch.
//
// What the reference draws with torch.randperm(n)[:k] from its CPU generator is, as a distribution, "a uniformly random k-subset":
// here every node / edge / feature column gets a Philox4x32-10 key (seed, stream, global element id) and the k smallest keys of a
// graph are the subset (ties broken by index).  The draws therefore do not replay the reference's mt19937 stream -- nothing on a
// device can -- and serve the engine's "device" RNG mode; the reference-order CPU path stays for bit-exact parity.  The STRUCTURE
// is the reference's, and tests/test_gpu_augment.py holds it to that: counts (n - max(1, int(.2 n)) kept nodes for n >= 3,
// max(1, int(.15 n)) masked nodes, E' - max(1, int(.2 E')) kept edges when the coin falls and E' >= 3, max(1, int(.2 F)) zeroed
// columns), kept nodes sorted, edges relabelled exactly as PyG subgraph(relabel_nodes=True) does, common-node sets -- and to the
// oracle itself, by replaying the device's decisions through oracle.augment.create_two_views as injected permutations.
//
// Layout: one workgroup per graph draws BOTH views (the common-node sets need both).  Kept-node counts are a function of the
// graph sizes alone, so `rows` is written at its final place; edge and common-node counts are random, so the first kernel leaves
// every graph's survivors compacted at the start of the graph's own slot (its original edge / node range) and a second kernel
// moves the slots to their final offsets (exclusive scan of the counts) in view-local numbering.
//
// Link-prediction negatives (gmp_aug_negative_edges, at the end of the file): torch_geometric's batched_negative_sampling(
// to_undirected(edge_index), batch, num_neg) as pretrain/tasks.py restates it, one workgroup per graph.  The graph's undirected
// adjacency (both directions, duplicates coalesced, self loops ignored) is a bitmap in the caller's workspace; cnt = its set bits,
// pop = n (n - 1), M = pop - cnt non-edges (ordered pairs i != j, not adjacent).  n < 2 or cnt >= pop give nothing.  The host's
// fp64 test pop <= int(1.1 * num_neg / (1.0 - cnt / pop)), in its evaluation order, decides between
//   no draw : the first min(M, num_neg) non-edges in ascending code i * n + j -- what the host returns, bit for bit;
//   sampled : every non-edge gets the key key32(seed, stream, S_NEG, (s + i) << 32 | (s + j)) (s = the graph's first node: the id is
//             unique per ordered pair of the batch); the num_neg smallest keys are the sample, ties to the lower code, emitted in
//             ascending code order.  A uniform num_neg-subset without replacement.
// Two departures from PyG in the sampled case: the count is always exactly min(M, num_neg) (PyG may come back short after its three
// tries), and the order within a graph is ascending, not random (the scorer's loss is a sum over pairs: order carries no meaning).
// The k-th smallest key is found by a 4 x 8-bit radix select whose passes recompute the keys (no key array: a 1,024-node graph
// has a million pairs); as for the views, a build kernel leaves each graph's codes in a slot of the workspace and an emit kernel
// moves them to their final offsets.  LDS: two ints per node of the batch's largest graph + a 256-bin histogram (<= 10 KB).
#include "gnnmp_internal.h"

namespace {

constexpr int AB = 256;                 // threads per graph
constexpr int MAX_NODES = 4096;         // per graph: keep flags / new ids / keys of both views live in LDS
constexpr int EDGES_LDS = 4096;
constexpr uint32_t S_NODE = 0x6e6f6465u, S_EDGE = 0x65646765u, S_ECOIN = 0x65636f69u, S_ACOIN = 0x61636f69u, S_ATTR = 0x61747472u,
                   S_NFM = 0x6e666d6bu, S_NEG = 0x6e656773u;
constexpr int NEG_MAX_NODES = 1024;     // per graph, link-prediction negatives: codes i * n + j fit 2^20, rows of 32 bitmap words

__device__ __forceinline__ uint32_t key32(uint64_t seed, uint32_t stream, uint32_t purpose, uint64_t idx) {
    return gmp::philox4x32(make_uint4((uint32_t)idx, (uint32_t)(idx >> 32), stream, purpose), make_uint2((uint32_t)seed, (uint32_t)(seed >> 32))).x;
}
__device__ __forceinline__ float unif(uint64_t seed, uint32_t stream, uint32_t purpose, uint64_t idx) {
    return (float)key32(seed, stream, purpose, idx) * 2.3283064365386963e-10f;        // [0, 1)
}
__device__ __forceinline__ int drop_count(int n, double rate) {                      // max(1, int(n * rate)), Python double arithmetic
    const int k = (int)((double)n * rate);
    return k > 1 ? k : 1;
}

// ---- node-feature-masking indices: per graph with n >= 3 the max(1, int(.15 n)) nodes of smallest key, ascending -------------------
__device__ __forceinline__ void nfm_masks_body(const int64_t* __restrict__ ptr, const int64_t* __restrict__ out_ptr, uint64_t seed,
                                               uint32_t stream, int64_t* __restrict__ out, const int g) {
    __shared__ uint32_t keys[MAX_NODES];
    __shared__ uint8_t chosen[MAX_NODES];
    const int64_t s = ptr[g];
    const int n = (int)(ptr[g + 1] - s);
    if (n < 3) return;
    const int k = drop_count(n, 0.15);
    for (int i = threadIdx.x; i < n; i += AB) keys[i] = key32(seed, stream, S_NFM, (uint64_t)(s + i));
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += AB) {
        const uint32_t ki = keys[i];
        int rank = 0;
        for (int j = 0; j < n; ++j) rank += (keys[j] < ki) || (keys[j] == ki && j < i);
        chosen[i] = rank < k;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < n; i += AB) {
        if (!chosen[i]) continue;
        int before = 0;
        for (int j = 0; j < i; ++j) before += chosen[j];
        out[out_ptr[g] + before] = s + i;
    }
}
__global__ __launch_bounds__(AB) void nfm_masks_kernel(const int64_t* __restrict__ ptr, const int64_t* __restrict__ out_ptr, uint64_t seed,
                                                       uint32_t stream, int64_t* __restrict__ out) {
    nfm_masks_body(ptr, out_ptr, seed, stream, out, blockIdx.x);
}

// Batched forms: ONE launch for all the (task, domain) jobs of a step -- the jobs ride in the kernel arguments, a workgroup finds its job
// from the running graph counts.  Same arithmetic, same keys: results identical to the per-job launches.
constexpr int AUG_MAXJ = 8;
struct MaskJob { const int64_t* ptr; const int64_t* out_ptr; int64_t* out; uint32_t stream; };
struct MaskBatch { MaskJob job[AUG_MAXJ]; int first[AUG_MAXJ + 1]; int count; uint64_t seed; };
__device__ __forceinline__ int job_of(const int* first, int count, int b) {
    int j = 0;
    while (j + 1 < count && b >= first[j + 1]) ++j;
    return j;
}
__global__ __launch_bounds__(AB) void nfm_masks_batch_kernel(const MaskBatch b) {
    const int j = job_of(b.first, b.count, blockIdx.x);
    nfm_masks_body(b.job[j].ptr, b.job[j].out_ptr, b.seed, b.job[j].stream, b.job[j].out, blockIdx.x - b.first[j]);
}

struct ViewArgs {
    const int64_t* ptr;          // [G + 1] node offsets of the batch (domain-local row ids)
    const int64_t* eptr;         // [G + 1] edge offsets
    const int64_t* src;          // [E] edge_index[0]
    const int64_t* dst;          // [E] edge_index[1]
    const int64_t* vptr;         // [G + 1] node offsets of a VIEW (both views keep the same number of nodes per graph)
    int G, F;
    uint64_t seed;
    uint32_t stream;             // views use stream and stream + 1
    int64_t* rows[2];            // [vptr[G]] kept nodes, batch numbering, ascending            (final)
    uint64_t* rowmask[2];        // [vptr[G]] bit c set = feature column c zeroed               (final)
    int64_t* slot_src[2];        // [E] surviving edges of graph g compacted at eptr[g], graph-LOCAL new ids
    int64_t* slot_dst[2];
    int64_t* slot_common[2];     // [N] common nodes of graph g compacted at ptr[g], graph-local new ids of that view
    int32_t* edge_count[2];      // [G]
    int32_t* common_count;       // [G] (the same for both views)
    int32_t* mask_flag[2];       // [G] this graph drew an attribute mask in view v
    uint32_t* ekey;              // [E] scratch: key of a surviving edge (a graph's block only touches its own range)
    uint8_t* eflag;              // [E] scratch: survives node drop / survives edge drop
};

// LDS is sized per launch from the batch's largest graph (ncap nodes, ecap edges; a few KB for TUDataset graphs): these blocks run
// beside the step's GEMMs, whose 64 KB blocks leave little LDS free on a CU -- a 56 KB static footprint waited for a GEMM block to
// retire before it could start (58 us per launch in the step against ~10 alone)
__device__ __forceinline__ void two_views_body(const ViewArgs& a, const int ncap, const int ecap, const int g, unsigned char* dyn) {
    unsigned long long* const s_bits_p = reinterpret_cast<unsigned long long*>(dyn);
    int* const s_cnt = reinterpret_cast<int*>(dyn + 8);
    uint32_t* const keys = reinterpret_cast<uint32_t*>(dyn + 32);
    uint32_t* const s_ekey = keys + ncap;           // edge keys / flags of the graph: in LDS when they fit (every TUDataset graph does),
    uint16_t* const newid0 = reinterpret_cast<uint16_t*>(s_ekey + ecap);      // in the workspace otherwise: the rank loops are latency-bound
    uint16_t* const newid1 = newid0 + ncap;                                   // new ids per view; 0xffff = dropped
    uint8_t* const s_eflag = reinterpret_cast<uint8_t*>(newid1 + ncap);
    uint16_t* const newid[2] = {newid0, newid1};
#define s_bits (*s_bits_p)
    const int t = threadIdx.x;
    const int64_t s = a.ptr[g], es = a.eptr[g];
    const int n = (int)(a.ptr[g + 1] - s), ne = (int)(a.eptr[g + 1] - es);
    const int keep_n = n >= 3 ? n - drop_count(n, 0.2) : n;
    for (int v = 0; v < 2; ++v) {
        // ---- node drop: the keep_n smallest keys stay; new id = number of kept nodes in front (sorted kept list, subgraph's relabelling)
        __syncthreads();
        for (int i = t; i < n; i += AB) keys[i] = key32(a.seed, a.stream + v, S_NODE, (uint64_t)(s + i));
        __syncthreads();
        for (int i = t; i < n; i += AB) {
            const uint32_t ki = keys[i];
            int rank = 0;
            for (int j = 0; j < n; ++j) rank += (keys[j] < ki) || (keys[j] == ki && j < i);
            newid[v][i] = rank < keep_n ? 1 : 0xffff;            // provisional: kept flag
        }
        __syncthreads();
        for (int i = t; i < n; i += AB) {
            if (newid[v][i] == 0xffff) continue;
            int before = 0;
            for (int j = 0; j < i; ++j) before += newid[v][j] != 0xffff;
            keys[i] = (uint32_t)before;                           // (keys are spent: reuse the array for the prefix counts)
        }
        __syncthreads();
        // attribute mask of this (view, graph): coin, then the max(1, int(.2 F)) smallest of F column keys (thread c ranks column c)
        if (t == 0) s_bits = 0ull;
        __syncthreads();
        if (a.F >= 3 && unif(a.seed, a.stream + v, S_ACOIN, (uint64_t)(s)) < 0.2f) {
            const int m = drop_count(a.F, 0.2);
            if (t < a.F) {
                const uint32_t kc = key32(a.seed, a.stream + v, S_ATTR, (uint64_t)s * 64 + t);
                int rank = 0;
                for (int q = 0; q < a.F; ++q) {
                    const uint32_t kq = key32(a.seed, a.stream + v, S_ATTR, (uint64_t)s * 64 + q);
                    rank += (kq < kc) || (kq == kc && q < t);
                }
                if (rank < m) atomicOr(&s_bits, 1ull << t);
            }
        }
        __syncthreads();
        const uint64_t bits = s_bits;
        if (t == 0) a.mask_flag[v][g] = bits != 0ull;
        for (int i = t; i < n; i += AB) {
            if (newid[v][i] == 0xffff) continue;
            const int id = (int)keys[i];
            newid[v][i] = (uint16_t)id;
            a.rows[v][a.vptr[g] + id] = s + i;
            a.rowmask[v][a.vptr[g] + id] = bits;
        }
    }
    __syncthreads();
    // ---- common nodes (augmentations.py:77-85): kept in both views; listed per view in that view's local numbering, ascending
    if (t == 0) {
        int c = 0;
        for (int i = 0; i < n; ++i)
            if (newid[0][i] != 0xffff && newid[1][i] != 0xffff) {
                a.slot_common[0][s + c] = newid[0][i];
                a.slot_common[1][s + c] = newid[1][i];
                ++c;
            }
        a.common_count[g] = c;
    }
    // ---- edges: subgraph() keeps an edge when both endpoints stay (order preserved); then, if the coin falls and at least 3 are
    // left, the E' - max(1, int(.2 E')) smallest edge keys stay (kept in their original order)
    uint32_t* const ekey = ne <= ecap ? s_ekey : a.ekey + es;          // (generic pointers: LDS or global)
    uint8_t* const eflag = ne <= ecap ? s_eflag : a.eflag + es;
    for (int v = 0; v < 2; ++v) {
        __syncthreads();
        if (t == 0) s_cnt[0] = 0;
        __syncthreads();
        int alive_mine = 0;
        for (int e = t; e < ne; e += AB) {
            const int i = (int)(a.src[es + e] - s), j = (int)(a.dst[es + e] - s);
            const bool al = newid[v][i] != 0xffff && newid[v][j] != 0xffff;
            eflag[e] = al;
            ekey[e] = al ? key32(a.seed, a.stream + v, S_EDGE, (uint64_t)(es + e)) : 0u;
            alive_mine += al;
        }
        atomicAdd(&s_cnt[0], alive_mine);
        __threadfence_block();
        __syncthreads();
        const int alive = s_cnt[0];
        const bool drop = alive >= 3 && unif(a.seed, a.stream + v, S_ECOIN, (uint64_t)s) < 0.2f;
        const int keep_e = drop ? alive - drop_count(alive, 0.2) : alive;
        if (drop) {                                  // rank among the survivors; the keep_e smallest keys stay
            uint8_t mine[(8192 + AB - 1) / AB];      // this thread's verdicts (ne <= 8192 is checked by the host wrapper)
            int m = 0;
            for (int e = t; e < ne; e += AB, ++m) {
                bool kept = eflag[e];
                if (kept) {
                    const uint32_t ke = ekey[e];
                    int rank = 0;
                    for (int q = 0; q < ne; ++q) rank += eflag[q] && ((ekey[q] < ke) || (ekey[q] == ke && q < e));
                    kept = rank < keep_e;
                }
                mine[m] = kept;
            }
            __syncthreads();                          // every rank is taken before any flag changes
            m = 0;
            for (int e = t; e < ne; e += AB, ++m) eflag[e] = mine[m];
            __threadfence_block();
            __syncthreads();
        }
        for (int e = t; e < ne; e += AB) {           // position among the kept edges = kept edges in front (original order preserved)
            if (!eflag[e]) continue;
            int pos = 0;
            for (int q = 0; q < e; ++q) pos += eflag[q];
            a.slot_src[v][es + pos] = newid[v][(int)(a.src[es + e] - s)];
            a.slot_dst[v][es + pos] = newid[v][(int)(a.dst[es + e] - s)];
        }
        if (t == 0) a.edge_count[v][g] = keep_e;
    }
#undef s_bits
}

struct EmitArgs {
    const int64_t *ptr, *eptr, *vptr;
    int G;
    const int64_t* slot_src[2];
    const int64_t* slot_dst[2];
    const int64_t* slot_common[2];
    const int32_t* edge_count[2];
    const int32_t* common_count;
    const int32_t* mask_flag[2];
    int64_t* edges[2];          // [2, ecap]: row 0 at edges[v], row 1 at edges[v] + ecap
    int64_t ecap;
    int64_t* common[2];
    int32_t* totals;            // [5]: edges of view 0, edges of view 1, common nodes, any attribute mask in view 0 / view 1
};

// slots -> final offsets (exclusive scan of the per-graph counts), graph-local new ids -> view numbering (+ vptr[g])
__device__ __forceinline__ void emit_views_body(const EmitArgs& a, const int g) {
    const int t = threadIdx.x;
    for (int v = 0; v < 2; ++v) {
        int64_t off = 0;
        for (int q = 0; q < g; ++q) off += a.edge_count[v][q];
        const int cnt = a.edge_count[v][g];
        for (int e = t; e < cnt; e += AB) {
            a.edges[v][off + e] = a.slot_src[v][a.eptr[g] + e] + a.vptr[g];
            a.edges[v][a.ecap + off + e] = a.slot_dst[v][a.eptr[g] + e] + a.vptr[g];
        }
        if (g == a.G - 1 && t == 0) a.totals[v] = (int32_t)(off + cnt);
    }
    int64_t coff = 0;
    for (int q = 0; q < g; ++q) coff += a.common_count[q];
    const int cc = a.common_count[g];
    for (int c = t; c < cc; c += AB) {
        a.common[0][coff + c] = a.slot_common[0][a.ptr[g] + c] + a.vptr[g];
        a.common[1][coff + c] = a.slot_common[1][a.ptr[g] + c] + a.vptr[g];
    }
    if (g == a.G - 1 && t == 0) {
        a.totals[2] = (int32_t)(coff + cc);
        for (int v = 0; v < 2; ++v) {           // (written by every launch: no memset in front of the kernels)
            int any = 0;
            for (int q = 0; q < a.G; ++q) any |= a.mask_flag[v][q];
            a.totals[3 + v] = any;
        }
    }
}
__global__ __launch_bounds__(AB) void emit_views_kernel(const EmitArgs a) { emit_views_body(a, blockIdx.x); }
__global__ __launch_bounds__(AB) void two_views_kernel(const ViewArgs a, int ncap, int ecap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    two_views_body(a, ncap, ecap, blockIdx.x, dyn);
}
struct ViewBatch { ViewArgs job[AUG_MAXJ]; int first[AUG_MAXJ + 1]; int count; };
struct EmitBatch { EmitArgs job[AUG_MAXJ]; int first[AUG_MAXJ + 1]; int count; };
__global__ __launch_bounds__(AB) void two_views_batch_kernel(const ViewBatch b, int ncap, int ecap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int j = job_of(b.first, b.count, blockIdx.x);
    two_views_body(b.job[j], ncap, ecap, blockIdx.x - b.first[j], dyn);
}
__global__ __launch_bounds__(AB) void emit_views_batch_kernel(const EmitBatch b) {
    const int j = job_of(b.first, b.count, blockIdx.x);
    emit_views_body(b.job[j], blockIdx.x - b.first[j]);
}

}  // namespace

extern "C" size_t gmp_aug_workspace_bytes(int64_t num_nodes, int64_t num_edges, int num_graphs) {
    if (num_nodes < 0 || num_edges < 0 || num_graphs < 0) return 0;
    // slot_src / slot_dst x 2 views, slot_common x 2, edge_count x 2 + common_count
    return (size_t)(4 * num_edges + 2 * num_nodes) * sizeof(int64_t) + (size_t)num_edges * 5 + 512;      // + edge keys (u32) and flags (u8)
}

extern "C" int gmp_aug_node_masks(const int64_t* ptr, const int64_t* out_ptr, int num_graphs, int64_t max_graph_nodes, uint64_t seed,
                                  uint32_t stream_id, int64_t* out_idx, gmp_stream_t stream) {
    if (num_graphs < 0 || (num_graphs > 0 && (!ptr || !out_ptr || !out_idx))) return gmp::fail(GMP_ERR_ARG, "aug_node_masks: bad argument");
    if (max_graph_nodes > MAX_NODES) return gmp::fail(GMP_ERR_UNSUPPORTED, "aug_node_masks: a graph of %lld nodes (limit %d)", (long long)max_graph_nodes, MAX_NODES);
    if (num_graphs == 0) return GMP_OK;
    hipLaunchKernelGGL(nfm_masks_kernel, dim3(num_graphs), dim3(AB), 0, (hipStream_t)stream, ptr, out_ptr, seed, stream_id, out_idx);
    return gmp::check_launch("nfm_masks_kernel");
}

namespace {
struct ViewsCall {            // plain-argument form of one two-views job (what both entry points validate and turn into kernel arguments)
    const int64_t *ptr, *eptr, *edge_index;
    int64_t num_nodes, num_edges;
    const int64_t* view_ptr;
    int num_graphs, num_features;
    uint32_t stream_id;
    int64_t *rows1, *rows2;
    uint64_t *rowmask1, *rowmask2;
    int64_t *edges1, *edges2;
    int64_t edge_capacity;
    int64_t *common1, *common2;
    int32_t *counts, *totals_and_flags;
    void* workspace;
    size_t workspace_bytes;
};
int views_check(const ViewsCall& c, int64_t max_graph_nodes, int64_t max_graph_edges) {
    if (c.num_graphs < 0 || c.num_edges < 0 || c.num_features < 0 || c.num_features > 64)
        return gmp::fail(GMP_ERR_ARG, "aug_two_views: bad sizes (attribute masks are 64-bit column sets)");
    if (c.num_graphs == 0) return GMP_OK;
    if (!c.ptr || !c.eptr || !c.view_ptr || !c.rows1 || !c.rows2 || !c.rowmask1 || !c.rowmask2 || !c.edges1 || !c.edges2 || !c.common1 || !c.common2 ||
        !c.counts || !c.totals_and_flags || (c.num_edges > 0 && !c.edge_index))
        return gmp::fail(GMP_ERR_ARG, "aug_two_views: null pointer");
    if (max_graph_nodes > MAX_NODES) return gmp::fail(GMP_ERR_UNSUPPORTED, "aug_two_views: a graph of %lld nodes (limit %d)", (long long)max_graph_nodes, MAX_NODES);
    if (c.edge_capacity < c.num_edges) return gmp::fail(GMP_ERR_ARG, "aug_two_views: edge capacity below the batch's edge count");
    if (max_graph_edges > 8192) return gmp::fail(GMP_ERR_UNSUPPORTED, "aug_two_views: a graph of %lld edges (limit 8192)", (long long)max_graph_edges);
    if (!c.workspace || c.workspace_bytes < gmp_aug_workspace_bytes(c.num_nodes, c.num_edges, c.num_graphs)) return gmp::fail(GMP_ERR_WORKSPACE, "aug_two_views: workspace");
    return GMP_OK;
}
void views_args(const ViewsCall& c, uint64_t seed, ViewArgs* ap, EmitArgs* ep) {
    int64_t* w = (int64_t*)c.workspace;
    ViewArgs a{};
    a.ptr = c.ptr; a.eptr = c.eptr; a.src = c.edge_index; a.dst = c.edge_index ? c.edge_index + c.num_edges : nullptr; a.vptr = c.view_ptr;
    a.G = c.num_graphs; a.F = c.num_features; a.seed = seed; a.stream = c.stream_id;
    a.rows[0] = c.rows1; a.rows[1] = c.rows2; a.rowmask[0] = c.rowmask1; a.rowmask[1] = c.rowmask2;
    a.slot_src[0] = w; a.slot_dst[0] = w + c.num_edges; a.slot_src[1] = w + 2 * c.num_edges; a.slot_dst[1] = w + 3 * c.num_edges;
    a.slot_common[0] = w + 4 * c.num_edges; a.slot_common[1] = a.slot_common[0] + c.num_nodes;
    a.ekey = (uint32_t*)(a.slot_common[1] + c.num_nodes);
    a.eflag = (uint8_t*)(a.ekey + c.num_edges);
    a.edge_count[0] = c.counts; a.edge_count[1] = c.counts + c.num_graphs; a.common_count = c.counts + 2 * c.num_graphs;
    a.mask_flag[0] = c.counts + 3 * c.num_graphs; a.mask_flag[1] = c.counts + 4 * c.num_graphs;
    EmitArgs e{};
    e.ptr = c.ptr; e.eptr = c.eptr; e.vptr = c.view_ptr; e.G = c.num_graphs;
    for (int v = 0; v < 2; ++v) { e.slot_src[v] = a.slot_src[v]; e.slot_dst[v] = a.slot_dst[v]; e.slot_common[v] = a.slot_common[v]; e.edge_count[v] = a.edge_count[v]; }
    e.common_count = a.common_count;
    e.mask_flag[0] = a.mask_flag[0]; e.mask_flag[1] = a.mask_flag[1];
    e.edges[0] = c.edges1; e.edges[1] = c.edges2; e.ecap = c.edge_capacity; e.common[0] = c.common1; e.common[1] = c.common2; e.totals = c.totals_and_flags;
    *ap = a; *ep = e;
}
size_t views_lds(int64_t max_graph_nodes, int64_t max_graph_edges, int* ncap, int* ecap) {
    *ncap = (int)((max_graph_nodes + 63) / 64 * 64);
    *ecap = max_graph_edges <= EDGES_LDS ? (int)((max_graph_edges + 63) / 64 * 64) : 0;
    return 32 + (size_t)*ncap * 4 + (size_t)*ecap * 4 + (size_t)*ncap * 4 + (size_t)*ecap + 64;
}
}  // namespace

extern "C" int gmp_aug_two_views(const int64_t* ptr, const int64_t* eptr, const int64_t* edge_index, int64_t num_nodes, int64_t num_edges,
                                 const int64_t* view_ptr, int num_graphs, int64_t max_graph_nodes, int64_t max_graph_edges, int num_features, uint64_t seed, uint32_t stream_id,
                                 int64_t* rows1, int64_t* rows2, uint64_t* rowmask1, uint64_t* rowmask2, int64_t* edges1, int64_t* edges2,
                                 int64_t edge_capacity, int64_t* common1, int64_t* common2, int32_t* counts, int32_t* totals_and_flags,
                                 void* workspace, size_t workspace_bytes, gmp_stream_t stream) {
    const ViewsCall c{ptr, eptr, edge_index, num_nodes, num_edges, view_ptr, num_graphs, num_features, stream_id, rows1, rows2, rowmask1, rowmask2,
                      edges1, edges2, edge_capacity, common1, common2, counts, totals_and_flags, workspace, workspace_bytes};
    if (int rc = views_check(c, max_graph_nodes, max_graph_edges)) return rc;
    if (num_graphs == 0) return GMP_OK;
    ViewArgs a;
    EmitArgs e;
    views_args(c, seed, &a, &e);
    int ncap, ecap;
    const size_t lds = views_lds(max_graph_nodes, max_graph_edges, &ncap, &ecap);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(two_views_kernel, dim3(num_graphs), dim3(AB), lds, st, a, ncap, ecap);
    hipLaunchKernelGGL(emit_views_kernel, dim3(num_graphs), dim3(AB), 0, st, e);
    return gmp::check_launch("aug_two_views kernels");
}

// All the two-views jobs of a step -- one per contrastive (task, domain) pair -- in TWO launches (build, emit) instead of two per
// job: the draws ride the aux stream beside a running step, where sixteen 10-60 us launches per step cost it 0.3 ms.
extern "C" int gmp_aug_two_views_batch(const gmp_aug_views_job* jobs, int count, int64_t max_graph_nodes, int64_t max_graph_edges, uint64_t seed,
                                       gmp_stream_t stream) {
    if (count < 0 || (count > 0 && !jobs)) return gmp::fail(GMP_ERR_ARG, "aug_two_views_batch: bad job list");
    int ncap, ecap;
    const size_t lds = views_lds(max_graph_nodes, max_graph_edges, &ncap, &ecap);
    hipStream_t st = (hipStream_t)stream;
    for (int j0 = 0; j0 < count;) {
        ViewBatch vb{};
        EmitBatch eb{};
        int n = 0, blocks = 0;
        for (; j0 < count && n < AUG_MAXJ; ++j0) {
            const gmp_aug_views_job& q = jobs[j0];
            const ViewsCall c{q.ptr, q.eptr, q.edge_index, q.num_nodes, q.num_edges, q.view_ptr, q.num_graphs, q.num_features, q.stream_id, q.rows1, q.rows2,
                              q.rowmask1, q.rowmask2, q.edges1, q.edges2, q.edge_capacity, q.common1, q.common2, q.counts, q.totals_and_flags, q.workspace,
                              q.workspace_bytes};
            if (int rc = views_check(c, max_graph_nodes, max_graph_edges)) return rc;
            if (c.num_graphs == 0) continue;
            views_args(c, seed, &vb.job[n], &eb.job[n]);
            vb.first[n] = eb.first[n] = blocks;
            blocks += c.num_graphs;
            ++n;
        }
        if (n == 0) continue;
        vb.first[n] = eb.first[n] = blocks;
        vb.count = eb.count = n;
        hipLaunchKernelGGL(two_views_batch_kernel, dim3(blocks), dim3(AB), lds, st, vb, ncap, ecap);
        hipLaunchKernelGGL(emit_views_batch_kernel, dim3(blocks), dim3(AB), 0, st, eb);
    }
    return gmp::check_launch("aug_two_views_batch kernels");
}

extern "C" int gmp_aug_node_masks_batch(const gmp_aug_masks_job* jobs, int count, int64_t max_graph_nodes, uint64_t seed, gmp_stream_t stream) {
    if (count < 0 || (count > 0 && !jobs)) return gmp::fail(GMP_ERR_ARG, "aug_node_masks_batch: bad job list");
    if (max_graph_nodes > MAX_NODES) return gmp::fail(GMP_ERR_UNSUPPORTED, "aug_node_masks_batch: a graph of %lld nodes (limit %d)", (long long)max_graph_nodes, MAX_NODES);
    for (int j0 = 0; j0 < count;) {
        MaskBatch mb{};
        int n = 0, blocks = 0;
        for (; j0 < count && n < AUG_MAXJ; ++j0) {
            const gmp_aug_masks_job& q = jobs[j0];
            if (q.num_graphs < 0 || (q.num_graphs > 0 && (!q.ptr || !q.out_ptr || !q.out_idx))) return gmp::fail(GMP_ERR_ARG, "aug_node_masks_batch: bad job");
            if (q.num_graphs == 0) continue;
            mb.job[n] = MaskJob{q.ptr, q.out_ptr, q.out_idx, q.stream_id};
            mb.first[n] = blocks;
            blocks += q.num_graphs;
            ++n;
        }
        if (n == 0) continue;
        mb.first[n] = blocks;
        mb.count = n;
        mb.seed = seed;
        hipLaunchKernelGGL(nfm_masks_batch_kernel, dim3(blocks), dim3(AB), 0, (hipStream_t)stream, mb);
    }
    return gmp::check_launch("nfm_masks_batch_kernel");
}


// ---- link-prediction negatives (rule and layout: header comment) -------------------------------------------------------------------
namespace {

struct NegArgs {
    const int64_t *ptr, *eptr, *src, *dst;
    int64_t N, E;
    int G;
    int64_t num_neg;
    uint32_t stream;
    uint32_t* bits;              // [N, W] adjacency rows (workspace): node s + i of the batch owns row s + i
    int32_t* slot;               // [capacity] codes i * n + j; graph g's start at sum_{q < g} min(num_neg, n_q (n_q - 1))
    int64_t capacity;
    int64_t* neg;                // [2, capacity]
    int32_t* counts;             // [G]
    int32_t* total;              // [1]
};

// exclusive scan of a[0 .. n) in place by the first wave; *tot = the sum (the caller synchronises)
__device__ __forceinline__ void neg_scan_rows(int* a, const int n, int* tot) {
    const int t = threadIdx.x;
    if (t >= 64) return;
    int run = 0;
    for (int c = 0; c < n; c += 64) {
        const int i = c + t;
        const int v = i < n ? a[i] : 0;
        int inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(inc, d, 64);
            if (t >= d) inc += u;
        }
        if (i < n) a[i] = run + inc - v;
        run += __shfl(inc, 63, 64);
    }
    if (t == 0) *tot = run;
}

__device__ __forceinline__ uint32_t neg_key(uint64_t seed, uint32_t stream, int64_t s, int i, int j) {
    return key32(seed, stream, S_NEG, ((uint64_t)(s + i) << 32) | (uint64_t)(uint32_t)(s + j));
}

__device__ __forceinline__ void negatives_body(const NegArgs& a, const int W, const uint64_t seed, const int g, unsigned char* dyn) {
    const int ncap = W * 32;
    unsigned long long* const s_off = reinterpret_cast<unsigned long long*>(dyn);      // slot offset of this graph
    int* const s_misc = reinterpret_cast<int*>(dyn + 8);                                 // cnt | total below | total ties | prefix | remaining
    uint32_t* const s_hist = reinterpret_cast<uint32_t*>(dyn + 32);                       // [256]
    int* const s_less = reinterpret_cast<int*>(dyn + 32 + 1024);                           // [ncap] per row: selected below the threshold
    int* const s_tie = s_less + ncap;                                                       // [ncap] per row: keys equal to the threshold
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const int64_t s = a.ptr[g], es = a.eptr[g];
    const int64_t n64 = a.ptr[g + 1] - s, ne64 = a.eptr[g + 1] - es;
    // (a graph the arguments do not cover gives nothing rather than an access outside the workspace)
    if (n64 < 2 || n64 > ncap || s < 0 || s + n64 > a.N || es < 0 || ne64 < 0 || es + ne64 > a.E) {
        if (t == 0) a.counts[g] = 0;
        return;
    }
    const int n = (int)n64, ne = (int)ne64;
    if (t == 0) { *s_off = 0ull; s_misc[0] = 0; }
    __syncthreads();
    {
        unsigned long long mine = 0ull;
        for (int q = t; q < g; q += AB) {
            const int64_t nq = a.ptr[q + 1] - a.ptr[q];
            if (nq >= 2 && nq <= ncap) mine += (unsigned long long)(a.num_neg < nq * (nq - 1) ? a.num_neg : nq * (nq - 1));
        }
        if (mine) atomicAdd(s_off, mine);
    }
    uint32_t* const bits = a.bits + (size_t)s * W;
    for (int q = t; q < n * W; q += AB) bits[q] = 0u;
    __threadfence_block();
    __syncthreads();
    for (int e = t; e < ne; e += AB) {
        const int64_t i = a.src[es + e] - s, j = a.dst[es + e] - s;
        if (i < 0 || i >= n || j < 0 || j >= n || i == j) continue;
        atomicOr(&bits[i * W + (j >> 5)], 1u << (j & 31));
        atomicOr(&bits[j * W + (i >> 5)], 1u << (i & 31));
    }
    __threadfence_block();
    __syncthreads();
    const int wn = (n + 31) >> 5;
    {
        int deg_mine = 0;
        for (int i = t; i < n; i += AB) {
            int deg = 0;
            for (int w = 0; w < wn; ++w) deg += __popc(bits[i * W + w]);
            s_less[i] = n - 1 - deg;                 // non-edges of row i (the diagonal bit is never set)
            s_tie[i] = 0;
            deg_mine += deg;
        }
        if (deg_mine) atomicAdd(&s_misc[0], deg_mine);
    }
    __syncthreads();
    const int cnt = s_misc[0], pop = n * (n - 1);
    int64_t room = a.capacity - (int64_t)*s_off;
    if (cnt >= pop || room <= 0) {
        if (t == 0) a.counts[g] = 0;
        return;
    }
    const int M = pop - cnt;
    int k = a.num_neg < M ? (int)a.num_neg : M;
    if (k > room) k = (int)room;                     // (never with the documented capacity: memory safety only)
    // the host's rule, its fp64 arithmetic and evaluation order: prob = 1.0 - cnt / pop; size = int(1.1 * num_neg / prob)
    const double prob = 1.0 - (double)cnt / (double)pop;
    const double size = trunc(1.1 * (double)a.num_neg / prob);
    const bool sampled = !((double)pop <= size) && k < M;
    uint32_t T = 0xffffffffu;                        // no draw: every non-edge is "below the threshold", cut at k in code order
    int take = 0;
    if (sampled) {
        // ---- the k-th smallest key: four 8-bit digits from the top; remaining = rank wanted inside the current prefix group
        if (t == 0) { s_misc[3] = 0; s_misc[4] = k; }
        for (int pass = 0; pass < 4; ++pass) {
            const int shift = 24 - 8 * pass;
            s_hist[t] = 0u;                          // (AB == 256 bins)
            __syncthreads();
            const uint32_t prefix = (uint32_t)s_misc[3];
            for (int i = wave; i < n; i += AB / 64)
                for (int c = 0; c < n; c += 64) {
                    const int j = c + lane;
                    if (j >= n || j == i || ((bits[i * W + (j >> 5)] >> (j & 31)) & 1u)) continue;
                    const uint32_t key = neg_key(seed, a.stream, s, i, j);
                    if (pass == 0 || (key >> (shift + 8)) == prefix) atomicAdd(&s_hist[(key >> shift) & 255u], 1u);
                }
            __syncthreads();
            if (t == 0) {
                int rem = s_misc[4], b = 0;
                while (b < 255 && (int)s_hist[b] < rem) { rem -= (int)s_hist[b]; ++b; }
                s_misc[3] = (int)((prefix << 8) | (uint32_t)b);
                s_misc[4] = rem;
            }
            __syncthreads();
        }
        T = (uint32_t)s_misc[3];
        take = s_misc[4];                            // how many of the keys equal to T belong to the sample (>= 1): the lowest codes
        // ---- per row: keys below T, keys equal to T
        for (int i = wave; i < n; i += AB / 64) {
            int below = 0, equal = 0;
            for (int c = 0; c < n; c += 64) {
                const int j = c + lane;
                const bool ne_ = j < n && j != i && !((bits[i * W + (j >> 5)] >> (j & 31)) & 1u);
                const uint32_t key = ne_ ? neg_key(seed, a.stream, s, i, j) : 0u;
                below += __popcll(__ballot(ne_ && key < T));
                equal += __popcll(__ballot(ne_ && key == T));
            }
            if (lane == 0) { s_less[i] = below; s_tie[i] = equal; }
        }
        __syncthreads();
    }
    neg_scan_rows(s_less, n, &s_misc[1]);
    __syncthreads();
    if (sampled) {
        neg_scan_rows(s_tie, n, &s_misc[2]);
        __syncthreads();
    }
    // ---- emit in code order: position = selected pairs in front = keys below T in front + min(ties in front, take)
    int32_t* const out = a.slot + *s_off;
    for (int i = wave; i < n; i += AB / 64) {
        int below = s_less[i], ties = s_tie[i];
        if (below + (ties < take ? ties : take) >= k) continue;       // (wave-uniform) the row starts behind the cut
        for (int c = 0; c < n; c += 64) {
            const int j = c + lane;
            const bool ne_ = j < n && j != i && !((bits[i * W + (j >> 5)] >> (j & 31)) & 1u);
            bool lo = ne_, eq = false;
            if (sampled) {
                const uint32_t key = ne_ ? neg_key(seed, a.stream, s, i, j) : 0u;
                lo = ne_ && key < T;
                eq = ne_ && key == T;
            }
            const unsigned long long blo = __ballot(lo), beq = __ballot(eq);
            const int tie_front = ties + __popcll(beq & lt);
            const int pos = below + __popcll(blo & lt) + (tie_front < take ? tie_front : take);
            if ((lo || (eq && tie_front < take)) && pos < k) out[pos] = i * n + j;
            below += __popcll(blo);
            ties += __popcll(beq);
        }
    }
    if (t == 0) a.counts[g] = k;
}

// slots -> final offsets (exclusive scan of the counts), codes -> pairs in batch numbering
__device__ __forceinline__ void emit_negatives_body(const NegArgs& a, const int W, const int g) {
    __shared__ unsigned long long s_acc[2];          // counts in front | slot offset
    const int t = threadIdx.x, ncap = W * 32;
    if (t < 2) s_acc[t] = 0ull;
    __syncthreads();
    unsigned long long c_mine = 0ull, o_mine = 0ull;
    for (int q = t; q < g; q += AB) {
        c_mine += (unsigned long long)a.counts[q];
        const int64_t nq = a.ptr[q + 1] - a.ptr[q];
        if (nq >= 2 && nq <= ncap) o_mine += (unsigned long long)(a.num_neg < nq * (nq - 1) ? a.num_neg : nq * (nq - 1));
    }
    if (c_mine) atomicAdd(&s_acc[0], c_mine);
    if (o_mine) atomicAdd(&s_acc[1], o_mine);
    __syncthreads();
    const int64_t off = (int64_t)s_acc[0];
    const int k = a.counts[g];
    if (k > 0) {
        const int64_t s = a.ptr[g];
        const int n = (int)(a.ptr[g + 1] - s);
        const int32_t* const in = a.slot + s_acc[1];
        for (int e = t; e < k; e += AB) {
            const int code = in[e];
            a.neg[off + e] = s + code / n;
            a.neg[a.capacity + off + e] = s + code % n;
        }
    }
    if (g == a.G - 1 && t == 0) *a.total = (int32_t)(off + k);
}

constexpr int NEG_MAXJ = 8;
struct NegBatch { NegArgs job[NEG_MAXJ]; int first[NEG_MAXJ + 1]; int count; uint64_t seed; };
__global__ __launch_bounds__(AB) void negatives_kernel(const NegArgs a, int W, uint64_t seed) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    negatives_body(a, W, seed, blockIdx.x, dyn);
}
__global__ __launch_bounds__(AB) void emit_negatives_kernel(const NegArgs a, int W) { emit_negatives_body(a, W, blockIdx.x); }
__global__ __launch_bounds__(AB) void negatives_batch_kernel(const NegBatch b, int W) {
    extern __shared__ __attribute__((aligned(16))) unsigned char dyn[];
    const int j = job_of(b.first, b.count, blockIdx.x);
    negatives_body(b.job[j], W, b.seed, blockIdx.x - b.first[j], dyn);
}
__global__ __launch_bounds__(AB) void emit_negatives_batch_kernel(const NegBatch b, int W) {
    const int j = job_of(b.first, b.count, blockIdx.x);
    emit_negatives_body(b.job[j], W, blockIdx.x - b.first[j]);
}

int neg_words(int64_t max_graph_nodes) { return (int)((max_graph_nodes < 1 ? 1 : max_graph_nodes) + 31) / 32; }
size_t neg_lds(int W) { return 32 + 1024 + (size_t)W * 32 * 2 * sizeof(int); }
size_t neg_bitmap_bytes(int64_t num_nodes, int W) { return ((size_t)num_nodes * W * sizeof(uint32_t) + 255) / 256 * 256; }

int neg_check(const gmp_aug_neg_job& q, int64_t max_graph_nodes) {
    if (q.num_graphs < 0 || q.num_nodes < 0 || q.num_edges < 0 || q.num_neg < 0 || q.capacity < 0) return gmp::fail(GMP_ERR_ARG, "aug_negative_edges: bad sizes");
    if (q.num_graphs == 0) return GMP_OK;
    if (max_graph_nodes > NEG_MAX_NODES)
        return gmp::fail(GMP_ERR_ARG, "aug_negative_edges: a graph of %lld nodes (limit %d)", (long long)max_graph_nodes, NEG_MAX_NODES);
    if (!q.ptr || !q.eptr || !q.counts || !q.total || (q.num_edges > 0 && !q.edge_index) || (q.capacity > 0 && !q.neg_out))
        return gmp::fail(GMP_ERR_ARG, "aug_negative_edges: null pointer");
    if (!q.workspace || q.workspace_bytes < gmp_aug_negative_edges_workspace_bytes(q.num_nodes, max_graph_nodes, q.capacity))
        return gmp::fail(GMP_ERR_WORKSPACE, "aug_negative_edges: workspace");
    return GMP_OK;
}
NegArgs neg_args(const gmp_aug_neg_job& q, int W) {
    NegArgs a{};
    a.ptr = q.ptr; a.eptr = q.eptr; a.src = q.edge_index; a.dst = q.edge_index ? q.edge_index + q.num_edges : nullptr;
    a.N = q.num_nodes; a.E = q.num_edges; a.G = q.num_graphs; a.num_neg = q.num_neg; a.stream = q.stream_id;
    a.bits = (uint32_t*)q.workspace;
    a.slot = (int32_t*)((unsigned char*)q.workspace + neg_bitmap_bytes(q.num_nodes, W));
    a.capacity = q.capacity; a.neg = q.neg_out; a.counts = q.counts; a.total = q.total;
    return a;
}
}  // namespace

extern "C" size_t gmp_aug_negative_edges_workspace_bytes(int64_t num_nodes, int64_t max_graph_nodes, int64_t capacity) {
    if (num_nodes < 0 || max_graph_nodes < 0 || capacity < 0) return 0;
    return neg_bitmap_bytes(num_nodes, neg_words(max_graph_nodes)) + (size_t)capacity * sizeof(int32_t) + 256;
}

extern "C" int gmp_aug_negative_edges_batch(const gmp_aug_neg_job* jobs, int count, int64_t max_graph_nodes, uint64_t seed, gmp_stream_t stream) {
    if (count < 0 || (count > 0 && !jobs)) return gmp::fail(GMP_ERR_ARG, "aug_negative_edges_batch: bad job list");
    const int W = neg_words(max_graph_nodes);
    hipStream_t st = (hipStream_t)stream;
    for (int j0 = 0; j0 < count;) {
        NegBatch nb{};
        int n = 0, blocks = 0;
        for (; j0 < count && n < NEG_MAXJ; ++j0) {
            if (int rc = neg_check(jobs[j0], max_graph_nodes)) return rc;
            if (jobs[j0].num_graphs == 0) continue;
            nb.job[n] = neg_args(jobs[j0], W);
            nb.first[n] = blocks;
            blocks += jobs[j0].num_graphs;
            ++n;
        }
        if (n == 0) continue;
        nb.first[n] = blocks;
        nb.count = n;
        nb.seed = seed;
        hipLaunchKernelGGL(negatives_batch_kernel, dim3(blocks), dim3(AB), neg_lds(W), st, nb, W);
        hipLaunchKernelGGL(emit_negatives_batch_kernel, dim3(blocks), dim3(AB), 0, st, nb, W);
    }
    return gmp::check_launch("aug_negative_edges_batch kernels");
}

extern "C" int gmp_aug_negative_edges(const int64_t* ptr, const int64_t* eptr, const int64_t* edge_index, int64_t num_nodes, int64_t num_edges,
                                      int num_graphs, int64_t max_graph_nodes, int64_t num_neg, uint64_t seed, uint32_t stream_id,
                                      int64_t* neg_out, int64_t capacity, int32_t* counts, int32_t* total, void* workspace,
                                      size_t workspace_bytes, gmp_stream_t stream) {
    gmp_aug_neg_job q{};
    q.ptr = ptr; q.eptr = eptr; q.edge_index = edge_index; q.num_nodes = num_nodes; q.num_edges = num_edges; q.num_graphs = num_graphs;
    q.stream_id = stream_id; q.num_neg = num_neg; q.neg_out = neg_out; q.capacity = capacity; q.counts = counts; q.total = total;
    q.workspace = workspace; q.workspace_bytes = workspace_bytes;
    if (int rc = neg_check(q, max_graph_nodes)) return rc;
    if (num_graphs == 0) return GMP_OK;
    const int W = neg_words(max_graph_nodes);
    const NegArgs a = neg_args(q, W);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(negatives_kernel, dim3(num_graphs), dim3(AB), neg_lds(W), st, a, W, seed);
    hipLaunchKernelGGL(emit_negatives_kernel, dim3(num_graphs), dim3(AB), 0, st, a, W);
    return gmp::check_launch("aug_negative_edges kernels");
}
