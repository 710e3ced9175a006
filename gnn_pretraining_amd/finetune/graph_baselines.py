"""The model-free baseline of graph classification: the Weisfeiler-Lehman subtree kernel (Shervashidze et al., JMLR 2011) on the raw graphs,
refined, sorted and counted on the GPU (csrc/wl.hip; the definition is above gmp_wl_refine in include/gnnmp.h), with the pinned k-NN vote
and softmax regression of the embedding probes on top.  A GIN is bounded by the 1-WL test, so this is what the backbone's probes have to
beat.  It reads the datasets only: no model, no generator, no dropout counter, no BatchNorm state.

    initial_labels(x)                                 the discrete node labels behind one-hot features, None for continuous ones
    wl_features(batch, iters, dim=256, labels="auto") WLFeatures of one collated Batch: the exact (sorted) and the hashed (hist) feature map
    wl_kernel(feat_a, feat_b)                         the int64 Gram of the subtree kernel between two WLFeatures
    normalised_similarity(K_et, K_ee, K_tt)           K / sqrt(K_ee K_tt) in fp64
    wl_neighbours(sim, k)                             the k most similar columns per row, ties to the lower index
    wl_baseline(train_ds, eval_ds, num_classes, iters, k=20, device="cuda")    {"knn_accuracy", "logreg_accuracy"}

Beside it the shortest-path kernel (Borgwardt & Kriegel, ICDM 2005; csrc/sp.hip, the definition is above gmp_sp_features): where WL sees
rooted neighbourhoods, it compares graphs by their distributions of (label, label, hop distance) over node pairs.  Same protocol on top.

    sp_features(batch, max_dist, dim=256, labels="auto")  SPFeatures: per graph the sorted distinct keys with their counts, and the hashed hist
    sp_kernel(feat_a, feat_b)                             the int64 Gram of the shortest-path kernel between two SPFeatures
    sp_self_similarity(feat)                              the Gram's diagonal from the counts alone
    sp_baseline(train_ds, eval_ds, num_classes, max_dist, k=20, device="cuda") {"knn_accuracy", "logreg_accuracy"}

And the two baselines that read the FEATURES, which the kernels above never do on continuous ones: the structure-blind classifier on pooled
raw features (Errica et al., ICLR 2020) and SGC's S^t X (Wu et al., ICML 2019) pooled per graph and concatenated over t = 0 .. K (the
multi-scale concatenation of SIGN, Frasca et al. 2020), pooled on the GPU in one launch per batch (csrc/graph_feat.hip; the definition is
above gmp_graph_feature_map) -- the graph-level pair of node_baselines' rawfeat / sgc.

    pooled_features(batch, rounds)                        fp32 [G, (rounds + 1) * 3 * d]: per level t the sum, mean and max pool of S^t X
    standardise(train, other)                             both by the train rows' column mean and population deviation (float64, rounded once)
    feature_baseline(train_ds, eval_ds, num_classes, rounds, k=20, device="cuda")
        {"rawpool_knn_accuracy", "rawpool_logreg_accuracy", "sgcpool_knn_accuracy", "sgcpool_logreg_accuracy"}
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional, Tuple, Union

import torch
from torch import Tensor

from .. import ops
from .._lib import GnnmpError
from .link_heuristics import simple_graph
from .node_baselines import sgc_graph, softmax_fit


class WLFeatures(NamedTuple):
    sorted: Tensor                 # int64 [(iters + 1) * N]: per graph, all its colours in ascending unsigned order
    hist: Tensor                   # int32 [G, dim]
    ptr: Tensor                    # int64 [G + 1]
    iters: int


def initial_labels(x: Tensor) -> Optional[Tensor]:
    """The int64 argmax per row when every row of x [N, F] is one-hot -- exactly one non-zero entry and it equals 1 (MUTAG, NCI1, PTC_MR)
    -- and None otherwise: on the standardised continuous features of ENZYMES and PROTEINS the refinement then starts from the node
    degrees, the usual start for graphs without discrete labels."""
    if x.dim() != 2 or x.size(1) == 0:
        return None
    nz = x != 0
    if not bool(((nz.sum(dim=1) == 1) & ((x == 1).sum(dim=1) == 1)).all()):
        return None
    return nz.to(torch.int64).argmax(dim=1)


def _gpu_batch(who: str, batch) -> None:
    if not batch.x.is_cuda:
        raise GnnmpError(f"{who}: expected a batch on the GPU (the HIP path has no CPU fallback), got {batch.x.device}")


def _kernel_inputs(who: str, batch, labels: Union[str, None, Tensor]):
    """(ptr, rowptr, col, labels) as ops.wl_refine / ops.sp_features take them: the batch's int64 ptr, its simple_graph, and the int64 [N]
    start labels or None for degrees -- "auto" = initial_labels(batch.x), None, or a tensor."""
    _gpu_batch(who, batch)
    if isinstance(labels, str):
        if labels != "auto":
            raise ValueError(f"{who}: labels={labels!r} (\"auto\", None or an int64 tensor)")
        labels = initial_labels(batch.x)
    rowptr, col = simple_graph(batch.edge_index.contiguous(), batch.num_nodes)
    return batch.ptr.to(torch.int64).contiguous(), rowptr, col, None if labels is None else labels.to(torch.int64).contiguous()


def _check_status(who: str, status: Tensor, batch, node_limit: int, extra=()) -> None:
    """One read-back of a per-graph kernel's status words (csrc/graph_block.h); GnnmpError naming the first graph with bit 0 (more than
    node_limit nodes), then with a mask of `extra` -- rows (mask, what the graph has) -- then with skipped entries counted in bits 8 .."""
    status = status.cpu()
    if bool((status & 1).any()):
        g = int((status & 1).nonzero()[0])
        raise GnnmpError(f"{who}: graph {g} has {batch.ptr_host[g + 1] - batch.ptr_host[g]} nodes, more than the "
                         f"{node_limit} the kernel takes (there is no host fallback)")
    for mask, what in extra:
        if bool((status & mask).any()):
            raise GnnmpError(f"{who}: graph {int((status & mask).nonzero()[0])} has {what}")
    if bool((status >> 8).any()):
        g = int((status >> 8).nonzero()[0])
        raise GnnmpError(f"{who}: {int(status[g] >> 8)} adjacency entries of graph {g} point outside the graph and were skipped")


def wl_features(batch, iters: int, dim: int = ops.WL_MAX_DIM, labels: Union[str, None, Tensor] = "auto") -> WLFeatures:
    """`iters` rounds of WL refinement of one collated Batch on the GPU (ops.wl_refine on simple_graph(batch.edge_index)).  labels: "auto" =
    initial_labels(batch.x), None = degrees, or an int64 [N] tensor.  Raises GnnmpError naming the first graph the kernel refuses (more
    than ops.WL_MAX_GRAPH_NODES nodes), and when a CSR entry was skipped for leaving its graph (one read-back of the status words)."""
    ptr, rowptr, col, labels = _kernel_inputs("wl_features", batch, labels)
    out = ops.wl_refine(ptr, rowptr, col, labels, iters, dim, max_graph_nodes=batch.max_graph_nodes)
    _check_status("wl_features", out.status, batch, ops.WL_MAX_GRAPH_NODES)
    return WLFeatures(out.sorted, out.hist, ptr, int(iters))


def wl_kernel(feat_a: WLFeatures, feat_b: WLFeatures) -> Tensor:
    """K int64 [Ga, Gb]: the WL subtree kernel between the graphs of two refinements made with the same number of rounds."""
    if feat_a.iters != feat_b.iters:
        raise GnnmpError(f"wl_kernel: the two refinements ran {feat_a.iters} and {feat_b.iters} rounds")
    return ops.wl_gram(feat_a.sorted, feat_a.ptr, feat_b.sorted, feat_b.ptr, feat_a.iters)


def normalised_similarity(K_et: Tensor, K_ee: Tensor, K_tt: Tensor) -> Tensor:
    """s [n_eval, n_train] = K_et / sqrt(K_ee[:, None] * K_tt[None, :]) in fp64 from the integer Gram and the two self-similarity vectors;
    0 where a self-similarity is 0 (an empty graph)."""
    den = torch.sqrt(K_ee.to(torch.float64)[:, None] * K_tt.to(torch.float64)[None, :])
    ok = den > 0
    return torch.where(ok, K_et.to(torch.float64) / torch.where(ok, den, torch.ones_like(den)), torch.zeros_like(den))


def wl_neighbours(sim: Tensor, k: int) -> Tuple[Tensor, Tensor]:
    """(idx int64 [n, k'], sim fp64 [n, k']), k' = min(k, columns): the most similar columns of every row by a stable descending sort,
    so ties go to the lower index."""
    val, idx = torch.sort(sim, dim=1, descending=True, stable=True)
    kk = min(int(k), sim.size(1))
    return idx[:, :kk].contiguous(), val[:, :kk].contiguous()


def _collated_splits(who: str, train_ds, eval_ds, k: int, device):
    """The two splits as ONE batch each, in dataset order, after the checks every baseline makes: 1 <= k <= ops.KNN_MAX_K, no empty split."""
    if not 1 <= int(k) <= ops.KNN_MAX_K:
        raise ValueError(f"{who}: k={k} (1 <= k <= {ops.KNN_MAX_K})")
    if len(train_ds) == 0 or len(eval_ds) == 0:
        raise ValueError(f"{who}: {len(train_ds)} train and {len(eval_ds)} evaluation graphs (both splits need one)")
    return tuple(ds.collate(torch.arange(len(ds))).to(device) for ds in (train_ds, eval_ds))


def _accuracies(sim: Tensor, y_train: Tensor, y_eval: Tensor, num_classes: int, k: int, lr_pred: Tensor) -> Tuple[float, float]:
    """(knn accuracy, accuracy of the caller's logreg predictions) on the evaluation split.  knn: wl_neighbours(sim, k) of sim (fp64
    [n_eval, n_train]), their similarities in fp32 through ops.knn_vote at its default temperature.  (So the callers fit and predict
    before the vote; the two share no state and no random draw.)"""
    idx, val = wl_neighbours(sim, k)
    _, knn_pred = ops.knn_vote(idx, val.to(torch.float32).contiguous(), y_train, num_classes)
    return float((knn_pred == y_eval).float().mean()), float((lr_pred == y_eval).float().mean())


def _kernel_baseline(who: str, features, kernel, train_ds, eval_ds, num_classes: int, k: int, device) -> Dict[str, float]:
    """The protocol the graph-kernel baselines share.  features(batch) -> a feature map with the hashed histogram in .hist, kernel(a, b) ->
    the int64 Gram between two of them; each split is collated into ONE batch, in dataset order.
    knn: s = K[eval, train] / sqrt(K_ee K_tt) in fp64 (the self-similarities are the diagonals of the same Gram kernel, 0 where one is 0),
    the min(k, n_train) nearest by a stable descending sort (ties to the lower train index), then s in fp32 through ops.knn_vote at its
    default temperature.  The [n_eval, n_train] matrix IS the product here -- the kernel's Gram -- and is a few hundred squared on the TU
    datasets: there is nothing to stream.
    logreg: ops.logreg_fit on the train split's hashed histogram (as fp32, at its defaults: 100 iterations, lr 0.01), ops.logreg_predict
    on the evaluation split's."""
    tb, eb = _collated_splits(who, train_ds, eval_ds, k, device)
    ft, fe = features(tb), features(eb)
    y_train, y_eval = tb.y.to(torch.int64).contiguous(), eb.y.to(torch.int64).contiguous()
    sim = normalised_similarity(kernel(fe, ft), kernel(fe, fe).diagonal(), kernel(ft, ft).diagonal())
    fit = ops.logreg_fit(ft.hist.to(torch.float32).contiguous(), y_train, num_classes)
    lr_pred = ops.logreg_predict(fe.hist.to(torch.float32).contiguous(), fit.state.weight, fit.state.bias)
    knn, logreg = _accuracies(sim, y_train, y_eval, num_classes, k, lr_pred)
    return {"knn_accuracy": knn, "logreg_accuracy": logreg}


def wl_baseline(train_ds, eval_ds, num_classes: int, iters: int, k: int = 20, device="cuda") -> Dict[str, float]:
    """{"knn_accuracy", "logreg_accuracy"} of the WL subtree features with `iters` rounds, fitted on train_ds and scored on eval_ds (two
    graph datasets with collate()) by the protocol of _kernel_baseline: a k-NN vote on the fp64-normalised exact kernel and a softmax
    regression on the hashed histogram."""
    if not 1 <= int(iters) <= ops.WL_MAX_ITERS:
        raise ValueError(f"wl_baseline: iters={iters} (1 <= iters <= {ops.WL_MAX_ITERS})")
    return _kernel_baseline("wl_baseline", lambda b: wl_features(b, iters), wl_kernel, train_ds, eval_ds, num_classes, k, device)


class SPFeatures(NamedTuple):
    keys: Tensor                   # int64 [G, cap]: per graph its distinct (label, label, distance) keys, ascending, in [:nuniq[g]]
    counts: Tensor                 # int32 [G, cap]: the node pairs per key
    nuniq: Tensor                  # int32 [G]
    hist: Tensor                   # int32 [G, dim]
    max_dist: int


def sp_features(batch, max_dist: int, dim: int = ops.SP_MAX_DIM, labels: Union[str, None, Tensor] = "auto") -> SPFeatures:
    """The shortest-path feature map of one collated Batch on the GPU (ops.sp_features on simple_graph(batch.edge_index)), distances up to
    max_dist.  labels as for wl_features: "auto" = initial_labels(batch.x), None = degrees, or an int64 [N] tensor.  The row stride is
    the most keys a graph of the batch can have -- its node pairs -- up to what the kernel takes.  Raises GnnmpError naming the first
    graph the kernel refuses -- more than ops.SP_MAX_GRAPH_NODES nodes, more distinct keys than the row stride, a label outside
    [0, ops.SP_MAX_LABEL) -- and when a CSR entry was skipped for leaving its graph (one read-back of the status words)."""
    ptr, rowptr, col, labels = _kernel_inputs("sp_features", batch, labels)
    n = int(batch.max_graph_nodes)
    cap = max(1, min(ops.sp_max_unique(n), n * (n - 1) // 2))
    out = ops.sp_features(ptr, rowptr, col, labels, max_dist, dim, max_graph_nodes=n, cap=cap)
    _check_status("sp_features", out.status, batch, ops.SP_MAX_GRAPH_NODES, extra=(
        (2, f"more than {cap} distinct (label, label, distance) keys, the most the kernel takes for graphs of up to {n} nodes "
            f"(there is no host fallback)"),
        (4, f"a node label outside [0, {ops.SP_MAX_LABEL})")))
    return SPFeatures(out.keys, out.counts, out.nuniq, out.hist, int(max_dist))


def sp_kernel(feat_a: SPFeatures, feat_b: SPFeatures) -> Tensor:
    """K int64 [Ga, Gb]: the shortest-path kernel between the graphs of two feature maps made with the same largest distance."""
    if feat_a.max_dist != feat_b.max_dist:
        raise GnnmpError(f"sp_kernel: the two feature maps count distances up to {feat_a.max_dist} and {feat_b.max_dist}")
    return ops.sp_gram(feat_a.keys, feat_a.counts, feat_a.nuniq, feat_b.keys, feat_b.counts, feat_b.nuniq)


def sp_self_similarity(feat: SPFeatures) -> Tensor:
    """int64 [G]: K[g, g] = the sum of counts^2 over graph g's keys, without the Gram kernel."""
    live = torch.arange(feat.counts.size(1), device=feat.counts.device)[None, :] < feat.nuniq[:, None]
    c = torch.where(live, feat.counts, torch.zeros_like(feat.counts)).to(torch.int64)
    return (c * c).sum(dim=1)


def sp_baseline(train_ds, eval_ds, num_classes: int, max_dist: int, k: int = 20, device="cuda") -> Dict[str, float]:
    """{"knn_accuracy", "logreg_accuracy"} of the shortest-path features with distances up to max_dist, fitted on train_ds and scored on
    eval_ds (two graph datasets with collate()) by the protocol of _kernel_baseline, as wl_baseline."""
    if not 1 <= int(max_dist) <= ops.SP_MAX_DIST:
        raise ValueError(f"sp_baseline: max_dist={max_dist} (1 <= max_dist <= {ops.SP_MAX_DIST})")
    return _kernel_baseline("sp_baseline", lambda b: sp_features(b, max_dist), sp_kernel, train_ds, eval_ds, num_classes, k, device)


def pooled_features(batch, rounds: int) -> Tensor:
    """fp32 [G, (rounds + 1) * 3 * d] of one collated Batch on the GPU: for t = 0 .. rounds the sum, mean and max pool (in that order, d
    columns each) over every graph's nodes of S^t X, S = D~^-1/2 (A + I) D~^-1/2 (ops.graph_feature_map on node_baselines.sgc_graph: the
    simple graph plus one self-loop per node, the host-computed 1 / sqrt(deg + 1) as both scales).  The first 3 d columns are the pools of
    the raw features: no graph.  Raises GnnmpError naming the first graph the kernel refuses (more than ops.GRAPH_FEAT_MAX_GRAPH_NODES
    nodes), and when a CSR entry was skipped for leaving its graph (one read-back of the status words)."""
    _gpu_batch("pooled_features", batch)
    rowptr, col, scale = sgc_graph(batch.edge_index.contiguous(), batch.num_nodes)
    res = ops.graph_feature_map(batch.ptr.to(torch.int64).contiguous(), rowptr, col, batch.x.to(torch.float32), rounds, left=scale, right=scale,
                                max_graph_nodes=batch.max_graph_nodes)
    _check_status("pooled_features", res.status, batch, ops.GRAPH_FEAT_MAX_GRAPH_NODES)
    return res.out.reshape(res.out.size(0), -1)


def standardise(train: Tensor, other: Tensor) -> Tuple[Tensor, Tensor]:
    """(train', other') fp32 on their devices: per column, minus the TRAIN rows' mean, divided by their population standard deviation;
    a column whose deviation is 0 becomes all zeros in both.  Mean, deviation and the quotient are float64 on the host, rounded once to
    fp32 (the rule of node_baselines.degree_scales: the device's arithmetic never enters a value)."""
    t, o = train.detach().to("cpu", torch.float64), other.detach().to("cpu", torch.float64)
    mean = t.mean(dim=0, keepdim=True)
    std = ((t - mean) ** 2).mean(dim=0, keepdim=True).sqrt()
    ok = std > 0
    safe = torch.where(ok, std, torch.ones_like(std))
    z = lambda m: torch.where(ok, (m - mean) / safe, torch.zeros_like(m)).to(torch.float32)          # noqa: E731
    return z(t).to(train.device), z(o).to(other.device)


FEATURE_KINDS = ("rawpool", "sgcpool")


def feature_baseline(train_ds, eval_ds, num_classes: int, rounds: int, k: int = 20, device="cuda") -> Dict[str, float]:
    """{"rawpool_knn_accuracy", "rawpool_logreg_accuracy", "sgcpool_knn_accuracy", "sgcpool_logreg_accuracy"}, fitted on train_ds and
    scored on eval_ds (two graph datasets with collate()).  Each split is collated into ONE batch in dataset order and gets one
    pooled_features call with `rounds` rounds.  rawpool is its t = 0 slice -- the 3 d pools of the raw features, no graph: the
    structure-blind baseline -- and sgcpool all rounds + 1 slices; both are standardised by the train split.
    knn, by the protocol of _kernel_baseline: the Gram Z_e Z_t^T and the two diagonals in torch fp64 (a few hundred squared), then
    normalised_similarity, wl_neighbours(sim, k) and ops.knn_vote at its default temperature.
    logreg: node_baselines.softmax_fit at its defaults on the train rows, prediction ops.gemm(NT, Z_e, W, bias).argmax, as
    node_baselines.feature_baselines does for nodes."""
    if not 1 <= int(rounds) <= ops.GRAPH_FEAT_MAX_ROUNDS:
        raise ValueError(f"feature_baseline: rounds={rounds} (1 <= rounds <= {ops.GRAPH_FEAT_MAX_ROUNDS})")
    tb, eb = _collated_splits("feature_baseline", train_ds, eval_ds, k, device)
    pt, pe = pooled_features(tb, int(rounds)), pooled_features(eb, int(rounds))
    y_train, y_eval = tb.y.to(torch.int64).contiguous(), eb.y.to(torch.int64).contiguous()
    raw = pt.size(1) // (int(rounds) + 1)                                          # 3 d: the t = 0 slice
    scores: Dict[str, float] = {}
    for name, width in zip(FEATURE_KINDS, (raw, pt.size(1))):
        zt, ze = standardise(pt[:, :width], pe[:, :width])
        zt, ze = zt.contiguous(), ze.contiguous()
        zt64, ze64 = zt.to(torch.float64), ze.to(torch.float64)
        sim = normalised_similarity(ze64 @ zt64.T, (ze64 * ze64).sum(dim=1), (zt64 * zt64).sum(dim=1))
        weight, bias, _ = softmax_fit(zt, y_train, num_classes)
        lr_pred = ops.gemm(ops.NT, ze, weight, bias=bias).argmax(dim=1)
        scores[f"{name}_knn_accuracy"], scores[f"{name}_logreg_accuracy"] = _accuracies(sim, y_train, y_eval, num_classes, k, lr_pred)
    return scores
