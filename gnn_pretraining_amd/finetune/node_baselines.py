"""The model-free baselines of node classification: label spreading (Zhou et al., NIPS 2004) and label propagation (Zhu & Ghahramani,
2002) over the raw graph, iterated on the GPU (csrc/label_prop.hip; the definition is above gmp_label_propagate in include/gnnmp.h).  On
citation graphs this is the number a GNN is expected to beat.  They read the graph and the train split's labels only: no model, no
generator, no dropout counter, no BatchNorm state.  And the two baselines that read the FEATURES: a softmax regression on the raw
features (no graph) and SGC (Wu et al., ICML 2019), the same regression on S^K X with S = D~^-1/2 (A + I) D~^-1/2, propagated on the GPU
(csrc/feature_prop.hip; the definition is above gmp_feature_propagate in include/gnnmp.h) and fitted on the train split's rows.

    degree_scales(rowptr, kind)                      (left, right) fp32 scales of the propagation: "sym" D^-1/2 A D^-1/2, "rw" D^-1 A
    label_spreading(edge_index, num_nodes, seeds, seed_labels, num_classes, rounds=50, alpha=0.9)    ops.LabelPropagation
    label_propagation(edge_index, num_nodes, seeds, seed_labels, num_classes, rounds=50)             ops.LabelPropagation
    label_baselines(data, train_idx, eval_idx, num_classes, rounds, device="cuda")
        {"labelspread_accuracy", "labelprop_accuracy", "labelspread_unreached", "labelprop_unreached"}
    sgc_graph(edge_index, num_nodes)                 (rowptr, col, scale): the simple graph plus one self-loop per node, 1 / sqrt(deg + 1)
    sgc_features(x, edge_index, num_nodes, rounds)   S^rounds X, dense [n, d]; x dense or graph.SparseFeatures
    softmax_fit(features, labels, num_classes, iters=100, lr=0.2, l2=5e-6)    (weight [C, d], bias [C], loss_history [iters])
    feature_baselines(data, train_idx, eval_idx, num_classes, rounds, device="cuda")    {"rawfeat_accuracy", "sgc_accuracy"}
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch
from torch import Tensor

from .. import ops
from .._lib import GnnmpError
from ..graph import SparseFeatures
from .link_heuristics import simple_graph, symmetric_csr

KINDS = ("sym", "rw")


def degree_scales(rowptr: Tensor, kind: str) -> Tuple[Tensor, Optional[Tensor]]:
    """(left, right) for ops.label_propagate on the CSR behind rowptr [n + 1], fp32 on rowptr's device: kind "sym" left = right =
    1 / sqrt(deg), kind "rw" left = 1 / deg and right = None; 0 where deg = 0.  Float64 arithmetic on the integer degrees on the host,
    rounded once to fp32 (the rule of link_heuristics.node_weights: the device's rsqrt never enters a score)."""
    if kind not in KINDS:
        raise ValueError(f"kind={kind!r} is not one of {KINDS}")
    d = (rowptr[1:] - rowptr[:-1]).detach().to("cpu", torch.float64)
    pos = d > 0
    safe = torch.where(pos, d, torch.ones_like(d))
    if kind == "sym":
        s = torch.where(pos, 1.0 / torch.sqrt(safe), torch.zeros_like(d)).to(torch.float32).to(rowptr.device)
        return s, s
    return torch.where(pos, 1.0 / safe, torch.zeros_like(d)).to(torch.float32).to(rowptr.device), None


def _seeds(who: str, edge_index: Tensor, num_nodes: int, seeds: Tensor, seed_labels: Tensor, num_classes: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(f0 fp32 [n, classes] one-hot on the seeds, seed mask uint8 [n], (rowptr, col)) on edge_index's device."""
    if not edge_index.is_cuda:
        raise GnnmpError(f"{who}: expected edge_index on the GPU (the HIP path has no CPU fallback), got {edge_index.device}")
    if not 1 <= int(num_classes) <= ops.LABELPROP_MAX_CLASSES:
        raise GnnmpError(f"{who}: num_classes={num_classes} (1 <= classes <= {ops.LABELPROP_MAX_CLASSES})")
    dev = edge_index.device
    seeds, seed_labels = seeds.to(dev, torch.int64).reshape(-1), seed_labels.to(dev, torch.int64).reshape(-1)
    if seeds.numel() != seed_labels.numel():
        raise GnnmpError(f"{who}: {seeds.numel()} seeds with {seed_labels.numel()} labels")
    if seeds.numel() and (int(seeds.min()) < 0 or int(seeds.max()) >= num_nodes):
        raise GnnmpError(f"{who}: a seed lies outside [0, {num_nodes})")
    if seeds.numel() and (int(seed_labels.min()) < 0 or int(seed_labels.max()) >= num_classes):
        raise GnnmpError(f"{who}: a seed label lies outside [0, {num_classes})")
    graph = simple_graph(edge_index, num_nodes)
    f0 = torch.zeros(num_nodes, int(num_classes), device=dev)
    f0[seeds, seed_labels] = 1.0
    mask = torch.zeros(num_nodes, dtype=torch.uint8, device=dev)
    mask[seeds] = 1
    return f0, mask, graph


def _checked(who: str, res):
    """res (ops.LabelPropagation or ops.FeaturePropagation) when the kernel skipped nothing; status[1] counts skipped feature entries
    only in the latter."""
    skipped, second = (int(v) for v in res.status.tolist())
    if skipped:
        raise GnnmpError(f"{who}: {skipped} adjacency entries point outside the graph and were skipped")
    if second and isinstance(res, ops.FeaturePropagation):
        raise GnnmpError(f"{who}: {second} feature entries have a column outside the matrix or out of order and were skipped")
    return res


def label_spreading(edge_index: Tensor, num_nodes: int, seeds: Tensor, seed_labels: Tensor, num_classes: int, rounds: int = 50,
                    alpha: float = 0.9) -> ops.LabelPropagation:
    """Zhou et al. 2004: F <- alpha S F + (1 - alpha) Y for `rounds` rounds from F = Y, S = D^-1/2 A D^-1/2 on the simple undirected
    graph of edge_index [2, E] (int64, on the GPU), Y the one-hot rows of the seeds (int64 node ids and their labels).  1 - alpha is
    taken in float64 and rounded once to fp32; no row is clamped."""
    f0, _, (rowptr, col) = _seeds("label_spreading", edge_index, num_nodes, seeds, seed_labels, num_classes)
    left, right = degree_scales(rowptr, "sym")
    return _checked("label_spreading", ops.label_propagate(rowptr, col, f0, rounds, float(alpha), 1.0 - float(alpha), left=left, right=right))


def label_propagation(edge_index: Tensor, num_nodes: int, seeds: Tensor, seed_labels: Tensor, num_classes: int,
                      rounds: int = 50) -> ops.LabelPropagation:
    """Zhu & Ghahramani 2002: F <- D^-1 A F for `rounds` rounds from F = Y, the seeds' rows put back to Y after every round."""
    f0, mask, (rowptr, col) = _seeds("label_propagation", edge_index, num_nodes, seeds, seed_labels, num_classes)
    left, _ = degree_scales(rowptr, "rw")
    return _checked("label_propagation", ops.label_propagate(rowptr, col, f0, rounds, 1.0, 0.0, left=left, clamp=mask))


def _splits(who: str, data, train_idx, eval_idx, device) -> Tuple[int, Tensor, Tensor, Tensor, Tensor]:
    """(n, train_idx, eval_idx, edge_index, y) of a transductive split on `device`, int64: both splits non-empty (ValueError) and inside
    [0, n) (GnnmpError)."""
    n = int(data.num_nodes)
    train_idx, eval_idx = torch.as_tensor(train_idx).to(device, torch.int64).reshape(-1), torch.as_tensor(eval_idx).to(device, torch.int64).reshape(-1)
    if train_idx.numel() == 0 or eval_idx.numel() == 0:
        raise ValueError(f"{who}: {train_idx.numel()} train and {eval_idx.numel()} evaluation nodes (both splits need one)")
    for name, idx in (("train_idx", train_idx), ("eval_idx", eval_idx)):
        if int(idx.min()) < 0 or int(idx.max()) >= n:
            raise GnnmpError(f"{who}: {name} has an entry outside [0, {n})")
    return n, train_idx, eval_idx, data.edge_index.to(device, torch.int64).contiguous(), data.y.to(device, torch.int64).reshape(-1)


def label_baselines(data, train_idx: Tensor, eval_idx: Tensor, num_classes: int, rounds: int,
                    device: Union[str, torch.device] = "cuda") -> Dict[str, float]:
    """{"labelspread_accuracy", "labelprop_accuracy", "labelspread_unreached", "labelprop_unreached"} of the two baselines at their
    defaults with `rounds` rounds.  Transductive: the graph is the whole data.edge_index (data.num_nodes nodes, labels data.y), the seeds
    are train_idx with their labels, the accuracy is over eval_idx.  *_unreached counts the nodes of eval_idx whose row of scores is all
    zero -- no label reached them; their prediction is class 0 by the tie rule and they are counted, not hidden.  GnnmpError on an index
    outside the graph and when the kernel skipped an adjacency entry."""
    if not 1 <= int(rounds) <= ops.LABELPROP_MAX_ROUNDS:
        raise ValueError(f"label_baselines: rounds={rounds} (1 <= rounds <= {ops.LABELPROP_MAX_ROUNDS})")
    n, train_idx, eval_idx, edge_index, y = _splits("label_baselines", data, train_idx, eval_idx, device)
    scores: Dict[str, float] = {}
    for name, run in (("labelspread", label_spreading), ("labelprop", label_propagation)):
        res = run(edge_index, n, train_idx, y[train_idx], num_classes, rounds=int(rounds))
        scores[f"{name}_accuracy"] = float((res.pred[eval_idx] == y[eval_idx]).float().mean())
        scores[f"{name}_unreached"] = int((res.out[eval_idx] == 0).all(dim=1).sum())
    return scores


# ---------------------------------------------------------------------------- the feature baselines: raw features and SGC
SOFTMAX_MAX_CLASSES = 32
ADAM_BETAS, ADAM_EPS = (0.9, 0.999), 1e-8


def sgc_graph(edge_index: Tensor, num_nodes: int) -> Tuple[Tensor, Tensor, Tensor]:
    """(rowptr int32 [n + 1], col int32 [nnz], scale fp32 [n]) of SGC's operator S = D~^-1/2 (A + I) D~^-1/2 on edge_index's device
    (CPU tensors work too): the simple undirected graph of simple_graph -- both directions, duplicates and the input's own loops dropped,
    rows ascending -- plus ONE self-loop per node at its sorted position, and scale = 1 / sqrt(deg + 1) with deg the simple graph's
    degree, computed in float64 on the host and rounded once to fp32 (the rule of degree_scales: the device's rsqrt never enters a
    value).  S = diag(scale) (A + I) diag(scale): pass scale as both left and right of ops.feature_propagate."""
    rowptr, col = symmetric_csr("sgc_graph", edge_index, num_nodes, self_loops=True)
    d = (rowptr[1:] - rowptr[:-1]).to("cpu", torch.float64)                       # deg + 1: the loop is counted
    scale = (1.0 / torch.sqrt(d)).to(torch.float32).to(edge_index.device)
    return rowptr, col, scale


def sgc_features(x: Union[Tensor, SparseFeatures], edge_index: Tensor, num_nodes: int, rounds: int) -> Tensor:
    """S^rounds X as a dense fp32 [n, d] tensor (ops.feature_propagate on sgc_graph): x dense fp32 [n, d] or SparseFeatures, on
    edge_index's device (the GPU); the sparse form goes to the kernel as it is.  rounds = 0 returns x densified.  GnnmpError when the
    kernel skipped an adjacency or a feature entry."""
    if not edge_index.is_cuda:
        raise GnnmpError(f"sgc_features: expected edge_index on the GPU (the HIP path has no CPU fallback), got {edge_index.device}")
    if not 0 <= int(rounds) <= ops.FEATPROP_MAX_ROUNDS:
        raise GnnmpError(f"sgc_features: rounds={rounds} (0 <= rounds <= {ops.FEATPROP_MAX_ROUNDS})")
    if int(x.shape[0]) != int(num_nodes):
        raise GnnmpError(f"sgc_features: x has {x.shape[0]} rows for {num_nodes} nodes")
    if int(rounds) == 0:
        return x.to_dense() if isinstance(x, SparseFeatures) else x.to(torch.float32).contiguous()
    rowptr, col, scale = sgc_graph(edge_index, num_nodes)
    return _checked("sgc_features", ops.feature_propagate(rowptr, col, x, int(rounds), left=scale, right=scale)).out


def adam_step_(param: Tensor, grad: Tensor, exp_avg: Tensor, exp_avg_sq: Tensor, step: int, lr: float) -> None:
    """torch.optim.Adam's update (betas 0.9 / 0.999, eps 1e-8, bias correction, no amsgrad) for step `step` >= 1, in place, written out
    in elementwise torch: m <- b1 m + (1 - b1) g, v <- b2 v + (1 - b2) g g, param <- param - (lr / (1 - b1^t)) m / (sqrt(v) /
    sqrt(1 - b2^t) + eps)."""
    b1, b2 = ADAM_BETAS
    exp_avg.mul_(b1).add_(grad, alpha=1.0 - b1)
    exp_avg_sq.mul_(b2).addcmul_(grad, grad, value=1.0 - b2)
    denom = (exp_avg_sq.sqrt() / (1.0 - b2 ** step) ** 0.5).add_(ADAM_EPS)
    param.addcdiv_(exp_avg, denom, value=-(lr / (1.0 - b1 ** step)))


def softmax_fit(features: Tensor, labels: Tensor, num_classes: int, iters: int = 100, lr: float = 0.2,
                l2: float = 5e-6) -> Tuple[Tensor, Tensor, Tensor]:
    """(weight [C, d], bias [C], loss_history [iters]) of a full-batch softmax regression on features fp32 [m, d] (on the GPU) with
    labels int64 [m], started from zeros, `iters` Adam steps: no random state.  Per step: logits = ops.gemm(NT, F, W, bias), the mean
    cross-entropy and dL/dlogits by ops.cross_entropy_sum_fwd / _bwd with g_scale = 1 / m, gW = ops.gemm(TN, G, F) + l2 * W,
    gb = ops.colsum(G), then adam_step_ on both.  loss_history[t] is the mean cross-entropy before step t + 1 (the ridge term is not in
    it).  lr, l2 and iters are the defaults of SGC's published code; the one stated difference is that the ridge applies to the weights
    alone (Adam's weight_decay there covers the bias too).  No rocBLAS call, no row normalisation; any d >= 1, 2 <= C <= 32.  Bitwise
    repeatable: the GEMM's split-K sums its slices in order and every other operation is elementwise or a fixed-order sum."""
    if not features.is_cuda:
        raise GnnmpError(f"softmax_fit: expected features on the GPU (the HIP path has no CPU fallback), got {features.device}")
    C = int(num_classes)
    if features.dtype != torch.float32 or features.dim() != 2 or features.size(0) < 1 or features.size(1) < 1:
        raise GnnmpError(f"softmax_fit: features must be a non-empty fp32 [m, d] tensor, got {features.dtype} {tuple(features.shape)}")
    if not 2 <= C <= SOFTMAX_MAX_CLASSES or int(iters) < 1:
        raise GnnmpError(f"softmax_fit: num_classes={num_classes} iters={iters} (2 <= classes <= {SOFTMAX_MAX_CLASSES}, iters >= 1)")
    dev, (m, d) = features.device, features.shape
    F = features.contiguous()
    y = labels.to(dev, torch.int64).reshape(-1).contiguous()
    if y.numel() != m or int(y.min()) < 0 or int(y.max()) >= C:
        raise GnnmpError(f"softmax_fit: {y.numel()} labels for {m} rows, or a label outside [0, {C})")
    W, b = torch.zeros(C, d, device=dev), torch.zeros(C, device=dev)
    state = [torch.zeros_like(t) for t in (W, W, b, b)]
    g_scale = torch.full((1,), 1.0 / m, device=dev)
    history = torch.empty(int(iters), device=dev)
    for t in range(1, int(iters) + 1):
        logits = ops.gemm(ops.NT, F, W, bias=b)
        history[t - 1] = (ops.cross_entropy_sum_fwd(logits, y) * g_scale)[0]
        G = ops.cross_entropy_sum_bwd(logits, y, g_scale)
        gW = ops.gemm(ops.TN, G, F).add_(W, alpha=float(l2))
        gb = ops.colsum(G)
        adam_step_(W, gW, state[0], state[1], t, float(lr))
        adam_step_(b, gb, state[2], state[3], t, float(lr))
    return W, b, history


def feature_baselines(data, train_idx: Tensor, eval_idx: Tensor, num_classes: int, rounds: int,
                      device: Union[str, torch.device] = "cuda") -> Dict[str, float]:
    """{"rawfeat_accuracy", "sgc_accuracy"}: softmax_fit at its defaults on the raw features (sgc_features with 0 rounds: no graph) and
    on S^rounds X (SGC).  Transductive: the features data.x (dense or SparseFeatures) are propagated over the whole data.edge_index
    (data.num_nodes nodes, labels data.y), the regression is fitted on the rows of train_idx and the accuracy is over eval_idx.
    GnnmpError on an index outside the graph and when the kernel skipped an adjacency or a feature entry."""
    if not 1 <= int(rounds) <= ops.FEATPROP_MAX_ROUNDS:
        raise ValueError(f"feature_baselines: rounds={rounds} (1 <= rounds <= {ops.FEATPROP_MAX_ROUNDS})")
    n, train_idx, eval_idx, edge_index, y = _splits("feature_baselines", data, train_idx, eval_idx, device)
    x = data.x.to(device)
    scores: Dict[str, float] = {}
    for name, k in (("rawfeat", 0), ("sgc", int(rounds))):
        feats = sgc_features(x, edge_index, n, k)
        weight, bias, _ = softmax_fit(feats[train_idx], y[train_idx], num_classes)
        pred = ops.gemm(ops.NT, feats[eval_idx], weight, bias=bias).argmax(dim=1)
        scores[f"{name}_accuracy"] = float((pred == y[eval_idx]).float().mean())
    return scores
