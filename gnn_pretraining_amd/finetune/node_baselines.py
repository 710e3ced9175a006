"""The model-free baselines of node classification: label spreading (Zhou et al., NIPS 2004) and label propagation (Zhu & Ghahramani,
2002) over the raw graph, iterated on the GPU (csrc/label_prop.hip; the definition is above gmp_label_propagate in include/gnnmp.h).  On
citation graphs this is the number a GNN is expected to beat.  They read the graph and the train split's labels only: no model, no
generator, no dropout counter, no BatchNorm state.

    degree_scales(rowptr, kind)                      (left, right) fp32 scales of the propagation: "sym" D^-1/2 A D^-1/2, "rw" D^-1 A
    label_spreading(edge_index, num_nodes, seeds, seed_labels, num_classes, rounds=50, alpha=0.9)    ops.LabelPropagation
    label_propagation(edge_index, num_nodes, seeds, seed_labels, num_classes, rounds=50)             ops.LabelPropagation
    label_baselines(data, train_idx, eval_idx, num_classes, rounds, device="cuda")
        {"labelspread_accuracy", "labelprop_accuracy", "labelspread_unreached", "labelprop_unreached"}
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple, Union

import torch
from torch import Tensor

from .. import ops
from .._lib import GnnmpError
from .link_heuristics import simple_graph

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


def _checked(who: str, res: ops.LabelPropagation) -> ops.LabelPropagation:
    skipped = int(res.status[0])
    if skipped:
        raise GnnmpError(f"{who}: {skipped} adjacency entries point outside the graph and were skipped")
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


def label_baselines(data, train_idx: Tensor, eval_idx: Tensor, num_classes: int, rounds: int,
                    device: Union[str, torch.device] = "cuda") -> Dict[str, float]:
    """{"labelspread_accuracy", "labelprop_accuracy", "labelspread_unreached", "labelprop_unreached"} of the two baselines at their
    defaults with `rounds` rounds.  Transductive: the graph is the whole data.edge_index (data.num_nodes nodes, labels data.y), the seeds
    are train_idx with their labels, the accuracy is over eval_idx.  *_unreached counts the nodes of eval_idx whose row of scores is all
    zero -- no label reached them; their prediction is class 0 by the tie rule and they are counted, not hidden.  GnnmpError on an index
    outside the graph and when the kernel skipped an adjacency entry."""
    if not 1 <= int(rounds) <= ops.LABELPROP_MAX_ROUNDS:
        raise ValueError(f"label_baselines: rounds={rounds} (1 <= rounds <= {ops.LABELPROP_MAX_ROUNDS})")
    n = int(data.num_nodes)
    train_idx, eval_idx = torch.as_tensor(train_idx).to(device, torch.int64).reshape(-1), torch.as_tensor(eval_idx).to(device, torch.int64).reshape(-1)
    if train_idx.numel() == 0 or eval_idx.numel() == 0:
        raise ValueError(f"label_baselines: {train_idx.numel()} train and {eval_idx.numel()} evaluation nodes (both splits need one)")
    for name, idx in (("train_idx", train_idx), ("eval_idx", eval_idx)):
        if int(idx.min()) < 0 or int(idx.max()) >= n:
            raise GnnmpError(f"label_baselines: {name} has an entry outside [0, {n})")
    edge_index = data.edge_index.to(device, torch.int64).contiguous()
    y = data.y.to(device, torch.int64).reshape(-1)
    scores: Dict[str, float] = {}
    for name, run in (("labelspread", label_spreading), ("labelprop", label_propagation)):
        res = run(edge_index, n, train_idx, y[train_idx], num_classes, rounds=int(rounds))
        scores[f"{name}_accuracy"] = float((res.pred[eval_idx] == y[eval_idx]).float().mean())
        scores[f"{name}_unreached"] = int((res.out[eval_idx] == 0).all(dim=1).sum())
    return scores
