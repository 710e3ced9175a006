"""The classical neighbourhood baselines of link prediction -- common neighbours, Jaccard, Adamic-Adar, resource allocation -- scored and
ranked on the GPU under the protocol of LinkPredictionEngine.rank (csrc/lp_heuristics.hip; the contract is above gmp_lp_cn_score in
include/gnnmp.h).  They read a graph only: no model, no generator, no dropout counter, no BatchNorm state.

    simple_graph(edge_index, num_nodes)      the simple undirected graph of an edge list as an int32 CSR, checked once, cached per tensor
    node_weights(deg, kind)                  the per-node weight of the sum (host float64, rounded once to fp32); None for cn / jaccard
    scorer(edge_index, num_nodes, kind)                                           the LinkScorer of `kind` (link_eval.py)
    heuristic_scores(edge_index, num_nodes, pairs, kind)                          score [P]
    heuristic_ranks(edge_index, num_nodes, edges, kind, filter_edges=None)        LinkRanks, the score in the logit slot
"""
from __future__ import annotations

import weakref
from typing import Dict, Optional, Tuple

import torch
from torch import Tensor

from .. import ops
from .._lib import GnnmpError
from . import link_eval as LE
from .engine import LinkRanks

KINDS = ("cn", "jaccard", "aa", "ra")

_GRAPH_CACHE: Dict[int, Tuple[weakref.ref, int, int, Tuple[Tensor, Tensor], Dict[str, Optional[Tensor]]]] = {}
_GRAPH_CACHE_MAX = 64


def symmetric_csr(who: str, edge_index: Tensor, num_nodes: int, self_loops: bool) -> Tuple[Tensor, Tensor]:
    """(rowptr int32 [num_nodes + 1], col int32 [nnz]) of edge_index [2, E] (int64, any device) with both directions of every edge, rows
    ascending, duplicates removed; self_loops False drops every loop, True leaves exactly one per node at its sorted position."""
    n = int(num_nodes)
    if edge_index.dtype != torch.int64 or edge_index.dim() != 2 or edge_index.size(0) != 2:
        raise GnnmpError(f"{who}: edge_index must be an int64 [2, E] tensor, got {edge_index.dtype} {tuple(edge_index.shape)}")
    if not 0 <= n < 2 ** 31:
        raise GnnmpError(f"{who}: num_nodes={num_nodes}")
    if edge_index.numel() and (int(edge_index.min()) < 0 or int(edge_index.max()) >= n):
        raise GnnmpError(f"{who}: an endpoint lies outside [0, {n})")
    both = torch.cat([edge_index, edge_index.flip(0)], dim=1)                      # symmetrised
    if self_loops:
        both = torch.cat([both, torch.arange(n, dtype=torch.int64, device=edge_index.device).expand(2, n)], dim=1)
    else:
        both = both[:, both[0] != both[1]]
    key = torch.unique(both[0] * n + both[1])                                      # sorted by (row, col), no duplicates: a loop stands once
    if key.numel() >= 2 ** 31:
        raise GnnmpError(f"{who}: {key.numel()} entries do not fit an int32 CSR")
    row = torch.div(key, max(n, 1), rounding_mode="floor")
    rowptr = torch.zeros(n + 1, dtype=torch.int64, device=edge_index.device)
    rowptr[1:] = torch.cumsum(torch.bincount(row, minlength=n), dim=0)
    return rowptr.to(torch.int32).contiguous(), (key - row * n).to(torch.int32).contiguous()


def _build_simple_graph(edge_index: Tensor, num_nodes: int) -> Tuple[Tensor, Tensor]:
    rowptr, col = symmetric_csr("simple_graph", edge_index, num_nodes, self_loops=False)
    bad = int(ops.graph_simple_check(rowptr, col).item())
    if bad:
        raise GnnmpError(f"simple_graph: the CSR built from edge_index has {bad} entries that break the simple-graph contract")
    return rowptr, col


def _graph(edge_index: Tensor, num_nodes: int):
    key = id(edge_index)
    hit = _GRAPH_CACHE.get(key)
    if hit is not None and hit[0]() is edge_index and hit[1] == edge_index._version and hit[2] == num_nodes:
        return hit
    entry = (weakref.ref(edge_index), edge_index._version, num_nodes, _build_simple_graph(edge_index, num_nodes), {})
    if len(_GRAPH_CACHE) >= _GRAPH_CACHE_MAX:
        for k in [k for k, v in _GRAPH_CACHE.items() if v[0]() is None] or list(_GRAPH_CACHE)[: _GRAPH_CACHE_MAX // 2]:
            _GRAPH_CACHE.pop(k, None)
    _GRAPH_CACHE[key] = entry
    return entry


def simple_graph(edge_index: Tensor, num_nodes: int) -> Tuple[Tensor, Tensor]:
    """(rowptr int32 [num_nodes + 1], col int32 [nnz]) of the simple undirected graph behind edge_index [2, E] (int64, on the GPU): both
    directions of every edge, self-loops dropped, rows sorted, duplicates removed.  Built with torch ops once per tensor (cached like
    operators.csr_of) and passed through ops.graph_simple_check; GnnmpError if that counts a violation or an endpoint is out of range."""
    return _graph(edge_index, num_nodes)[3]


def node_weights(deg: Tensor, kind: str) -> Optional[Tensor]:
    """The weight vector of the common-neighbour sum for `kind`, fp32 on the host: aa 1 / ln(deg) where deg >= 2 else 0, ra 1 / deg where
    deg >= 1 else 0 -- float64 arithmetic on the integer degrees, rounded once to fp32 (the device's log never enters a score).  None for
    cn (every weight is 1) and jaccard."""
    LE.check_kind(kind, KINDS)
    if kind in ("cn", "jaccard"):
        return None
    d = deg.detach().to("cpu", torch.float64)
    if kind == "aa":
        w = torch.where(d >= 2, 1.0 / torch.log(d.clamp(min=2.0)), torch.zeros_like(d))
    else:
        w = torch.where(d >= 1, 1.0 / d.clamp(min=1.0), torch.zeros_like(d))
    return w.to(torch.float32)


def _kernel_args(edge_index: Tensor, num_nodes: int, kind: str):
    LE.check_kind(kind, KINDS)
    _, _, _, (rowptr, col), weights = _graph(edge_index, num_nodes)
    if kind not in weights:
        w = node_weights(rowptr[1:] - rowptr[:-1], kind)
        weights[kind] = None if w is None else w.to(rowptr.device)
    return rowptr, col, weights[kind], "jaccard" if kind == "jaccard" else "sum"


def scorer(edge_index: Tensor, num_nodes: int, kind: str) -> LE.LinkScorer:
    """`kind` on the simple graph of edge_index (cached) as link_eval scores and ranks with it."""
    rowptr, col, weight, mode = _kernel_args(edge_index, num_nodes, kind)
    return LE.LinkScorer("heuristic", num_nodes, lambda s, d: ops.lp_cn_score(rowptr, col, s, d, weight, mode),
                         lambda s, d, frowptr, fcol: ops.lp_cn_rank(rowptr, col, s, d, weight, mode, frowptr, fcol))


def heuristic_scores(edge_index: Tensor, num_nodes: int, pairs: Tensor, kind: str) -> Tensor:
    """score [P] (fp32) of the pairs [2, P] under `kind` on the simple graph of edge_index."""
    return LE.scores(scorer(edge_index, num_nodes, kind), pairs)


def heuristic_ranks(edge_index: Tensor, num_nodes: int, edges: Tensor, kind: str, filter_edges: Optional[Tensor] = None) -> LinkRanks:
    """link_eval.ranks under `kind` on the simple graph of edge_index, as LinkPredictionEngine.rank ranks with the trained scorer."""
    return LE.ranks(scorer(edge_index, num_nodes, kind), edges, filter_edges)
