"""The walk-based baselines of link prediction -- the Katz index, rooted (personalised) PageRank and the hop distance -- scored and ranked
on the GPU under the protocol of LinkPredictionEngine.rank (csrc/lp_walk.hip; the definition is above gmp_lp_walk_score in
include/gnnmp.h).  Where the neighbourhood baselines of link_heuristics.py see two hops, these see `rounds`.  They read a graph only: no
model, no generator, no dropout counter, no BatchNorm state.

All three are parametrisations of one damped walk sum, acc = sum over l <= rounds of y_l with y_l = damping * A diag(weight) y_{l-1}:

    katz   weight None, damping KATZ_BETA: the truncated Katz index, sum over l <= rounds of beta^l (A^l)[s, c]
    ppr    weight 1 / deg (node_weights(deg, "ra")), damping 1 - PPR_ALPHA: the `rounds`-term rooted PageRank of s at c DIVIDED BY alpha --
           the constant factor alpha is left out, the order is the same
    hops   minus the BFS distance, -(rounds + 1) for everything further away (the kernel's integer mode, not acc > 0)

    walk_scores(edge_index, num_nodes, pairs, kind, rounds)                          score [P]
    walk_ranks(edge_index, num_nodes, edges, kind, rounds, filter_edges=None)        LinkRanks, the score in the logit slot
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import ops
from ..operators import _lp_filter
from . import link_heuristics as LH
from .engine import LinkRanks

KINDS = ("katz", "ppr", "hops")
KATZ_BETA = 0.05
PPR_ALPHA = 0.15


def _check_kind(kind: str) -> None:
    if kind not in KINDS:
        raise ValueError(f"kind={kind!r} is not one of {KINDS}")


def damping_of(kind: str) -> float:
    """The damping of `kind` as the kernel takes it: the float64 constant rounded once to fp32 (1.0, unread, for hops)."""
    _check_kind(kind)
    value = {"katz": KATZ_BETA, "ppr": 1.0 - PPR_ALPHA, "hops": 1.0}[kind]
    return torch.tensor(value, dtype=torch.float64).to(torch.float32).item()


def _scorer(edge_index: Tensor, num_nodes: int, kind: str):
    _check_kind(kind)
    rowptr, col, weight, _ = LH._scorer(edge_index, num_nodes, "ra" if kind == "ppr" else "cn")        # the cached graph and 1 / deg
    return rowptr, col, weight, damping_of(kind), "hops" if kind == "hops" else "sum"


def walk_scores(edge_index: Tensor, num_nodes: int, pairs: Tensor, kind: str, rounds: int) -> Tensor:
    """score [P] (fp32) of the pairs [2, P] under `kind` with `rounds` rounds on the simple graph of edge_index."""
    rowptr, col, weight, damping, mode = _scorer(edge_index, num_nodes, kind)
    p = LH._pairs("walk_scores", pairs)
    return ops.lp_walk_score(rowptr, col, p[0], p[1], rounds, damping, weight, mode)


def walk_ranks(edge_index: Tensor, num_nodes: int, edges: Tensor, kind: str, rounds: int, filter_edges: Optional[Tensor] = None) -> LinkRanks:
    """Every true pair of edges [2, Q] ranked against all nodes as destinations under `kind` with `rounds` rounds on the simple graph of
    edge_index, exactly as link_heuristics.heuristic_ranks ranks: the source, the destination and every c with (source, c) in
    filter_edges [2, E] are no candidates; rank = 1 + n_greater + n_equal / 2.  The true pair's score stands in LinkRanks.logit."""
    rowptr, col, weight, damping, mode = _scorer(edge_index, num_nodes, kind)
    e = LH._pairs("walk_ranks", edges)
    frowptr, fcol = _lp_filter("walk_ranks", filter_edges, num_nodes)
    score, n_greater, n_equal = ops.lp_walk_rank(rowptr, col, e[0], e[1], rounds, damping, weight, mode, frowptr, fcol)
    return LinkRanks.from_counts(n_greater, n_equal, score)
