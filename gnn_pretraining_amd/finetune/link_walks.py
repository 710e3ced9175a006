"""The walk-based baselines of link prediction -- the Katz index, rooted (personalised) PageRank and the hop distance -- scored and ranked
on the GPU under the protocol of LinkPredictionEngine.rank (csrc/lp_walk.hip; the definition is above gmp_lp_walk_score in
include/gnnmp.h).  Where the neighbourhood baselines of link_heuristics.py see two hops, these see `rounds`.  They read a graph only: no
model, no generator, no dropout counter, no BatchNorm state.

All three are parametrisations of one damped walk sum, acc = sum over l <= rounds of y_l with y_l = damping * A diag(weight) y_{l-1}:

    katz   weight None, damping KATZ_BETA: the truncated Katz index, sum over l <= rounds of beta^l (A^l)[s, c]
    ppr    weight 1 / deg (node_weights(deg, "ra")), damping 1 - PPR_ALPHA: the `rounds`-term rooted PageRank of s at c DIVIDED BY alpha --
           the constant factor alpha is left out, the order is the same
    hops   minus the BFS distance, -(rounds + 1) for everything further away (the kernel's integer mode, not acc > 0)

    scorer(edge_index, num_nodes, kind, rounds)                                      the LinkScorer of `kind` (link_eval.py)
    walk_scores(edge_index, num_nodes, pairs, kind, rounds)                          score [P]
    walk_ranks(edge_index, num_nodes, edges, kind, rounds, filter_edges=None)        LinkRanks, the score in the logit slot
"""
from __future__ import annotations

from typing import Optional

import torch
from torch import Tensor

from .. import ops
from . import link_eval as LE, link_heuristics as LH
from .engine import LinkRanks

KINDS = ("katz", "ppr", "hops")
KATZ_BETA = 0.05
PPR_ALPHA = 0.15


def damping_of(kind: str) -> float:
    """The damping of `kind` as the kernel takes it: the float64 constant rounded once to fp32 (1.0, unread, for hops)."""
    LE.check_kind(kind, KINDS)
    value = {"katz": KATZ_BETA, "ppr": 1.0 - PPR_ALPHA, "hops": 1.0}[kind]
    return torch.tensor(value, dtype=torch.float64).to(torch.float32).item()


def _kernel_args(edge_index: Tensor, num_nodes: int, kind: str):
    LE.check_kind(kind, KINDS)
    rowptr, col, weight, _ = LH._kernel_args(edge_index, num_nodes, "ra" if kind == "ppr" else "cn")   # the cached graph and 1 / deg
    return rowptr, col, weight, damping_of(kind), "hops" if kind == "hops" else "sum"


def scorer(edge_index: Tensor, num_nodes: int, kind: str, rounds: int) -> LE.LinkScorer:
    """`kind` with `rounds` rounds on the simple graph of edge_index (cached) as link_eval scores and ranks with it."""
    rowptr, col, weight, damping, mode = _kernel_args(edge_index, num_nodes, kind)
    return LE.LinkScorer("walk", num_nodes, lambda s, d: ops.lp_walk_score(rowptr, col, s, d, rounds, damping, weight, mode),
                         lambda s, d, frowptr, fcol: ops.lp_walk_rank(rowptr, col, s, d, rounds, damping, weight, mode, frowptr, fcol))


def walk_scores(edge_index: Tensor, num_nodes: int, pairs: Tensor, kind: str, rounds: int) -> Tensor:
    """score [P] (fp32) of the pairs [2, P] under `kind` with `rounds` rounds on the simple graph of edge_index."""
    return LE.scores(scorer(edge_index, num_nodes, kind, rounds), pairs)


def walk_ranks(edge_index: Tensor, num_nodes: int, edges: Tensor, kind: str, rounds: int, filter_edges: Optional[Tensor] = None) -> LinkRanks:
    """link_eval.ranks under `kind` with `rounds` rounds on the simple graph of edge_index, as link_heuristics.heuristic_ranks ranks."""
    return LE.ranks(scorer(edge_index, num_nodes, kind, rounds), edges, filter_edges)
