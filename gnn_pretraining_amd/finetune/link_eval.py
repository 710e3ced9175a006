"""The protocol of LinkPredictionEngine.rank, once, for every scorer that is not the trained one: a LinkScorer says how a family scores
explicit pairs and ranks true pairs against all nodes (link_heuristics.scorer, link_walks.scorer, link_probe.scorer); scores() and ranks()
check the pairs, build the filter CSR and turn the counts into ranks."""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Tuple

import torch
from torch import Tensor

from .._lib import GnnmpError
from ..operators import _lp_filter
from .engine import LinkRanks


@dataclass(frozen=True)
class LinkScorer:
    name: str               # the family, as its public wrappers are called: {name}_scores / {name}_ranks
    num_nodes: int
    score: Callable         # (src [P], dst [P]) -> score [P]
    rank: Callable          # (src [Q], dst [Q], filter_rowptr, filter_col) -> (score_true [Q], n_greater [Q], n_equal [Q])


def check_kind(kind: str, kinds: Tuple[str, ...]) -> None:
    if kind not in kinds:
        raise ValueError(f"kind={kind!r} is not one of {kinds}")


def _pairs(who: str, pairs: Tensor) -> Tensor:
    if pairs.dtype != torch.int64 or pairs.dim() != 2 or pairs.size(0) != 2:
        raise GnnmpError(f"{who}: pairs must be an int64 [2, P] tensor, got {pairs.dtype} {tuple(pairs.shape)}")
    return pairs.contiguous()


def scores(scorer: LinkScorer, pairs: Tensor) -> Tensor:
    """score [P] (fp32) of the pairs [2, P] under `scorer`."""
    p = _pairs(f"{scorer.name}_scores", pairs)
    return scorer.score(p[0], p[1])


def ranks(scorer: LinkScorer, edges: Tensor, filter_edges: Optional[Tensor] = None) -> LinkRanks:
    """Every true pair of edges [2, Q] ranked against all nodes as destinations under `scorer`, exactly as LinkPredictionEngine.rank ranks
    with the trained scorer: the source, the destination and every c with (source, c) in filter_edges [2, E] are no candidates; rank =
    1 + n_greater + n_equal / 2.  The true pair's score stands in LinkRanks.logit."""
    e = _pairs(f"{scorer.name}_ranks", edges)
    frowptr, fcol = _lp_filter(f"{scorer.name}_ranks", filter_edges, scorer.num_nodes)
    score, n_greater, n_equal = scorer.rank(e[0], e[1], frowptr, fcol)
    return LinkRanks.from_counts(n_greater, n_equal, score)
