"""The embedding link probe -- what the GAE, DGI and GRACE-style link evaluations report: the backbone's node embeddings taken as they
are, a pair scored by the cosine or the inner product of its two rows, scored and ranked on the GPU under the protocol of
LinkPredictionEngine.rank (csrc/emb_link.hip; the definition is above gmp_emb_link_score in include/gnnmp.h).  Where --lp-ranking
measures the trained 768 -> 256 -> 1 scorer and link_heuristics.py / link_walks.py never see the model, this reads the embeddings alone:
no parameters, no fitting, no random state -- no generator, no dropout counter, no BatchNorm state -- so it means something before the
first training step too.

    cos    the cosine of the two rows, rows normalised as the k-NN probe normalises them (a zero row scores 0)
    dot    the inner product of the raw rows (the GAE decoder without its sigmoid: the order is the same)

    embedding_scores(emb, pairs, kind)                           score [P]
    embedding_ranks(emb, edges, kind, filter_edges=None)         LinkRanks, the score in the logit slot
    pair_auc(scores, labels)                                     the area under the ROC curve, ties counted one half
    link_probe(emb, edges, filter_edges, pairs, labels)          {"embed_{kind}_mrr", "_hits@1", "_hits@10", "_hits@50", "_auc"} per kind
"""
from __future__ import annotations

from typing import Dict, Optional

import torch
from torch import Tensor

from .. import ops
from ..operators import _lp_filter
from .engine import LinkRanks
from .link_heuristics import _pairs
from .metrics import ranking_metrics

KINDS = ("cos", "dot")


def _check_kind(kind: str) -> None:
    if kind not in KINDS:
        raise ValueError(f"kind={kind!r} is not one of {KINDS}")


def embedding_scores(emb: Tensor, pairs: Tensor, kind: str) -> Tensor:
    """score [P] (fp32) of the pairs [2, P] under `kind` from the rows of emb [N, d <= 256]."""
    _check_kind(kind)
    p = _pairs("embedding_scores", pairs)
    return ops.emb_link_score(emb.detach().contiguous(), p[0], p[1], kind)


def embedding_ranks(emb: Tensor, edges: Tensor, kind: str, filter_edges: Optional[Tensor] = None) -> LinkRanks:
    """Every true pair of edges [2, Q] ranked against all nodes as destinations under `kind`, exactly as LinkPredictionEngine.rank ranks
    with the trained scorer: the source, the destination and every c with (source, c) in filter_edges [2, E] are no candidates; rank =
    1 + n_greater + n_equal / 2.  The true pair's score stands in LinkRanks.logit."""
    _check_kind(kind)
    e = _pairs("embedding_ranks", edges)
    frowptr, fcol = _lp_filter("embedding_ranks", filter_edges, emb.size(0))
    score, n_greater, n_equal = ops.emb_link_rank(emb.detach().contiguous(), e[0], e[1], kind, frowptr, fcol)
    return LinkRanks.from_counts(n_greater, n_equal, score)


def pair_auc(scores: Tensor, labels: Tensor) -> float:
    """The Mann-Whitney statistic of scores [P] against labels [P] (nonzero = positive): the share of (positive, negative) pairs the
    positive wins, a tie counted one half -- roc_auc_score's value.  Integer counts from one sort of the negatives, made where the
    tensors live, so it is exact whatever the order; nan when a class is empty."""
    s, y = scores.detach().reshape(-1), labels.reshape(-1) != 0
    if s.numel() != y.numel():
        raise ValueError(f"pair_auc: {s.numel()} scores for {y.numel()} labels")
    pos, neg = s[y], torch.sort(s[~y]).values
    if pos.numel() == 0 or neg.numel() == 0:
        return float("nan")
    below = torch.searchsorted(neg, pos.contiguous(), right=False)          # negatives strictly below each positive
    upto = torch.searchsorted(neg, pos.contiguous(), right=True)            # ... at or below it
    twice = int((below + upto).sum())                                       # 2 wins + ties
    return twice / (2.0 * pos.numel() * neg.numel())


def link_probe(emb: Tensor, edges: Tensor, filter_edges: Optional[Tensor], pairs: Tensor, labels: Tensor) -> Dict[str, float]:
    """Both kinds on one embedding matrix: embed_{kind}_mrr / _hits@1 / _hits@10 / _hits@50 of the true edges [2, Q] ranked by
    embedding_ranks under filter_edges, and embed_{kind}_auc of the labelled pairs [2, P] (pair_auc of embedding_scores)."""
    out = {}
    for kind in KINDS:
        ranks = embedding_ranks(emb, edges, kind, filter_edges).rank
        out.update({f"embed_{kind}_{k}": v for k, v in ranking_metrics(ranks).items()})
        out[f"embed_{kind}_auc"] = pair_auc(embedding_scores(emb, pairs, kind), labels)
    return out
