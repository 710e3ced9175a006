"""The embedding link probe -- what the GAE, DGI and GRACE-style link evaluations report: the backbone's node embeddings taken as they
are, a pair scored by the cosine or the inner product of its two rows, scored and ranked on the GPU under the protocol of
LinkPredictionEngine.rank (csrc/emb_link.hip; the definition is above gmp_emb_link_score in include/gnnmp.h).  Where --lp-ranking
measures the trained 768 -> 256 -> 1 scorer and link_heuristics.py / link_walks.py never see the model, this reads the embeddings alone:
no parameters, no fitting, no random state -- no generator, no dropout counter, no BatchNorm state -- so it means something before the
first training step too.

    cos    the cosine of the two rows, rows normalised as the k-NN probe normalises them (a zero row scores 0)
    dot    the inner product of the raw rows (the GAE decoder without its sigmoid: the order is the same)

    scorer(emb, kind)                                            the LinkScorer of `kind` (link_eval.py)
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
from . import link_eval as LE
from .engine import LinkRanks
from .metrics import ranking_metrics

KINDS = ("cos", "dot")


def scorer(emb: Tensor, kind: str) -> LE.LinkScorer:
    """`kind` on the rows of emb [N, d <= 256] as link_eval scores and ranks with it."""
    LE.check_kind(kind, KINDS)
    h = emb.detach().contiguous()
    return LE.LinkScorer("embedding", emb.size(0), lambda s, d: ops.emb_link_score(h, s, d, kind),
                         lambda s, d, frowptr, fcol: ops.emb_link_rank(h, s, d, kind, frowptr, fcol))


def embedding_scores(emb: Tensor, pairs: Tensor, kind: str) -> Tensor:
    """score [P] (fp32) of the pairs [2, P] under `kind` from the rows of emb [N, d <= 256]."""
    return LE.scores(scorer(emb, kind), pairs)


def embedding_ranks(emb: Tensor, edges: Tensor, kind: str, filter_edges: Optional[Tensor] = None) -> LinkRanks:
    """link_eval.ranks under `kind` on the rows of emb [N, d <= 256], as LinkPredictionEngine.rank ranks with the trained scorer."""
    return LE.ranks(scorer(emb, kind), edges, filter_edges)


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
