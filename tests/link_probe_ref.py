"""Shared by test_link_probe_host.py and test_gpu_link_probe.py: the float64 definition of the embedding link probe of csrc/emb_link.hip
(gnnmp.h gmp_emb_link_score / gmp_emb_link_rank, finetune/link_probe.py), written from the contract and not from the kernel.

  scores       S [N, N] float64: mode "cos" normalize(h) normalize(h)^T (knn_ref.normalize: z / max(||z||, 1e-12), a zero row stays
               zero), mode "dot" h h^T
  pair_scores  S[src, dst] per pair; an endpoint outside [0, N) is a zero row: 0
  ranks        per true pair (s, d), by plain loops over the candidates c in [0, N) except c == s, c == d and every c with (s, c) in
               filter_edges [2, E] (any order, duplicates and out-of-range entries allowed): n_greater = #{score(s, c) > score(s, d)},
               n_equal = #{==}; a source outside [0, N) scores 0 against everything and has no filter row.  `similarity=` [Q, N] replays
               the counting on someone else's scores (row q = query q: the kernel's own matrix); the true score is then
               similarity[q, d], 0 for d outside.
  rank_of      1 + n_greater + n_equal / 2
  auc          the share of (positive, negative) pairs the positive wins, a tie one half; nan when a class is empty
plus the two exact-arithmetic row generators of knn_ref."""
import numpy as np

import link_rank_ref as P
from link_rank_ref import rank_of  # noqa: F401  (re-exported)

from knn_ref import four_ones, normalize, sixteen_signs  # noqa: F401  (the generators are re-exported)

KINDS = ("cos", "dot")


def scores(h, mode="cos"):
    h = np.asarray(h, dtype=np.float64)
    if mode not in KINDS:
        raise ValueError(mode)
    z = normalize(h) if mode == "cos" else h
    return z @ z.T


def _row(S, q, s, n, per_query):
    """the scores of source s against every node"""
    if per_query:
        return np.asarray(S[q])
    return np.asarray(S[s]) if 0 <= s < n else np.zeros(n, dtype=np.asarray(S).dtype)


def pair_scores(h, src, dst, mode="cos"):
    S = scores(h, mode)
    n = S.shape[0]
    return np.array([S[s, d] if 0 <= s < n and 0 <= d < n else 0.0 for s, d in zip(src, dst)], dtype=np.float64)


def ranks(S, src, dst, filter_edges=None, similarity=None):
    """(score_true [Q], n_greater [Q] int64, n_equal [Q] int64); S [N, N] or None with similarity [Q, N]"""
    per_query = similarity is not None
    M = np.asarray(similarity) if per_query else np.asarray(S)
    n = M.shape[1]
    return P.ranks(n, src, dst, lambda q, s: _row(M, q, s, n, per_query), lambda q, s, d, row: row[d] if 0 <= d < n else row.dtype.type(0),
                   P.filter_rows(filter_edges, n))


def auc(scores_, labels):
    s, y = np.asarray(scores_, dtype=np.float64), np.asarray(labels) != 0
    pos, neg = s[y], s[~y]
    if pos.size == 0 or neg.size == 0:
        return float("nan")
    wins = sum(float(p > m) + 0.5 * float(p == m) for p in pos for m in neg)
    return wins / (pos.size * neg.size)
