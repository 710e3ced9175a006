"""CPU reference of the structural link baselines (include/gnnmp.h above gmp_lp_cn_score), numpy only, restating the contract literally:
the simple graph of an edge list, the node weights in float64 rounded once, a float32 accumulator over all candidates that adds w[z] for z
in N(s) ascending, counts from a validity mask, Jaccard compared through Python integers."""
import math

import numpy as np

import link_rank_ref as P
from link_rank_ref import filter_rows, rank_of  # noqa: F401  (re-exported)

KINDS = ("cn", "jaccard", "aa", "ra")


def simple_csr(edge_index, n):
    """(rowptr, col) int64 of the simple undirected graph: both directions, no loops, rows ascending, no duplicates."""
    e = np.asarray(edge_index, dtype=np.int64).reshape(2, -1)
    both = np.concatenate([e, e[::-1]], axis=1)
    both = both[:, both[0] != both[1]]
    key = np.unique(both[0] * n + both[1])
    row, col = key // max(n, 1), key % max(n, 1)
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n))
    return rowptr, col


def weights(rowptr, kind):
    """float32 [n] or None: aa 1 / ln(deg) for deg >= 2 else 0, ra 1 / deg for deg >= 1 else 0, float64 rounded once."""
    if kind in ("cn", "jaccard"):
        return None
    deg = np.diff(rowptr)
    if kind == "aa":
        w = [1.0 / math.log(int(d)) if d >= 2 else 0.0 for d in deg]
    else:
        w = [1.0 / int(d) if d >= 1 else 0.0 for d in deg]
    return np.asarray(w, dtype=np.float64).astype(np.float32)


def _row(rowptr, col, v):
    return col[rowptr[v]:rowptr[v + 1]] if 0 <= v < len(rowptr) - 1 else col[:0]


def accumulate(rowptr, col, s, w):
    """acc [n] float32: the weighted common-neighbour sum of s with every node, z ascending, one float32 add each."""
    acc = np.zeros(len(rowptr) - 1, dtype=np.float32)
    for z in _row(rowptr, col, s):
        acc[_row(rowptr, col, z)] += np.float32(1.0 if w is None else w[z])       # (a row has no duplicates: one add per slot)
    return acc


def pair_scores(rowptr, col, src, dst, w=None, mode="sum"):
    """(score float64 [P] holding the float32 sums exactly / the float64 Jaccard quotient, cn, union) of explicit pairs."""
    out, cns, unis = [], [], []
    for s, d in zip(np.asarray(src).tolist(), np.asarray(dst).tolist()):
        rd = set(_row(rowptr, col, d).tolist())
        acc, cn = np.float32(0.0), 0
        for z in _row(rowptr, col, s):
            if int(z) in rd:
                acc = np.float32(acc + np.float32(1.0 if w is None else w[z]))
                cn += 1
        uni = len(_row(rowptr, col, s)) + len(rd) - cn
        cns.append(cn); unis.append(uni)
        out.append((cn / uni if uni > 0 else 0.0) if mode == "jaccard" else float(acc))
    return np.asarray(out, dtype=np.float64), cns, unis


def ranks(rowptr, col, src, dst, w=None, mode="sum", filt=None):
    """(score_true [Q], n_greater [Q], n_equal [Q]) of the ranking query: candidates c in [0, n) except src, dst and filt[src]."""
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    st = pair_scores(rowptr, col, src, dst, w, mode)[0]
    _, tcn, tuni = pair_scores(rowptr, col, src, dst, None, "jaccard")

    def jaccard(q, s, acc):
        cn = acc.astype(np.int64).astype(object)
        uni = (deg + (deg[s] if 0 <= s < n else 0)).astype(object) - cn
        cn, uni = np.where(uni > 0, cn, 0), np.where(uni > 0, uni, 1)                           # an empty union scores 0 / 1
        a, b = (tcn[q], tuni[q]) if tuni[q] > 0 else (0, 1)
        left, right = cn * b, a * uni                                                           # Python integers
        return (left > right).astype(bool), (left == right).astype(bool)

    return P.ranks(n, src, dst, lambda q, s: accumulate(rowptr, col, s, w), lambda q, s, d, row: st[q], filt, jaccard if mode == "jaccard" else None)
