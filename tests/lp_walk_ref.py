"""CPU reference of the walk-based link baselines (include/gnnmp.h above gmp_lp_walk_score), numpy only, restating the definition
literally: y_0 = e_s, y_l[v] = a * (the float32 fold of w[z] * y_{l-1}[z] over z in N(v) ascending), acc += y_l; hops from an integer BFS;
counts from a validity mask.  Every numpy operation on float32 arrays rounds once (a rounded multiply and a rounded add, never a fused
one) and x86 keeps subnormals.  Vectorised over the rows (and the sources) with a loop over the neighbour POSITION, as labelprop_ref.py:
row v's p-th entry is its p-th add.  The graph, the 1 / deg weights, the filter rows and the half-tie rank are lp_heur_ref's."""
import numpy as np

import link_rank_ref as P

from lp_heur_ref import filter_rows, rank_of, simple_csr, weights  # noqa: F401  (re-exported for the tests)

KINDS = ("katz", "ppr", "hops")
KATZ_BETA, PPR_ALPHA = 0.05, 0.15
FAR = 2 ** 62                                                       # no path


def params(rowptr, kind):
    """(w float32 [n] or None, damping float32, mode) of a kind: constants in float64, rounded once."""
    if kind == "katz":
        return None, np.float32(KATZ_BETA), "sum"
    if kind == "ppr":
        return weights(rowptr, "ra"), np.float32(1.0 - PPR_ALPHA), "sum"
    if kind == "hops":
        return None, np.float32(1.0), "hops"
    raise ValueError(kind)


def _steps(rowptr, col):
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    inside = (col >= 0) & (col < n)
    steps = []                                                      # per neighbour position: the rows that have one inside the graph, and it
    for p in range(int(deg.max()) if n else 0):
        rows = np.nonzero(deg > p)[0]
        k = rowptr[rows] + p
        steps.append((rows[inside[k]], col[k][inside[k]]))
    return steps


def walk_acc(rowptr, col, sources, rounds, damping, w=None):
    """acc float32 [len(sources), n]; a source outside [0, n) has an all-zero row."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n, sources = len(rowptr) - 1, np.asarray(sources, dtype=np.int64).reshape(-1)
    a = np.float32(damping)
    w = None if w is None else np.asarray(w, dtype=np.float32)
    y = np.zeros((n, len(sources)), dtype=np.float32)               # a column per source
    ok = (sources >= 0) & (sources < n)
    y[sources[ok], np.nonzero(ok)[0]] = 1.0
    acc = np.zeros_like(y)
    steps = _steps(rowptr, col)
    for _ in range(rounds):
        t = np.zeros_like(y)
        for rows, z in steps:
            t[rows] = t[rows] + (y[z] if w is None else w[z][:, None] * y[z])
        y = a * t
        acc = acc + y
    return np.ascontiguousarray(acc.T)


def hop_dist(rowptr, col, s, limit=None):
    """int64 [n]: the BFS distance from s, FAR where there is no path or s lies outside the graph (or, with a limit, where the path is
    longer than that)."""
    n = len(rowptr) - 1
    dist = np.full(n, FAR, dtype=np.int64)
    if not 0 <= s < n:
        return dist
    dist[s], frontier, d = 0, [int(s)], 0
    while frontier and (limit is None or d < limit):
        d += 1
        nxt = []
        for v in frontier:
            for z in col[rowptr[v]:rowptr[v + 1]].tolist():
                if 0 <= z < n and dist[z] == FAR:
                    dist[z] = d
                    nxt.append(z)
        frontier = nxt
    return dist


def cut_dist(dist, rounds):
    """The distance as the scorer sees it: dist where dist <= rounds, else rounds + 1."""
    return np.where(dist <= rounds, dist, rounds + 1)


def hop_scores(dist, rounds):
    """float32: -dist where dist <= rounds, else -(rounds + 1)."""
    return -cut_dist(dist, rounds).astype(np.float32)


def all_scores(rowptr, col, sources, rounds, damping=1.0, w=None, mode="sum"):
    """float32 [len(sources), n]: the score of every node as a destination of every source."""
    if mode == "hops":
        assert w is None
        sources = np.asarray(sources, dtype=np.int64).reshape(-1)
        out = np.zeros((len(sources), len(rowptr) - 1), dtype=np.float32)
        for i, s in enumerate(sources.tolist()):
            out[i] = hop_scores(hop_dist(rowptr, col, s, limit=rounds), rounds)
        return out
    return walk_acc(rowptr, col, sources, rounds, damping, w)


def _none(rounds, mode):
    return np.float32(-(rounds + 1)) if mode == "hops" else np.float32(0.0)


def pair_scores(rowptr, col, src, dst, rounds, damping=1.0, w=None, mode="sum"):
    """float32 [P]; a destination outside the graph scores 0 / -(rounds + 1)."""
    n = len(rowptr) - 1
    src, dst = np.asarray(src, dtype=np.int64).reshape(-1), np.asarray(dst, dtype=np.int64).reshape(-1)
    uniq, inv = np.unique(src, return_inverse=True)
    every = all_scores(rowptr, col, uniq, rounds, damping, w, mode)
    out = np.full(len(src), _none(rounds, mode), dtype=np.float32)
    ok = (dst >= 0) & (dst < n)
    out[ok] = every[inv[ok], dst[ok]]
    return out


def ranks(rowptr, col, src, dst, rounds, damping=1.0, w=None, mode="sum", filt=None):
    """(score_true float32 [Q], n_greater int64 [Q], n_equal int64 [Q]): candidates c in [0, n) except src, dst and filt[src]."""
    src = np.asarray(src, dtype=np.int64).reshape(-1)
    uniq, inv = np.unique(src, return_inverse=True)
    every = all_scores(rowptr, col, uniq, rounds, damping, w, mode)
    st = pair_scores(rowptr, col, src, dst, rounds, damping, w, mode)
    return P.ranks(len(rowptr) - 1, src, dst, lambda q, s: every[inv[q]], lambda q, s, d, row: st[q], filt)
