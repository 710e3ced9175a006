"""The counting protocol of every all-candidate link ranker (gmp_lp_rank, gmp_lp_cn_rank, gmp_lp_walk_rank, gmp_emb_link_rank), once, numpy
only: the true pair (s, d) of a query is compared with the candidates c in [0, n) other than s, d and the destinations of s's filter
row; n_greater and n_equal count them, rank = 1 + n_greater + n_equal / 2.  What a score is belongs to each family's reference
(lp_heur_ref, lp_walk_ref, link_probe_ref), which hands in one score row per query."""
import numpy as np


def filter_rows(filter_edges, n):
    """{source: destinations} of known edges [2, E]; entries outside [0, n) are dropped."""
    rows = {}
    if filter_edges is not None:
        for s, d in np.asarray(filter_edges, dtype=np.int64).reshape(2, -1).T.tolist():
            if 0 <= s < n and 0 <= d < n:
                rows.setdefault(s, []).append(d)
    return rows


def candidates(n, s, d, filt=None):
    """bool [n]: the candidates of the true pair (s, d) under the filter rows filt ({source: destinations}, any order, duplicates and
    entries outside [0, n) allowed)."""
    valid = np.ones(n, dtype=bool)
    for c in [s, d] + list((filt or {}).get(s, [])):
        if 0 <= c < n:
            valid[c] = False
    return valid


def ranks(n, src, dst, score_row, true_score, filt=None, compare=None):
    """(score_true [Q], n_greater [Q] int64, n_equal [Q] int64).  score_row(q, s) -> the scores [n] of source s against every node;
    true_score(q, s, d, row) -> the true pair's; compare(q, s, row) -> (greater, equal) bool [n] where > and == on the scores are not
    the family's order (Jaccard)."""
    st, ng, ne = [], [], []
    for q, (s, d) in enumerate(zip(np.asarray(src).reshape(-1).tolist(), np.asarray(dst).reshape(-1).tolist())):
        row = score_row(q, s)
        true = true_score(q, s, d, row)
        greater, equal = compare(q, s, row) if compare else (row > true, row == true)
        valid = candidates(n, s, d, filt)
        st.append(true); ng.append(int((greater & valid).sum())); ne.append(int((equal & valid).sum()))
    return np.asarray(st), np.asarray(ng, dtype=np.int64), np.asarray(ne, dtype=np.int64)


def rank_of(n_greater, n_equal):
    return 1.0 + np.asarray(n_greater, dtype=np.float64) + 0.5 * np.asarray(n_equal, dtype=np.float64)
