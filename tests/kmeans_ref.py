"""Shared by test_kmeans_host.py and test_gpu_kmeans.py: the float64 definition of the clustering probe of csrc/kmeans.hip (gnnmp.h
gmp_kmeans_assign / gmp_kmeans_fit / gmp_contingency, metrics.clustering_scores), written from the contract and not from the kernels.

  normalize    knn_ref's: z / max(||z||, 1e-12) per row (a zero row stays zero)
  assign       per row the centroid of greatest cosine similarity, ties to the lower index (numpy's argmax returns the first maximum);
               `similarity=` replays the selection on someone else's scores (the kernel's own matrix)
  update       centroid j = normalize(sum of xn[i] over labels[i] == j); a cluster without rows keeps c_prev[j]
  fit          c = normalize(init); per iteration: assign, changed = n on the first pass and the number of labels that moved afterwards,
               stop when changed == 0, otherwise update.  Returns (centroids, labels, sim, info), info = [iterations run, changed of the
               last pass, clusters the last update found empty, 0]
  contingency  table[a[i], b[i]] += 1 in int64
  scores       nmi (arithmetic normalisation), ari, purity, accuracy from the table [clusters, classes], by the textbook formulas in
               float64 / Python integers; accuracy by brute force over the one-to-one matchings (small tables only: beyond 8 groups on
               the smaller side it is left out)"""
import itertools
import math

import numpy as np

from knn_ref import cosine, normalize  # noqa: F401  (re-exported)


def assign(x, c, similarity=None):
    """(labels [n] int64, sim [n] in the dtype of the scores)"""
    S = cosine(x, c) if similarity is None else np.asarray(similarity)
    labels = np.argmax(S, axis=1).astype(np.int64)
    return labels, S[np.arange(S.shape[0]), labels]


def update(xn, labels, c_prev):
    xn, c = np.asarray(xn, dtype=np.float64), np.array(c_prev, dtype=np.float64)
    for j in range(c.shape[0]):
        rows = xn[np.asarray(labels) == j]
        if rows.shape[0]:
            c[j] = normalize(rows.sum(axis=0, keepdims=True))[0]
    return c


def fit(x, init, max_iter):
    xn, c = normalize(x), normalize(init)
    n, kc = xn.shape[0], c.shape[0]
    labels, sim, info = np.zeros(n, dtype=np.int64), np.zeros(n), [0, 0, 0, 0]
    for it in range(1, max_iter + 1):
        new, sim = assign(xn, c)
        changed = n if it == 1 else int((new != labels).sum())
        labels = new
        info[0], info[1] = it, changed
        if changed == 0:
            break
        c = update(xn, labels, c)
        info[2] = kc - np.unique(labels).size
    return c, labels, sim, info


def contingency(a, b, na, nb):
    table = np.zeros((na, nb), dtype=np.int64)
    np.add.at(table, (np.asarray(a), np.asarray(b)), 1)
    return table


def _entropy(counts, n):
    return -sum(int(v) / n * math.log(int(v) / n) for v in counts if v > 0)


def scores(table):
    t = np.asarray(table, dtype=np.int64)
    n = int(t.sum())
    nk, nc = t.sum(axis=1), t.sum(axis=0)
    groups_k, groups_c = int((nk > 0).sum()), int((nc > 0).sum())
    mi = sum(int(t[k, c]) / n * math.log(n * int(t[k, c]) / (int(nk[k]) * int(nc[c]))) for k, c in zip(*np.nonzero(t)))
    if groups_k == 1 and groups_c == 1:
        nmi = 1.0
    elif groups_k == 1 or groups_c == 1 or mi <= 0.0:
        nmi = 0.0
    else:
        nmi = mi / ((_entropy(nk, n) + _entropy(nc, n)) / 2.0)

    def pairs(v):
        return int(v) * (int(v) - 1) // 2

    same_both = sum(pairs(v) for v in t.ravel())                    # pairs together in the clustering and in the classes
    same_k, same_c, total = sum(pairs(v) for v in nk), sum(pairs(v) for v in nc), pairs(n)
    tp, fp, fn = same_both, same_k - same_both, same_c - same_both
    tn = total - tp - fp - fn
    ari = 1.0 if fp == 0 and fn == 0 else 2.0 * (tp * tn - fn * fp) / ((tp + fn) * (fn + tn) + (tp + fp) * (fp + tn))
    out = {"nmi": nmi, "ari": ari, "purity": int(t.max(axis=1).sum()) / n}
    small = t if t.shape[0] <= t.shape[1] else t.T
    if small.shape[0] <= 6 and small.shape[1] <= 8:
        best = max(sum(int(small[i, p[i]]) for i in range(small.shape[0])) for p in itertools.permutations(range(small.shape[1]), small.shape[0]))
        out["accuracy"] = best / n
    return out
