"""CPU reference of the shortest-path kernel baseline (include/gnnmp.h above gmp_sp_features; csrc/sp.hip), written from the definition in
numpy and plain Python -- a BFS per source, a dict of key counts, sorted keys, the hashed histogram, the status word, the Gram -- plus a
second, independent route to the distances (Floyd-Warshall on the dense matrix).  The graph sets are those of wl_ref.

A batch is wl_ref.Batch(ptr int64 [G + 1], rowptr int32 [N + 1], col int32 [nnz], labels int64 [N])."""
from collections import namedtuple

import numpy as np

import wl_ref as W
from wl_ref import INDEX, baseline_graphs, fixed_graphs, make_batch, permuted, with_wide_labels  # noqa: F401  (the shared graph sets)

MAX_GRAPH_NODES, MAX_DIST, MAX_DIM, MAX_LABEL = 1024, 1023, 256, 2 ** 24
SMALL_NODES, SMALL_CAP, LARGE_CAP = 256, 4096, 1024

Features = namedtuple("Features", "keys counts nuniq hist status")


def max_unique(max_graph_nodes):
    """gmp_sp_max_unique"""
    return LARGE_CAP if max_graph_nodes > SMALL_NODES else SMALL_CAP


def pack(la, lb, d):
    lo, hi = (la, lb) if la <= lb else (lb, la)
    return (int(lo) << 35) | (int(hi) << 11) | int(d)


def unpack(key):
    key = int(key)
    return key >> 35, (key >> 11) & (2 ** 24 - 1), key & 2047


def bin_of(key, dim):
    """The histogram bin of a key: (uint32(mix(key + K1) >> 32) * dim) >> 32."""
    with np.errstate(over="ignore"):
        z = W.mix(np.array([key], dtype=np.uint64) + W.K1)[0]
    return ((int(z) >> 32) * dim) >> 32


def _graph_parts(batch, g):
    """(n, neighbour sets of graph g with local ids -- symmetric closure, no loops --, entries of its rows inside it, entries skipped)."""
    p0, p1 = int(batch.ptr[g]), int(batch.ptr[g + 1])
    n = p1 - p0
    nbrs, inside, skipped = [set() for _ in range(n)], [0] * n, 0
    for v in range(n):
        for i in range(int(batch.rowptr[p0 + v]), int(batch.rowptr[p0 + v + 1])):
            u = int(batch.col[i]) - p0
            if not 0 <= u < n:
                skipped += 1
                continue
            inside[v] += 1
            if u != v:
                nbrs[v].add(u)
                nbrs[u].add(v)
    return n, nbrs, inside, skipped


def bfs_distances(n, nbrs):
    """D int32 [n, n]: the hop distance of every ordered pair by one BFS per source, 0 on the diagonal and for unreachable pairs."""
    D = np.zeros((n, n), dtype=np.int32)
    for s in range(n):
        seen, frontier, d, found = {s}, [s], 0, []
        while frontier:
            d += 1
            nxt = []
            for a in frontier:
                for b in nbrs[a]:
                    if b not in seen:
                        seen.add(b)
                        nxt.append(b)
            found.append(nxt)
            frontier = nxt
        for d, level in enumerate(found, 1):
            D[s, level] = d
    return D


def floyd_warshall_distances(n, nbrs):
    """The same matrix by Floyd-Warshall on the dense n x n matrix (vectorised over rows and columns)."""
    inf = np.iinfo(np.int64).max // 4
    D = np.full((n, n), inf, dtype=np.int64)
    np.fill_diagonal(D, 0)
    for v in range(n):
        for u in nbrs[v]:
            D[v, u] = 1
    for k in range(n):
        np.minimum(D, D[:, k:k + 1] + D[k:k + 1, :], out=D)
    D[D >= inf] = 0
    return D.astype(np.int32)


def batch_distances(batch, route=bfs_distances):
    """The distance matrix of every graph of the batch (None for a graph above MAX_GRAPH_NODES): computed once, shared by every call of
    features() on that batch."""
    out = []
    for g in range(batch.ptr.size - 1):
        n, nbrs, _, _ = _graph_parts(batch, g)
        out.append(route(n, nbrs) if n <= MAX_GRAPH_NODES else None)
    return out


def key_counts(D, label, max_dist):
    """{key: pairs} of one graph from its distance matrix and its labels: the unordered pairs u < v with 1 <= D[u, v] <= max_dist."""
    iu, iv = np.triu_indices(D.shape[0], 1)
    d = D[iu, iv].astype(np.int64)
    keep = (d >= 1) & (d <= max_dist)
    lab = np.asarray(label, dtype=np.int64)
    la, lb, d = lab[iu[keep]], lab[iv[keep]], d[keep]
    keys, counts = np.unique((np.minimum(la, lb) << 35) | (np.maximum(la, lb) << 11) | d, return_counts=True)
    return dict(zip(keys.tolist(), counts.tolist()))


def features(batch, max_dist, dim, use_labels=True, max_graph_nodes=MAX_GRAPH_NODES, cap=None, fill=0, dist=None):
    """gmp_sp_features: Features(keys int64 [G, cap], counts int32 [G, cap], nuniq int32 [G], hist int32 [G, dim], status int32 [G]).  What
    the kernel leaves alone holds `fill`.  dist: batch_distances(batch) when the caller has it."""
    G = batch.ptr.size - 1
    cap = max_unique(max_graph_nodes) if cap is None else cap
    keys = np.full((G, cap), fill, dtype=np.int64)
    counts = np.full((G, cap), fill, dtype=np.int32)
    hist = np.full((G, dim), fill, dtype=np.int32)
    nuniq, status = np.zeros(G, dtype=np.int32), np.zeros(G, dtype=np.int32)
    N = batch.rowptr.size - 1
    for g in range(G):
        p0, p1 = int(batch.ptr[g]), int(batch.ptr[g + 1])
        if p1 - p0 < 0 or p1 - p0 > min(max_graph_nodes, MAX_GRAPH_NODES) or p0 < 0 or p1 > N:
            status[g] = 1
            continue
        n, nbrs, inside, skipped = _graph_parts(batch, g)
        word = min(skipped, 2 ** 23 - 1) << 8
        label = [int(l) for l in batch.labels[p0:p1]] if use_labels else inside
        if any(not 0 <= l < MAX_LABEL for l in label):
            status[g] = word | 4
            continue
        D = dist[g] if dist is not None and dist[g] is not None else bfs_distances(n, nbrs)
        table = key_counts(D, label, max_dist)
        if len(table) > cap:
            status[g] = word | 2
            continue
        status[g] = word
        order = sorted(table)
        nuniq[g] = len(order)
        keys[g, :len(order)] = order
        counts[g, :len(order)] = [table[k] for k in order]
        hist[g] = 0
        for k in order:
            hist[g, bin_of(k, dim)] += table[k]
    return Features(keys, counts, nuniq, hist, status)


def row(feat, g):
    """{key: count} of graph g."""
    m = int(feat.nuniq[g])
    return dict(zip(feat.keys[g, :m].tolist(), feat.counts[g, :m].tolist()))


def gram(a, b):
    """gmp_sp_gram: K int64 [Ga, Gb], the sum over shared keys of count_a * count_b."""
    rows_b = [row(b, j) for j in range(b.nuniq.size)]
    K = np.zeros((a.nuniq.size, b.nuniq.size), dtype=np.int64)
    for i in range(a.nuniq.size):
        ra = row(a, i)
        for j, rb in enumerate(rows_b):
            K[i, j] = sum(c * rb[k] for k, c in ra.items() if k in rb)
    return K


def self_similarity(feat):
    return np.array([sum(c * c for c in row(feat, g).values()) for g in range(feat.nuniq.size)], dtype=np.int64)


def distinct_label_path(n):
    """The path on n nodes with the labels 0 .. n - 1: every pair has a key of its own, n (n - 1) / 2 in all."""
    return n, [(i, i + 1) for i in range(n - 1)], np.arange(n, dtype=np.int64)


normalised_similarity, top_k = W.normalised_similarity, W.top_k
