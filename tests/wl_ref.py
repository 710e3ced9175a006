"""CPU reference of the Weisfeiler-Lehman subtree baseline (include/gnnmp.h above gmp_wl_refine; csrc/wl.hip), written from the definition
in numpy uint64 -- colours, sorted lists, histogram, Gram -- plus a second, independent classical WL (sorted tuples of neighbour colours
relabelled jointly across all graphs) and the fixed graph sets that the host and the GPU tests share.

A graph is (n, edges, labels): edges an int array [m, 2] of undirected pairs with local ids, labels an int64 array [n].  A batch is
Batch(ptr int64 [G + 1], rowptr int32 [N + 1], col int32 [nnz], labels int64 [N]) with the CSR symmetric, loop-free and sorted."""
from collections import namedtuple

import numpy as np

K1 = np.uint64(0x9E3779B97F4A7C15)
K2 = np.uint64(0xD1B54A32D192ED03)
M1 = np.uint64(0xBF58476D1CE4E5B9)
M2 = np.uint64(0x94D049BB133111EB)
MAX_GRAPH_NODES = 1024

Batch = namedtuple("Batch", "ptr rowptr col labels")
Refined = namedtuple("Refined", "colors sorted hist status")


def mix(z):
    """The splitmix64 finaliser on a uint64 array (modulo 2^64)."""
    z = np.asarray(z, dtype=np.uint64).copy()
    with np.errstate(over="ignore"):
        z ^= z >> np.uint64(30)
        z *= M1
        z ^= z >> np.uint64(27)
        z *= M2
        z ^= z >> np.uint64(31)
    return z


# ---------------------------------------------------------------------------- batches
def make_batch(graphs):
    """The block-diagonal batch of `graphs`: duplicates, both directions and loops of an edge list collapse into the simple CSR."""
    ptr = np.zeros(len(graphs) + 1, dtype=np.int64)
    for g, (n, _, _) in enumerate(graphs):
        ptr[g + 1] = ptr[g] + n
    N = int(ptr[-1])
    keys = []
    for g, (n, edges, _) in enumerate(graphs):
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        e = e[e[:, 0] != e[:, 1]] + ptr[g]
        keys.append(np.concatenate([e[:, 0] * N + e[:, 1], e[:, 1] * N + e[:, 0]]))
    key = np.unique(np.concatenate(keys)) if keys else np.zeros(0, dtype=np.int64)
    row, col = key // max(N, 1), key % max(N, 1)
    rowptr = np.zeros(N + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=N))
    labels = np.concatenate([np.asarray(l, dtype=np.int64).reshape(-1) for _, _, l in graphs] + [np.zeros(0, dtype=np.int64)])
    assert labels.size == N
    return Batch(ptr, rowptr.astype(np.int32), col.astype(np.int32), labels)


def edge_index_of(batch):
    """The batch's CSR as an int64 [2, nnz] edge list (both directions): what simple_graph() turns back into the same CSR."""
    N = batch.rowptr.size - 1
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(batch.rowptr.astype(np.int64)))
    return np.stack([row, batch.col.astype(np.int64)])


def _graph_of(ptr, v):
    return np.searchsorted(ptr, v, side="right") - 1


def _entries(batch):
    """(row, col, inside) of every CSR entry: inside = the entry's column lies in its row's own graph."""
    ptr, N = batch.ptr, batch.rowptr.size - 1
    row = np.repeat(np.arange(N, dtype=np.int64), np.diff(batch.rowptr.astype(np.int64)))
    col = batch.col.astype(np.int64)
    g = _graph_of(ptr, row)
    inside = (col >= ptr[g]) & (col < ptr[g + 1]) if row.size else np.zeros(0, dtype=bool)
    return row, col, inside


# ---------------------------------------------------------------------------- the definition
def refine(batch, iters, dim, use_labels=True, max_graph_nodes=MAX_GRAPH_NODES, fill=0):
    """gmp_wl_refine: Refined(colors uint64 [iters + 1, N], sorted uint64 [(iters + 1) N], hist int32 [G, dim], status int32 [G]).  The
    parts of a refused graph (status bit 0) hold `fill`."""
    ptr = batch.ptr
    G, N, hp1 = ptr.size - 1, batch.rowptr.size - 1, iters + 1
    row, col, inside = _entries(batch)
    sizes = np.diff(ptr)
    refused = sizes > min(max_graph_nodes, MAX_GRAPH_NODES)
    skipped = np.bincount(_graph_of(ptr, row[~inside]), minlength=G) if row.size else np.zeros(G, dtype=np.int64)
    status = np.where(refused, 1, np.minimum(skipped, 2 ** 23 - 1) << 8).astype(np.int32)
    r, c = row[inside], col[inside]
    label = batch.labels if use_labels else np.bincount(r, minlength=N).astype(np.int64)
    colors = np.zeros((hp1, N), dtype=np.uint64)
    with np.errstate(over="ignore"):
        colors[0] = mix(label.astype(np.uint64) + K1)
        for t in range(iters):
            s = np.zeros(N, dtype=np.uint64)
            np.add.at(s, r, mix(colors[t])[c])
            colors[t + 1] = mix(colors[t] * K1 + s + np.uint64(t + 1) * K2)
    srt = np.full(hp1 * N, fill, dtype=np.int64).view(np.uint64)
    hist = np.full((G, dim), fill, dtype=np.int32)
    for g in range(G):
        if refused[g]:
            colors[:, ptr[g]:ptr[g + 1]] = np.int64(fill).astype(np.uint64)
            continue
        mine = colors[:, ptr[g]:ptr[g + 1]].reshape(-1)
        srt[hp1 * ptr[g]:hp1 * ptr[g + 1]] = np.sort(mine)
        b = ((mine >> np.uint64(32)) * np.uint64(dim)) >> np.uint64(32)
        hist[g] = np.bincount(b.astype(np.int64), minlength=dim)
    return Refined(colors, srt, hist, status)


def segment(srt, ptr, g, iters):
    return srt[(iters + 1) * ptr[g]:(iters + 1) * ptr[g + 1]]


def gram(sorted_a, ptr_a, sorted_b, ptr_b, iters):
    """gmp_wl_gram: K int64 [Ga, Gb], the equal pairs between segment i of sorted_a and segment j of sorted_b."""
    Ga, Gb = ptr_a.size - 1, ptr_b.size - 1
    K = np.zeros((Ga, Gb), dtype=np.int64)
    cb = [np.unique(segment(sorted_b, ptr_b, j, iters), return_counts=True) for j in range(Gb)]
    for i in range(Ga):
        va, na = np.unique(segment(sorted_a, ptr_a, i, iters), return_counts=True)
        for j, (vb, nb) in enumerate(cb):
            _, ia, ib = np.intersect1d(va, vb, assume_unique=True, return_indices=True)
            K[i, j] = int(np.sum(na[ia].astype(np.int64) * nb[ib].astype(np.int64)))
    return K


# ---------------------------------------------------------------------------- classical WL, independent of the hash
def classical(batch, iters, use_labels=True):
    """ids int64 [iters + 1, N]: the textbook relabelling -- a node's next colour is the pair (its colour, the sorted tuple of its
    neighbours' colours), compressed to consecutive integers jointly over every graph of the batch, per iteration."""
    N = batch.rowptr.size - 1
    row, col, inside = _entries(batch)
    nbrs = [[] for _ in range(N)]
    for a, b in zip(row[inside].tolist(), col[inside].tolist()):
        nbrs[a].append(b)
    start = batch.labels.tolist() if use_labels else [len(x) for x in nbrs]
    table = {}
    cur = [table.setdefault(("label", l), len(table)) for l in start]
    ids = [cur]
    for _ in range(iters):
        table = {}
        cur = [table.setdefault((cur[v], tuple(sorted(cur[u] for u in nbrs[v]))), len(table)) for v in range(N)]
        ids.append(cur)
    return np.asarray(ids, dtype=np.int64).reshape(iters + 1, N)


def same_partition(a, b):
    """Whether two labellings of the same items induce the same partition."""
    a, b = np.asarray(a).reshape(-1), np.asarray(b).reshape(-1)
    pairs = set(zip(a.tolist(), b.tolist()))
    return len(pairs) == len(set(a.tolist())) == len(set(b.tolist()))


def classical_gram(ids_a, ptr_a, ids_b, ptr_b):
    """The WL subtree kernel from classical ids made by ONE classical() call over both sets (so equal ids mean equal subtrees): the sum over
    iterations and colours of count_i * count_j."""
    Ga, Gb = ptr_a.size - 1, ptr_b.size - 1
    K = np.zeros((Ga, Gb), dtype=np.int64)
    for t in range(ids_a.shape[0]):
        m = int(max(ids_a[t].max(initial=-1), ids_b[t].max(initial=-1))) + 1
        ca = np.stack([np.bincount(ids_a[t, ptr_a[i]:ptr_a[i + 1]], minlength=m) for i in range(Ga)]) if Ga else np.zeros((0, m), dtype=np.int64)
        cb = np.stack([np.bincount(ids_b[t, ptr_b[j]:ptr_b[j + 1]], minlength=m) for j in range(Gb)]) if Gb else np.zeros((0, m), dtype=np.int64)
        K += ca.astype(np.int64) @ cb.astype(np.int64).T
    return K


# ---------------------------------------------------------------------------- graphs
def permuted(graphs, seed):
    """Every graph with its node ids renamed by a random permutation (and its edge list shuffled)."""
    rng = np.random.RandomState(seed)
    out = []
    for n, edges, labels in graphs:
        perm = rng.permutation(n)
        e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
        e = perm[e][rng.permutation(e.shape[0])] if e.size else e
        lab = np.zeros(n, dtype=np.int64)
        lab[perm] = np.asarray(labels, dtype=np.int64)
        out.append((n, e, lab))
    return out


def _cycle(n, off=0):
    return [(off + i, off + (i + 1) % n) for i in range(n)]


def _random_graph(rng, n, p, num_labels):
    iu = np.triu_indices(n, 1)
    keep = rng.random_sample(iu[0].size) < p
    return n, np.stack([iu[0][keep], iu[1][keep]], axis=1), rng.randint(0, num_labels, size=n)


INDEX = {name: i for i, name in enumerate(["empty", "single", "two_isolated", "edge", "star65", "path64", "c6", "c3c3", "k40", "cycle1024",
                                            "random257", "random256"])}
NUM_NAMED = len(INDEX)


def fixed_graphs():
    """The fixed set of the WL tests, one batch: the named graphs of INDEX, then 20 random graphs of 1 to 39 nodes with 3 labels."""
    rng = np.random.RandomState(20111)
    z = lambda n: np.zeros(n, dtype=np.int64)
    graphs = [
        (0, [], z(0)),
        (1, [], z(1)),
        (2, [], z(2)),
        (2, [(0, 1)], np.array([0, 1])),
        (65, [(0, i) for i in range(1, 65)], np.arange(65) % 3),
        (64, [(i, i + 1) for i in range(63)], np.arange(64) % 2),
        (6, _cycle(6), z(6)),
        (6, _cycle(3) + _cycle(3, 3), z(6)),
        (40, [(i, j) for i in range(40) for j in range(i + 1, 40)], z(40)),
        (1024, _cycle(1024), z(1024)),
        _random_graph(rng, 257, 0.03, 3),
        _random_graph(rng, 256, 0.03, 3),
    ]
    for _ in range(20):
        graphs.append(_random_graph(rng, int(rng.randint(1, 40)), 0.15, 3))
    return graphs


WIDE_LABELS = np.array([-2 ** 63, -1, 2 ** 63 - 1], dtype=np.int64)     # an injective image of the labels 0, 1, 2


def with_wide_labels(graphs):
    """The same graphs with the labels 0, 1, 2 sent to negative values and values next to 2^63."""
    return [(n, e, WIDE_LABELS[np.asarray(l, dtype=np.int64)]) for n, e, l in graphs]


BASELINE_TRAIN, BASELINE_EVAL, BASELINE_K, BASELINE_ITERS = 40, 20, 20, 3


def baseline_graphs():
    """60 unlabelled graphs in two classes that differ in structure, (graphs, y): class 0 a cycle, class 1 a star, each with a few noise
    edges; the first BASELINE_TRAIN are the train split, the rest the evaluation split."""
    rng = np.random.RandomState(7)
    graphs, y = [], []
    for i in range(BASELINE_TRAIN + BASELINE_EVAL):
        cls = i % 2
        n = 8 + (i // 2) % 23 + (3 if i >= BASELINE_TRAIN else 0)
        edges = _cycle(n) if cls == 0 else [(0, j) for j in range(1, n)]
        for _ in range(1 + int(rng.randint(0, 3))):
            a, b = rng.randint(0, n, size=2)
            if a != b:
                edges.append((int(a), int(b)))
        graphs.append((n, edges, np.zeros(n, dtype=np.int64)))
        y.append(cls)
    return graphs, np.asarray(y, dtype=np.int64)


def normalised_similarity(K_et, K_ee, K_tt):
    """s = K[eval, train] / sqrt(K_ee K_tt) in float64, 0 where a self-similarity is 0 (K_ee, K_tt: the two diagonals)."""
    den = np.sqrt(K_ee.astype(np.float64)[:, None] * K_tt.astype(np.float64)[None, :])
    return np.where(den > 0, K_et.astype(np.float64) / np.where(den > 0, den, 1.0), 0.0)


def top_k(sim, k):
    """The k most similar train indices per row, ties to the lower index."""
    return np.argsort(-sim, axis=1, kind="stable")[:, :k]
