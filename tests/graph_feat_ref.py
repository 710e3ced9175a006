"""The CPU definition of gmp_graph_feature_map (include/gnnmp.h), operation for operation in numpy fp32, the float64 twin of
graph_baselines.standardise / feature_baseline, and the fixtures of test_graph_feat_host.py / test_gpu_graph_feat.py.

feature_map() works in fp32: every numpy operation on float32 arrays rounds once, so a multiply and an add are never fused, and x86 keeps
subnormals.  The propagation is sgc_ref's round over labelprop_ref's position-ordered loop -- row i's p-th entry is added as its p-th add
-- with the entries restricted to the row's own graph.  The sum pool is a Python loop over the row POSITION inside a graph, one fp32 add
per row in ascending order (vectorised over the graphs and the columns, never over the rows); the mean is one fp32 division; the max
goes through labelprop_ref.orderable, the integer order the kernel compares in."""
import functools
from typing import NamedTuple

import numpy as np

import labelprop_ref as LP
import sgc_ref as SG

MAX_ROUNDS, MAX_DIM, MAX_GRAPH_NODES, SKIP_MAX = 16, 256, 1024, 2 ** 23 - 1
POOLS = ("sum", "mean", "max")


class Batch(NamedTuple):
    ptr: np.ndarray                # int64 [G + 1]
    rowptr: np.ndarray             # int32 [N + 1]
    col: np.ndarray                # int32 [nnz], batch-wide node ids
    scale: np.ndarray              # fp32 [N]: 1 / sqrt(row length + 1) from float64, rounded once


class Result(NamedTuple):
    out: np.ndarray                # fp32 [G, rounds + 1, 3, d]
    status: np.ndarray             # int32 [G]


def from_orderable(u: np.ndarray) -> np.ndarray:
    u = np.asarray(u, np.uint32)
    return np.where(u & np.uint32(0x80000000), u & np.uint32(0x7FFFFFFF), ~u).astype(np.uint32).view(np.float32)


def _graph_of(ptr, v):
    return np.searchsorted(ptr, v, side="right") - 1


def window_steps(ptr, rowptr, col):
    """labelprop_ref.steps with the window: per neighbour position p the rows whose p-th entry lies inside the row's own graph, and that
    entry; and the number of entries that do not, per graph."""
    ptr, rowptr, col = np.asarray(ptr, np.int64), np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    N, G = rowptr.size - 1, ptr.size - 1
    deg = rowptr[1:] - rowptr[:-1]
    row = np.repeat(np.arange(N, dtype=np.int64), deg)
    g = _graph_of(ptr, row)
    inside = (col >= ptr[g]) & (col < ptr[g + 1]) if row.size else np.zeros(0, bool)
    out = []
    for p in range(int(deg.max()) if N else 0):
        rows = np.nonzero(deg > p)[0]
        k = rowptr[rows] + p
        out.append((rows[inside[k]], col[k][inside[k]]))
    skipped = np.bincount(g[~inside], minlength=G) if row.size else np.zeros(G, np.int64)
    return out, skipped


def pools(H, ptr, refused) -> np.ndarray:
    """fp32 [G, 3, d]: the three pools of H's rows per graph; +0 for an empty or a refused graph."""
    ptr = np.asarray(ptr, np.int64)
    G, d = ptr.size - 1, H.shape[1]
    sizes = np.where(refused, 0, np.diff(ptr))
    out = np.zeros((G, 3, d), np.float32)
    s = np.zeros((G, d), np.float32)
    for i in range(int(sizes.max()) if G else 0):                   # the i-th row of every graph that has one: its i-th add
        gs = np.nonzero(sizes > i)[0]
        s[gs] = s[gs] + H[ptr[gs] + i]
    out[:, 0] = s
    keys = LP.orderable(H).reshape(H.shape)
    for g in np.nonzero(sizes > 0)[0]:
        out[g, 1] = s[g] / np.float32(sizes[g])
        out[g, 2] = from_orderable(keys[ptr[g]:ptr[g + 1]].max(axis=0))
    return out


def feature_map(ptr, rowptr, col, x, rounds, left=None, right=None, max_graph_nodes=MAX_GRAPH_NODES) -> Result:
    ptr = np.asarray(ptr, np.int64)
    H = np.asarray(x, dtype=np.float32).copy()
    N, G = H.shape[0], ptr.size - 1
    left, right = SG._scales(N, left, right)
    refused = np.diff(ptr) > min(max_graph_nodes, MAX_GRAPH_NODES)
    steps, skipped = window_steps(ptr, rowptr, col)
    out = np.zeros((G, rounds + 1, 3, H.shape[1]), np.float32)
    with np.errstate(under="ignore"):
        for t in range(rounds + 1):
            out[:, t] = pools(H, ptr, refused)
            if t < rounds:
                H = SG._round(steps, H, left, right)
    counted = skipped if rounds else np.zeros(G, np.int64)          # rounds == 0 reads no adjacency entry
    return Result(out, np.where(refused, 1, np.minimum(counted, SKIP_MAX) << 8).astype(np.int32))


def levels(rowptr, col, x, rounds, left, right):
    """[H(0), .. H(rounds)] of the whole batch by sgc_ref.propagate's round: what gmp_feature_propagate leaves after t rounds."""
    H = np.asarray(x, np.float32).copy()
    left, right = SG._scales(H.shape[0], left, right)
    steps, _ = LP.steps(rowptr, col, H.shape[0])
    out = [H]
    for _ in range(rounds):
        H = SG._round(steps, H, left, right)
        out.append(H)
    return out


# ---------------------------------------------------------------------------- batches
SMALL_SIZES = (0, 1, 2, 3, 63, 64, 65, 255, 256)
LARGE_SIZES = SMALL_SIZES + (257, 1023, 1024)


def make_batch(sizes, seed: int, max_degree: int = 20) -> Batch:
    """A raw CSR written row by row (not symmetric): row v of a graph of n nodes holds a random number 0 .. min(n, max_degree) of distinct
    nodes of its own graph, ascending, itself allowed -- a random degree ladder, so every remainder of the row fold's batches of 8 occurs
    around one and two full batches."""
    rng = np.random.default_rng(seed)
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    rows = []
    for g, n in enumerate(sizes):
        for _ in range(n):
            deg = int(rng.integers(0, min(n, max_degree) + 1))
            rows.append(np.sort(rng.choice(n, size=deg, replace=False)) + ptr[g])
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int32)
    col = (np.concatenate(rows) if rows else np.zeros(0)).astype(np.int32)
    scale = (1.0 / np.sqrt(np.diff(rowptr).astype(np.float64) + 1.0)).astype(np.float32)
    return Batch(ptr, rowptr, col, scale)


def features(n: int, d: int, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)


def with_strays(b: Batch, g: int, other: int):
    """b with five entries of graph g's rows redirected: two into graph `other`, one each to -1, N and -2^31.  Graph g needs five rows
    with an entry.  Returns (batch, 5)."""
    col = b.col.copy()
    N = int(b.ptr[-1])
    rows = [v for v in range(int(b.ptr[g]), int(b.ptr[g + 1])) if b.rowptr[v + 1] > b.rowptr[v]][:5]
    assert len(rows) == 5 and b.ptr[other + 1] > b.ptr[other]
    targets = [int(b.ptr[other]), int(b.ptr[other + 1]) - 1, -1, N, -2 ** 31]
    for k, (v, tgt) in enumerate(zip(rows, targets)):
        at = int(b.rowptr[v]) + (k % int(b.rowptr[v + 1] - b.rowptr[v]))      # not always the row's first entry
        col[at] = tgt
    return b._replace(col=col), 5


# ---------------------------------------------------------------------------- the float64 twin of standardise, the fit and the vote
def standardise(train, other):
    """Per column: minus the train rows' mean, over their population deviation, in float64, rounded once to fp32; a column whose
    deviation is 0 becomes zeros."""
    t, o = np.asarray(train, np.float64), np.asarray(other, np.float64)
    mean = t.mean(axis=0, keepdims=True)
    std = np.sqrt(((t - mean) ** 2).mean(axis=0, keepdims=True))
    ok = std > 0
    safe = np.where(ok, std, 1.0)
    return (np.where(ok, (t - mean) / safe, 0.0).astype(np.float32), np.where(ok, (o - mean) / safe, 0.0).astype(np.float32))


def knn_predict(z_eval, z_train, y_train, classes: int, k: int, temperature: float = 0.07) -> np.ndarray:
    """The protocol of graph_baselines._kernel_baseline in float64: the cosine of the rows (0 where a norm is 0), the k nearest by a stable
    descending sort, the vote exp(s / T) per class, ties to the lower class."""
    ze, zt = np.asarray(z_eval, np.float64), np.asarray(z_train, np.float64)
    den = np.sqrt((ze * ze).sum(axis=1)[:, None] * (zt * zt).sum(axis=1)[None, :])
    sim = np.where(den > 0, (ze @ zt.T) / np.where(den > 0, den, 1.0), 0.0)
    idx = np.argsort(-sim, axis=1, kind="stable")[:, :min(k, zt.shape[0])]
    w = np.exp(np.take_along_axis(sim, idx, axis=1) / temperature)
    score = np.stack([(w * (np.asarray(y_train)[idx] == c)).sum(axis=1) for c in range(classes)], axis=1)
    return score.argmax(axis=1)


# ---------------------------------------------------------------------------- the separable fixture
CYCLES = (6, 8, 10, 12)
N_TRAIN, N_EVAL, FIXTURE_ROUNDS, FIXTURE_K, FIXTURE_CLASSES = 40, 20, 2, 20, 2


def fixture_graphs():
    """[(n, edges [n, 2], x fp32 [n, 2], class)] x 60: cycles of 6, 8, 10 and 12 nodes with features (v, -v), v = +1 on half of the nodes
    and -1 on the others.  Class 0 places the +1s contiguously, class 1 alternates them; the classes alternate in dataset order.  Every
    graph has the same raw pools -- sum 0, mean 0, max 1 in both columns -- so nothing that ignores the graph can tell the classes apart;
    one propagation over the cycle leaves 1 under the max pool where three +1s meet and 1 / 3 where they alternate."""
    out = []
    for i in range(N_TRAIN + N_EVAL):
        cls, n = i % 2, CYCLES[(i // 2) % len(CYCLES)]
        v = np.where(np.arange(n) < n // 2, 1.0, -1.0) if cls == 0 else np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        x = np.stack([v, -v], axis=1).astype(np.float32)
        edges = np.stack([np.arange(n), (np.arange(n) + 1) % n], axis=1).astype(np.int64)
        out.append((n, edges, x, cls))
    return out


def pooled(graphs, rounds: int) -> np.ndarray:
    """graph_baselines.pooled_features by the fp32 definition: [G, (rounds + 1) * 3 * d] over sgc_ref.sgc_graph of the collated graphs."""
    ptr = np.concatenate([[0], np.cumsum([n for n, _, _, _ in graphs])]).astype(np.int64)
    edges = np.concatenate([e + ptr[g] for g, (_, e, _, _) in enumerate(graphs)])
    rowptr, col, scale = SG.sgc_graph(LP.simple_csr(int(ptr[-1]), edges))
    res = feature_map(ptr, rowptr, col, np.concatenate([x for _, _, x, _ in graphs]), rounds, scale, scale)
    assert not res.status.any()
    return res.out.reshape(len(graphs), -1)


class Baseline(NamedTuple):
    z_train: np.ndarray            # fp32: the standardised features
    z_eval: np.ndarray
    logits: np.ndarray             # float64 [eval, classes]
    logreg_accuracy: float
    knn_accuracy: float
    margin: float                  # the smallest gap between the two largest logits of an evaluation row
    live_columns: int              # the columns that are not constant over the train split


@functools.lru_cache(maxsize=None)
def reference_baseline(kind: str, rounds: int = FIXTURE_ROUNDS, k: int = FIXTURE_K) -> Baseline:
    """feature_baseline on the fixture: the features by the fp32 definition (what the kernel leaves, bit for bit), standardise, the
    regression (sgc_ref.fit) and the vote in float64.  kind "rawpool" = the t = 0 slice, "sgcpool" = every slice.  Computed once and
    shared; callers must not write into it."""
    graphs = fixture_graphs()
    y = np.array([c for _, _, _, c in graphs], np.int64)
    pt, pe = pooled(graphs[:N_TRAIN], rounds), pooled(graphs[N_TRAIN:], rounds)
    width = pt.shape[1] // (rounds + 1) if kind == "rawpool" else pt.shape[1]
    zt, ze = standardise(pt[:, :width], pe[:, :width])
    W, b, _ = SG.fit(np.float64, zt, y[:N_TRAIN], FIXTURE_CLASSES)
    logits = ze.astype(np.float64) @ W.T + b
    top = np.sort(logits, axis=1)
    acc = lambda pred: float((pred == y[N_TRAIN:]).astype(np.float32).mean())     # noqa: E731
    return Baseline(zt, ze, logits, acc(logits.argmax(axis=1)), acc(knn_predict(ze, zt, y[:N_TRAIN], FIXTURE_CLASSES, k)),
                    float((top[:, -1] - top[:, -2]).min()), int((zt != 0).any(axis=0).sum()))
