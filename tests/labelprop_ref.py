"""The CPU definition of gmp_label_propagate (include/gnnmp.h), operation for operation in numpy, and the fixed graphs of its tests.

propagate() works in fp32: every numpy operation on float32 arrays rounds once, so `acc + right[j] * F[j]` is a rounded multiply and a
rounded add, never a fused one, and x86 keeps subnormals.  It is vectorised over the rows and loops over the neighbour POSITION, so row
i's p-th entry is added as its p-th add: the sequential ascending order of the definition.  propagate64() is the same iteration in
float64 on the same inputs."""
from typing import NamedTuple

import numpy as np


ALPHA = np.float32(0.9)                        # label spreading's defaults as the kernel is given them:
BETA = np.float32(1.0 - 0.9)                   # 1 - alpha in float64, rounded once


class Result(NamedTuple):
    out: np.ndarray                # [n, classes]
    pred: np.ndarray               # int64 [n]
    status: np.ndarray             # int32 [2]
    residual: np.ndarray           # [rounds]


def orderable(x32: np.ndarray) -> np.ndarray:
    """float32 bits as uint32 that order like the floats (-0.0 below +0.0), as gmp::orderable does."""
    u = np.ascontiguousarray(x32, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000))


def argmax_rows(out: np.ndarray) -> np.ndarray:
    """The kernel's argmax: the greatest key (orderable score bits, ~class) per row -- ties go to the lower class."""
    n, c = out.shape
    key = (orderable(out).astype(np.uint64) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.arange(c, dtype=np.uint64))[None, :]
    best = key.max(axis=1) if n else np.zeros(0, np.uint64)
    return (np.uint64(0xFFFFFFFF) - (best & np.uint64(0xFFFFFFFF))).astype(np.int64)


def steps(rowptr, col, n):
    """Per neighbour position p: the rows whose p-th entry lies inside the graph, and that entry -- the bookkeeping of the sequential row
    sum, no arithmetic -- and the number of entries outside [0, n)."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    deg = rowptr[1:] - rowptr[:-1]
    inside = (col >= 0) & (col < n)
    out = []
    for p in range(int(deg.max()) if n else 0):
        rows = np.nonzero(deg > p)[0]
        k = rowptr[rows] + p
        out.append((rows[inside[k]], col[k][inside[k]]))
    return out, int((~inside).sum())


def _propagate(dtype, rowptr, col, f0, rounds, alpha, beta, left, right, clamp, f_init) -> Result:
    f0 = np.asarray(f0, dtype=dtype)
    n, classes = f0.shape
    alpha, beta = dtype(alpha), dtype(beta)
    left = np.ones(n, dtype) if left is None else np.asarray(left, dtype=dtype)
    right = np.ones(n, dtype) if right is None else np.asarray(right, dtype=dtype)
    F = f0.copy() if f_init is None else np.asarray(f_init, dtype=dtype).copy()
    positions, stray = steps(rowptr, col, n)
    residual = np.zeros(rounds, dtype)
    for t in range(rounds):
        acc = np.zeros((n, classes), dtype)
        for rows, j in positions:
            acc[rows] = acc[rows] + right[j][:, None] * F[j]        # an entry outside the graph is skipped, not added as zero
        v = left[:, None] * acc
        o = alpha * v + beta * f0
        new = o if clamp is None else np.where(np.asarray(clamp)[:, None] != 0, f0, o)
        residual[t] = np.abs(new - F).max() if new.size else 0
        F = new
    pred = argmax_rows(F) if dtype is np.float32 else F.argmax(axis=1)
    top = F[np.arange(n), pred] if n else np.zeros(0, dtype)
    status = np.array([stray, int((~(top > 0)).sum())], dtype=np.int32)
    return Result(F, pred.astype(np.int64), status, residual)


def propagate(rowptr, col, f0, rounds, alpha, beta, left=None, right=None, clamp=None, f_init=None) -> Result:
    return _propagate(np.float32, rowptr, col, f0, rounds, alpha, beta, left, right, clamp, f_init)


def propagate64(rowptr, col, f0, rounds, alpha, beta, left=None, right=None, clamp=None, f_init=None) -> Result:
    return _propagate(np.float64, rowptr, col, f0, rounds, alpha, beta, left, right, clamp, f_init)


def degree_scales(rowptr, kind: str):
    """(left, right) in fp32: float64 arithmetic on the integer degrees, rounded once.  sym: 1 / sqrt(deg) twice; rw: 1 / deg and None."""
    d = (np.asarray(rowptr, np.int64)[1:] - np.asarray(rowptr, np.int64)[:-1]).astype(np.float64)
    safe = np.where(d > 0, d, 1.0)
    if kind == "sym":
        s = np.where(d > 0, 1.0 / np.sqrt(safe), 0.0).astype(np.float32)
        return s, s
    return np.where(d > 0, 1.0 / safe, 0.0).astype(np.float32), None


# ---------------------------------------------------------------------------- graphs
class Graph(NamedTuple):
    n: int
    rowptr: np.ndarray             # int32 [n + 1]
    col: np.ndarray                # int32 [nnz]
    edges: np.ndarray              # int64 [2, E]: every undirected edge once (the edge_index a caller would hold)


def simple_csr(n: int, edges) -> Graph:
    """The simple undirected graph of an edge list: both directions, no loops, rows ascending, no duplicates."""
    e = np.asarray(edges, dtype=np.int64).reshape(-1, 2)
    e = e[e[:, 0] != e[:, 1]]
    both = np.concatenate([e, e[:, ::-1]])
    key = np.unique(both[:, 0] * n + both[:, 1]) if len(both) else np.zeros(0, np.int64)
    row, col = key // max(n, 1), key % max(n, 1)
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=n))
    once = np.stack([row[row < col], col[row < col]]) if len(key) else np.zeros((2, 0), np.int64)
    return Graph(n, rowptr.astype(np.int32), col.astype(np.int32), once.astype(np.int64))


PLANTED_N, PLANTED_CLASSES = 300, 7


def planted(n: int = PLANTED_N, classes: int = PLANTED_CLASSES, p_in: float = 0.08, p_out: float = 0.004, seed: int = 0):
    """(graph, labels int64 [n], seeds int64): a planted partition -- node v has class v % classes, an edge with probability p_in inside a
    class and p_out between two -- with node 0 isolated and every tenth node (3, 13, 23, ...) a seed.  Node 0 is no seed, so no label
    ever reaches it."""
    rng = np.random.default_rng(seed)
    y = np.arange(n, dtype=np.int64) % classes
    prob = np.where(y[:, None] == y[None, :], p_in, p_out)
    upper = np.triu(rng.random((n, n)) < prob, 1)
    upper[0, :] = False
    src, dst = np.nonzero(upper)
    return simple_csr(n, np.stack([src, dst], axis=1)), y, np.arange(3, n, 10, dtype=np.int64)


def one_hot(n: int, classes: int, seeds, labels) -> np.ndarray:
    f0 = np.zeros((n, classes), np.float32)
    f0[np.asarray(seeds), np.asarray(labels)] = 1.0
    return f0


def seed_mask(n: int, seeds) -> np.ndarray:
    m = np.zeros(n, np.uint8)
    m[np.asarray(seeds)] = 1
    return m


def random_graph(n: int, mean_degree: float, seed: int) -> Graph:
    rng = np.random.default_rng(seed)
    m = int(n * mean_degree / 2)
    return simple_csr(n, rng.integers(0, max(n, 1), size=(m, 2)))


def star(leaves: int = 300, chords: int = 5) -> Graph:
    """Node 0 is joined to nodes 1 .. leaves; a few chords between leaves: the hub's row has `leaves` entries."""
    e = [(0, v) for v in range(1, leaves + 1)] + [(1 + 7 * i, 2 + 11 * i) for i in range(chords)]
    return simple_csr(leaves + 1, e)


def path(n: int = 80) -> Graph:
    return simple_csr(n, [(v, v + 1) for v in range(n - 1)])


def subnormal_case():
    """(graph, f0, left, right, alpha, beta, rounds): a path of 80 nodes seeded at one end; with alpha = 0.01 every hop costs two decimal
    digits and more, so after 60 rounds the far entries are fp32 subnormals."""
    g = path(80)
    left, right = degree_scales(g.rowptr, "sym")
    return g, one_hot(80, 1, [0], [0]), left, right, np.float32(0.01), np.float32(0.99), 60


def empty(n: int) -> Graph:
    return simple_csr(n, np.zeros((0, 2), np.int64))


def with_stray_columns(g: Graph):
    """g's CSR with two more entries that point outside [0, n): col = n at the head of row 1's list, col = -1 at the end of the last row's."""
    rp, cl = g.rowptr.astype(np.int64), g.col.astype(np.int64)
    a, b = int(rp[1]), int(rp[g.n])
    col = np.concatenate([cl[:a], [g.n], cl[a:b], [-1]])
    rowptr = rp.copy()
    rowptr[2:] += 1
    rowptr[g.n] += 1
    return Graph(g.n, rowptr.astype(np.int32), col.astype(np.int32), g.edges)


LADDER_N = 24


def degree_ladder(stray: bool = True) -> Graph:
    """A raw CSR written by hand (not symmetric; `edges` is empty): row v holds v entries inside [0, n), ascending, so the degrees 0, 7, 8,
    9, 15, 16 and 17 -- every remainder of a batch of 8 around one and two full batches -- all occur.  With `stray`, row 12 gets col = n
    at position 3 (inside its full batch) and row 17 gets col = -1 as its last entry (in the tail after two full batches)."""
    n = LADDER_N
    rows = [sorted((v + 1 + p) % n for p in range(v)) for v in range(n)]          # the v nodes after v, cyclically
    if stray:
        rows[12].insert(3, n)
        rows[17].append(-1)
    rowptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    return Graph(n, rowptr.astype(np.int32), np.array([c for r in rows for c in r], np.int32), np.zeros((2, 0), np.int64))


def random_inputs(n: int, classes: int, seed: int):
    """(f0, f_init, left, right, clamp): dense positive and negative fp32 values, so every lane of every width has something to round."""
    rng = np.random.default_rng(seed)
    f0 = rng.standard_normal((n, classes)).astype(np.float32)
    f_init = rng.standard_normal((n, classes)).astype(np.float32)
    left = rng.uniform(0.1, 1.0, n).astype(np.float32)
    right = rng.uniform(0.1, 1.0, n).astype(np.float32)
    clamp = (rng.random(n) < 0.2).astype(np.uint8)
    return f0, f_init, left, right, clamp
