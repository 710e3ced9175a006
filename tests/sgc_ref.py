"""The CPU definition of gmp_feature_propagate (include/gnnmp.h), operation for operation in numpy fp32, the float64 twin of
node_baselines.softmax_fit, and the fixtures of test_sgc_host.py / test_gpu_sgc.py.  The graphs are those of labelprop_ref.py.

propagate() works in fp32: every numpy operation on float32 arrays rounds once, so `acc + right[j] * H[j]` is a rounded multiply and a
rounded add, never a fused one, and x86 keeps subnormals.  It is vectorised over the rows and loops over the neighbour POSITION, so row
i's p-th entry is added as its p-th add: the sequential ascending order of the definition.  propagate_csr() takes the features in CSR form
and walks the first round entry by entry -- a neighbour's stored entries only, the malformed ones skipped and counted -- and then goes on
densely.  fit() is the written-out Adam loop of softmax_fit in the dtype it is given."""
import functools
from typing import NamedTuple

import numpy as np

import labelprop_ref as LP
from labelprop_ref import Graph, empty, path, planted, random_graph, star, subnormal_case, with_stray_columns  # noqa: F401  (the graphs)


class Result(NamedTuple):
    out: np.ndarray                # fp32 [n, d]
    status: np.ndarray             # int32 [2]: adjacency entries outside [0, n), feature entries that break the CSR form


def _round(steps, H, left, right):
    acc = np.zeros(H.shape, np.float32)
    for rows, j in steps:
        acc[rows] = acc[rows] + right[j][:, None] * H[j]            # an entry outside the graph is skipped, not added as zero
    return left[:, None] * acc


def _scales(n, left, right):
    return (np.ones(n, np.float32) if left is None else np.asarray(left, np.float32),
            np.ones(n, np.float32) if right is None else np.asarray(right, np.float32))


def propagate(rowptr, col, x, rounds, left=None, right=None) -> Result:
    H = np.asarray(x, dtype=np.float32).copy()
    n = H.shape[0]
    left, right = _scales(n, left, right)
    steps, stray = LP.steps(rowptr, col, n)
    for _ in range(rounds):
        H = _round(steps, H, left, right)
    return Result(H, np.array([stray, 0], np.int32))


def csr_valid(x_rowptr, x_col, d) -> np.ndarray:
    """Per stored feature entry: its column lies in [0, d) and is greater than the stored column before it in its row."""
    x_rowptr, x_col = np.asarray(x_rowptr, np.int64), np.asarray(x_col, np.int64)
    prev = np.concatenate([[-1], x_col[:-1]]) if x_col.size else np.zeros(0, np.int64)
    starts = x_rowptr[:-1][x_rowptr[:-1] < x_rowptr[1:]]
    prev[starts] = -1
    return (x_col >= 0) & (x_col < d) & (x_col > prev)


def propagate_csr(rowptr, col, x_rowptr, x_col, x_val, d, rounds, left=None, right=None) -> Result:
    rp, cl = np.asarray(rowptr, np.int64), np.asarray(col, np.int64)
    xr, xc, xv = np.asarray(x_rowptr, np.int64), np.asarray(x_col, np.int64), np.asarray(x_val, np.float32)
    n = len(rp) - 1
    left, right = _scales(n, left, right)
    valid = csr_valid(xr, xc, d)
    acc = np.zeros((n, d), np.float32)
    for i in range(n):
        for k in range(rp[i], rp[i + 1]):
            j = cl[k]
            if not 0 <= j < n:
                continue
            for e in range(xr[j], xr[j + 1]):                       # entry by entry: a column may stand twice in a malformed row
                if valid[e]:
                    acc[i, xc[e]] = acc[i, xc[e]] + right[j] * xv[e]
    H = left[:, None] * acc
    steps, stray = LP.steps(rp, cl, n)
    for _ in range(rounds - 1):
        H = _round(steps, H, left, right)
    return Result(H, np.array([stray, int((~valid).sum())], np.int32))


def to_dense(x_rowptr, x_col, x_val, n, d) -> np.ndarray:
    """The densified matrix of a WELL-FORMED CSR (stored zeros become zeros)."""
    out = np.zeros((n, d), np.float32)
    rows = np.repeat(np.arange(n), np.diff(np.asarray(x_rowptr, np.int64)))
    out[rows, np.asarray(x_col, np.int64)] = np.asarray(x_val, np.float32)
    return out


def sparse_features(n: int, d: int, seed: int, density: float = 0.02):
    """(x_rowptr int32, x_col int32, x_val fp32): about `density` of the entries stored, columns strictly ascending, every seventh
    stored value an explicit zero, and row min(3, n - 1) empty."""
    rng = np.random.default_rng(seed)
    mask = rng.random((n, d)) < density
    mask[min(3, n - 1)] = False
    rows, cols = np.nonzero(mask)
    val = rng.standard_normal(rows.size).astype(np.float32)
    val[::7] = 0.0
    rowptr = np.zeros(n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(rows, minlength=n))
    return rowptr.astype(np.int32), cols.astype(np.int32), val


def with_bad_feature_entries(x_rowptr, x_col, x_val, d):
    """The CSR with three entries spoilt in place, in three different rows that hold at least three entries each: a row's last column set
    to d, a row's first to -1, and one set equal to the column before it (a non-ascending pair) -- placed so that the entry after each is
    still greater than what is stored before it, and exactly these three are skipped.  Returns (x_col', the three entry positions)."""
    xr, xc = np.asarray(x_rowptr, np.int64), np.asarray(x_col, np.int32).copy()
    rows = np.nonzero(np.diff(xr) >= 3)[0][:3]
    assert len(rows) == 3
    at = [int(xr[rows[0] + 1]) - 1, int(xr[rows[1]]), int(xr[rows[2]]) + 2]
    xc[at[0]], xc[at[1]], xc[at[2]] = d, -1, xc[at[2] - 1]
    return xc, at


def sgc_graph(g: Graph):
    """(rowptr, col, scale): g plus one self-loop per node at its sorted position, scale = 1 / sqrt(deg + 1) from float64, rounded once."""
    loops = np.stack([np.arange(g.n), np.arange(g.n)], axis=1)
    both = np.concatenate([g.edges.T, g.edges.T[:, ::-1], loops]).astype(np.int64)
    key = np.unique(both[:, 0] * g.n + both[:, 1])
    row, col = key // max(g.n, 1), key % max(g.n, 1)
    rowptr = np.zeros(g.n + 1, np.int64)
    rowptr[1:] = np.cumsum(np.bincount(row, minlength=g.n))
    scale = (1.0 / np.sqrt(np.diff(rowptr).astype(np.float64))).astype(np.float32)
    return rowptr.astype(np.int32), col.astype(np.int32), scale


def sgc_features(g: Graph, x, rounds: int) -> np.ndarray:
    if rounds == 0:
        return np.asarray(x, np.float32).copy()
    rowptr, col, scale = sgc_graph(g)
    return propagate(rowptr, col, x, rounds, scale, scale).out


# ---------------------------------------------------------------------------- the fit
ITERS, LR, L2 = 100, 0.2, 5e-6
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8


def fit(dtype, features, labels, classes, iters=ITERS, lr=LR, l2=L2):
    """(W [C, d], b [C], loss_history [iters]) of the full-batch softmax regression from zeros in `dtype`: the mean cross-entropy, the ridge
    l2 * W on the weights alone, then torch.optim.Adam's rule with bias correction."""
    F, y = np.asarray(features, dtype), np.asarray(labels, np.int64)
    m, d = F.shape
    W, b = np.zeros((classes, d), dtype), np.zeros(classes, dtype)
    mW, vW, mb, vb = np.zeros_like(W), np.zeros_like(W), np.zeros_like(b), np.zeros_like(b)
    onehot = np.zeros((m, classes), dtype)
    onehot[np.arange(m), y] = 1
    history = np.zeros(iters, dtype)
    c = lambda v: dtype(v)                                           # noqa: E731
    for t in range(1, iters + 1):
        z = F @ W.T + b
        z = z - z.max(axis=1, keepdims=True)
        lse = np.log(np.exp(z).sum(axis=1, keepdims=True))
        history[t - 1] = (lse[:, 0] - z[np.arange(m), y]).sum() / c(m)
        G = (np.exp(z - lse) - onehot) / c(m)
        gW, gb = G.T @ F + c(l2) * W, G.sum(axis=0)
        for p, g, mm, vv in ((W, gW, mW, vW), (b, gb, mb, vb)):
            mm *= c(BETA1); mm += c(1 - BETA1) * g
            vv *= c(BETA2); vv += c(1 - BETA2) * g * g
            denom = np.sqrt(vv) / c((1 - BETA2 ** t) ** 0.5) + c(EPS)
            p -= c(lr / (1 - BETA1 ** t)) * (mm / denom)
    return W, b, history


# ---------------------------------------------------------------------------- the fixture of the fit and of feature_baselines
FIXTURE_DIM, FIXTURE_ROUNDS = 45, 2


class Fixture(NamedTuple):
    graph: Graph
    y: np.ndarray                  # int64 [300]
    train: np.ndarray              # the seeds of planted(): every tenth node
    evaluate: np.ndarray           # all the others
    x: np.ndarray                  # fp32 [300, 45]


@functools.lru_cache(maxsize=None)
def fixture() -> Fixture:
    g, y, seeds = planted()
    rng = np.random.default_rng(1)
    means = rng.standard_normal((LP.PLANTED_CLASSES, FIXTURE_DIM))
    x = (means[y] + 1.5 * rng.standard_normal((g.n, FIXTURE_DIM))).astype(np.float32)
    return Fixture(g, y, seeds, np.setdiff1d(np.arange(g.n), seeds), x)


class Fit(NamedTuple):
    features: np.ndarray           # fp32 [n, d]: S^K X by the fp32 definition
    logits: np.ndarray             # [eval, C] in the fit's dtype
    pred: np.ndarray
    accuracy: float
    margin: float                  # the smallest gap between the two largest logits of an evaluation row


@functools.lru_cache(maxsize=None)
def reference_fit(rounds: int, dtype=np.float64) -> Fit:
    """The fit of the fixture at K = rounds: features by the fp32 definition (what the kernel leaves, bit for bit), the regression in
    `dtype` on the train rows, scored on the evaluation rows.  Computed once and shared; callers must not write into it."""
    fx = fixture()
    feats = sgc_features(fx.graph, fx.x, rounds)
    W, b, _ = fit(dtype, feats[fx.train], fx.y[fx.train], LP.PLANTED_CLASSES)
    logits = feats[fx.evaluate].astype(dtype) @ W.T + b
    top = np.sort(logits, axis=1)
    pred = logits.argmax(axis=1)
    return Fit(feats, logits, pred, float((pred == fx.y[fx.evaluate]).astype(np.float32).mean()), float((top[:, -1] - top[:, -2]).min()))
