"""The streaming k-nearest-neighbour probe (csrc/knn.hip: ops.knn_topk / ops.knn_vote, metrics.knn_probe_accuracy, --knn-probe) on the
GPU against the fp64 definition of tests/knn_ref.py, at the bars of tests/test_gpu_miner_stream.py: (a) where the arithmetic is exact,
neighbours, order and similarities equal the reference's bit for bit, across every tile width, the part boundaries and the merge; (b) on
random embeddings the selection equals the reference's selection replayed on the kernel's own similarity matrix and the similarities
agree to 1e-5; (c) - (e) all-equal scores, leave-one-out, the edges of the contract; (f) the vote; (g) the probe of
metrics.py above them (finetune() with the probe on: tests/test_gpu_probes.py)."""
import functools

import numpy as np
import pytest
import torch

import knn_ref as R
from gnn_pretraining_amd import ops
from gnn_pretraining_amd._lib import GnnmpError
from gnn_pretraining_amd.finetune.metrics import knn_probe_accuracy

pytestmark = pytest.mark.gpu
DEV = "cuda"
NINF = float("-inf")
CLASSES = 7


def _topk(q, db, k, **kw):
    out = ops.knn_topk(torch.as_tensor(q).to(DEV), torch.as_tensor(db).to(DEV), k, **kw)
    return tuple(t.cpu().numpy() for t in out)


def _loo(z, k, **kw):
    z = torch.as_tensor(z).to(DEV)
    return tuple(t.cpu().numpy() for t in ops.knn_topk(z, z, k, exclude_self=True, **kw))


# ---------------------------------------------------------------------------- (a) exact arithmetic
def _check_exact(q, db, k):
    idx, sim = _topk(q, db, k)
    want_idx, want_sim = R.topk(q, db, k)
    assert np.array_equal(idx, want_idx)                             # same neighbours, same order (ties: lower index), same tail
    assert sim.dtype == np.float32 and np.array_equal(sim.astype(np.float64), want_sim)
    return want_sim


@pytest.mark.parametrize("nq,ndb,d,k", [(1, 1, 8, 1), (5, 3, 6, 4), (129, 33, 16, 8), (301, 1000, 24, 20), (1000, 70, 32, 64),
                                        (301, 2500, 32, 64), (301, 2500, 40, 64), (301, 2500, 100, 64), (301, 2500, 160, 64),
                                        (301, 2500, 256, 64)])      # one per tile width; 2,500 rows: 16 parts, so the merge orders them
def test_bit_exact_on_four_ones_rows(nq, ndb, d, k):
    want_sim = _check_exact(R.four_ones(nq, d, nq + d), R.four_ones(ndb, d, ndb + d + 1), k)
    if (nq, ndb, k) == (5, 3, 4):
        assert (want_sim[:, 3] == NINF).all() and np.isfinite(want_sim[:, :3]).all()


def test_bit_exact_on_sixteen_sign_rows_with_k_inside_a_tie_group():
    q, db, k = R.sixteen_signs(301, 32, 11), R.sixteen_signs(2500, 32, 12), 20
    _check_exact(q, db, k)
    _, s21 = R.topk(q, db, k + 1)
    assert (s21[:, k - 1] == s21[:, k]).mean() > 0.5                 # the k-th and the (k + 1)-th score tie: the index decides who stays


# ---------------------------------------------------------------------------- (b) random embeddings
RANDOM_CASES = [("randn", 300, 1000, 256, 20), ("randn", 257, 2500, 40, 64), ("abs", 500, 140, 256, 20)]


def _random_inputs(kind, nq, ndb, d):
    g = torch.Generator().manual_seed(nq + ndb)
    q, db = torch.randn(nq, d, generator=g), torch.randn(ndb, d, generator=g)
    if kind == "abs":
        q, db = q.abs(), db.abs()
    return q.numpy(), db.numpy(), torch.randint(0, CLASSES, (ndb,), generator=g).numpy()


@functools.lru_cache(maxsize=None)
def _random_case(i):
    """inputs, the kernel's (idx, sim, matrix) and the fp64 cosine of RANDOM_CASES[i]: computed once, read by (b) and (f)"""
    kind, nq, ndb, d, k = RANDOM_CASES[i]
    q, db, labels = _random_inputs(kind, nq, ndb, d)
    idx, sim, mat = _topk(q, db, k, return_matrix=True)
    return dict(q=q, db=db, labels=labels, k=k, idx=idx, sim=sim, mat=mat, cos=R.cosine(q, db))


@pytest.mark.parametrize("i", range(len(RANDOM_CASES)))
def test_selection_is_exact_on_its_own_scores_and_scores_match_fp64(i):
    c = _random_case(i)
    idx, sim, mat, cos, k = c["idx"], c["sim"], c["mat"], c["cos"], c["k"]
    err = float(np.abs(mat - cos).max())
    print(f"{RANDOM_CASES[i]}: max |S - fp64| = {err:.3e}")
    assert err < 1e-5
    # index work on the same floats is exact
    want_idx, want_sim = R.topk(None, None, k, similarity=mat)
    assert np.array_equal(idx, want_idx) and np.array_equal(sim, want_sim)
    assert (sim[:, :-1] >= sim[:, 1:]).all()
    assert np.array_equal(sim, np.take_along_axis(mat, idx, axis=1))
    # against fp64's own scores: the k-th score agrees, every pick lies at or above it ...
    _, ref_sim = R.topk(None, None, k, similarity=cos)
    kth = ref_sim[:, -1:]
    print(f"{RANDOM_CASES[i]}: max |k-th - fp64's| = {float(np.abs(sim[:, -1:] - kth).max()):.3e}")
    assert float(np.abs(sim[:, -1:] - kth).max()) < 1e-5
    assert (np.take_along_axis(cos, idx, axis=1) >= kth - 2e-5).all()
    # ... and no database row clearly above the returned k-th score is missing
    picked = np.zeros(cos.shape, dtype=bool)
    np.put_along_axis(picked, idx, True, axis=1)
    assert not ((cos > sim[:, -1:].astype(np.float64) + 2e-5) & ~picked).any()


# ---------------------------------------------------------------------------- (c) all-equal scores
def test_all_equal_scores_return_the_first_k_indices():
    g = torch.Generator().manual_seed(5)
    idx, sim = _topk(torch.randn(200, 12, generator=g), torch.ones(1500, 12), 20)      # every database row is the same row
    assert np.array_equal(idx, np.tile(np.arange(20), (200, 1)))
    assert (sim == sim[:, :1]).all()
    n, k = 1500, 64
    idx, sim = _loo(torch.ones(n, 4), k)
    want = np.array([[j for j in range(k + 1) if j != i][:k] for i in range(n)])
    assert np.array_equal(idx, want) and (sim == 1.0).all()


# ---------------------------------------------------------------------------- (d) exclude_self on random rows
def test_leave_one_out_on_random_rows():
    n, k = 700, 20
    z = torch.randn(n, 50, generator=torch.Generator().manual_seed(700)).numpy()
    idx, sim, mat = _loo(z, k, return_matrix=True)
    assert float(np.abs(mat - R.cosine(z, z)).max()) < 1e-5           # the matrix keeps its diagonal; the selection leaves it out
    want_idx, want_sim = R.topk(None, None, k, exclude_self=True, similarity=mat)
    assert np.array_equal(idx, want_idx) and np.array_equal(sim, want_sim)
    assert not (idx == np.arange(n)[:, None]).any()
    zd = torch.as_tensor(z).to(DEV)
    with pytest.raises(GnnmpError):
        ops.knn_topk(zd, zd.clone(), k, exclude_self=True)           # equal values are not the same set
    with pytest.raises(GnnmpError):
        ops.knn_topk(zd[:600], zd, k, exclude_self=True)


# ---------------------------------------------------------------------------- (e) edges
def test_zero_rows_bounds_short_tail_determinism_and_cpu_tensors():
    g = torch.Generator().manual_seed(1)
    q, db = torch.zeros(40, 8), torch.zeros(90, 8)
    q[:10], db[:30] = torch.randn(10, 8, generator=g), torch.randn(30, 8, generator=g)
    idx, sim, mat = _topk(q, db, 16, return_matrix=True)            # zero rows: score 0, no NaN
    assert np.isfinite(sim).all() and np.isfinite(mat).all() and (mat[10:] == 0).all() and (mat[:, 30:] == 0).all()
    want_idx, want_sim = R.topk(None, None, 16, similarity=mat)
    assert np.array_equal(idx, want_idx) and np.array_equal(sim, want_sim)
    qd, dbd = q.to(DEV), db.to(DEV)
    for k in (0, 65):
        with pytest.raises(GnnmpError):
            ops.knn_topk(qd, dbd, k)
    with pytest.raises(GnnmpError):
        ops.knn_topk(torch.zeros(4, 257, device=DEV), torch.zeros(5, 257, device=DEV), 2)
    with pytest.raises(GnnmpError):
        ops.knn_topk(q, db, 4)                                       # CPU tensors: there is no fallback
    # fewer database rows than k: the rows in order, then -1 / -inf
    q, db = torch.randn(70, 10, generator=g).numpy(), torch.randn(6, 10, generator=g).numpy()
    idx, sim, mat = _topk(q, db, 40, return_matrix=True)
    want_idx, want_sim = R.topk(None, None, 40, similarity=mat)
    assert np.array_equal(idx, want_idx) and np.array_equal(sim, want_sim)
    assert (idx[:, 6:] == -1).all() and (sim[:, 6:] == NINF).all() and (idx[:, :6] >= 0).all()
    idx, sim = _loo(torch.randn(1, 10, generator=g), 3)             # leave-one-out over one row: no candidate at all
    assert (idx == -1).all() and (sim == NINF).all()
    # the output is a pure function of the input
    q, db = torch.randn(700, 40, generator=g), torch.randn(3000, 40, generator=g)
    a, b = _topk(q, db, 33), _topk(q, db, 33)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---------------------------------------------------------------------------- (f) the vote
@pytest.mark.parametrize("i", range(len(RANDOM_CASES)))
def test_vote_on_the_kernels_own_neighbours(i):
    c = _random_case(i)
    idx, sim, labels = c["idx"], c["sim"], c["labels"]
    scores, pred = ops.knn_vote(torch.as_tensor(idx).to(DEV), torch.as_tensor(sim).to(DEV), torch.as_tensor(labels).to(DEV), CLASSES)
    scores, pred = scores.cpu().numpy(), pred.cpu().numpy()
    want, want_pred, status = R.vote(idx, sim, labels, CLASSES)
    assert status == 0
    rel = np.abs(scores - want) / np.maximum(want, 1e-300)
    print(f"{RANDOM_CASES[i]}: max relative error of class_scores = {float(rel[want > 0].max()):.3e}")
    assert (scores[want == 0] == 0).all() and float(rel[want > 0].max()) < 1e-5
    assert np.array_equal(pred, scores.argmax(axis=1))               # (numpy's argmax: the first maximum, i.e. the lower class)
    top = np.sort(want, axis=1)
    clear = (top[:, -1] - top[:, -2]) / top[:, -1] > 1e-4
    print(f"{RANDOM_CASES[i]}: rows inside the 1e-4 margin: {int((~clear).sum())} of {clear.size}")
    assert (~clear).mean() <= 0.01
    assert np.array_equal(pred[clear], want_pred[clear])


def test_vote_without_neighbours_and_with_a_label_out_of_range():
    idx = torch.tensor([[0, 2, -1], [-1, -1, -1], [1, 1, 0]], device=DEV)
    sim = torch.tensor([[0.5, 0.25, NINF], [NINF, NINF, NINF], [0.7, 0.7, 0.1]], device=DEV)
    labels = torch.tensor([3, 0, 3], device=DEV)
    scores, pred = ops.knn_vote(idx, sim, labels, 4, temperature=0.5)
    want, want_pred, _ = R.vote(idx.cpu().numpy(), sim.cpu().numpy(), labels.cpu().numpy(), 4, 0.5)
    assert pred.tolist() == [3, -1, 0] and want_pred.tolist() == [3, -1, 0]
    assert np.allclose(scores.cpu().numpy(), want, rtol=1e-5, atol=0) and not scores[1].any()
    for bad in (4, -1):
        with pytest.raises(GnnmpError, match="outside"):
            ops.knn_vote(idx, sim, torch.tensor([3, 0, bad], device=DEV), 4)
    for kw in (dict(num_classes=1), dict(num_classes=33), dict(num_classes=4, temperature=0.0)):
        with pytest.raises(GnnmpError):
            ops.knn_vote(idx, sim, labels, **kw)
    with pytest.raises(GnnmpError):
        ops.knn_vote(idx.cpu(), sim.cpu(), labels.cpu(), 4)


# ---------------------------------------------------------------------------- (g) planted clusters
def test_probe_accuracy_on_planted_clusters():
    g = torch.Generator().manual_seed(7)
    centroids = torch.randn(CLASSES, 64, generator=g)
    db_y, q_y = torch.randint(0, CLASSES, (400,), generator=g), torch.randint(0, CLASSES, (200,), generator=g)
    db = (centroids[db_y] + 0.05 * torch.randn(400, 64, generator=g)).to(DEV)
    q = (centroids[q_y] + 0.05 * torch.randn(200, 64, generator=g)).to(DEV)
    m = knn_probe_accuracy(db, db_y.to(DEV), q, q_y.to(DEV), CLASSES, k=20)
    assert m["accuracy"] == 1.0 and m["correct"] == 200 and m["num_samples"] == 200
    shuffled = db_y[torch.randperm(400, generator=g)]
    m = knn_probe_accuracy(db, shuffled.to(DEV), q, q_y.to(DEV), CLASSES, k=20)
    print(f"accuracy with permuted database labels: {m['accuracy']:.3f}")
    assert m["accuracy"] < 0.5 and m["accuracy"] == m["correct"] / 200
