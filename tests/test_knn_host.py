"""Host-side contract of the streaming k-nearest-neighbour probe (csrc/knn.hip): the fp64 reference of tests/knn_ref.py pinned on cases
worked out by hand, declaration / binding / export of the three C-ABI entry points, a workspace without the nq x ndb matrix, and every bad call refused with its error code before anything is launched (so this runs
without a GPU)."""
import ctypes

import numpy as np
import pytest

import knn_ref as R
from gnn_pretraining_amd import _lib as L

ERR_ARG, ERR_WORKSPACE = -1, -3
NINF = float("-inf")


# ---------------------------------------------------------------------------- the reference, by hand
def test_reference_orders_by_score_then_lower_index_and_pads_the_tail():
    q = np.array([[2.0, 0.0], [0.0, 0.0]])
    db = np.array([[0.0, 3.0], [5.0, 0.0], [1.0, 1.0], [7.0, 0.0], [-1.0, 0.0]])
    # cosines of row 0: 0, 1, 1/sqrt(2), 1, -1: rows 1 and 3 tie and the lower index goes first
    idx, sim = R.topk(q, db, 3)
    assert idx[0].tolist() == [1, 3, 2]
    assert sim[0, 0] == 1.0 and sim[0, 1] == 1.0 and abs(sim[0, 2] - 2 ** -0.5) < 1e-15
    # a zero query scores 0 against everything, no NaN: all tied, index order
    assert idx[1].tolist() == [0, 1, 2] and sim[1].tolist() == [0.0, 0.0, 0.0]
    # k beyond the database: every row in order, then -1 / -inf
    idx, sim = R.topk(q, db, 7)
    assert idx[0].tolist() == [1, 3, 2, 0, 4, -1, -1]
    assert sim[0, 3] == 0.0 and sim[0, 4] == -1.0 and sim[0, 5] == NINF and sim[0, 6] == NINF


def test_reference_exclude_self_zero_database_rows_and_replay_on_given_scores():
    z = np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 0.0], [0.0, 2.0]])
    idx, sim = R.topk(z, z, 3, exclude_self=True)
    assert idx.tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2]]        # never i itself; the zero row scores 0 like the orthogonal one
    assert sim[0].tolist() == [1.0, 0.0, 0.0] and sim[3].tolist() == [0.0, 0.0, 0.0]
    idx, sim = R.topk(z, z, 4, exclude_self=True)
    assert idx[:, 3].tolist() == [-1] * 4 and sim[:, 3].tolist() == [NINF] * 4       # three candidates only
    with pytest.raises(ValueError):
        R.topk(z, z[:3], 2, exclude_self=True)
    # the selection on someone else's scores, in their dtype
    S = np.array([[0.5, 0.75, 0.75, 0.25]], dtype=np.float32)
    idx, sim = R.topk(None, None, 3, similarity=S)
    assert idx.tolist() == [[1, 2, 0]] and sim.dtype == np.float32 and sim.tolist() == [[0.75, 0.75, 0.5]]


def test_reference_vote_sums_in_order_skips_bad_labels_and_breaks_ties_to_the_lower_class():
    T = 0.5
    idx = np.array([[0, 1, 2], [3, 1, -1], [-1, -1, -1], [4, 0, -1]])
    sim = np.array([[1.0, 0.5, 0.5], [0.5, 0.5, NINF], [NINF, NINF, NINF], [1.0, 0.0, NINF]])
    labels = np.array([2, 0, 0, 1, 9])                                         # row 4 carries a label outside [0, 3)
    scores, pred, status = R.vote(idx, sim, labels, 3, T)
    e = np.exp
    assert np.allclose(scores[0], [2 * e(1.0), 0.0, e(2.0)]) and pred[0] == 2       # e^2 = 7.39 > 2 e = 5.44
    assert np.allclose(scores[1], [e(1.0), e(1.0), 0.0]) and pred[1] == 0           # a tie: the lower class
    assert not scores[2].any() and pred[2] == -1                                    # no neighbour at all
    assert np.allclose(scores[3], [0.0, 0.0, 1.0]) and pred[3] == 2 and status == 1  # the bad label is skipped and counted


# ---------------------------------------------------------------------------- the C ABI
def test_workspace_holds_no_matrix_and_grows_at_most_linearly():
    ws = L.lib().gmp_knn_workspace_bytes
    assert 0 < ws(1 << 20, 1 << 20, 256, 64) < 4 << 30                           # two normalised copies of 1 GiB + the lists
    for nq, ndb, d, k in [(1000, 140, 256, 20), (2708, 2708, 256, 20), (301, 2500, 40, 64), (19717, 19717, 256, 20), (65535, 65535, 256, 64),
                          (1 << 20, 1 << 20, 256, 64)]:
        a, b = ws(nq, ndb, d, k), ws(nq, 2 * ndb, d, k)
        assert 0 < a <= b <= 2 * a, (nq, ndb, d, k, a, b)
        assert a < 4 * nq * ndb or nq * ndb < 1 << 20                            # far below the matrix once the problem is not tiny
        dpad = (d + 3) // 4 * 4
        assert a <= 4 * (nq + ndb) * dpad + 8 * 16 * nq * k + 2048
    assert ws(19717, 19717, 256, 20) < 64 << 20 and ws(65535, 65535, 256, 20) < 150 << 20      # the matrices: 1.6 GB and 17 GB
    for bad in [(-1, 5, 8, 4), (5, -1, 8, 4), (1 << 31, 5, 8, 4), (5, 1 << 31, 8, 4), (5, 5, 0, 4), (5, 5, 257, 4), (5, 5, 8, 0), (5, 5, 8, 65)]:
        assert ws(*bad) == 0


def topk_call(q=0x1000, nq=9, db=0x2000, ndb=7, dim=8, k=4, excl=0, idx=0x3000, sim=0x4000, mat=0, ws=0x5000, ws_bytes=1 << 20):
    """the pointers are never dereferenced by the host and nothing is launched on a refused call"""
    vp = ctypes.c_void_p
    return L.lib().gmp_knn_topk(vp(q), nq, vp(db), ndb, dim, k, excl, vp(idx), vp(sim), vp(mat), vp(ws), ws_bytes, None)


def vote_call(idx=0x1000, sim=0x2000, nq=9, k=4, labels=0x3000, ndb=7, classes=7, temperature=0.07, scores=0x4000, pred=0x5000, status=0x6000):
    vp = ctypes.c_void_p
    return L.lib().gmp_knn_vote(vp(idx), vp(sim), nq, k, vp(labels), ndb, classes, temperature, vp(scores), vp(pred), vp(status), None)


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=65), dict(k=-1), dict(dim=0), dict(dim=257), dict(nq=-1), dict(ndb=-1), dict(nq=1 << 31),
                                dict(ndb=1 << 31), dict(q=0), dict(db=0), dict(idx=0), dict(sim=0)])
def test_topk_refuses_bad_sizes_and_null_pointers(kw):
    assert topk_call(**kw) == ERR_ARG
    assert b"knn_topk" in L.lib().gmp_last_error_string()


def test_topk_exclude_self_needs_one_set_and_a_short_workspace_is_refused():
    assert topk_call(excl=1) == ERR_ARG                                          # q != db
    assert topk_call(excl=1, db=0x1000) == ERR_ARG                               # q == db but nq != ndb
    assert b"exclude_self" in L.lib().gmp_last_error_string()
    need = L.lib().gmp_knn_workspace_bytes(9, 7, 8, 4)
    assert topk_call(ws_bytes=need - 1) == ERR_WORKSPACE and topk_call(ws=0) == ERR_WORKSPACE
    assert topk_call(excl=1, db=0x1000, ndb=9, ws_bytes=0) == ERR_WORKSPACE      # a well-formed leave-one-out call gets as far as the workspace
    assert topk_call(nq=0, ws=0, ws_bytes=0) == 0                                # no queries: a no-op


@pytest.mark.parametrize("kw", [dict(k=0), dict(k=65), dict(classes=1), dict(classes=33), dict(temperature=0.0), dict(temperature=-1.0),
                                dict(temperature=float("nan")), dict(nq=-1), dict(ndb=-1), dict(idx=0), dict(sim=0), dict(labels=0),
                                dict(scores=0), dict(pred=0), dict(status=0)])
def test_vote_refuses_bad_sizes_and_null_pointers(kw):
    assert vote_call(**kw) == ERR_ARG
    assert b"knn_vote" in L.lib().gmp_last_error_string()
