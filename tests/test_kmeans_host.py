"""Host-side contract of the k-means clustering probe (csrc/kmeans.hip): the fp64 reference of tests/kmeans_ref.py pinned on cases worked
out by hand, its scores and metrics.clustering_scores against scikit-learn and a brute-force matching, declaration / binding / export of
the four C-ABI entry points, a workspace without the n x kc matrix, and every bad
call refused with its error code before anything is launched (so this runs without a GPU)."""
import ctypes
import itertools

import numpy as np
import pytest

import kmeans_ref as R
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd.finetune.metrics import clustering_scores

ERR_ARG, ERR_WORKSPACE = -1, -3


# ---------------------------------------------------------------------------- the reference, by hand
def test_reference_assign_ties_go_to_the_lower_index_and_a_zero_row_lands_on_centroid_0():
    x = np.array([[2.0, 0.0], [0.0, 0.0], [0.0, 3.0], [1.0, 1.0]])
    c = np.array([[0.0, 1.0], [5.0, 0.0], [7.0, 0.0], [0.0, 2.0]])                # 1 and 2 are one direction, so are 0 and 3
    labels, sim = R.assign(x, c)
    assert labels.tolist() == [1, 0, 0, 0]                                       # row 3 ties between 0 / 3 (and 1 / 2) at 1 / sqrt(2)
    assert sim[0] == 1.0 and sim[1] == 0.0 and sim[2] == 1.0 and abs(sim[3] - 2 ** -0.5) < 1e-15
    # the selection on someone else's scores, in their dtype
    S = np.array([[0.5, 0.75, 0.75, 0.25], [-1.0, -1.0, -2.0, -1.0]], dtype=np.float32)
    labels, sim = R.assign(None, None, similarity=S)
    assert labels.tolist() == [1, 0] and sim.dtype == np.float32 and sim.tolist() == [0.75, -1.0]


def test_reference_update_normalises_the_sum_and_an_empty_cluster_keeps_its_centroid():
    xn = R.normalize(np.array([[1.0, 0.0], [0.0, 1.0], [1.0, 0.0]]))
    prev = np.array([[0.6, 0.8], [0.0, 1.0], [-1.0, 0.0]])
    c = R.update(xn, [0, 0, 0], prev)
    assert np.allclose(c[0], np.array([2.0, 1.0]) / 5 ** 0.5, atol=1e-15)
    assert c[1].tolist() == [0.0, 1.0] and c[2].tolist() == [-1.0, 0.0]          # no rows: untouched
    assert prev[0].tolist() == [0.6, 0.8]                                        # (the input is not written)


def test_reference_fit_on_three_points_worked_on_paper():
    # rows at 0, 90 and 80 degrees; centroids start on rows 0 and 1
    x = np.array([[3.0, 0.0], [0.0, 2.0], [np.cos(np.radians(80.0)), np.sin(np.radians(80.0))]])
    init = x[:2]
    # pass 1: row 2 is 10 degrees from centroid 1 and 80 from centroid 0 -> labels [0, 1, 1], changed = n = 3; update: centroid 1 moves to 85
    # degrees (the bisector of two unit rows).  pass 2: the same labels, changed = 0: converged after 2 iterations, no empty cluster
    c, labels, sim, info = R.fit(x, init, 10)
    assert labels.tolist() == [0, 1, 1] and info == [2, 0, 0, 0]
    assert np.allclose(c, [[1.0, 0.0], [np.cos(np.radians(85.0)), np.sin(np.radians(85.0))]], atol=1e-15)
    assert np.allclose(sim, [1.0, np.cos(np.radians(5.0)), np.cos(np.radians(5.0))], atol=1e-15)
    # max_iter = 1: one assignment and one update, not converged
    c1, labels1, sim1, info1 = R.fit(x, init, 1)
    assert labels1.tolist() == [0, 1, 1] and info1 == [1, 3, 0, 0] and np.allclose(c1, c, atol=1e-15)
    assert np.allclose(sim1, [1.0, 1.0, np.cos(np.radians(10.0))], atol=1e-15)   # against the initial centroids
    # duplicate initial centroids: the tie goes to the lower one, the higher one stays empty and keeps its (normalised) start
    # (both point away from every row, so after the update centroid 0 is nearer to all of them)
    c, labels, _, info = R.fit(x, np.array([[0.0, -2.0], [0.0, -2.0]]), 10)
    assert labels.tolist() == [0, 0, 0] and info == [2, 0, 1, 0] and c[1].tolist() == [0.0, -1.0]


def test_reference_contingency_counts_pairs():
    t = R.contingency([0, 1, 1, 2, 1], [1, 0, 0, 1, 1], 3, 2)
    assert t.tolist() == [[0, 1], [2, 1], [0, 1]] and t.dtype == np.int64


# ---------------------------------------------------------------------------- the scores
def labelings():
    rng = np.random.default_rng(7)
    for classes, clusters in [(2, 1), (2, 2), (3, 5), (7, 7), (7, 40), (33, 33), (33, 17), (12, 1), (6, 6), (2, 40)]:
        n = int(rng.integers(50, 400))
        yield rng.integers(0, classes, n), rng.integers(0, clusters, n), classes, clusters
    y = np.repeat(np.arange(5), 20)
    yield y, (y + 2) % 5, 5, 5                                                   # a perfect clustering under another numbering
    yield y, y // 2, 5, 3                                                        # classes merged
    yield np.zeros(30, dtype=np.int64), np.zeros(30, dtype=np.int64), 2, 3       # one class, one cluster: both 1.0
    yield np.zeros(30, dtype=np.int64), np.arange(30) % 3, 2, 3                  # one class, three clusters
    yield np.arange(30) % 2, np.zeros(30, dtype=np.int64), 2, 1                  # two classes, one cluster
    yield np.arange(12), np.arange(12), 12, 12                                   # every row its own group


def test_scores_equal_scikit_learn_on_random_and_degenerate_labelings():
    from sklearn.metrics import adjusted_rand_score, normalized_mutual_info_score
    for y, k, classes, clusters in labelings():
        table = R.contingency(k, y, clusters, classes)
        nmi, ari = normalized_mutual_info_score(y, k), adjusted_rand_score(y, k)
        for got in (R.scores(table), clustering_scores(table)):
            assert abs(got["nmi"] - nmi) < 1e-12 and abs(got["ari"] - ari) < 1e-12, (classes, clusters, got, nmi, ari)
        a, b = R.scores(table), clustering_scores(table)
        assert a["purity"] == b["purity"] and ("accuracy" not in a or a["accuracy"] == b["accuracy"])
    one = clustering_scores([[30]])
    assert one["nmi"] == 1.0 and one["ari"] == 1.0 and one["purity"] == 1.0 and one["accuracy"] == 1.0
    with pytest.raises(ValueError):
        clustering_scores(np.zeros((3, 3), dtype=np.int64))


def test_accuracy_equals_a_brute_force_matching():
    rng = np.random.default_rng(11)
    for clusters, classes in [(1, 1), (2, 2), (3, 3), (4, 6), (6, 4), (5, 5), (6, 6), (2, 7)]:
        table = rng.integers(0, 30, (clusters, classes))
        table[0, 0] += 1
        small = table if clusters <= classes else table.T
        best = max(sum(int(small[i, p[i]]) for i in range(small.shape[0])) for p in itertools.permutations(range(small.shape[1]), small.shape[0]))
        assert clustering_scores(table)["accuracy"] == best / int(table.sum())
        assert R.scores(table)["accuracy"] == best / int(table.sum())
    assert clustering_scores([[0, 9], [8, 1]])["accuracy"] == 17 / 18            # clusters and classes numbered differently


# ---------------------------------------------------------------------------- the C ABI
def test_symbols_are_declared_bound_and_exported():
    assert ops.KMEANS_MAX_CLUSTERS == 1024
    assert ops.KMeansFit._fields == ("centroids", "labels", "sim", "n_iter", "converged", "empty")


def test_workspace_holds_no_matrix_and_is_zero_out_of_range():
    ws = L.lib().gmp_kmeans_workspace_bytes
    n, kc, d = 1 << 20, 1024, 256
    assert 0 < ws(n, kc, d) < 4 * (n + kc) * d + 64 * n + (1 << 20) < 4 * n * kc
    for n, kc, d in [(1, 1, 1), (5, 3, 6), (3, 1024, 256), (2708, 7, 256), (2500, 64, 40), (19717, 64, 256), (65535, 1024, 256), (1 << 20, 7, 130)]:
        dpad = (d + 3) // 4 * 4
        a, b = ws(n, kc, d), ws(2 * n, kc, d)
        assert 0 < a <= b <= 2 * a, (n, kc, d, a, b)
        # the normalised rows and centroids, the cluster sums, the sorted row list, the counts per chunk of 256 rows, a constant
        assert a <= 4 * (n + 2 * kc) * dpad + 4 * n + 4 * kc * -(-n // 256) + 8 * kc + 4096, (n, kc, d, a)
    for bad in [(-1, 5, 8), (1 << 31, 5, 8), (5, 0, 8), (5, -1, 8), (5, 1025, 8), (5, 5, 0), (5, 5, 257), (5, 5, -3)]:
        assert ws(*bad) == 0


def assign_call(x=0x1000, n=9, c=0x2000, kc=3, dim=8, labels=0x3000, sim=0x4000, mat=0, ws=0x5000, ws_bytes=1 << 20):
    """the pointers are never dereferenced by the host and nothing is launched on a refused call"""
    vp = ctypes.c_void_p
    return L.lib().gmp_kmeans_assign(vp(x), n, vp(c), kc, dim, vp(labels), vp(sim), vp(mat), vp(ws), ws_bytes, None)


def fit_call(x=0x1000, n=9, init=0x2000, kc=3, dim=8, max_iter=5, c=0x6000, labels=0x3000, sim=0x4000, info=0x7000, ws=0x5000, ws_bytes=1 << 20):
    vp = ctypes.c_void_p
    return L.lib().gmp_kmeans_fit(vp(x), n, vp(init), kc, dim, max_iter, vp(c), vp(labels), vp(sim), vp(info), vp(ws), ws_bytes, None)


def contingency_call(a=0x1000, b=0x2000, n=9, na=3, nb=4, table=0x3000, status=0x4000):
    vp = ctypes.c_void_p
    return L.lib().gmp_contingency(vp(a), vp(b), n, na, nb, vp(table), vp(status), None)


@pytest.mark.parametrize("kw", [dict(kc=0), dict(kc=1025), dict(kc=-1), dict(dim=0), dict(dim=257), dict(n=-1), dict(n=1 << 31), dict(x=0),
                                dict(c=0), dict(labels=0), dict(sim=0)])
def test_assign_refuses_bad_sizes_and_null_pointers(kw):
    assert assign_call(**kw) == ERR_ARG
    assert b"kmeans_assign" in L.lib().gmp_last_error_string()


@pytest.mark.parametrize("kw", [dict(kc=0), dict(kc=1025), dict(dim=0), dict(dim=257), dict(n=-1), dict(n=1 << 31), dict(max_iter=0),
                                dict(max_iter=10001), dict(max_iter=-1), dict(x=0), dict(init=0), dict(c=0), dict(labels=0), dict(sim=0),
                                dict(info=0)])
def test_fit_refuses_bad_sizes_and_null_pointers(kw):
    assert fit_call(**kw) == ERR_ARG
    assert b"kmeans_fit" in L.lib().gmp_last_error_string()


@pytest.mark.parametrize("kw", [dict(n=-1), dict(n=1 << 31), dict(na=0), dict(na=1025), dict(nb=0), dict(nb=1025), dict(a=0), dict(b=0),
                                dict(table=0), dict(status=0)])
def test_contingency_refuses_bad_sizes_and_null_pointers(kw):
    assert contingency_call(**kw) == ERR_ARG
    assert b"contingency" in L.lib().gmp_last_error_string()


def test_a_short_workspace_is_refused_and_no_rows_is_a_no_op():
    need = L.lib().gmp_kmeans_workspace_bytes(9, 3, 8)
    assert assign_call(ws_bytes=need - 1) == ERR_WORKSPACE and assign_call(ws=0) == ERR_WORKSPACE
    assert fit_call(ws_bytes=need - 1) == ERR_WORKSPACE and fit_call(ws=0) == ERR_WORKSPACE
    assert b"kmeans_fit" in L.lib().gmp_last_error_string()
    assert assign_call(n=0, ws=0, ws_bytes=0) == 0 and fit_call(n=0, ws=0, ws_bytes=0) == 0 and contingency_call(n=0) == 0
