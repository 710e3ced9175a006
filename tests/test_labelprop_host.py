"""What the label-propagation baselines rest on, without a GPU: the fp32 definition of tests/labelprop_ref.py (which the kernel is pinned to
bit for bit in test_gpu_labelprop.py) against float64 and against the closed form, that it classifies a planted partition, that its
subnormal case is one, and the flag, the config field and the bindings."""
import functools

import numpy as np
import pytest
import torch

import labelprop_ref as R
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd.finetune import finetune as FT

ALPHA, BETA = R.ALPHA, R.BETA


@functools.lru_cache(maxsize=None)
def _planted():
    g, y, seeds = R.planted()
    return g, y, seeds, R.one_hot(g.n, R.PLANTED_CLASSES, seeds, y[seeds])


@functools.lru_cache(maxsize=None)
def _spread(rounds, wide=False):
    g, _, _, f0 = _planted()
    left, right = R.degree_scales(g.rowptr, "sym")
    return (R.propagate64 if wide else R.propagate)(g.rowptr, g.col, f0, rounds, ALPHA, BETA, left, right)


def _rounding_bound(F) -> float:
    """(d_max + 4) 2^-24 ||F||_2 / (1 - alpha): a row's sum takes deg adds and deg multiplies of products that are summed, the update
    four more roundings -- first order, (d_max + 4) u per round with u = 2^-24; ||S||_2 <= 1 for the symmetric scaling, and the map
    contracts by alpha, so the rounds' errors sum to at most 1 / (1 - alpha) of one round's."""
    g = _planted()[0]
    d_max = int((g.rowptr[1:] - g.rowptr[:-1]).max())
    return (d_max + 4) * 2.0 ** -24 * float(np.linalg.norm(F)) / (1.0 - float(ALPHA))


def test_the_planted_graph_is_what_the_tests_assume():
    g, y, seeds, f0 = _planted()
    deg = g.rowptr[1:] - g.rowptr[:-1]
    assert g.n == 300 and deg[0] == 0 and 0 not in seeds and len(seeds) == 30 and f0.sum() == 30
    assert (deg[1:] > 0).sum() > 290 and np.array_equal(np.bincount(y), np.bincount(np.arange(300) % 7))


# ---------------------------------------------------------------------------- 1. fp32 against fp64
@pytest.mark.parametrize("rounds", [50, 200])
def test_fp32_definition_against_float64(rounds):
    got, want = _spread(rounds), _spread(rounds, wide=True)
    gap, bound = float(np.linalg.norm(got.out.astype(np.float64) - want.out)), _rounding_bound(want.out)
    print(f"T={rounds}: fp32 against fp64 {gap:.3e}, bound {bound:.3e}")
    assert gap <= bound
    assert np.array_equal(got.status, want.status)


# ---------------------------------------------------------------------------- 2. the closed form
def test_definition_converges_to_the_closed_form():
    """F* = (1 - alpha) (I - alpha S)^-1 Y by a dense float64 solve, S = D^-1/2 A D^-1/2 and alpha = 0.9 in float64 throughout (the
    iteration is given both rounded to fp32: a relative 2^-24 each, inside the bound).  After T rounds from F = Y the exact iteration is
    within alpha^T ||Y|| of it."""
    g, _, _, f0 = _planted()
    deg = (g.rowptr[1:] - g.rowptr[:-1]).astype(np.float64)
    A = np.zeros((g.n, g.n))
    A[np.repeat(np.arange(g.n), deg.astype(np.int64)), g.col] = 1.0
    s = np.where(deg > 0, 1.0 / np.sqrt(np.where(deg > 0, deg, 1.0)), 0.0)
    S = s[:, None] * A * s[None, :]
    alpha = 0.9
    closed = (1.0 - alpha) * np.linalg.solve(np.eye(g.n) - alpha * S, f0.astype(np.float64))
    got = _spread(200)
    gap = float(np.linalg.norm(got.out.astype(np.float64) - closed))
    bound = alpha ** 200 * float(np.linalg.norm(f0)) + _rounding_bound(closed)
    print(f"T=200 against the closed form {gap:.3e}, bound {bound:.3e}")
    assert gap <= bound


# ---------------------------------------------------------------------------- 3. it classifies
def test_both_baselines_score_well_above_chance_on_the_planted_graph():
    g, y, seeds, f0 = _planted()
    rest = np.setdiff1d(np.arange(g.n), seeds)
    spread = _spread(50)
    left, _ = R.degree_scales(g.rowptr, "rw")
    prop = R.propagate(g.rowptr, g.col, f0, 50, 1.0, 0.0, left, None, clamp=R.seed_mask(g.n, seeds))
    acc_s, acc_p = float((spread.pred[rest] == y[rest]).mean()), float((prop.pred[rest] == y[rest]).mean())
    print(f"label spreading {acc_s:.3f}, label propagation {acc_p:.3f}, chance {1 / 7:.3f}")
    assert acc_s > 0.5 and acc_p > 0.5
    assert np.array_equal(prop.out[seeds], f0[seeds])                                     # clamped rows stay at their labels
    assert not spread.out[0].any() and spread.pred[0] == 0 and spread.status[1] >= 1      # the isolated node: unreached, class 0 by the tie rule


# ---------------------------------------------------------------------------- 4. the subnormal case is one
def test_the_path_case_reaches_subnormals():
    g, f0, left, right, alpha, beta, rounds = R.subnormal_case()
    out = R.propagate(g.rowptr, g.col, f0, rounds, alpha, beta, left, right).out
    tiny = float(np.finfo(np.float32).tiny)
    positive = out[out > 0]
    print(f"smallest positive value {positive.min():.3e}, {int((positive < tiny).sum())} subnormal entries")
    assert positive.min() < tiny and (positive < tiny).sum() >= 2
    flushed = np.where(np.abs(out) < tiny, 0, out)
    assert not np.array_equal(flushed, out)                                              # a kernel that flushed them would differ


# ---------------------------------------------------------------------------- the reference's own conventions
def test_argmax_ties_go_to_the_lower_class_and_zero_rows_count_as_unreached():
    out = np.array([[0.5, 0.5, 0.1], [0.0, 0.0, 0.0], [0.1, 0.7, 0.7], [-1.0, -0.5, -0.5]], np.float32)
    assert R.argmax_rows(out).tolist() == [0, 0, 1, 1]
    g = R.empty(4)
    res = R.propagate(g.rowptr, g.col, out, 1, 0.0, 1.0)
    assert np.array_equal(res.out, out) and res.pred.tolist() == [0, 0, 1, 1] and res.status.tolist() == [0, 2]


def test_stray_columns_are_counted_and_skipped():
    g = R.random_graph(40, 4.0, 1)
    f0, f_init, left, right, clamp = R.random_inputs(40, 3, 2)
    s = R.with_stray_columns(g)
    assert s.col.size == g.col.size + 2 and s.col[s.rowptr[1]] == 40 and s.col[-1] == -1
    a = R.propagate(g.rowptr, g.col, f0, 3, 0.5, 0.5, left, right, clamp, f_init)
    b = R.propagate(s.rowptr, s.col, f0, 3, 0.5, 0.5, left, right, clamp, f_init)
    assert a.status[0] == 0 and b.status[0] == 2 and np.array_equal(a.out.view(np.uint32), b.out.view(np.uint32))


def test_chained_single_rounds_equal_one_call():
    g = R.random_graph(40, 4.0, 1)
    f0, f_init, left, right, clamp = R.random_inputs(40, 3, 2)
    whole = R.propagate(g.rowptr, g.col, f0, 4, 0.5, 0.5, left, right, clamp, f_init)
    f = f_init
    for t in range(4):
        step = R.propagate(g.rowptr, g.col, f0, 1, 0.5, 0.5, left, right, clamp, f)
        assert step.residual[0] == whole.residual[t]
        f = step.out
    assert np.array_equal(f.view(np.uint32), whole.out.view(np.uint32))


# ---------------------------------------------------------------------------- 5. flag and config
@pytest.mark.parametrize("bad", [-1, 10001])
def test_rounds_are_bounded(bad):
    assert (ops.LABELPROP_MAX_CLASSES, ops.LABELPROP_MAX_ROUNDS) == (32, 10000)
    with pytest.raises(ValueError, match="label_propagation"):
        FT.FinetuneConfig("Cora_NC", "full_finetune", "b1", 1, label_propagation=bad)


def test_host_tensors_are_refused():
    g = R.path(5)
    with pytest.raises(L.GnnmpError, match="GPU"):
        ops.label_propagate(torch.from_numpy(g.rowptr), torch.from_numpy(g.col), torch.zeros(5, 2), 1, 0.5, 0.5)
    from gnn_pretraining_amd.finetune import node_baselines as NB
    with pytest.raises(L.GnnmpError, match="GPU"):
        NB.label_spreading(torch.from_numpy(g.edges), 5, torch.tensor([0]), torch.tensor([0]), 2)
    with pytest.raises(ValueError, match="kind"):
        NB.degree_scales(torch.from_numpy(g.rowptr), "gcn")


def test_degree_scales_follow_the_host_rule():
    from gnn_pretraining_amd.finetune import node_baselines as NB
    g = R.planted()[0]
    for kind in ("sym", "rw"):
        got, want = NB.degree_scales(torch.from_numpy(g.rowptr), kind), R.degree_scales(g.rowptr, kind)
        assert got[0].dtype == torch.float32 and np.array_equal(got[0].numpy().view(np.uint32), want[0].view(np.uint32))
        assert (got[1] is None) == (want[1] is None) and got[0][0] == 0                    # the isolated node scales to zero, not to inf
    d = np.array([0, 3, 7, 16], np.int32)
    sym = NB.degree_scales(torch.from_numpy(np.concatenate([[0], np.cumsum(d)]).astype(np.int32)), "sym")[0].numpy()
    assert sym.tolist() == [0.0, np.float32(1 / np.sqrt(3.0)), np.float32(1 / np.sqrt(7.0)), 0.25]
