"""What the SGC and raw-feature baselines rest on, without a GPU: the fp32 definition of tests/sgc_ref.py (which the kernel is pinned to bit
for bit in test_gpu_sgc.py) is consistent between its dense and its CSR form, the fixture of the fit has the margins the GPU test relies
on, sgc_graph follows the host rule, and the flag, the config field and the bindings."""

import numpy as np
import pytest
import torch

import labelprop_ref as LP
import sgc_ref as R
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd.finetune import finetune as FT, node_baselines as NB



def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---------------------------------------------------------------------------- 1. the reference agrees with itself
@pytest.mark.parametrize("rounds", [1, 3])
def test_csr_reference_has_the_bits_of_the_dense_reference(rounds):
    g = R.random_graph(60, 4.0, 2)
    d = 37
    xr, xc, xv = R.sparse_features(g.n, d, 3, density=0.1)
    assert (xv == 0).sum() >= 5 and xr[4] == xr[3] and xv.size > 100             # explicit zeros are stored, one row is empty
    rng = np.random.default_rng(4)
    left, right = rng.uniform(-1.0, 1.0, g.n).astype(np.float32), rng.uniform(-1.0, 1.0, g.n).astype(np.float32)   # negative scales: -0 terms
    dense = R.propagate(g.rowptr, g.col, R.to_dense(xr, xc, xv, g.n, d), rounds, left, right)
    sparse = R.propagate_csr(g.rowptr, g.col, xr, xc, xv, d, rounds, left, right)
    assert np.array_equal(_bits(dense.out), _bits(sparse.out)) and sparse.status.tolist() == [0, 0]


def test_csr_reference_skips_and_counts_malformed_entries():
    g = R.random_graph(60, 4.0, 2)
    d = 37
    xr, xc, xv = R.sparse_features(g.n, d, 3, density=0.1)
    bad, at = R.with_bad_feature_entries(xr, xc, xv, d)
    assert bad[at[0]] == d and bad[at[1]] == -1 and bad[at[2]] == bad[at[2] - 1]
    keep = np.ones(xc.size, bool)
    keep[at] = False
    counts = np.bincount(np.repeat(np.arange(g.n), np.diff(xr))[keep], minlength=g.n)
    without = R.propagate_csr(g.rowptr, g.col, np.concatenate([[0], np.cumsum(counts)]), xc[keep], xv[keep], d, 2)
    got = R.propagate_csr(g.rowptr, g.col, xr, bad, xv, d, 2)
    assert got.status.tolist() == [0, 3] and np.array_equal(_bits(got.out), _bits(without.out))


def test_reference_is_label_propagation_per_column():
    g = R.random_graph(50, 5.0, 6)
    f0, _, left, right, _ = LP.random_inputs(g.n, 5, 7)
    want = LP.propagate(g.rowptr, g.col, f0, 3, 1.0, 0.0, left, right)
    got = R.propagate(g.rowptr, g.col, f0, 3, left, right)
    assert np.array_equal(_bits(got.out), _bits(want.out))
    s = R.with_stray_columns(g)
    stray = R.propagate(s.rowptr, s.col, f0, 3, left, right)
    assert stray.status.tolist() == [2, 0] and np.array_equal(_bits(stray.out), _bits(got.out))


def test_degree_ladder_places_its_strays_and_both_references_skip_them():
    """The case of the GPU ladder tests: every degree 0 .. 23 (so 0, 7, 8, 9, 15, 16, 17), one stray column inside a full batch of 8 and
    one at the end of a tail.  Both references count the two and leave the bits of the same CSR without them."""
    s, g = LP.degree_ladder(), LP.degree_ladder(stray=False)
    n = LP.LADDER_N
    assert n == 24 and np.diff(g.rowptr).tolist() == list(range(n)) and ((g.col >= 0) & (g.col < n)).all()
    assert all((np.diff(g.col[g.rowptr[v]:g.rowptr[v + 1]]) > 0).all() for v in range(n))
    assert s.col[s.rowptr[12] + 3] == n and s.rowptr[13] - s.rowptr[12] == 13             # position 3 of 13: inside the full batch
    assert s.col[s.rowptr[18] - 1] == -1 and s.rowptr[18] - s.rowptr[17] == 18            # the last of 18: the tail after two batches
    keep = (s.col >= 0) & (s.col < n)
    assert (~keep).sum() == 2 and np.array_equal(s.col[keep], g.col)
    f0, f_init, left, right, clamp = LP.random_inputs(n, 5, 31)
    for rounds in (1, 3):
        a = LP.propagate(s.rowptr, s.col, f0, rounds, 0.75, 0.5, left, right, clamp, f_init)
        b = LP.propagate(g.rowptr, g.col, f0, rounds, 0.75, 0.5, left, right, clamp, f_init)
        assert a.status[0] == 2 and b.status[0] == 0 and np.array_equal(_bits(a.out), _bits(b.out)) and np.array_equal(a.pred, b.pred)
        a, b = R.propagate(s.rowptr, s.col, f0, rounds, left, right), R.propagate(g.rowptr, g.col, f0, rounds, left, right)
        assert a.status.tolist() == [2, 0] and b.status.tolist() == [0, 0] and np.array_equal(_bits(a.out), _bits(b.out))


# ---------------------------------------------------------------------------- 2. the fixture of the fit
def test_fixture_has_the_margins_the_gpu_test_relies_on():
    """The GPU test asks the fp32 fit for the fp64 reference's predictions and bounds every logit by half of the reference's smallest
    top-2 margin.  That is only a test while the margins are real: at least 0.05 at K = 0 and K = 2 (measured 0.196 and 0.090, against
    an fp32-to-fp64 logit deviation of 3e-4 for the numpy twin), and SGC has to beat the raw features (0.956 against 0.841)."""
    fx = R.fixture()
    assert fx.x.shape == (300, 45) and fx.x.dtype == np.float32 and len(fx.train) == 30 and len(fx.evaluate) == 270
    assert np.array_equal(fx.train, np.arange(3, 300, 10)) and not np.intersect1d(fx.train, fx.evaluate).size
    rng = np.random.default_rng(1)
    means = rng.standard_normal((7, 45))
    assert np.array_equal(fx.x, (means[fx.y] + 1.5 * rng.standard_normal((300, 45))).astype(np.float32))
    raw, sgc = R.reference_fit(0), R.reference_fit(2)
    raw32, sgc32 = R.reference_fit(0, np.float32), R.reference_fit(2, np.float32)
    gap = max(float(np.abs(a.logits - b.logits).max()) for a, b in ((raw, raw32), (sgc, sgc32)))
    print(f"margins {raw.margin:.3f} {sgc.margin:.3f}, accuracies {raw.accuracy:.3f} {sgc.accuracy:.3f}, fp32 against fp64 logits {gap:.1e}")
    assert raw.margin >= 0.05 and sgc.margin >= 0.05
    assert sgc.accuracy > raw.accuracy > 1.0 / 7
    assert gap < 0.5 * min(raw.margin, sgc.margin)
    assert np.array_equal(raw.pred, raw32.pred) and np.array_equal(sgc.pred, sgc32.pred)


def test_reference_fit_descends_and_is_torch_adam():
    """The written-out rule against torch.optim.Adam itself (float64, CPU) on the fixture's train rows."""
    fx = R.fixture()
    F, y = fx.x[fx.train].astype(np.float64), fx.y[fx.train]
    W, b, history = R.fit(np.float64, F, y, 7, iters=20)
    assert history[0] == pytest.approx(np.log(7.0)) and history[-1] < 0.2 * history[0]
    Ft, yt = torch.from_numpy(F), torch.from_numpy(y)
    Wt, bt = torch.zeros(7, 45, dtype=torch.float64, requires_grad=True), torch.zeros(7, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([Wt, bt], lr=R.LR)
    for _ in range(20):
        opt.zero_grad()
        (torch.nn.functional.cross_entropy(Ft @ Wt.T + bt, yt) + 0.5 * R.L2 * (Wt ** 2).sum()).backward()
        opt.step()
    assert np.allclose(W, Wt.detach().numpy(), rtol=0, atol=1e-9) and np.allclose(b, bt.detach().numpy(), rtol=0, atol=1e-9)


def test_adam_step_matches_the_reference_rule():
    rng = np.random.default_rng(0)
    p, m, v = (rng.standard_normal((3, 4)) for _ in range(3))
    v = np.abs(v)
    g = rng.standard_normal((3, 4))
    tp, tm, tv = (torch.from_numpy(a.copy()) for a in (p, m, v))
    NB.adam_step_(tp, torch.from_numpy(g), tm, tv, 3, 0.2)
    m2, v2 = R.BETA1 * m + (1 - R.BETA1) * g, R.BETA2 * v + (1 - R.BETA2) * g * g
    want = p - 0.2 / (1 - R.BETA1 ** 3) * m2 / (np.sqrt(v2) / (1 - R.BETA2 ** 3) ** 0.5 + R.EPS)
    assert np.allclose(tp.numpy(), want, rtol=0, atol=1e-12) and np.allclose(tm.numpy(), m2) and np.allclose(tv.numpy(), v2)
    assert (NB.ADAM_BETAS, NB.ADAM_EPS) == ((R.BETA1, R.BETA2), R.EPS)


# ---------------------------------------------------------------------------- 3. sgc_graph on the host
def test_sgc_graph_adds_one_loop_per_row_in_its_place():
    g = R.planted()[0]
    edges = torch.from_numpy(np.concatenate([g.edges, g.edges[:, :40][::-1], np.array([[5, 5], [9, 9]]).T], axis=1))   # duplicates, loops
    rowptr, col, scale = NB.sgc_graph(edges, g.n)
    want_rp, want_col, want_scale = R.sgc_graph(g)
    assert rowptr.dtype == torch.int32 and col.dtype == torch.int32 and scale.dtype == torch.float32
    assert np.array_equal(rowptr.numpy(), want_rp) and np.array_equal(col.numpy(), want_col)
    assert np.array_equal(_bits(scale.numpy()), _bits(want_scale))
    rp, cl = rowptr.numpy().astype(np.int64), col.numpy()
    assert np.array_equal(np.diff(rp), np.diff(g.rowptr.astype(np.int64)) + 1)
    for i in range(g.n):
        row = cl[rp[i]:rp[i + 1]]
        assert (np.diff(row) > 0).all() and (row == i).sum() == 1
    assert rp[1] - rp[0] == 1 and scale[0] == 1.0                                  # the isolated node keeps its own features
    deg = np.array([0, 2, 3, 15], np.int64)                                        # a star's hub and chain: 1 / sqrt(deg + 1) from float64
    e = [(3, v) for v in range(4, 19)] + [(1, 2), (1, 19), (2, 19), (2, 20)]
    _, _, s = NB.sgc_graph(torch.tensor(e, dtype=torch.int64).T.contiguous(), 21)
    assert s[:4].tolist() == [np.float32(1 / np.sqrt(d + 1.0)) for d in deg] and s[3] == 0.25
    empty_rp, empty_col, empty_s = NB.sgc_graph(torch.zeros(2, 0, dtype=torch.int64), 3)
    assert empty_rp.tolist() == [0, 1, 2, 3] and empty_col.tolist() == [0, 1, 2] and empty_s.tolist() == [1.0, 1.0, 1.0]
    with pytest.raises(L.GnnmpError, match="outside"):
        NB.sgc_graph(torch.tensor([[0], [3]]), 3)


# ---------------------------------------------------------------------------- 4. flag and config
@pytest.mark.parametrize("bad", [-1, 65])
def test_rounds_are_bounded(bad):
    assert (ops.FEATPROP_MAX_DIM, ops.FEATPROP_MAX_ROUNDS) == (16384, 64)
    with pytest.raises(ValueError, match="sgc_baseline"):
        FT.FinetuneConfig("Cora_NC", "full_finetune", "b1", 1, sgc_baseline=bad)


def test_host_tensors_are_refused():
    g = R.path(5)
    rp, cl = torch.from_numpy(g.rowptr), torch.from_numpy(g.col)
    with pytest.raises(L.GnnmpError, match="GPU"):
        ops.feature_propagate(rp, cl, torch.zeros(5, 2), 1)
    with pytest.raises(L.GnnmpError, match="GPU"):
        NB.sgc_features(torch.zeros(5, 2), torch.from_numpy(g.edges), 5, 2)
    with pytest.raises(L.GnnmpError, match="GPU"):
        NB.softmax_fit(torch.zeros(5, 2), torch.zeros(5, dtype=torch.int64), 2)
    assert ops.FeaturePropagation._fields == ("out", "status")
