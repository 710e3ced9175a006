"""gmp_feature_propagate on the GPU (csrc/feature_prop.hip: ops.feature_propagate, finetune/node_baselines.py, --sgc-baseline) against the
fp32 definition of tests/sgc_ref.py.  A row's sum is sequential and every operation is rounded on its own, so every float output of the
propagation is compared for BIT EQUALITY and status exactly.  The fit is pinned to itself bit for bit and to the float64 reference by a
bound taken from the reference's own margins.  test_sgc_host.py holds the preconditions of the fixture."""
import ctypes as C

import numpy as np
import pytest
import torch

import labelprop_ref as LP
import sgc_ref as R
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd._lib import GnnmpError
from gnn_pretraining_amd.finetune import node_baselines as NB
from gnn_pretraining_amd.graph import SparseFeatures
from node_prop_util import DEV, SENTINEL, bits as _bits, run_cli as _run_cli, t as _t

pytestmark = pytest.mark.gpu
GMP_OK, GMP_ERR_ARG = 0, -1


def _gpu(g, x, rounds, left=None, right=None, out=None):
    return ops.feature_propagate(_t(g.rowptr, torch.int32), _t(g.col, torch.int32), _t(x), rounds, left=_t(left), right=_t(right), out=out)


def _check(g, x, rounds, left=None, right=None):
    got, want = _gpu(g, x, rounds, left, right), R.propagate(g.rowptr, g.col, x, rounds, left, right)
    assert got.out.dtype == torch.float32 and got.status.dtype == torch.int32 and got.out.shape == want.out.shape
    assert np.array_equal(_bits(got.out), _bits(want.out)), (x.shape, rounds)
    assert np.array_equal(got.status.cpu().numpy(), want.status)
    return got


def _inputs(n, d, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((n, d)).astype(np.float32), rng.uniform(0.1, 1.0, n).astype(np.float32),
            rng.uniform(-1.0, 1.0, n).astype(np.float32))


def _sparse(xr, xc, xv, n, d):
    return SparseFeatures(_t(xr, torch.int32), _t(xc, torch.int32), _t(xv), (n, d))


# ---------------------------------------------------------------------------- 1. bit for bit against the definition
@pytest.mark.parametrize("d", [1, 3, 33, 256, 257, 261, 1030])
def test_widths_and_rounds(d):
    """Strip boundaries (256 | 257), a 6-column tail (1030 = 4 * 256 + 6), widths that are no multiple of 4; zero, one and two workspace
    buffers (rounds 1, 2, 3 and 5)."""
    g = R.random_graph(300, 4.0, 100 + d)
    x, left, right = _inputs(g.n, d, d)
    for rounds in (1, 2, 3, 5):
        _check(g, x, rounds, left, right)
    _check(g, x, 2)                                                                       # no scales
    _check(g, x, 1, left, None)
    _check(g, x, 1, None, right)


def test_star_path_empty_and_single_node():
    g = R.star(300, 5)
    assert g.rowptr[1] - g.rowptr[0] == 300                                               # 37 unrolled chunks and a tail of 4
    for d in (33, 261):
        x, left, right = _inputs(g.n, d, 3)
        _check(g, x, 3, left, right)
    rowptr, col, scale = R.sgc_graph(g)                                                   # with self-loops: a tail of 5
    _check(R.Graph(g.n, rowptr, col, g.edges), _inputs(g.n, 7, 4)[0], 2, scale, scale)
    x, left, right = _inputs(80, 257, 5)
    _check(R.path(80), x, 5, left, right)
    x, left, right = _inputs(70, 33, 6)
    got = _check(R.empty(70), x, 2, left, right)
    assert not got.out.any() and got.status.tolist() == [0, 0]
    for d in (1, 261):
        x, left, right = _inputs(1, d, 7)
        assert not _check(R.empty(1), x, 3, left, right).out.any()
        loop = R.Graph(1, np.array([0, 1], np.int32), np.array([0], np.int32), np.zeros((2, 0), np.int64))
        assert _check(loop, x, 3, left, right).out.any()


def test_strided_input_and_output_leave_the_padding_alone():
    g = R.random_graph(300, 4.0, 8)
    for d, ldx, ldo in ((261, 266, 263), (33, 36, 33), (3, 5, 8)):
        x, left, right = _inputs(g.n, d, d)
        wide = torch.full((g.n, ldx), 3.0, device=DEV)
        wide[:, :d] = _t(x)
        keep = wide.clone()
        for rounds in (1, 3):
            store = torch.full((g.n, ldo), SENTINEL, device=DEV)
            got = _gpu(g, wide[:, :d], rounds, left, right, out=store[:, :d])
            want = R.propagate(g.rowptr, g.col, x, rounds, left, right)
            assert got.out.data_ptr() == store.data_ptr() and np.array_equal(_bits(store[:, :d].contiguous()), _bits(want.out))
            assert bool((store[:, d:] == SENTINEL).all()) and torch.equal(wide, keep)


@pytest.mark.parametrize("d", [1, 7, 32])
def test_same_bits_as_label_propagate(d):
    g = R.random_graph(300, 4.0, 20 + d)
    x, left, right = _inputs(g.n, d, 30 + d)
    rp, cl = _t(g.rowptr, torch.int32), _t(g.col, torch.int32)
    for rounds in (1, 4):
        want = ops.label_propagate(rp, cl, _t(x), rounds, 1.0, 0.0, left=_t(left), right=_t(right))
        got = ops.feature_propagate(rp, cl, _t(x), rounds, left=_t(left), right=_t(right))
        assert torch.equal(got.out.view(torch.int32), want.out.view(torch.int32))
        assert int(got.status[0]) == int(want.status[0]) == 0


@pytest.mark.parametrize("rounds", [1, 3])
@pytest.mark.parametrize("d", [5, 257])
def test_degree_ladder_with_strays_inside_a_batch_and_in_a_tail(d, rounds):
    """labelprop_ref.degree_ladder: degrees 0 .. 23 with col = n at position 3 of row 12 (inside its full batch of 8) and col = -1 as the
    last entry of row 17 (its tail), on dense and on CSR features; at d = 5 the columns are label_propagate's with alpha 1, beta 0."""
    s = LP.degree_ladder()
    x, _, left, right, _ = LP.random_inputs(s.n, d, 31)
    got = _check(s, x, rounds, left, right)
    assert got.status.tolist() == [2, 0]
    xr, xc, xv = R.sparse_features(s.n, d, 32, density=0.3)
    sparse = _gpu(s, _sparse(xr, xc, xv, s.n, d), rounds, left, right)
    want = R.propagate_csr(s.rowptr, s.col, xr, xc, xv, d, rounds, left, right)
    assert np.array_equal(_bits(sparse.out), _bits(want.out)) and np.array_equal(sparse.status.cpu().numpy(), want.status)
    assert want.status.tolist() == [2, 0]
    if d == 5:
        label = ops.label_propagate(_t(s.rowptr, torch.int32), _t(s.col, torch.int32), _t(x), rounds, 1.0, 0.0, left=_t(left), right=_t(right))
        assert torch.equal(got.out.view(torch.int32), label.out.view(torch.int32)) and int(label.status[0]) == 2


# ---------------------------------------------------------------------------- 2. CSR features
@pytest.mark.parametrize("d", [45, 261, 1030])
def test_csr_features_have_the_bits_of_the_dense_call(d):
    g = R.random_graph(300, 4.0, 40 + d)
    xr, xc, xv = R.sparse_features(g.n, d, d)
    assert (xv == 0).sum() >= 1 and xr[4] == xr[3]                                        # stored zeros, an empty feature row
    _, left, right = _inputs(g.n, d, d)
    x = _sparse(xr, xc, xv, g.n, d)
    dense = x.to_dense()
    assert np.array_equal(_bits(dense), _bits(R.to_dense(xr, xc, xv, g.n, d)))
    for rounds in (1, 3):
        got = _gpu(g, x, rounds, left, right)
        want = _gpu(g, dense, rounds, left, right)
        ref = R.propagate_csr(g.rowptr, g.col, xr, xc, xv, d, rounds, left, right)
        assert torch.equal(got.out.view(torch.int32), want.out.view(torch.int32)) and got.status.tolist() == [0, 0]
        assert np.array_equal(_bits(got.out), _bits(ref.out))


def test_csr_features_with_long_rows_and_a_hub():
    """Feature rows of more than 64 entries (a second pass of the lanes over one neighbour) under the star's hub (unrolled neighbours)."""
    g = R.star(300, 5)
    xr, xc, xv = R.sparse_features(g.n, 261, 9, density=0.4)
    assert np.diff(xr).max() > 64
    _, left, right = _inputs(g.n, 261, 9)
    got = _gpu(g, _sparse(xr, xc, xv, g.n, 261), 2, left, right)
    want = _gpu(g, R.to_dense(xr, xc, xv, g.n, 261), 2, left, right)
    assert torch.equal(got.out.view(torch.int32), want.out.view(torch.int32)) and got.status.tolist() == [0, 0]


def test_malformed_feature_entries_are_skipped_and_counted():
    g = R.random_graph(300, 4.0, 11)
    d = 261
    xr, xc, xv = R.sparse_features(g.n, d, 12)
    bad, at = R.with_bad_feature_entries(xr, xc, xv, d)
    assert bad[at[0]] == d and bad[at[1]] == -1 and bad[at[2]] == bad[at[2] - 1]
    _, left, right = _inputs(g.n, d, 13)
    for rounds in (1, 3):
        got = _gpu(g, _sparse(xr, bad, xv, g.n, d), rounds, left, right)
        want = R.propagate_csr(g.rowptr, g.col, xr, bad, xv, d, rounds, left, right)
        assert want.status.tolist() == [0, 3] and got.status.tolist() == [0, 3]
        assert np.array_equal(_bits(got.out), _bits(want.out))


# ---------------------------------------------------------------------------- 3. status[0], subnormals
@pytest.mark.parametrize("rounds", [1, 3])
def test_stray_columns_are_counted_once_and_skipped(rounds):
    g = R.random_graph(300, 4.0, 14)
    s = R.with_stray_columns(g)
    for d in (7, 261):
        x, left, right = _inputs(g.n, d, 15)
        want = R.propagate(g.rowptr, g.col, x, rounds, left, right)                       # the graph without them
        ref = R.propagate(s.rowptr, s.col, x, rounds, left, right)
        got = _gpu(s, x, rounds, left, right)
        assert ref.status.tolist() == [2, 0] and got.status.tolist() == [2, 0]
        assert np.array_equal(_bits(got.out), _bits(want.out))
    xr, xc, xv = R.sparse_features(g.n, 45, 16)
    got = _gpu(s, _sparse(xr, xc, xv, g.n, 45), rounds, left, right)
    want = R.propagate_csr(g.rowptr, g.col, xr, xc, xv, 45, rounds, left, right)
    assert got.status.tolist() == [2, 0] and np.array_equal(_bits(got.out), _bits(want.out))


def test_subnormals_are_kept():
    g, f0, left, right, alpha, beta, rounds = LP.subnormal_case()
    x = LP.propagate(g.rowptr, g.col, f0, rounds, alpha, beta, left, right).out           # the far entries are fp32 subnormals
    tiny = np.finfo(np.float32).tiny
    assert ((x > 0) & (x < tiny)).sum() >= 2
    out = _check(g, x, 2, left, right).out.cpu().numpy()
    assert ((out > 0) & (out < tiny)).sum() >= 2                                          # kept, not flushed: the denormal mode is part of the contract
    xr, xc, xv = np.arange(g.n + 1, dtype=np.int32), np.zeros(g.n, np.int32), x[:, 0].copy()
    got = _gpu(g, _sparse(xr, xc, xv, g.n, 1), 2, left, right)
    assert np.array_equal(_bits(got.out), _bits(out))


# ---------------------------------------------------------------------------- 4. determinism
def test_one_call_equals_chained_single_rounds_and_two_calls_agree():
    g = R.random_graph(300, 4.0, 17)
    d = 261
    x, left, right = _inputs(g.n, d, 18)
    xr, xc, xv = R.sparse_features(g.n, d, 19)
    for feats in (_t(x), _sparse(xr, xc, xv, g.n, d)):
        before = feats.val.clone() if isinstance(feats, SparseFeatures) else feats.clone()
        whole = _gpu(g, feats, 4, left, right)
        again = _gpu(g, feats, 4, left, right)
        assert torch.equal(whole.out.view(torch.int32), again.out.view(torch.int32)) and torch.equal(whole.status, again.status)
        h = feats
        for _ in range(4):
            h = _gpu(g, h, 1, left, right).out
        assert torch.equal(h.view(torch.int32), whole.out.view(torch.int32))
        assert torch.equal(before, feats.val if isinstance(feats, SparseFeatures) else feats)


# ---------------------------------------------------------------------------- 5. the error path
def test_errors_launch_nothing():
    g = R.random_graph(300, 4.0, 21)
    n, d = g.n, 33
    xh = _inputs(n, d, 22)[0]
    rp, cl, x = _t(g.rowptr, torch.int32), _t(g.col, torch.int32), _t(xh)
    xr, xc, xv = (_t(a) for a in R.sparse_features(n, d, 23))
    out = torch.full((n, d), SENTINEL, device=DEV)
    status = torch.full((2,), int(SENTINEL), dtype=torch.int32, device=DEV)
    need = L.lib().gmp_feature_propagate_workspace_bytes(n, d, 3)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())                   # noqa: E731

    def call(x_=x, csr=(None, None, None), d_=d, rounds=3, out_=out, ldx=d, ldo=d, ws_=ws, ws_bytes=need, n_=n, status_=status, rp_=rp):
        return L.lib().gmp_feature_propagate(p(rp_), p(cl), n_, cl.numel(), None, None, p(x_), ldx, p(csr[0]), p(csr[1]), p(csr[2]),
                                             0 if csr[2] is None else csr[2].numel(), d_, rounds, p(out_), ldo, p(status_), p(ws_), ws_bytes, None)

    for rc in (call(d_=0), call(d_=16385), call(rounds=0), call(rounds=65), call(csr=(xr, xc, xv)), call(x_=None), call(out_=x),
               call(ldx=d - 1), call(ldo=d - 1), call(ws_bytes=need - 1), call(ws_=None), call(out_=ws.view(torch.float32)), call(n_=-1),
               call(n_=2 ** 31), call(rp_=None), call(out_=None), call(status_=None), call(x_=None, csr=(xr, None, xv))):
        assert rc == GMP_ERR_ARG
    assert "feature_propagate" in L.lib().gmp_last_error_string().decode()
    assert call(n_=0) == GMP_OK                                                           # nothing to do, nothing written
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and bool((status == int(SENTINEL)).all()) and torch.equal(x.cpu(), torch.from_numpy(xh))
    with pytest.raises(GnnmpError, match="d=0"):
        ops.feature_propagate(rp, cl, torch.zeros(n, 0, device=DEV), 1)
    with pytest.raises(GnnmpError, match="d=16385"):
        ops.feature_propagate(rp, cl, torch.zeros(n, 16385, device=DEV), 1)
    for rounds in (0, 65):
        with pytest.raises(GnnmpError, match="rounds"):
            ops.feature_propagate(rp, cl, x, rounds, out=out)
    with pytest.raises(GnnmpError, match="overlaps"):
        ops.feature_propagate(rp, cl, x, 2, out=x)
    with pytest.raises(GnnmpError, match="float32"):
        ops.feature_propagate(rp, cl, x.double(), 1, out=out)
    with pytest.raises(GnnmpError, match="int32"):
        ops.feature_propagate(rp.long(), cl, x, 1, out=out)
    with pytest.raises(GnnmpError, match="GPU"):
        ops.feature_propagate(rp, cl, x.cpu(), 1, out=out)
    with pytest.raises(GnnmpError, match="GPU"):
        ops.feature_propagate(rp, cl, x, 1, left=torch.ones(n), out=out)
    with pytest.raises(GnnmpError, match="left has"):
        ops.feature_propagate(rp, cl, x, 1, left=torch.ones(n - 1, device=DEV), out=out)
    with pytest.raises(GnnmpError, match="dense fp32 tensor or SparseFeatures"):
        ops.feature_propagate(rp, cl, None, 1, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all()) and torch.equal(x.cpu(), torch.from_numpy(xh))
    assert call() == GMP_OK and call(rounds=1, ws_=None, ws_bytes=0) == GMP_OK            # and the same arguments, unbroken, run
    assert call(x_=None, csr=(xr, xc, xv), rounds=1, ws_=None, ws_bytes=0) == GMP_OK      # one round from CSR features needs no workspace
    torch.cuda.synchronize()
    assert status.cpu().tolist() == [0, 0] and not bool((out == SENTINEL).any())
    none = ops.feature_propagate(torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV),
                                 torch.zeros(0, 4, device=DEV), 2)
    assert none.out.shape == (0, 4) and none.status.tolist() == [0, 0]


# ---------------------------------------------------------------------------- 6. the fit
def _hand_rolled_fit(F, y, classes, iters, lr=R.LR, l2=R.L2):
    """softmax_fit written out once more from the same operations."""
    m, d = F.shape
    W, b = torch.zeros(classes, d, device=DEV), torch.zeros(classes, device=DEV)
    mW, vW, mb, vb = torch.zeros_like(W), torch.zeros_like(W), torch.zeros_like(b), torch.zeros_like(b)
    g_scale = torch.full((1,), 1.0 / m, device=DEV)
    losses = []
    for t in range(1, iters + 1):
        logits = ops.gemm(ops.NT, F, W, bias=b)
        losses.append(ops.cross_entropy_sum_fwd(logits, y) * g_scale)
        G = ops.cross_entropy_sum_bwd(logits, y, g_scale)
        gW = ops.gemm(ops.TN, G, F).add_(W, alpha=l2)
        gb = ops.colsum(G)
        for param, grad, mm, vv in ((W, gW, mW, vW), (b, gb, mb, vb)):
            mm.mul_(R.BETA1).add_(grad, alpha=1.0 - R.BETA1)
            vv.mul_(R.BETA2).addcmul_(grad, grad, value=1.0 - R.BETA2)
            denom = (vv.sqrt() / (1.0 - R.BETA2 ** t) ** 0.5).add_(R.EPS)
            param.addcdiv_(mm, denom, value=-(lr / (1.0 - R.BETA1 ** t)))
    return W, b, torch.cat(losses)


def test_softmax_fit_is_repeatable_and_is_the_written_out_loop():
    fx = R.fixture()
    F, y = _t(R.reference_fit(2).features[fx.train]), _t(fx.y[fx.train])
    a, b = NB.softmax_fit(F, y, 7, iters=12), NB.softmax_fit(F, y, 7, iters=12)
    hand = _hand_rolled_fit(F, y, 7, 12)
    for u, v, w in zip(a, b, hand):
        assert torch.equal(u.view(torch.int32), v.view(torch.int32)) and torch.equal(u.view(torch.int32), w.view(torch.int32))
    assert a[0].shape == (7, 45) and a[1].shape == (7,) and a[2].shape == (12,)
    assert float(a[2][0]) == pytest.approx(np.log(7.0), rel=1e-6) and float(a[2][-1]) < float(a[2][0])
    wide = torch.cat([F, F[:, :20]], dim=1)                                               # d = 65, two classes: other shapes of the same GEMMs
    two = NB.softmax_fit(wide, y % 2, 2, iters=3)
    assert two[0].shape == (2, 65) and torch.isfinite(two[0]).all() and float(two[2][-1]) < float(two[2][0])
    with pytest.raises(GnnmpError, match="classes"):
        NB.softmax_fit(F, y, 33)
    with pytest.raises(GnnmpError, match="label"):
        NB.softmax_fit(F, y, 6)


@pytest.mark.parametrize("rounds", [0, 2])
def test_softmax_fit_against_the_float64_reference(rounds):
    """The eval predictions equal the reference's, and every logit lies within half of the reference's own smallest top-2 margin of the
    fp64 logit: the distance at which a prediction could flip.  The bound comes from the reference (test_sgc_host.py asserts it is at
    least 0.025); nothing is tuned."""
    fx, ref = R.fixture(), R.reference_fit(rounds)
    feats = NB.sgc_features(_t(fx.x), _t(fx.graph.edges), fx.graph.n, rounds)
    assert np.array_equal(_bits(feats), _bits(ref.features))
    W, b, history = NB.softmax_fit(feats[_t(fx.train)], _t(fx.y[fx.train]), 7)
    logits = ops.gemm(ops.NT, feats[_t(fx.evaluate)], W, bias=b).cpu().numpy().astype(np.float64)
    gap, bound = float(np.abs(logits - ref.logits).max()), 0.5 * ref.margin
    print(f"K={rounds}: largest logit deviation {gap:.3e}, bound {bound:.3e}, final loss {float(history[-1]):.4f}")
    assert history.shape == (R.ITERS,) and gap <= bound
    assert np.array_equal(logits.argmax(axis=1), ref.pred)


# ---------------------------------------------------------------------------- 7. the baselines
class _Data:
    def __init__(self, g, y, x):
        self.edge_index, self.num_nodes, self.y, self.x = torch.from_numpy(g.edges), g.n, torch.from_numpy(y), x


def test_feature_baselines_on_the_fixture():
    fx = R.fixture()
    want = {"rawfeat_accuracy": R.reference_fit(0).accuracy, "sgc_accuracy": R.reference_fit(R.FIXTURE_ROUNDS).accuracy}
    dense = torch.from_numpy(fx.x)
    for x in (dense, SparseFeatures.from_dense(dense)):
        got = NB.feature_baselines(_Data(fx.graph, fx.y, x), torch.from_numpy(fx.train), torch.from_numpy(fx.evaluate), 7, R.FIXTURE_ROUNDS, device=DEV)
        print("feature_baselines", type(x).__name__, got)
        assert got == want and got["sgc_accuracy"] > got["rawfeat_accuracy"]
    rowptr, col, scale = NB.sgc_graph(_t(fx.graph.edges), fx.graph.n)
    ref = R.sgc_graph(fx.graph)
    assert scale.is_cuda and np.array_equal(rowptr.cpu().numpy(), ref[0]) and np.array_equal(col.cpu().numpy(), ref[1])
    assert np.array_equal(_bits(scale), _bits(ref[2]))


def test_feature_baselines_refuse_bad_indices_and_malformed_features():
    fx = R.fixture()
    ok, x = torch.from_numpy(fx.train), torch.from_numpy(fx.x)
    for train, evaluate in ((torch.tensor([0, fx.graph.n]), ok), (ok, torch.tensor([-1, 4]))):
        with pytest.raises(GnnmpError, match="outside"):
            NB.feature_baselines(_Data(fx.graph, fx.y, x), train, evaluate, 7, 2, device=DEV)
    with pytest.raises(ValueError, match="rounds"):
        NB.feature_baselines(_Data(fx.graph, fx.y, x), ok, ok, 7, 0, device=DEV)
    sp = SparseFeatures.from_dense(x)
    sp.col[5] = sp.col[4]                                                                 # a non-ascending pair (to_dense stays in bounds)
    with pytest.raises(GnnmpError, match="feature entries"):
        NB.feature_baselines(_Data(fx.graph, fx.y, sp), ok, ok, 7, 2, device=DEV)


# ---------------------------------------------------------------------------- 8. the command-line path
def test_cli_logs_the_two_keys_and_leaves_training_alone(tmp_path, monkeypatch):
    """python -m gnn_pretraining_amd.finetune.finetune ... --sgc-baseline 2, in process: one epoch on the synthetic Cora_NC stand-in.  The
    test record carries the two keys, equal to feature_baselines called directly on the same splits; every other key but the timing ones,
    and the checkpoint, are bit for bit those of the same run without the flag."""
    from gnn_pretraining_amd.constants import NUM_CLASSES
    from gnn_pretraining_amd.data.finetune_data_loaders import create_finetune_data_loader
    keys = ["test/rawfeat_accuracy", "test/sgc_accuracy"]
    rec1, state1 = _run_cli(tmp_path, monkeypatch, "with", ["--sgc-baseline", "2"])
    rec0, state0 = _run_cli(tmp_path, monkeypatch, "without", [])
    test1 = [r for r in rec1 if keys[0] in r]
    assert len(test1) == 1 and "test/accuracy" in test1[0] and all(k in test1[0] for k in keys)
    assert not any("sgc" in k or "rawfeat" in k for r in rec1 if r is not test1[0] for k in r)
    assert not any("sgc" in k or "rawfeat" in k for r in rec0 for k in r)
    sets = {sp: create_finetune_data_loader("Cora_NC", sp, -1, torch.Generator(), tmp_path / "data").dataset for sp in ("train", "test")}
    direct = NB.feature_baselines(sets["train"].data, sets["train"].indices, sets["test"].indices, NUM_CLASSES["Cora_NC"], 2, device=DEV)
    assert {k: test1[0][k] for k in keys} == {f"test/{k}": v for k, v in direct.items()}
    assert all(0.0 <= test1[0][k] <= 1.0 for k in keys)
    assert state1.keys() == state0.keys() and all(torch.equal(state1[k], state0[k]) for k in state1)
    for k, v in [r for r in rec0 if "test/accuracy" in r][0].items():
        assert "time" in k or test1[0][k] == v or (v != v and test1[0][k] != test1[0][k]), k
