"""Host-side contract of the linear-evaluation probe (csrc/logreg.hip): the fp64 reference of tests/logreg_ref.py against
torch.nn.functional.cross_entropy + torch.optim.Adam in float64, the blob cases of the GPU whole-fit test solved by the reference alone
(train accuracy 1.0 with a margin, so the GPU test may ask for every prediction), declaration / binding of the three C-ABI entry points,
a workspace without the n x classes matrix, and every bad call refused with its
error code before anything is launched (so this runs without a GPU)."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import logreg_ref as R
from gnn_pretraining_amd import _lib as L, ops

ERR_ARG, ERR_WORKSPACE = -1, -3


# ---------------------------------------------------------------------------- the reference against torch
@pytest.mark.parametrize("n,d,C,l2", [(50, 12, 5, 0.0), (64, 7, 2, 1e-2), (40, 33, 32, 1e-3)])
def test_reference_equals_torch_cross_entropy_and_adam_in_float64(n, d, C, l2):
    g = torch.Generator().manual_seed(n + C)
    x = torch.randn(n, d, generator=g, dtype=torch.float64)
    y = torch.randint(0, C, (n,), generator=g)
    W0, b0 = 0.3 * torch.randn(C, d, generator=g, dtype=torch.float64), 0.3 * torch.randn(C, generator=g, dtype=torch.float64)
    lr, iters = 0.01, 20
    xn = torch.nn.functional.normalize(x, dim=1, eps=1e-12)
    W, b = W0.clone().requires_grad_(True), b0.clone().requires_grad_(True)
    # the ridge term as weight decay: (l2 / 2) sum(W^2) has gradient l2 W; the bias's group carries none
    opt = torch.optim.Adam([{"params": [W], "weight_decay": l2}, {"params": [b], "weight_decay": 0.0}], lr=lr)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        ce = torch.nn.functional.cross_entropy(xn @ W.T + b, y)
        losses.append(float(ce.detach()) + 0.5 * l2 * float((W.detach() ** 2).sum()))
        ce.backward()
        opt.step()
    zero = np.zeros((C, d + 1))
    Wr, br, m, v, t, hist = R.fit(x.numpy(), y.numpy(), C, iters, lr, l2, state=(W0.numpy(), b0.numpy(), zero, zero, 0))
    assert t == iters
    assert float(np.abs(Wr - W.detach().numpy()).max()) < 1e-12 and float(np.abs(br - b.detach().numpy()).max()) < 1e-12
    assert float(np.abs(hist - np.array(losses)).max()) < 1e-12


def test_reference_by_hand():
    # two classes, zero parameters: p = 1/2 everywhere, L = log 2, g = (1/2 - onehot) averaged
    xn = np.array([[1.0, 0.0], [0.0, 1.0]])
    L0, g, status = R.loss_grad(xn, np.array([0, 1]), np.zeros((2, 2)), np.zeros(2))
    assert abs(L0 - np.log(2.0)) < 1e-15 and status == 0
    assert np.allclose(g, [[-0.25, 0.25, 0.0], [0.25, -0.25, 0.0]], atol=1e-15)
    # a label out of range contributes nothing, n stays n; the ridge term is on W alone
    L1, g1, status = R.loss_grad(xn, np.array([0, 7]), np.zeros((2, 2)), np.zeros(2))
    assert status == 1 and abs(L1 - np.log(2.0) / 2) < 1e-15 and np.allclose(g1, [[-0.25, 0.0, -0.25], [0.25, 0.0, 0.25]], atol=1e-15)
    W = np.array([[1.0, 2.0], [3.0, 4.0]])
    La, ga, _ = R.loss_grad(xn, np.array([0, 1]), W, np.array([5.0, 6.0]), 0.0)
    Lb, gb, _ = R.loss_grad(xn, np.array([0, 1]), W, np.array([5.0, 6.0]), 0.5)
    assert abs((Lb - La) - 0.25 * 30.0) < 1e-12 and np.allclose(gb - ga, np.concatenate([0.5 * W, np.zeros((2, 1))], axis=1), atol=1e-15)
    # Adam's first step from zero moments moves every entry by lr against the gradient's sign
    theta, m, v = R.adam_step(np.zeros(3), np.array([2.0, -0.5, 1e-3]), np.zeros(3), np.zeros(3), 1, 0.01)
    assert np.allclose(theta, [-0.01, 0.01, -0.01], rtol=1e-4) and np.allclose(m, [0.2, -0.05, 1e-4]) and np.allclose(v, [4e-3, 2.5e-4, 1e-9])
    # ties to the lower class; a zero row scores b alone
    pred, z = R.predict(np.array([[0.0, 0.0], [3.0, 0.0]]), np.array([[1.0, 0.0], [1.0, 0.0], [0.0, 1.0]]), np.array([0.5, 0.5, 0.25]))
    assert pred.tolist() == [0, 0] and z[0].tolist() == [0.5, 0.5, 0.25] and z[1].tolist() == [1.5, 1.5, 0.25]


# ---------------------------------------------------------------------------- the blob cases of the GPU whole-fit test
@functools.lru_cache(maxsize=None)
def _blob_fit(i):
    n, d, C, noise = R.BLOB_CASES[i]
    x, y = R.blobs(n, d, C, noise)
    return x, y, R.fit(x, y, C, 100, 0.01)


@pytest.mark.parametrize("i", range(len(R.BLOB_CASES)))
def test_reference_separates_the_blob_cases_with_a_margin(i):
    x, y, (W, b, _, _, t, hist) = _blob_fit(i)
    pred, z = R.predict(x, W, b)
    top = np.sort(z, axis=1)
    gap = float((top[:, -1] - top[:, -2]).min())
    print(f"{R.BLOB_CASES[i]}: smallest top-two logit gap {gap:.3f}, final loss {hist[-1]:.4f}")
    assert t == 100 and np.array_equal(pred, y)
    assert gap >= 0.5
    assert hist[-1] < hist[0] and abs(hist[0] - np.log(R.BLOB_CASES[i][2])) < 1e-12       # from zero: log C


# ---------------------------------------------------------------------------- declaration, binding, workspace, refusals
def test_the_three_entry_points_are_declared_and_bound():
    assert (ops.LOGREG_MAX_CLASSES, ops.LOGREG_MAX_DIM, ops.LOGREG_MAX_ITER) == (32, 256, 10000)
    assert ops.LogRegState._fields == ("weight", "bias", "exp_avg", "exp_avg_sq", "step")


def test_workspace_is_the_normalised_copy_and_a_bounded_block_of_partial_sums():
    l = L.lib()
    for n, C, d in [(1, 2, 1), (2708, 7, 256), (19717, 3, 256), (65535, 32, 256), (1 << 20, 32, 255), (300, 5, 6)]:
        dpad = (d + 3) // 4 * 4
        slot = (C * dpad + C + 2 + 63) // 64 * 64
        groups = min((n + 127) // 128, 256)
        got = l.gmp_logreg_workspace_bytes(n, C, d)
        want = 4 * n * dpad + 4 * groups * slot
        assert want <= got < want + 1024 + 512                      # (each of the two slices starts on 256 bytes)
        assert got < 4 * n * dpad + (9 << 20)                        # nothing of size n x classes: bounded beside the normalised copy
    for n, C, d in [(-1, 7, 8), (1 << 31, 7, 8), (10, 1, 8), (10, 33, 8), (10, 7, 0), (10, 7, 257)]:
        assert l.gmp_logreg_workspace_bytes(n, C, d) == 0


def test_bad_calls_are_refused_before_anything_is_launched():
    l = L.lib()
    buf = ctypes.create_string_buffer(1 << 16)                      # host memory: never dereferenced by a refused call
    q = ctypes.cast(buf, ctypes.c_void_p)

    def fit(n=10, C=7, d=8, iters=5, ws=q, ws_bytes=1 << 16, x=q, step=q):
        return l.gmp_logreg_fit(x, q, n, C, d, iters, 0.01, 0.0, q, q, q, q, step, q, q, None, None, ws, ws_bytes, None)

    def predict(n=10, C=7, d=8, ws=q, ws_bytes=1 << 16, pred=q):
        return l.gmp_logreg_predict(q, n, q, q, C, d, pred, None, ws, ws_bytes, None)

    for kw in (dict(C=1), dict(C=33), dict(d=0), dict(d=257), dict(n=-1), dict(n=1 << 31)):
        assert fit(**kw) == ERR_ARG and predict(**kw) == ERR_ARG
    for iters in (0, -3, 10001):
        assert fit(iters=iters) == ERR_ARG
    assert fit(x=None) == ERR_ARG and fit(step=None) == ERR_ARG and predict(pred=None) == ERR_ARG
    need = l.gmp_logreg_workspace_bytes(10, 7, 8)
    assert fit(ws_bytes=need - 1) == ERR_WORKSPACE and predict(ws_bytes=need - 1) == ERR_WORKSPACE
    assert fit(ws=None) == ERR_WORKSPACE and predict(ws=None) == ERR_WORKSPACE
    assert fit(n=0, ws=None, ws_bytes=0) == 0 and predict(n=0, ws=None, ws_bytes=0) == 0          # a no-op
    x = torch.zeros(4, 8)
    with pytest.raises(L.GnnmpError):
        ops.logreg_fit(x, torch.zeros(4, dtype=torch.int64), 3)      # CPU tensors: there is no fallback
    with pytest.raises(L.GnnmpError):
        ops.logreg_predict(x, torch.zeros(3, 8), torch.zeros(3))
