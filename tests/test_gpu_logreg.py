"""The linear-evaluation probe (csrc/logreg.hip: ops.logreg_fit / ops.logreg_predict, metrics.linear_eval_probe, --logreg-probe) on the
GPU against the fp64 definition of tests/logreg_ref.py: (a) where the arithmetic is exact the gradient of the first iteration equals the
reference's bit for bit across every tile width and both sides of the 128-row tile edge; (b) on random rows logits, gradient and loss agree
with fp64; (c) the update is Adam on the kernel's own gradient; (d) one call of T iterations is T calls of one, repeatable, and the hooks
change nothing; (e) a whole fit separates the blob cases the reference separates with a margin; (f) the edges of the contract; (g) the
probe of metrics.py above them (finetune() with the probe on: tests/test_gpu_probes.py)."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

import knn_ref
import logreg_ref as R
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd._lib import GnnmpError
from gnn_pretraining_amd.finetune.metrics import linear_eval_probe

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _dev(a):
    return torch.as_tensor(a).to(DEV).contiguous()


def _np(t):
    return t.cpu().numpy()


def _state(W, b, m=None, v=None, step=0):
    C, d = W.shape
    zero = np.zeros((C, d + 1), dtype=np.float32)
    return ops.LogRegState(_dev(np.asarray(W, dtype=np.float32)), _dev(np.asarray(b, dtype=np.float32)), _dev(zero if m is None else m),
                           _dev(zero if v is None else v), torch.tensor([step], dtype=torch.int64, device=DEV))


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def _state_np(s):
    return [_np(t) for t in s]


def _random_state(C, d, g):
    W = torch.randn(C, d, generator=g)
    W = (W / W.norm(dim=1, keepdim=True)).numpy()                    # unit rows
    b = (2.0 * torch.rand(C, generator=g) - 1.0).numpy()
    return W, b


# ---------------------------------------------------------------------------- (a) exact arithmetic
EXACT_SHAPES = [(1, 8), (5, 6), (127, 16), (128, 32), (129, 40), (301, 100), (300, 256)]


@pytest.mark.parametrize("n,d", EXACT_SHAPES)
def test_first_gradient_is_bit_exact_on_four_ones_and_sixteen_sign_rows(n, d):
    for gen in (knn_ref.four_ones, knn_ref.sixteen_signs):
        if gen is knn_ref.sixteen_signs and d < 16:
            continue
        x = gen(n, d, n + d)
        xd, xn = _dev(x), R.normalize(x)
        for C in (2, 4, 8, 16, 32):
            for y in (np.arange(n) % C, np.full(n, C - 1)) if C == 4 else (np.arange(n) % C,):     # one case: all rows of one class
                fit = ops.logreg_fit(xd, _dev(y.astype(np.int64)), C, iters=1, return_grad=True)
                _, g64, _ = R.loss_grad(xn, y, np.zeros((C, d)), np.zeros(C))                       # (S64 / n: p = 1 / C, every sum exact)
                assert _same_bits(_np(fit.grad), g64.astype(np.float32))
                loss = float(fit.loss_history[0])
                assert abs(loss - math.log(C)) <= 2e-5 * math.log(C)
                assert int(fit.state.step) == 1


# ---------------------------------------------------------------------------- (b) random rows against fp64
RANDOM_SHAPES = [(300, 256, 7), (257, 40, 31), (500, 256, 32), (130, 100, 2)]


def _random_case(n, d, C):
    g = torch.Generator().manual_seed(n + d + C)
    x = torch.randn(n, d, generator=g).numpy()
    y = torch.randint(0, C, (n,), generator=g).numpy()
    W, b = _random_state(C, d, g)
    return x, y, W, b


@pytest.mark.parametrize("n,d,C", RANDOM_SHAPES)
def test_logits_gradient_and_loss_match_fp64_from_a_random_state(n, d, C):
    x, y, W, b = _random_case(n, d, C)
    for l2 in (0.0, 1e-2):
        fit = ops.logreg_fit(_dev(x), _dev(y), C, iters=1, l2=l2, state=_state(W, b), return_grad=True, return_logits=True)
        xn = R.normalize(x)
        L64, g64, _ = R.loss_grad(xn, y, W, b, l2)
        e_logit = float(np.abs(_np(fit.logits) - R.logits(xn, W, b)).max())
        e_grad = float(np.abs(_np(fit.grad) - g64).max())
        e_loss = abs(float(fit.loss_history[0]) - L64)
        print(f"{(n, d, C)} l2={l2}: max |logits - fp64| = {e_logit:.3e}, max |grad - fp64| = {e_grad:.3e}, |loss - fp64| = {e_loss:.3e}")
        assert e_logit < 1e-5
        assert e_grad < 2e-5
        assert e_loss < 2e-5


# ---------------------------------------------------------------------------- (c) the update on the kernel's own gradient
@pytest.mark.parametrize("n,d,C", [(300, 256, 7), (257, 40, 31)])
@pytest.mark.parametrize("step", [0, 7])
def test_update_is_adam_on_the_kernels_own_gradient(n, d, C, step):
    x, y, W, b = _random_case(n, d, C)
    g = torch.Generator().manual_seed(step + 1)
    lr, l2 = 0.01, 1e-3
    m = v = None
    if step:
        m = (1e-2 * torch.randn(C, d + 1, generator=g)).numpy()
        v = (1e-4 * torch.rand(C, d + 1, generator=g)).numpy()
    before = _state(W, b, m, v, step)
    kept = _state_np(before)
    fit = ops.logreg_fit(_dev(x), _dev(y), C, iters=1, lr=lr, l2=l2, state=before, return_grad=True)
    assert all(_same_bits(a, c) for a, c in zip(kept, _state_np(before)))                          # the caller's state is not written
    assert int(fit.state.step) == step + 1
    theta0 = np.concatenate([kept[0], kept[1][:, None]], axis=1)
    theta, m1, v1 = R.adam_step(theta0, _np(fit.grad), kept[2], kept[3], step + 1, lr)
    got = np.concatenate([_np(fit.state.weight), _np(fit.state.bias)[:, None]], axis=1)
    for name, have, want in (("theta", got, theta), ("exp_avg", _np(fit.state.exp_avg), m1), ("exp_avg_sq", _np(fit.state.exp_avg_sq), v1)):
        excess = float((np.abs(have - want) - 1e-6 * (np.abs(want) + lr)).max())
        print(f"{(n, d, C)} step {step} {name}: max |kernel - fp64 Adam| = {float(np.abs(have - want).max()):.3e}")
        assert excess <= 0.0


# ---------------------------------------------------------------------------- (d) chaining and repeatability
# (33000 rows are 258 tiles of 128: more than the 256 workgroups of the row pass, so some walk two tiles)
CHAIN_CASES = [(1000, 256, 7), (2500, 40, 32), (33000, 40, 32)]
CHAIN_STEPS = 6


@pytest.mark.parametrize("n,d,C", CHAIN_CASES)
def test_one_call_equals_chained_single_iterations_and_is_repeatable(n, d, C):
    g = torch.Generator().manual_seed(n + C)
    xd, yd = torch.randn(n, d, generator=g).to(DEV), torch.randint(0, C, (n,), generator=g).to(DEV)
    kw = dict(lr=0.01, l2=1e-3)
    whole = ops.logreg_fit(xd, yd, C, iters=CHAIN_STEPS, **kw)
    again = ops.logreg_fit(xd, yd, C, iters=CHAIN_STEPS, **kw)
    hooked = ops.logreg_fit(xd, yd, C, iters=CHAIN_STEPS, return_grad=True, return_logits=True, **kw)
    state, losses = None, []
    for _ in range(CHAIN_STEPS):
        one = ops.logreg_fit(xd, yd, C, iters=1, state=state, **kw)
        state = one.state
        losses.append(_np(one.loss_history))
    want = _state_np(whole.state) + [_np(whole.loss_history)]
    for other, hist in ((again.state, _np(again.loss_history)), (hooked.state, _np(hooked.loss_history)), (state, np.concatenate(losses))):
        for a, c in zip(want, _state_np(other) + [hist]):                                          # W, b, m, v, step, the losses entry by entry
            assert _same_bits(a, c)
    assert int(whole.state.step) == CHAIN_STEPS and whole.grad is None and whole.logits is None
    assert tuple(hooked.grad.shape) == (C, d + 1) and tuple(hooked.logits.shape) == (n, C)
    assert abs(float(whole.loss_history[0]) - math.log(C)) < 1e-4                                   # from zero: log C


# ---------------------------------------------------------------------------- (e) a whole fit
@functools.lru_cache(maxsize=None)
def _blob_reference(i):
    n, d, C, noise = R.BLOB_CASES[i]
    x, y = R.blobs(n, d, C, noise)
    return x, y, R.fit(x, y, C, 100, 0.01)


@pytest.mark.parametrize("i", range(len(R.BLOB_CASES)))
def test_a_whole_fit_classifies_every_training_row_of_the_blob_cases(i):
    x, y, (W64, b64, _, _, _, hist64) = _blob_reference(i)
    C = R.BLOB_CASES[i][2]
    fit = ops.logreg_fit(_dev(x), _dev(y), C, iters=100, lr=0.01)
    pred = ops.logreg_predict(_dev(x), fit.state.weight, fit.state.bias)
    print(f"{R.BLOB_CASES[i]}: final loss {float(fit.loss_history[-1]):.6f} (fp64 {hist64[-1]:.6f}), "
          f"max |W - W_fp64| = {float(np.abs(_np(fit.state.weight) - W64).max()):.3e}")
    assert pred.dtype == torch.int64 and np.array_equal(_np(pred), y)
    assert int(fit.state.step) == 100


@pytest.mark.parametrize("n,d,C", RANDOM_SHAPES + [(77, 6, 5)])
def test_predict_logits_match_fp64_and_ties_go_to_the_lower_class(n, d, C):
    x, _, W, b = _random_case(n, d, C)
    W[C - 1] = W[0]
    b[0] = b[C - 1] = 1.5                                            # a duplicated class with the largest bias: exact ties wherever it wins
    x[3] = 0.0                                                       # a zero row scores b alone
    pred, logits = ops.logreg_predict(_dev(x), _dev(W), _dev(b), return_logits=True)
    want_pred, want = R.predict(x, W, b)
    err = float(np.abs(_np(logits) - want).max())
    print(f"{(n, d, C)}: max |logits - fp64| = {err:.3e}")
    assert err < 1e-5
    z = _np(logits)
    assert np.array_equal(z[:, 0], z[:, C - 1]) and np.array_equal(z[3], b)
    assert np.array_equal(_np(pred), z.argmax(axis=1)) and not (_np(pred) == C - 1).any()          # the first maximum of its own logits
    assert (_np(pred) == 0).any()
    rest = want[:, :C - 1]                                           # without the duplicate: fp64's argmax wherever it is clear
    top = np.sort(rest, axis=1)
    clear = top[:, -1] - top[:, -2] > 2e-5 if C > 2 else np.ones(n, dtype=bool)
    assert np.array_equal(_np(pred)[clear], rest.argmax(axis=1)[clear]) and np.array_equal(want_pred, rest.argmax(axis=1))
    assert torch.equal(ops.logreg_predict(_dev(x), _dev(W), _dev(b)), pred)                        # the hook changes nothing


# ---------------------------------------------------------------------------- (f) contract edges
def test_no_rows_is_a_no_op_and_bad_arguments_are_refused():
    x, y = torch.zeros(0, 8, device=DEV), torch.zeros(0, dtype=torch.int64, device=DEV)
    W, b = _random_state(3, 8, torch.Generator().manual_seed(1))
    before = _state(W, b, step=5)
    fit = ops.logreg_fit(x, y, 3, iters=4, state=before)
    assert all(_same_bits(a, c) for a, c in zip(_state_np(before), _state_np(fit.state))) and not fit.loss_history.any()
    assert ops.logreg_predict(x, _dev(W), _dev(b)).numel() == 0
    x, y = torch.randn(10, 8, device=DEV), torch.zeros(10, dtype=torch.int64, device=DEV)
    for C in (1, 33):
        with pytest.raises(GnnmpError):
            ops.logreg_fit(x, y, C)
        with pytest.raises(GnnmpError):
            ops.logreg_predict(x, torch.zeros(C, 8, device=DEV), torch.zeros(C, device=DEV))
        with pytest.raises(GnnmpError):
            ops.logreg_init(C, 8, DEV)
    for d in (0, 257):
        with pytest.raises(GnnmpError):
            ops.logreg_fit(torch.zeros(10, d, device=DEV), y, 3)
        with pytest.raises(GnnmpError):
            ops.logreg_predict(torch.zeros(10, d, device=DEV), torch.zeros(3, d, device=DEV), torch.zeros(3, device=DEV))
    for iters in (0, 10001):
        with pytest.raises(GnnmpError):
            ops.logreg_fit(x, y, 3, iters=iters)
    with pytest.raises(GnnmpError):
        ops.logreg_fit(x.double(), y, 3)
    with pytest.raises(GnnmpError):
        ops.logreg_fit(x, y[:9], 3)
    with pytest.raises(GnnmpError):
        ops.logreg_fit(x, y, 3, state=ops.logreg_init(4, 8, DEV))
    # a short workspace through the raw call: refused, nothing written
    l = L.lib()
    s = ops.logreg_init(3, 8, DEV)
    need = l.gmp_logreg_workspace_bytes(10, 3, 8)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    loss, status = torch.zeros(2, device=DEV), torch.full((1,), 9, dtype=torch.int32, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    rc = l.gmp_logreg_fit(p(x), p(y), 10, 3, 8, 2, 0.01, 0.0, p(s.weight), p(s.bias), p(s.exp_avg), p(s.exp_avg_sq), p(s.step), p(loss), p(status),
                          None, None, p(ws), need - 1, None)
    torch.cuda.synchronize()
    assert rc == -3 and int(status) == 9 and int(s.step) == 0 and not s.weight.any() and not loss.any()
    pred = torch.full((10,), -5, dtype=torch.int64, device=DEV)
    rc = l.gmp_logreg_predict(p(x), 10, p(s.weight), p(s.bias), 3, 8, p(pred), None, p(ws), need - 1, None)
    torch.cuda.synchronize()
    assert rc == -3 and bool((pred == -5).all())


def test_labels_out_of_range_are_counted_contribute_nothing_and_the_wrapper_raises():
    n, d, C = 300, 40, 5
    x, y, W, b = _random_case(n, d, C)
    y = y.copy()
    y[[0, 129, 299]] = [-1, C, 1 << 40]
    fit, status = ops._logreg_enqueue(_dev(x), _dev(y), C, 1, 0.01, 0.0, _state(W, b), True, False)
    L64, g64, bad = R.loss_grad(R.normalize(x), y, W, b)
    assert int(status) == bad == 3
    assert float(np.abs(_np(fit.grad) - g64).max()) < 2e-5 and abs(float(fit.loss_history[0]) - L64) < 2e-5      # n stays n
    with pytest.raises(GnnmpError, match="outside"):
        ops.logreg_fit(_dev(x), _dev(y), C, iters=1)


@pytest.mark.parametrize("d", [6, 100])
def test_a_dimension_that_is_no_multiple_of_four(d):
    n, C = 200, 5
    x, y, W, b = _random_case(n, d, C)
    x[7] = 0.0
    xn = R.normalize(x)
    # the third iteration against fp64 at the kernel's own parameters after the second
    fit = ops.logreg_fit(_dev(x), _dev(y), C, iters=3, l2=1e-2, state=_state(W, b), return_grad=True, return_logits=True)
    two = ops.logreg_fit(_dev(x), _dev(y), C, iters=2, l2=1e-2, state=_state(W, b))
    W2, b2 = _np(two.state.weight), _np(two.state.bias)
    L64, g64, _ = R.loss_grad(xn, y, W2, b2, 1e-2)
    assert float(np.abs(_np(fit.logits) - R.logits(xn, W2, b2)).max()) < 1e-5
    assert np.array_equal(_np(fit.logits)[7], b2)                    # the zero row
    assert float(np.abs(_np(fit.grad) - g64).max()) < 2e-5 and abs(float(fit.loss_history[2]) - L64) < 2e-5


# ---------------------------------------------------------------------------- (g) the probe
def test_linear_eval_probe_counts_equal_the_fp64_references():
    n, d, C, noise = R.BLOB_CASES[1]
    x, y = R.blobs(n, d, C, noise)
    tr, te = np.arange(n) < 500, np.arange(n) >= 500
    W, b, _, _, _, hist = R.fit(x[tr], y[tr], C, 100, 0.01)
    pred, z = R.predict(x[te], W, b)
    top = np.sort(z, axis=1)
    # a weight that moves by e moves a unit row's logit by at most e sqrt(256); the counts can differ from fp64's only where two logits
    # are closer than twice that.  The reference leaves a gap of 1.0 on every held-out row: room for e = 0.03 on every weight, where an
    # fp32 and an fp64 run of these hundred Adam steps end some 5e-4 apart (profiles/logreg.json, blob_fits)
    assert float((top[:, -1] - top[:, -2]).min()) > 1.0
    state = torch.random.get_rng_state()
    m = linear_eval_probe(_dev(x[tr]), _dev(y[tr]), _dev(x[te]), _dev(y[te]), C, iters=100, lr=0.01)
    assert torch.equal(state, torch.random.get_rng_state())          # no random state is involved
    assert m["num_samples"] == int(te.sum()) and m["correct"] == int((pred == y[te]).sum()) and m["accuracy"] == m["correct"] / m["num_samples"]
    assert m["train_accuracy"] == float((R.predict(x[tr], W, b)[0] == y[tr]).mean()) == 1.0
    own = ops.logreg_fit(_dev(x[tr]), _dev(y[tr]), C, iters=100, lr=0.01)
    assert m["train_loss"] == float(own.loss_history[-1])            # the fit is repeatable: the same bits
    print(f"held-out accuracy {m['accuracy']:.4f}, train loss {m['train_loss']:.6f} (fp64 {hist[-1]:.6f})")
    assert m == linear_eval_probe(_dev(x[tr]), _dev(y[tr]), _dev(x[te]), _dev(y[te]), C, iters=100, lr=0.01)
    bad = y[tr].copy()
    bad[0] = C
    with pytest.raises(ValueError, match="outside"):
        linear_eval_probe(_dev(x[tr]), _dev(bad), _dev(x[te]), _dev(y[te]), C, iters=2)
    with pytest.raises(ValueError):
        linear_eval_probe(_dev(x[tr]), _dev(y[tr]), _dev(x[:0]), _dev(y[:0]), C)
