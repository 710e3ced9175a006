"""The streaming NT-Xent (csrc/ntxent_stream.hip) against the loss and gradient in fp64 torch (the formula of oracle/tasks.py::nt_xent
in double, evaluated in row blocks so that the [2n, 2n] matrix never has to fit), never against the code under test.

Error measure and bars are those of tests/test_gpu_ops.py: max abs error over the tensor's max magnitude, 1e-4 for the loss, 2e-4 for
gradients.  Every parity case first asserts that the fp64 mean loss is at least 0.1: where the positives dominate completely the loss is
lse - s_pos of two nearly equal numbers and fp32 itself has no digits left.

For every case with n <= 8192 the matrix form's error against fp64 is computed on the same input and printed beside the stream form's
(`pytest -s` shows the NTX_ERR lines); no bar is set on their ratio.
"""
import ctypes as C
import json

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gnn_pretraining_amd import _lib as L, operators as O, ops          # noqa: E402

DEV = "cuda:0"
LOSS_TOL, GRAD_TOL = 1e-4, 2e-4
GS = 0.25


def rel_err(got, want):
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)


def make_inputs(n, d, clustered=None, seed=None):
    gen = torch.Generator().manual_seed(n + d if seed is None else seed)
    z1 = torch.randn(n, d, generator=gen)
    z2 = torch.randn(n, d, generator=gen) if clustered is None else z1 + clustered * torch.randn(n, d, generator=gen)
    return z1.to(DEV), z2.to(DEV)


def ref_fp64(z1, z2, T, g_scale=GS, block=2048, grads=True):
    """(loss_sum, g_z1, g_z2, lse[2n], zn, norm) in fp64 on the device, cross-entropy over row blocks of the similarity matrix."""
    n = z1.size(0)
    a = z1.double().clone().requires_grad_(grads)
    b = z2.double().clone().requires_grad_(grads)
    R = 2 * n
    idx = torch.arange(R, device=z1.device)
    pos = (idx + n) % R
    total = 0.0
    lse = torch.empty(R, dtype=torch.float64, device=z1.device)
    for r0 in range(0, R, block):
        r1 = min(r0 + block, R)
        with torch.set_grad_enabled(grads):
            zn = torch.cat([F.normalize(a, dim=1), F.normalize(b, dim=1)])
            s = zn[r0:r1] @ zn.t() / T
            s = s.masked_fill(idx[r0:r1, None] == idx[None, :], float("-inf"))
            l = F.cross_entropy(s, pos[r0:r1], reduction="sum")
            lse[r0:r1] = torch.logsumexp(s.detach(), dim=1)
            if grads:
                (l * g_scale).backward()
        total += l.item()
        del s, l
    with torch.no_grad():
        z = torch.cat([a, b]).detach()
        norm = z.norm(dim=1).clamp_min(1e-12)
        zn = z / norm[:, None]
    return total, (a.grad if grads else None), (b.grad if grads else None), lse, zn, norm


def stream(z1, z2, T, g_scale=GS):
    loss, ws = ops.nt_xent_stream_fwd(z1, z2, T)
    g1, g2 = ops.nt_xent_stream_bwd(z1, z2, T, torch.tensor([g_scale], device=DEV), ws)
    return loss, g1, g2


def matrix(z1, z2, T, g_scale=GS):
    loss, ws = ops.nt_xent_fwd(z1, z2, T)
    g1, g2 = ops.nt_xent_bwd(z1, z2, T, torch.tensor([g_scale], device=DEV), ws)
    return loss, g1, g2


def errors(res, want):
    loss, g1, g2 = res
    wl, w1, w2 = want
    return {"loss": abs(loss.item() - wl) / abs(wl), "g_z1": rel_err(g1, w1), "g_z2": rel_err(g2, w2)}


PARITY = [(2, 4, 1.0, None), (8, 128, 0.5, None), (170, 128, 0.5, None), (333, 128, 0.2, None), (1000, 64, 0.2, None),
          (2049, 256, 0.5, None), (8192, 128, 0.2, None), (8193, 128, 0.5, None), (10000, 128, 0.2, None), (2048, 128, 0.1, 0.3),
          (333, 20, 0.5, None), (333, 32, 0.5, None), (333, 160, 0.5, None), (70, 36, 0.2, None)]     # tile widths 32, 32, 192, 64


@pytest.mark.parametrize("n,d,T,clustered", PARITY)
def test_stream_matches_fp64(n, d, T, clustered):
    z1, z2 = make_inputs(n, d, clustered)
    wl, w1, w2, *_ = ref_fp64(z1, z2, T)
    assert wl / (2 * n) >= 0.1, f"fp64 mean loss {wl / (2 * n):.3e}: not a case fp32 can resolve"
    es = errors(stream(z1, z2, T), (wl, w1, w2))
    em = errors(matrix(z1, z2, T), (wl, w1, w2)) if n <= 8192 else None
    msg = "NTX_ERR " + json.dumps({"n": n, "d": d, "T": T, "clustered": clustered, "stream": es, "matrix": em})
    print(msg)
    assert es["loss"] <= LOSS_TOL, msg
    assert es["g_z1"] <= GRAD_TOL and es["g_z2"] <= GRAD_TOL, msg


def test_single_pair_has_zero_loss_and_zero_gradients():
    z1, z2 = make_inputs(1, 128)
    loss, g1, g2 = stream(z1, z2, 0.5)
    assert loss.item() == 0.0
    assert torch.equal(g1, torch.zeros_like(g1)) and torch.equal(g2, torch.zeros_like(g2))


def test_n_32768_runs_in_linear_memory():
    n, d, T = 32768, 128, 0.2
    z1, z2 = make_inputs(n, d)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    loss, g1, g2 = stream(z1, z2, T)
    torch.cuda.synchronize()
    growth = torch.cuda.max_memory_allocated() - base
    assert growth < 2**30, f"peak memory grew by {growth / 2**20:.0f} MiB (the matrix alone would be 17 GiB)"
    wl, _, _, lse, zn, norm = ref_fp64(z1, z2, T, block=1024, grads=False)
    el = abs(loss.item() - wl) / abs(wl)
    print("NTX_ERR " + json.dumps({"n": n, "d": d, "T": T, "stream_loss": el, "peak_growth_mib": growth / 2**20}))
    assert el <= LOSS_TOL, f"loss {loss.item()} vs fp64 {wl}: {el:.3e}"
    # gradients of the first and last 256 rows of each view, closed form in fp64:
    #   g_zn_i = 1/T sum_{j != i} (exp(s_ij - lse_i) + exp(s_ij - lse_j) - 2 [j = pos(i)]) zn_j, then the backward of the normalisation
    R = 2 * n
    rows = torch.cat([torch.arange(0, 256), torch.arange(n - 256, n), torch.arange(n, n + 256), torch.arange(R - 256, R)]).to(DEV)
    s = zn[rows] @ zn.t() / T
    w = torch.exp(s - lse[rows, None]) + torch.exp(s - lse[None, :])
    k = torch.arange(rows.numel(), device=DEV)
    w[k, (rows + n) % R] -= 2.0
    w[k, rows] = 0.0
    gzn = w @ zn / T
    want = GS * (gzn - zn[rows] * (zn[rows] * gzn).sum(1, keepdim=True)) / norm[rows, None]
    got = torch.cat([g1, g2])[rows]
    for name, sl in (("g_z1", slice(0, 512)), ("g_z2", slice(512, 1024))):
        e = rel_err(got[sl], want[sl])
        assert e <= GRAD_TOL, f"{name} rows: {e:.3e}"


def test_public_operator_takes_a_problem_beyond_the_matrix_form():
    """On the code before the streaming form this raises GnnmpError (n = 10000 > 8192)."""
    n, d, T = 10000, 128, 0.2
    z1, z2 = make_inputs(n, d)
    wl, w1, w2, *_ = ref_fp64(z1, z2, T)
    a, b = z1.clone().requires_grad_(), z2.clone().requires_grad_()
    loss, size = O.nt_xent(a, b, T)
    assert size == 2 * n
    (loss * GS).backward()
    e = errors((loss, a.grad, b.grad), (wl, w1, w2))
    assert e["loss"] <= LOSS_TOL and e["g_z1"] <= GRAD_TOL and e["g_z2"] <= GRAD_TOL, e


def test_public_operator_default_is_todays_path_and_stream_is_selectable():
    n, d, T = 170, 128, 0.5
    z1, z2 = make_inputs(n, d)
    a, b = z1.clone().requires_grad_(), z2.clone().requires_grad_()
    loss, _ = O.nt_xent(a, b, T)
    (loss * GS).backward()
    ml, m1, m2 = matrix(z1, z2, T)
    assert torch.equal(loss.detach().reshape(1), ml) and torch.equal(a.grad, m1) and torch.equal(b.grad, m2)
    wl, w1, w2, *_ = ref_fp64(z1, z2, T)
    a, b = z1.clone().requires_grad_(), z2.clone().requires_grad_()
    loss, _ = O.nt_xent(a, b, T, impl="stream")
    (loss * GS).backward()
    sl, s1, s2 = stream(z1, z2, T)
    assert torch.equal(loss.detach().reshape(1), sl) and torch.equal(a.grad, s1) and torch.equal(b.grad, s2)
    e = errors((loss, a.grad, b.grad), (wl, w1, w2))
    assert e["loss"] <= LOSS_TOL and e["g_z1"] <= GRAD_TOL and e["g_z2"] <= GRAD_TOL, e
    with pytest.raises(L.GnnmpError):
        O.nt_xent(*make_inputs(8200, 8), T, impl="matrix")


@pytest.mark.parametrize("n,zero_row", [(170, None), (8192, None), (170, 3)])
def test_stream_agrees_with_the_matrix_form(n, zero_row):
    d, T = 128, 0.2
    z1, z2 = make_inputs(n, d)
    keep = torch.ones(n, dtype=torch.bool, device=DEV)
    if zero_row is not None:
        # the zero row's own gradient is divided by the 1e-12 clamp and would swamp a max-magnitude measure: every other row is compared
        z1[zero_row] = 0.0
        keep[zero_row] = False
    sl, s1, s2 = stream(z1, z2, T)
    ml, m1, m2 = matrix(z1, z2, T)
    assert torch.isfinite(s1).all() and torch.isfinite(s2).all()
    e = {"loss": abs(sl.item() - ml.item()) / abs(ml.item()), "g_z1": rel_err(s1[keep], m1[keep]), "g_z2": rel_err(s2, m2)}
    print("NTX_ERR " + json.dumps({"n": n, "zero_row": zero_row, "stream_vs_matrix": e}))
    assert e["loss"] <= LOSS_TOL and e["g_z1"] <= GRAD_TOL and e["g_z2"] <= GRAD_TOL, e


@pytest.mark.parametrize("n", [333, 10000])
def test_two_calls_are_bitwise_equal(n):
    z1, z2 = make_inputs(n, 128)
    a, b = stream(z1, z2, 0.2), stream(z1, z2, 0.2)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


SENTINEL = -777.0


ERR_ARG, ERR_WORKSPACE = -1, -3        # include/gnnmp.h


@pytest.mark.parametrize("n,d,T,short,code", [(64, 6, 0.5, 0, ERR_ARG), (64, 260, 0.5, 0, ERR_ARG), (64, 128, 0.0, 0, ERR_ARG),
                                              (0, 128, 0.5, 0, ERR_ARG), (64, 128, 0.5, 1, ERR_WORKSPACE)])
def test_refusals_leave_the_outputs_untouched(n, d, T, short, code):
    lib = L.lib()
    rows = max(n, 1)
    z1 = torch.randn(rows, d, device=DEV); z2 = torch.randn(rows, d, device=DEV)
    loss = torch.full((1,), SENTINEL, device=DEV)
    g1 = torch.full((rows, d), SENTINEL, device=DEV); g2 = torch.full((rows, d), SENTINEL, device=DEV)
    gs = torch.ones(1, device=DEV)
    need = lib.gmp_nt_xent_stream_workspace_bytes(64, 128)
    ws = torch.empty(4 * need, dtype=torch.uint8, device=DEV)
    nbytes = need - 1 if short else ws.numel()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731
    rc = lib.gmp_nt_xent_stream_fwd(p(z1), p(z2), n, d, T, p(loss), p(ws), nbytes, st)
    assert rc == code, (rc, lib.gmp_last_error_string())
    rc = lib.gmp_nt_xent_stream_bwd(p(z1), p(z2), n, d, T, p(gs), p(g1), p(g2), p(ws), nbytes, st)
    assert rc == code, (rc, lib.gmp_last_error_string())
    torch.cuda.synchronize()
    assert loss.item() == SENTINEL and (g1 == SENTINEL).all() and (g2 == SENTINEL).all()


def test_non_default_stream_gives_the_same_bits():
    z1, z2 = make_inputs(333, 128)
    want = stream(z1, z2, 0.2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = stream(z1, z2, 0.2)
    side.synchronize()
    for x, y in zip(got, want):
        assert torch.equal(x, y)
