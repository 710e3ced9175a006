"""The loss kernels (csrc/losses.hip: MSE, sigmoid, BCE on probabilities, the fused and the signed sigmoid + BCE pass, row-wise
cross-entropy) and the mask-token row fill, through the C ABI against float64 torch on the CPU.  Companion of test_gpu_kernel_edges.py.

References: torch's own functions in float64 on the kernel's float32 inputs, gradients by autograd through them.  BCE on probabilities
is torch.nn.functional.binary_cross_entropy (-100 log clamp, 1e-12 denominator clamp in its backward) behind torch.sigmoid.  Beyond
|x| ~ 17 float32 sigmoid saturates to exactly 0 or 1 and the clamps make loss and gradient discontinuous in the rounding of p: the
`specials` batches (x = +-120, +-46, +-17, 0 with both labels beside a normal spread) are therefore compared with the reference evaluated
at the KERNEL's float32 p (p_out), p_out itself against float64 sigmoid; the `spread` batches (|x| <= 15) additionally against the whole
chain differentiated from x.  Every element of every output is compared in every batch.

Tolerances.  MSE: the running-sum bound (n_terms + 4) * 2^-24 * sum|terms| (terms are rounded products).  row_fill: bit for bit.  The
kernels through expf / logf / log1pf: error relative to the reference tensor's largest magnitude; the bar is 4 x the largest error measured
on the MI355X, rounded up to one digit, and never above the project's 1e-4.  `torch fp32`: the same comparison with torch's float32 CPU
kernels in the kernel's place (test_reference_figures_of_fp32_torch prints them), so nothing is held tighter than torch itself gets.

  output                                   measured MI355X   torch fp32 (CPU)   bar
  sigmoid_fwd p                            8.85e-08          8.8e-08            4e-07
  sigmoid_bwd                              2.91e-07          2.9e-07            2e-06
  bce_sum_fwd loss                         6.83e-08          1.2e-07            3e-07
  bce_sum_bwd g_p                          5.18e-08          5.2e-08            3e-07
  fused / signed p_out                     8.86e-08          8.9e-08            4e-07
  fused / signed loss (at the kernel's p)  1.32e-07          1.8e-07            6e-07
  fused / signed g_x (at the kernel's p)   2.74e-07          2.4e-07            2e-06
  fused / signed loss (from x, spread)     8.57e-06          2.0e-06            4e-05
  fused / signed g_x (from x, spread)      2.76e-07          3.0e-07            2e-06
  cross_entropy_sum_fwd loss               5.64e-08          1.6e-07            3e-07
  cross_entropy_sum_bwd g_logits           9.65e-06          2.5e-07            4e-05

The two figures near 1e-5 have known causes.  Loss from x: at x = 15 float32 p is 1 - 2^-22 or so, log1p(-p) inherits the 20 % rounding of
1 - p (torch's fp32 shows the same, 2e-6, on its own batches).  Cross-entropy gradient: the kernel takes expf(logit - lse) with lse = max
+ log(sum) rounded at the logits' magnitude (rows near -500 and +150 here: half an ulp of 500 is 1.5e-5), where torch subtracts the
maximum first; the error scales with |logit| and is ~1e-7 for logits of order 1.
"""
import pytest
import torch
import torch.nn.functional as Fn

from gnn_pretraining_amd import ops

DEV = "cuda:0"
gpu = pytest.mark.gpu
U = 2.0 ** -24
CAP = 1e-4                           # BASELINE.json north_star, RTOL of test_gpu_ops.py: no bar goes above it
# bar = 4 x measured, one digit, rounded up          measured on the MI355X | torch fp32 on the CPU
TOL = {
    "sigmoid p": 4e-07,                             # 8.846e-08 | 8.8e-08
    "sigmoid_bwd": 2e-06,                           # 2.906e-07 | 2.9e-07
    "bce loss": 3e-07,                              # 6.834e-08 | 1.2e-07
    "bce g_p": 3e-07,                               # 5.179e-08 | 5.2e-08
    "fused p": 4e-07,                               # 8.864e-08 | 8.9e-08
    "fused loss at p": 6e-07,                       # 1.320e-07 | 1.8e-07
    "fused g_x at p": 2e-06,                        # 2.744e-07 | 2.4e-07
    "fused loss from x": 4e-05,                     # 8.571e-06 | 2.0e-06
    "fused g_x from x": 2e-06,                      # 2.764e-07 | 3.0e-07
    "ce loss": 3e-07,                               # 5.642e-08 | 1.6e-07
    "ce g_logits": 4e-05,                           # 9.652e-06 | 2.5e-07
}
MEASURED = {}                        # key -> largest error seen in this process (printed by every check)
LIMITS = dict(TOL)                   # what check() holds an error to: the bars above for the kernels, CAP for torch's own fp32 kernels


def check(key, got, want, what):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if got.numel() == 0:
        return
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    err = (got - want).abs().max().item() / max(want.abs().max().item(), 1e-30)
    MEASURED[key] = max(MEASURED.get(key, 0.0), err)
    print(f"[measured] {key}: {err:.3e} ({what}); largest so far {MEASURED[key]:.3e}")
    assert LIMITS[key] <= CAP
    assert err <= LIMITS[key], f"{what}: {key} error {err:.3e} > {LIMITS[key]:.0e}"


def assert_exact(got, want, what):
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype == torch.float32, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    same = got.contiguous().view(torch.int32) == want.contiguous().view(torch.int32)            # bit for bit
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ"


# ------------------------------------------------------------------------------------------------ inputs
SIZES = [0, 1, 255, 256, 257, 262144 + 3]           # the last: past MAX_PARTS = 1024 blocks of 256, the grid-stride loop runs
SPECIALS = [120.0, -120.0, 46.0, -46.0, 17.0, -17.0, 0.0]


def scores(n, kind, seed):
    """(x, labels): a normal spread clamped to |x| <= 15; `specials`: the first 14 entries are every special score with label 1, then 0."""
    gen = torch.Generator().manual_seed(seed * 1000003 + n)
    x = (torch.randn(n, generator=gen) * 3).clamp(-15, 15)
    y = (torch.rand(n, generator=gen) < 0.5).float()
    if kind == "specials":
        k = min(n, 2 * len(SPECIALS))
        x[:k] = torch.tensor(SPECIALS + SPECIALS)[:k]
        y[:k] = torch.tensor([1.0] * len(SPECIALS) + [0.0] * len(SPECIALS))[:k]
    return x, y


def g_scale_of(n):
    return torch.tensor([0.37 / max(n, 1) ** 0.5])


# ------------------------------------------------------------------------------------------------ float64 references
def ref_bce_at_p(p32, y, w, gs):
    """BCE summed at given float32 probabilities: (loss, d (gs * loss) / d p) by autograd through torch's float64 BCE."""
    p = p32.detach().cpu().double().requires_grad_()
    loss = Fn.binary_cross_entropy(p, y.double(), weight=None if w is None else w.double(), reduction="sum")
    gp, = torch.autograd.grad(loss * gs.double(), p)
    return loss.detach().view(1), gp


def ref_chain_at_p(p32, y, w, gs):
    """... and pushed through the sigmoid whose OUTPUT is p (torch's own sigmoid backward, which takes the output)."""
    loss, gp = ref_bce_at_p(p32, y, w, gs)
    return loss, torch.ops.aten.sigmoid_backward(gp, p32.detach().cpu().double())


def ref_chain_from_x(x, y, w, gs):
    """(sigmoid(x), loss, d (gs * loss) / d x) by autograd through float64 sigmoid + BCE."""
    x64 = x.double().requires_grad_()
    p = torch.sigmoid(x64)
    loss = Fn.binary_cross_entropy(p, y.double(), weight=None if w is None else w.double(), reduction="sum")
    gx, = torch.autograd.grad(loss * gs.double(), x64)
    return p.detach(), loss.detach().view(1), gx


def ref_cross_entropy(logits, target, gs):
    """F.cross_entropy(reduction='sum') in float64 over the rows whose target lies in [0, C); the other rows add 0 and get no gradient."""
    l64 = logits.double().requires_grad_()
    ok = (target >= 0) & (target < logits.size(1))
    loss = Fn.cross_entropy(l64[ok], target[ok], reduction="sum")
    g, = torch.autograd.grad(loss * gs.double(), l64)
    return loss.detach().view(1), g, ok


def ce_problem(C, M, seed=0):
    gen = torch.Generator().manual_seed(C * 7919 + M + seed)
    logits = torch.randn(M, C, generator=gen) * 3
    logits[3] = 1.25                                            # a row of equal logits
    if C > 1:
        logits[5, 0], logits[5, C - 1] = 150.0, -150.0          # rows that span more than 200: the max shift at work
        logits[6, 0], logits[6, C - 1] = -120.0, 110.0
        logits[7] = logits[7] - 500.0
    target = torch.randint(0, C, (M,), generator=gen)
    target[5], target[6] = C - 1, 0                             # ... with the target at the small end
    target[10:16] = torch.tensor([-1, C, C + 5, -100, 2 ** 40, -2 ** 40])
    return logits, target


# ------------------------------------------------------------------------------------------------ implementations under comparison
class Kernels:
    """the HIP kernels"""
    dev = DEV
    sigmoid = staticmethod(ops.sigmoid_fwd)
    sigmoid_bwd = staticmethod(ops.sigmoid_bwd)
    bce = staticmethod(ops.bce_sum_fwd)
    bce_bwd = staticmethod(ops.bce_sum_bwd)
    ce = staticmethod(ops.cross_entropy_sum_fwd)
    ce_bwd = staticmethod(ops.cross_entropy_sum_bwd)

    @staticmethod
    def fused(x, y, w, gs):
        if w is None:
            return ops.sigmoid_bce_sum_fwd_bwd(x, y, gs)
        return ops.sigmoid_bce_signed_sum_fwd_bwd(x, torch.where(y > 0, w, -w), gs)


class TorchFp32:
    """torch's float32 CPU kernels in the kernels' place: the reference-versus-reference figure"""
    dev = "cpu"
    sigmoid = staticmethod(torch.sigmoid)
    sigmoid_bwd = staticmethod(lambda g, y: torch.ops.aten.sigmoid_backward(g, y))
    bce = staticmethod(lambda p, y: Fn.binary_cross_entropy(p, y, reduction="sum").view(1))
    ce = staticmethod(lambda l, t: Fn.cross_entropy(l, t, reduction="sum").view(1))

    @staticmethod
    def bce_bwd(p, y, gs):
        p = p.clone().requires_grad_()
        return torch.autograd.grad(Fn.binary_cross_entropy(p, y, reduction="sum") * gs, p)[0]

    @staticmethod
    def ce_bwd(l, t, gs):
        l = l.clone().requires_grad_()
        return torch.autograd.grad(Fn.cross_entropy(l, t, reduction="sum") * gs, l)[0]

    @staticmethod
    def fused(x, y, w, gs):
        x = x.clone().requires_grad_()
        p = torch.sigmoid(x)
        loss = Fn.binary_cross_entropy(p, y, weight=w, reduction="sum")
        return loss.detach().view(1), p.detach(), torch.autograd.grad(loss * gs, x)[0]


def run_separate_kernels(impl, n, kind):
    x, y = scores(n, kind, 1)
    gs = g_scale_of(n)
    d = lambda t: t.to(impl.dev)
    p = impl.sigmoid(d(x))
    check("sigmoid p", p, torch.sigmoid(x.double()), f"sigmoid_fwd n={n} {kind}")
    loss = impl.bce(p, d(y))
    gp = impl.bce_bwd(p, d(y), d(gs))
    want_loss, want_gp = ref_bce_at_p(p, y, None, gs)
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen)
    gx = impl.sigmoid_bwd(d(g), p)
    want_gx = torch.ops.aten.sigmoid_backward(g.double(), p.detach().cpu().double())
    if n == 0:
        assert_exact(loss, torch.zeros(1), "bce_sum_fwd of nothing")
        assert p.numel() == gp.numel() == gx.numel() == 0
        return
    check("bce loss", loss, want_loss, f"bce_sum_fwd n={n} {kind}")
    check("bce g_p", gp, want_gp, f"bce_sum_bwd n={n} {kind}")
    check("sigmoid_bwd", gx, want_gx, f"sigmoid_bwd n={n} {kind}")
    if kind == "spread":                                         # ... and sigmoid_bwd against autograd through float64 sigmoid itself
        x64 = x.double().requires_grad_()
        want, = torch.autograd.grad(torch.sigmoid(x64), x64, g.double())
        check("sigmoid_bwd", gx, want, f"sigmoid_bwd against autograd from x, n={n}")


def run_fused(impl, n, kind, weights):
    """weights: None (the unsigned pass) or 'mixed' / 'positive' / 'negative' (the signed pass: w in {1, 2, 3}, labels of both / one sign)"""
    x, y = scores(n, kind, 2)
    w = None
    if weights is not None:
        gen = torch.Generator().manual_seed(n + 5)
        w = torch.randint(1, 4, (n,), generator=gen).float()
        y = y if weights == "mixed" else torch.full_like(y, 1.0 if weights == "positive" else 0.0)
    gs = g_scale_of(n)
    d = lambda t: None if t is None else t.to(impl.dev)
    loss, p, gx = impl.fused(d(x), d(y), d(w), d(gs))
    what = f"n={n} {kind} weights={weights}"
    if n == 0:
        assert_exact(loss, torch.zeros(1), "loss of nothing")
        assert p.numel() == gx.numel() == 0
        return
    p64, loss_x, gx_x = ref_chain_from_x(x, y, w, gs)
    check("fused p", p, p64, "p_out " + what)
    loss_p, gx_p = ref_chain_at_p(p, y, w, gs)
    check("fused loss at p", loss, loss_p, "loss " + what)
    check("fused g_x at p", gx, gx_p, "g_x " + what)
    if kind == "spread":
        check("fused loss from x", loss, loss_x, "loss " + what)
        check("fused g_x from x", gx, gx_x, "g_x " + what)


def run_cross_entropy(impl, C, M):
    logits, target = ce_problem(C, M)
    gs = torch.tensor([0.37 / M])
    want_loss, want_g, ok = ref_cross_entropy(logits, target, gs)
    if impl is TorchFp32:                                       # torch raises on a target out of range: its rows are left out by hand
        loss = impl.ce(logits[ok], target[ok])
        g = torch.zeros_like(logits)
        g[ok] = impl.ce_bwd(logits[ok], target[ok], gs)
    else:
        loss = impl.ce(logits.to(DEV), target.to(DEV))
        g = impl.ce_bwd(logits.to(DEV), target.to(DEV), gs.to(DEV))
    assert_exact(g.cpu()[~ok], torch.zeros(int((~ok).sum()), C), "rows with a target out of range get no gradient")
    if C == 1:
        assert_exact(loss, torch.zeros(1), "C = 1: the loss is exactly 0")
        assert_exact(g, torch.zeros(M, 1), "C = 1: the gradient is exactly 0")
        assert float(want_loss) == 0.0 and float(want_g.abs().max()) == 0.0
        return
    check("ce loss", loss, want_loss, f"cross_entropy_sum_fwd C={C} M={M}")
    check("ce g_logits", g, want_g, f"cross_entropy_sum_bwd C={C} M={M}")


CE_CASES = [(1, 257), (2, 257), (7, 5003), (12, 257), (63, 257), (64, 257), (65, 257), (1000, 257)]


# ------------------------------------------------------------------------------------------------ CPU: the references against fp32 torch
def test_reference_figures_of_fp32_torch():
    """torch's float32 CPU kernels through the very comparisons the HIP kernels get: pins the float64 references (a reference that
    were wrong would sit far from torch's own fp32 result) and prints the fp32-versus-fp64 figures quoted in the module docstring."""
    saved, bars = dict(MEASURED), dict(LIMITS)
    MEASURED.clear()
    LIMITS.update({k: CAP for k in TOL})
    try:
        for n in SIZES:
            for kind in ("spread", "specials"):
                run_separate_kernels(TorchFp32, n, kind)
                run_fused(TorchFp32, n, kind, None)
                run_fused(TorchFp32, n, kind, "mixed")
        for C, M in CE_CASES:
            run_cross_entropy(TorchFp32, C, M)
        print("[torch fp32 on the CPU against float64]", {k: f"{v:.1e}" for k, v in sorted(MEASURED.items())})
        assert set(MEASURED) == set(TOL) and max(MEASURED.values()) <= CAP
    finally:
        MEASURED.clear()
        MEASURED.update(saved)
        LIMITS.update(bars)


def test_reference_mse_matches_torch():
    gen = torch.Generator().manual_seed(8)
    a, b = torch.randn(1000, 12, generator=gen), torch.randn(1000, 12, generator=gen)
    a32 = a.clone().requires_grad_()
    l32 = Fn.mse_loss(a32, b, reduction="sum")
    l32.backward()
    a64 = a.double().requires_grad_()
    l64 = Fn.mse_loss(a64, b.double(), reduction="sum")
    l64.backward()
    assert abs(l64.item() - l32.item()) <= 1e-5 * l64.item() and (a64.grad - a32.grad.double()).abs().max() <= 1e-6 * a64.grad.abs().max()


# ------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("n", SIZES)
def test_mse_sum(n):
    gen = torch.Generator().manual_seed(n + 1)
    a, b = torch.randn(n, generator=gen) * 2, torch.randn(n, generator=gen)
    gs = torch.tensor([0.37])
    a64 = a.double().requires_grad_()
    want = Fn.mse_loss(a64, b.double(), reduction="sum")
    ga64, = torch.autograd.grad(want * gs.double(), a64)
    loss = ops.mse_sum_fwd(a.to(DEV), b.to(DEV)).cpu().double()
    ga = ops.mse_sum_bwd(a.to(DEV), b.to(DEV), gs.to(DEV)).cpu().double()
    assert ga.shape == a.shape
    if n == 0:
        assert float(loss) == 0.0
        return
    err, bound = abs(float(loss) - float(want.detach())), (n + 4) * U * float(want.detach())              # the terms are squares: sum|terms| is the loss
    print(f"[sum bound] mse_sum_fwd n={n}: err/bound {err / bound:.3f}")
    assert err <= bound, f"mse_sum_fwd n={n}: {err:.3e} > {bound:.3e}"
    ratio = ((ga - ga64).abs() / ((1 + 4) * U * ga64.abs()).clamp(min=1e-300)).max().item()
    print(f"[sum bound] mse_sum_bwd n={n}: worst err/bound {ratio:.3f}")
    assert ratio <= 1.0 and bool(((ga == 0) == (ga64 == 0)).all()), f"mse_sum_bwd n={n}: worst err/bound {ratio:.3f}"


@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["spread", "specials"])
def test_sigmoid_and_bce_kernels(n, kind):
    """gmp_sigmoid_fwd / _bwd, gmp_bce_sum_fwd / _bwd one by one (g_scale != 1)"""
    run_separate_kernels(Kernels, n, kind)


@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["spread", "specials"])
def test_fused_sigmoid_bce(n, kind):
    """gmp_sigmoid_bce_sum_fwd_bwd: loss, p_out and the gradient, each against float64"""
    run_fused(Kernels, n, kind, None)


@gpu
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["spread", "specials"])
@pytest.mark.parametrize("weights", ["mixed", "positive", "negative"])
def test_signed_sigmoid_bce(n, kind, weights):
    """gmp_sigmoid_bce_signed_sum_fwd_bwd: weights in {1, 2, 3} of both signs, an all-positive and an all-negative batch; the weight
    scales the loss term AND the gradient"""
    run_fused(Kernels, n, kind, weights)


@gpu
def test_signed_pass_with_unit_weights_is_the_unsigned_pass_bitwise():
    x, y = scores(7937, "specials", 3)
    gs = g_scale_of(7937).to(DEV)
    a = ops.sigmoid_bce_sum_fwd_bwd(x.to(DEV), y.to(DEV), gs)
    b = ops.sigmoid_bce_signed_sum_fwd_bwd(x.to(DEV), (2 * y - 1).to(DEV), gs)
    for u, v, what in zip(a, b, ("loss", "p", "g_x")):
        assert torch.equal(u, v), what


@gpu
@pytest.mark.parametrize("C,M", CE_CASES)
def test_cross_entropy_sum(C, M):
    """one wave per row, lanes striding the classes: C below / at / above 64 (idle lanes, the stride loop), rows spanning > 200, targets
    out of range (contribute 0, get no gradient), C = 1 (exactly 0)"""
    run_cross_entropy(Kernels, C, M)


@gpu
@pytest.mark.parametrize("F", [4, 256, 260])
@pytest.mark.parametrize("broadcast", [True, False])
def test_row_fill(F, broadcast):
    """gmp_row_fill: dst[idx[m]] = src[0] (broadcast) or src[m]; negative / out-of-range indices are skipped, every other row of dst
    keeps its contents; M = 20,000 is past one sweep of the 2,048-block grid.  Duplicate indices carry equal source rows in the per-row
    form (which of two different rows would win is not defined, as in torch's index_put_)."""
    gen = torch.Generator().manual_seed(F + broadcast)
    N, M = 30000, 20000
    dst = torch.randn(N, F, generator=gen)
    idx = torch.randint(0, N, (M,), generator=gen)
    idx[1::7] = idx[0::7][:idx[1::7].numel()]                   # duplicates
    bad = torch.tensor([-1, -N, N, N + 1, 2 ** 40, -2 ** 40, 2 ** 31])
    idx[torch.randperm(M, generator=gen)[:bad.numel() * 4]] = bad.repeat(4)
    idx[0], idx[M - 1] = N, -1
    ok = (idx >= 0) & (idx < N)
    assert int(ok.sum()) > torch.unique(idx[ok]).numel() and int((~ok).sum()) >= 20
    table = torch.randn(N, F, generator=gen)
    src = torch.randn(F, generator=gen) if broadcast else table[torch.where(ok, idx, torch.zeros_like(idx))].contiguous()
    want = dst.clone()
    want[idx[ok]] = src if broadcast else src[ok]
    assert not torch.equal(want, dst)
    got = ops.row_fill_(dst.to(DEV), idx.to(DEV), src.to(DEV), broadcast)
    assert_exact(got, want, "row_fill")
    touched = torch.zeros(N, dtype=torch.bool)
    touched[idx[ok]] = True
    assert_exact(got.cpu()[~touched], dst[~touched], "rows no valid index names keep their contents")
    # no duplicates: every source row differs
    perm = torch.randperm(N, generator=gen)[:M]
    perm[::50] = N + 3
    src = torch.randn(M, F, generator=gen)
    want = dst.clone()
    okp = perm < N
    want[perm[okp]] = src[okp]
    assert_exact(ops.row_fill_(dst.to(DEV), perm.to(DEV), src.to(DEV), False), want, "row_fill, distinct rows")
