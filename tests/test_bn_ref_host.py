"""Pins tests/bn_ref.py, the float64 reference of the segment-wise BatchNorm that test_gpu_bn_regimes.py holds the HIP kernels to, on the
CPU: against torch.nn.functional.batch_norm plus autograd in float64, one segment at a time (1e-12 of the largest value), the conventions
torch does not have (one-row training segments, empty segments, seg_group) against literal values, and the condition the GPU tests put on
their inputs: at most 1 % of the elements of any case sit within delta of the ReLU kink."""
import pytest
import torch
import torch.nn.functional as F

import bn_ref as R
from bn_ref import TOL, YARDSTICK

RTOL = 1e-12


def _case():
    return R.make_case([70, 1, 0, 33, 2], 8, seed=5)


@pytest.mark.parametrize("training", [True, False])
@pytest.mark.parametrize("relu", [True, False])
@pytest.mark.parametrize("with_res", [True, False])
@pytest.mark.parametrize("gated", [False, True])
def test_bn_ref_equals_torch_batch_norm_and_autograd_in_float64(training, relu, with_res, gated):
    c = _case()
    res = c["res"] if with_res else None
    groups = [0, 1, 3, 5]
    gate = None
    if gated:                                                                # dropout at p = 0.25: 0 or 4/3, any fixed pattern will do
        gate = (torch.rand(c["rows"], c["C"], generator=torch.Generator().manual_seed(3)) > 0.25).double() / 0.75
    t = R.torch_segments(torch.float64, c["x"], res, c["seg"], c["gamma"], c["beta"], c["rm"], c["rv"], training, relu, c["gy"], groups, gate=gate)
    y, pre, mean, rstd, rm, rv = R.bn_ref_fwd(c["x"], res, c["seg"], None, c["gamma"], c["beta"], c["rm"], c["rv"], training, relu, gate=gate)
    full = (pre > 0).double() if relu else torch.ones_like(pre)
    if gate is not None:
        full = full * gate
    gu, gg, gb = R.bn_ref_bwd(c["gy"], c["x"], res, c["seg"], None, c["gamma"], mean, rstd, training, full, groups)
    live = torch.tensor([n > 0 for n in c["sizes"]])
    pairs = [("y", y, t["y"]), ("mean", mean[live], t["mean"][live]), ("rstd", rstd[live], t["rstd"][live]), ("g_u", gu, t["g_u"]),
             ("g_gamma", gg, t["g_gamma"]), ("g_beta", gb, t["g_beta"]), ("rm", rm.reshape(-1), t["rm"]), ("rv", rv.reshape(-1), t["rv"])]
    for what, got, want in pairs:
        assert got.dtype == torch.float64 and want.dtype == torch.float64
        assert R.share(got, want) <= RTOL, f"{what}: {R.share(got, want):.3e}"
    if training:
        assert not torch.equal(rm.reshape(-1), c["rm"].double().reshape(-1))          # the running pair did move
    else:
        assert torch.equal(rm.reshape(-1), c["rm"].double().reshape(-1)) and torch.equal(rv.reshape(-1), c["rv"].double().reshape(-1))


def test_torch_refuses_a_one_row_training_segment_so_the_convention_is_the_kernels_own():
    x = torch.randn(1, 8, dtype=torch.float64)
    with pytest.raises(ValueError):
        F.batch_norm(x, torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64), training=True)
    F.batch_norm(x, torch.zeros(8, dtype=torch.float64), torch.ones(8, dtype=torch.float64), training=False)     # eval takes it


def test_one_row_and_empty_segments_follow_the_kernels_convention():
    C = 4
    x = torch.tensor([[1.0, -2.0, 0.5, 3.0], [2.0, 2.0, 2.0, 2.0], [4.0, 0.0, 2.0, -2.0]])
    gamma, beta = torch.tensor([1.0, 2.0, 0.5, 1.5]), torch.tensor([0.25, -0.25, 0.0, 1.0])
    rm0, rv0 = torch.tensor([1.0, 1.0, 1.0, 1.0]), torch.tensor([2.0, 2.0, 2.0, 2.0])
    seg = [0, 1, 1, 3]                                                       # one row, empty, two rows
    y, pre, mean, rstd, rm, rv = R.bn_ref_fwd(x, None, seg, None, gamma, beta, rm0, rv0, True, False)
    assert torch.equal(mean[0], x[0].double()) and torch.equal(rstd[0], torch.full((C,), R.EPS, dtype=torch.float64).rsqrt())
    assert torch.equal(y[0], beta.double())                                  # xhat = 0
    assert torch.equal(mean[1], torch.zeros(C, dtype=torch.float64)) and torch.equal(rstd[1], torch.zeros(C, dtype=torch.float64))
    # two updates in order: the one-row segment folds (mean = its row, variance 0, biased), then the two-row one (unbiased: x 2 / 1)
    m2, v2 = x[1:3].double().mean(0), x[1:3].double().var(0, unbiased=True)
    want_rm = 0.9 * (0.9 * rm0.double() + 0.1 * x[0].double()) + 0.1 * m2
    want_rv = 0.9 * (0.9 * rv0.double() + 0.1 * 0.0) + 0.1 * v2
    assert R.share(rm, want_rm) <= RTOL and R.share(rv, want_rv) <= RTOL
    gy = torch.ones(3, C)
    gu, gg, gb = R.bn_ref_bwd(gy, x, None, seg, None, gamma, mean, rstd, True, None, [0, 2, 3])
    assert torch.equal(gu[0], torch.zeros(C, dtype=torch.float64))           # g - mean(g) - 0
    assert torch.equal(gb[0], torch.ones(C, dtype=torch.float64)) and torch.equal(gg[0], torch.zeros(C, dtype=torch.float64))


def test_seg_group_selects_the_parameter_row_and_folds_in_segment_order():
    sizes, table = [30, 1, 0, 20, 6], [2, 0, 2, 1, 0]
    c = R.make_case(sizes, 8, seed=11, groups=3)
    y, pre, mean, rstd, rm, rv = R.bn_ref_fwd(c["x"], c["res"], c["seg"], table, c["gamma"], c["beta"], c["rm"], c["rv"], True, True)
    rm_w, rv_w = c["rm"].double().clone(), c["rv"].double().clone()
    for s, k in enumerate(table):                                            # each segment alone, with its group's rows, in order
        a, b = c["seg"][s], c["seg"][s + 1]
        if b == a:
            continue
        ys, _, ms, rs, rm_w[k], rv_w[k] = R.bn_ref_fwd(c["x"][a:b], c["res"][a:b], [0, b - a], None, c["gamma"][k], c["beta"][k], rm_w[k], rv_w[k],
                                                       True, True)
        assert torch.equal(y[a:b], ys) and torch.equal(mean[s], ms[0]) and torch.equal(rstd[s], rs[0])
    assert torch.equal(rm, rm_w) and torch.equal(rv, rv_w)
    assert rm.shape == (3, 8) and not torch.equal(rm[0], c["rm"][0].double())
    ye, _, me, _, _, _ = R.bn_ref_fwd(c["x"], c["res"], c["seg"], table, c["gamma"], c["beta"], rm, rv, False, True)
    assert torch.equal(me[3], rm[1]) and torch.equal(me[4], rm[0]) and torch.equal(me[0], rm[2])


def _all_cases():
    for L, sync in R.SWEEP:
        for C in R.SWEEP_C:
            yield f"sweep {L} {sync} {C}", R.sweep_case(L, sync, C), None
    for L, sync in R.REGIME_ROWS:
        c, table = R.group_case(L, sync)
        yield f"seg_group {L} {sync}", c, table
        yield f"dropout {L} {sync}", R.dropout_case(L, sync), None


def test_the_share_of_elements_near_the_relu_kink_stays_below_one_percent_for_every_seed():
    """|pre64| <= delta (the forward bar times max |y|) is where the kernel's ReLU decision may differ from the reference's at rounding
    level; the GPU tests exclude those elements from the gate comparison, so they must be few: the reference alone decides that here."""
    worst = 0.0
    for name, c, table in _all_cases():
        y, pre, *_ = R.bn_ref_fwd(c["x"], c["res"], c["seg"], table, c["gamma"], c["beta"], c["rm"], c["rv"], True, True)
        near = (pre.abs() <= R.delta_of(y)).double().mean().item()
        worst = max(worst, near)
        assert near <= 0.01, f"{name}: {near:.4f} of the elements within delta of the kink"
    print(f"[measured] largest near-kink share {worst:.2e}")


def test_fp32_torch_reproduces_the_recorded_yardstick_and_meets_the_bars():
    """The bars of test_gpu_bn_regimes.py are 8 x the recorded error of fp32 torch against bn_ref over the sweep (bn_ref.YARDSTICK).  fp32
    torch measured here over the same sweep lies within a factor of 2 of every recorded figure -- its CPU kernels may round differently from
    build to build, hence no equality; a stale table is noticed -- and so inside every bar."""
    worst = {}
    for L, sync in R.SWEEP:
        for C in R.SWEEP_C:
            for k, v in R.yardstick(R.sweep_case(L, sync, C)).items():
                worst[k] = max(worst.get(k, 0.0), v)
    print("[measured] fp32 torch against bn_ref:", {k: f"{v:.3e}" for k, v in worst.items()})
    assert set(worst) == set(YARDSTICK)
    for k, v in worst.items():
        assert YARDSTICK[k] / 2 <= v <= YARDSTICK[k] * 2, f"{k}: fp32 torch {v:.3e}, recorded {YARDSTICK[k]:.3e}"
        assert v <= TOL[k]
