"""Shared by test_bn_ref_host.py and test_gpu_bn_regimes.py: the float64 definition of the segment-wise BatchNorm of csrc/batchnorm.hip
(residual add, per-segment batch statistics, affine, ReLU, an elementwise gate that carries dropout), its backward, the seeded inputs of
the regime tests and the float32 torch yardstick the tolerances are derived from.

bn_ref_fwd / bn_ref_bwd are plain torch float64 written from the definition: no autograd, no F.batch_norm.  torch_segments is the other
side: F.batch_norm plus autograd, one segment at a time, in the dtype asked for -- float64 to pin bn_ref (test_bn_ref_host.py), float32
as the yardstick of what fp32 arithmetic gets on the same inputs.

Conventions of the kernels that torch does not have, and that bn_ref writes down:
  a one-row training segment has variance 0, rstd = 1/sqrt(eps), and the running variance takes that (biased) 0 (torch raises);
  an empty segment touches nothing: no statistics row, no running update;
  with seg_group, gamma / beta / running statistics are [groups, C] and segment s reads and updates row seg_group[s], segments in order;
  in eval mode the backward treats the running statistics as constants and g_gamma is sum(g * xhat) with xhat from the running pair.
"""
import torch
import torch.nn.functional as F

EPS, MOMENTUM = 1e-5, 0.1
COMPANIONS = [1, 0, 37]              # every sweep launch: the long segment, a one-row one, an empty one in the middle, a partial tile
# longest segment of the regime sweep, and whether rendezvous words are given: both sides of every switch point of gmp_bn_fwd / gmp_bn_bwd
SWEEP = [(n, False) for n in (256, 257, 384, 385, 512, 513, 1024, 1025, 1536, 1537, 2048, 2049, 2560, 2561, 3072, 3073)] + \
        [(1025, True), (4096, True), (4097, True)]
SWEEP_C = [64, 192]                  # the smallest channel count of the ABI (one chunked column block); 6 short / 12 medium tiles, 3 chunked blocks
SWEEP_GROUPS = [0, 2, 4]             # gradient groups of the sweep (segments 0-1, 2-3)
REGIME_ROWS = [(300, False), (1100, False), (3100, False), (1100, True)]       # short, medium, chunked, slab


# Error of fp32 torch (torch_segments) against bn_ref, worst over the whole sweep, training step and eval step (yardstick(); the table in
# test_gpu_bn_regimes.py's docstring); a bar is 8 x that.  *_live: without the constant column; rstd_rel: elementwise relative.
YARDSTICK = {"y": 2.281e-06, "y_live": 2.262e-07, "mean": 9.393e-08, "rstd": 5.435e-08, "rstd_rel": 1.223e-07, "rm": 1.153e-07, "rv": 1.677e-07,
             "g_u": 1.925e-07, "g_u_live": 1.925e-07, "g_gamma": 8.216e-07, "g_beta": 5.573e-07}
TOL = {k: 8 * v for k, v in YARDSTICK.items()}


def delta_of(y_ref):
    """Half-width of the band around the ReLU kink in which the kernel's decision may differ from the reference's at rounding level."""
    return TOL["y"] * y_ref.abs().max().item()


def seg_ptr_of(sizes):
    ptr = [0]
    for n in sizes:
        ptr.append(ptr[-1] + int(n))
    return ptr


def make_case(sizes, C, seed, groups=1):
    """Seeded fp32 CPU inputs: x = mu_c + sigma_c * randn with mu_c in +-3 and sigma_c in [0.5, 2]; the last column of x + residual is the
    constant 0.75 (variance 0: eps alone decides rstd); gamma in [0.5, 1.5], beta in +-0.5, both [groups, C] like the running pair."""
    g = torch.Generator().manual_seed(seed)
    rows = sum(sizes)
    mu, sigma = torch.rand(C, generator=g) * 6 - 3, torch.rand(C, generator=g) * 1.5 + 0.5
    x = mu + sigma * torch.randn(rows, C, generator=g)
    res = torch.randn(rows, C, generator=g)
    x[:, C - 1], res[:, C - 1] = 1.25, -0.5
    return {
        "sizes": list(sizes), "seg": seg_ptr_of(sizes), "C": C, "rows": rows, "max": max(sizes),
        "x": x.contiguous(), "res": res.contiguous(), "gy": torch.randn(rows, C, generator=g),
        "gamma": torch.rand(groups, C, generator=g) + 0.5, "beta": torch.rand(groups, C, generator=g) - 0.5,
        "rm": torch.randn(groups, C, generator=g) * 0.1, "rv": torch.rand(groups, C, generator=g) + 0.5,
    }


def sweep_case(L, sync, C):
    return make_case([L] + COMPANIONS, C, seed=7 * L + C + int(sync))


def group_case(L, sync):
    """Three parameter groups, five segments (one row, empty, a group with two live segments: 0 gets segments 1 and 4); the table."""
    return make_case([L, 1, 0, 200, 64], 192, seed=13 * L + int(sync), groups=3), [2, 0, 2, 1, 0]


def dropout_case(L, sync):
    return make_case([L] + COMPANIONS, 192, seed=17 * L + int(sync))


def _d(t):
    return None if t is None else t.detach().cpu().double()


def bn_ref_fwd(x, res, seg, seg_group, gamma, beta, rm, rv, training, relu, eps=EPS, momentum=MOMENTUM, gate=None):
    """(y, pre, mean [S, C], rstd [S, C], running_mean, running_var) in float64.  pre = gamma * xhat + beta; y = relu(pre) * gate.  Rows
    of mean / rstd of empty segments stay 0.  The running pair comes back updated (training) in the shape it was given, or None."""
    x, res, gate = _d(x), _d(res), _d(gate)
    C = x.shape[1]
    gamma, beta = _d(gamma).reshape(-1, C), _d(beta).reshape(-1, C)
    shape = None if rm is None else rm.shape
    rm = None if rm is None else _d(rm).reshape(-1, C).clone()
    rv = None if rv is None else _d(rv).reshape(-1, C).clone()
    S = len(seg) - 1
    grp = [0] * S if seg_group is None else [int(v) for v in seg_group]
    u = x if res is None else x + res
    pre = torch.zeros_like(u)
    mean, rstd = torch.zeros(S, C, dtype=torch.float64), torch.zeros(S, C, dtype=torch.float64)
    for s in range(S):
        a, b = seg[s], seg[s + 1]
        n, k = b - a, grp[s]
        if n <= 0:
            continue
        if training:
            m = u[a:b].sum(0) / n
            var = ((u[a:b] - m) ** 2).sum(0) / n
            if rm is not None:
                rm[k] = (1 - momentum) * rm[k] + momentum * m
                rv[k] = (1 - momentum) * rv[k] + momentum * (var * n / (n - 1) if n > 1 else var)
        else:
            m, var = rm[k], rv[k]
        r = 1.0 / torch.sqrt(var + eps)
        mean[s], rstd[s] = m, r
        pre[a:b] = gamma[k] * ((u[a:b] - m) * r) + beta[k]
    y = pre.clamp_min(0) if relu else pre.clone()
    if gate is not None:
        y = y * gate
    if rm is not None:
        rm, rv = rm.reshape(shape), rv.reshape(shape)
    return y, pre, mean, rstd, rm, rv


def bn_ref_bwd(gy, x, res, seg, seg_group, gamma, mean, rstd, training, gate, group_seg_ptr):
    """(g_u, g_gamma [G, C], g_beta [G, C]) in float64 from the statistics bn_ref_fwd returned.  g = gy * gate (gate: ReLU mask times
    dropout scale, handed in; None = 1).  Training: g_u = gamma rstd (g - mean(g) - xhat mean(g xhat)); eval: gamma rstd g.  Gradient group
    j sums the segments group_seg_ptr[j] .. group_seg_ptr[j + 1]."""
    gy, x, res, gate, mean, rstd = _d(gy), _d(x), _d(res), _d(gate), _d(mean), _d(rstd)
    C = x.shape[1]
    gamma = _d(gamma).reshape(-1, C)
    S, G = len(seg) - 1, len(group_seg_ptr) - 1
    grp = [0] * S if seg_group is None else [int(v) for v in seg_group]
    u = x if res is None else x + res
    g = gy if gate is None else gy * gate
    gu = torch.zeros_like(u)
    s1, s2 = torch.zeros(S, C, dtype=torch.float64), torch.zeros(S, C, dtype=torch.float64)
    for s in range(S):
        a, b = seg[s], seg[s + 1]
        n = b - a
        if n <= 0:
            continue
        xh = (u[a:b] - mean[s]) * rstd[s]
        s1[s], s2[s] = g[a:b].sum(0), (g[a:b] * xh).sum(0)
        k = gamma[grp[s]] * rstd[s]
        gu[a:b] = k * (g[a:b] - s1[s] / n - xh * (s2[s] / n)) if training else k * g[a:b]
    gg = torch.stack([s2[group_seg_ptr[j]:group_seg_ptr[j + 1]].sum(0) for j in range(G)])
    gb = torch.stack([s1[group_seg_ptr[j]:group_seg_ptr[j + 1]].sum(0) for j in range(G)])
    return gu, gg, gb


def torch_segments(dtype, x, res, seg, gamma, beta, rm, rv, training, relu, gy, group_seg_ptr, eps=EPS, momentum=MOMENTUM, gate=None):
    """torch's own BatchNorm in `dtype` on the CPU: F.batch_norm per segment in order (== S module calls) and autograd through it, one
    parameter set [C].  A one-row training segment, which torch refuses, is done by hand in the kernels' convention.  Returns a dict of
    y, mean, rstd (of live segments; torch's mean / biased var), rm, rv (updated copies), g_u, g_gamma, g_beta (per gradient group, summed
    in segment order)."""
    c = lambda t: None if t is None else t.detach().to(dtype).clone()
    x, res, gy, gate, gamma, beta, rm, rv = c(x), c(res), c(gy), c(gate), c(gamma).reshape(-1), c(beta).reshape(-1), c(rm).reshape(-1), c(rv).reshape(-1)
    S, C = len(seg) - 1, x.shape[1]
    u_all = x if res is None else x + res
    y, gu = torch.zeros_like(u_all), torch.zeros_like(u_all)
    mean, rstd = torch.zeros(S, C, dtype=dtype), torch.zeros(S, C, dtype=dtype)
    sg, sb = torch.zeros(S, C, dtype=dtype), torch.zeros(S, C, dtype=dtype)
    for s in range(S):
        a, b = seg[s], seg[s + 1]
        n = b - a
        if n <= 0:
            continue
        u = u_all[a:b].clone().requires_grad_()
        gam, bet = gamma.clone().requires_grad_(), beta.clone().requires_grad_()
        if training and n == 1:
            m, var = u.detach()[0], torch.zeros(C, dtype=dtype)
            out = gam * ((u - m) * (var + eps).rsqrt()) + bet            # (u - m) is constant 0: xhat = 0 and carries no gradient
            rm.mul_(1 - momentum).add_(momentum * m)
            rv.mul_(1 - momentum).add_(momentum * var)
        else:
            if training:
                m, var = u.detach().mean(0), u.detach().var(0, unbiased=False)
            else:
                m, var = rm.clone(), rv.clone()
            out = F.batch_norm(u, rm, rv, gam, bet, training=training, momentum=momentum, eps=eps)
        mean[s], rstd[s] = m, (var + eps).rsqrt()
        if relu:
            out = torch.relu(out)
        if gate is not None:
            out = out * gate[a:b]
        out.backward(gy[a:b])
        y[a:b] = out.detach()
        gu[a:b] = u.grad if not (training and n == 1) else torch.zeros_like(u)     # by hand: the single row IS the mean
        sg[s], sb[s] = gam.grad, bet.grad
    G = len(group_seg_ptr) - 1
    gg, gb = torch.zeros(G, C, dtype=dtype), torch.zeros(G, C, dtype=dtype)
    for j in range(G):
        for s in range(group_seg_ptr[j], group_seg_ptr[j + 1]):
            gg[j] += sg[s]
            gb[j] += sb[s]
    return {"y": y, "mean": mean, "rstd": rstd, "rm": rm, "rv": rv, "g_u": gu, "g_gamma": gg, "g_beta": gb}


def share(got, want):
    """Largest |got - want| as a share of the largest |want|."""
    got, want = _d(got), _d(want)
    assert got.shape == want.shape, f"shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if got.numel() == 0:
        return 0.0
    return (got - want).abs().max().item() / max(want.abs().max().item(), 1e-300)


def errors_against_ref(case, out, training, relu=True, groups=SWEEP_GROUPS, seg_group=None, rm_in=None, rv_in=None, drop=None):
    """Per-quantity error of one forward + backward `out` (dict like torch_segments': any implementation, fp32) against bn_ref on the same
    inputs.  The backward reference takes its gate from out["y"] != 0 (times `drop`, the dropout scale, when given), so a ReLU decision at
    rounding level does not become an O(1) gradient difference.  Beside the issue's quantities: y_live and g_u_live are y and g_u without the constant column, and rstd_rel
    the largest elementwise relative rstd error (the constant column, xhat = rounding / sqrt(eps) and rstd = 1 / sqrt(eps), sets the scale of
    plain y and rstd).  Also returns the reference's tensors."""
    seg = case["seg"]
    rm_in, rv_in = case["rm"] if rm_in is None else rm_in, case["rv"] if rv_in is None else rv_in
    live = torch.tensor([b > a for a, b in zip(seg[:-1], seg[1:])])
    gate = None
    if relu or drop is not None:
        gate = (_d(out["y"]) != 0).double() * (1.0 if drop is None else drop)
    fgate = None if drop is None else gate                                  # forward: relu is the reference's own, the gate is dropout alone
    y, pre, mean, rstd, rm, rv = bn_ref_fwd(case["x"], case["res"], seg, seg_group, case["gamma"], case["beta"], rm_in, rv_in, training, relu,
                                            gate=fgate)
    gu, gg, gb = bn_ref_bwd(case["gy"], case["x"], case["res"], seg, seg_group, case["gamma"], mean, rstd, training, gate, groups)
    err = {"y": share(out["y"], y), "g_u": share(out["g_u"], gu), "g_gamma": share(out["g_gamma"], gg), "g_beta": share(out["g_beta"], gb)}
    err["g_u_live"] = share(out["g_u"][:, :-1], gu[:, :-1])                 # ... whose g_u is gamma (g - mean g) / sqrt(eps), 300 x the other columns'
    err["y_live"] = share(out["y"][:, :-1], y[:, :-1])                      # without the constant column, whose xhat is rounding / sqrt(eps)
    if training:
        err["mean"], err["rstd"] = share(out["mean"][live], mean[live]), share(out["rstd"][live], rstd[live])
        err["rstd_rel"] = ((_d(out["rstd"])[live] - rstd[live]).abs() / rstd[live]).max().item()
        err["rm"], err["rv"] = share(out["rm"].reshape(rm.shape), rm), share(out["rv"].reshape(rv.shape), rv)
    ref = {"y": y, "pre": pre, "mean": mean, "rstd": rstd, "rm": rm, "rv": rv, "g_u": gu, "g_gamma": gg, "g_beta": gb}
    return err, ref


def yardstick(case, relu=True, groups=SWEEP_GROUPS):
    """Errors of fp32 torch (training step, then eval on its updated running pair) against bn_ref on `case`: {quantity: worst share}."""
    a = (case["x"], case["res"], case["seg"], case["gamma"], case["beta"])
    t = torch_segments(torch.float32, *a, case["rm"], case["rv"], True, relu, case["gy"], groups)
    worst, _ = errors_against_ref(case, t, True, relu, groups)
    e = torch_segments(torch.float32, *a, t["rm"], t["rv"], False, relu, case["gy"], groups)
    ev, _ = errors_against_ref(case, e, False, relu, groups, rm_in=t["rm"], rv_in=t["rv"])
    for k, v in ev.items():
        worst[k] = max(worst[k], v)
    return worst
