"""csrc/batchnorm.hip, one operation implemented five ways, against the float64 definition in tests/bn_ref.py: every regime (short, medium,
chunked, slab, eval), both sides of every switch point of the two launch ladders, the seg_group paths, one-row and empty segments in every
regime, the dropout gate the backward kernels regenerate, the slab rendezvous across shapes, the silent slab fallback and the argument
errors.  Inputs: bn_ref.make_case (per-column mean in +-3, sigma in [0.5, 2], one constant column, gamma in [0.5, 1.5], beta in +-0.5).

Which kernel a longest segment of L rows selects (gmp_bn_fwd / gmp_bn_bwd):
  L <= 256        fwd bn_fwd_short_kernel<4, 64>          bwd bn_bwd_short_kernel<4, 64, 8, KEEP>
  257 .. 384      fwd <8, 64>                             bwd <6, 64, 8, KEEP>
  385 .. 512      fwd <8, 64>                             bwd <8, 64>
  513 .. 1024     fwd <16, 64>                            bwd <16, 64>
  1025 .. 1536    bn_*_short_kernel<6, 256, 4>      1537 .. 2048  <8, 256, 4>      2049 .. 2560  <10, 256, 4>      2561 .. 3072  <12, 256, 4>
  > 3072          bn_partial / bn_finalize / bn_apply_long and bn_bwd_partial / bn_bwd_finalize / bn_bwd_apply_long (256-row chunks)
  1025 .. 4096 with enough sync words: bn_fwd_slab_kernel<4> / bn_bwd_slab_kernel<4>; 4097 and beyond with sync words: chunked
  eval mode: the same kernels with the running pair as constants (the forward slab kernel then skips the rendezvous)

Tolerances: error as a share of the reference tensor's largest magnitude.  The yardstick is fp32 torch on the CPU (F.batch_norm per segment
plus autograd, bn_ref.torch_segments) against bn_ref on the very same inputs, worst value over the sweep below, training step and eval
step (bn_ref.yardstick; test_bn_ref_host.py re-measures it).  A bar is 8 x the yardstick: the kernels sum in another order than torch's
cascade (lane-serial, shuffle tree, LDS; Chan merges over up to 32 partials).  Beside the quantities of plain y and rstd, whose scale the
constant column sets (its xhat is rounding / sqrt(eps), its rstd 1 / sqrt(eps) = 316), and of plain g_u (there gamma (g - mean g) * 316: the
training-mode maximum is 1.9e3 against 6 in the other columns), y_live and g_u_live are y and g_u without that column, each as a share of
that slice's largest magnitude, and rstd_rel the largest elementwise relative error of rstd.

  quantity    fp32 torch (yardstick)   bar = 8 x    kernels on the MI355X (worst over this file)
  y           2.281e-06                1.825e-05    2.532e-07
  y_live      2.262e-07                1.810e-06    2.532e-07
  mean        9.393e-08                7.514e-07    1.166e-07
  rstd        5.435e-08                4.348e-07    4.216e-08
  rstd_rel    1.223e-07                9.784e-07    1.675e-07
  rm          1.153e-07                9.224e-07    1.177e-07
  rv          1.677e-07                1.342e-06    1.549e-07
  g_u         1.925e-07                1.540e-06    2.318e-07
  g_u_live    1.925e-07                1.540e-06    2.318e-07
  g_gamma     8.216e-07                6.573e-06    3.028e-07
  g_beta      5.573e-07                4.458e-06    2.628e-07

The backward reference takes its gate from the kernel's own forward output (y != 0), as test_fused_sigmoid_bce... does with the kernel's p:
a ReLU decision at rounding level then is no O(1) gradient difference.  The gate itself must equal pre64 > 0 wherever |pre64| > delta =
TOL["y"] * max |y|; test_bn_ref_host.py holds the share of elements within delta to 1 % for every seed used here.
"""
import ctypes as C

import pytest
import torch

import bn_ref as R
from gnn_pretraining_amd import _lib as L
from gnn_pretraining_amd import ops

DEV = "cuda:0"
gpu = pytest.mark.gpu
YARDSTICK, TOL = R.YARDSTICK, R.TOL   # the table above as constants; they live in bn_ref.py, which test_bn_ref_host.py shares
MEASURED = {}                        # quantity -> largest kernel error seen in this process (printed by every check)
ERR_ARG, ERR_WORKSPACE, MAX_GROUPS = -1, -3, 24         # include/gnnmp.h, GMP_MAX_GROUPS of csrc/gnnmp_internal.h
P = C.c_void_p


# ------------------------------------------------------------------------------------------------ launches
class Dev:
    """One case's tensors on the GPU."""

    def __init__(self, c, table=None):
        self.c, self.S, self.C, self.rows, self.max = c, len(c["sizes"]), c["C"], c["rows"], c["max"]
        for k in ("x", "res", "gy", "gamma", "beta", "rm", "rv"):
            setattr(self, k, c[k].to(DEV).contiguous())
        self.seg = torch.tensor(c["seg"], dtype=torch.int32, device=DEV)
        self.table = None if table is None else torch.tensor(table, dtype=torch.int32, device=DEV)


def nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=DEV)


def sync_words(C_, S, short=0):
    return torch.zeros(ops.bn_sync_words(C_, S) - short, dtype=torch.int32, device=DEV)


def raw_fwd(d, cfg, rm, rv, max_rows=None, stats=True, ws_short=0, Cc=None):
    """gmp_bn_fwd on NaN-filled outputs and a workspace of all-ones bytes (NaN as floats).  Returns (rc, y, save_mean, save_rstd)."""
    l = L.lib()
    y, sm, sr = nan(d.rows, d.C), (nan(d.S, d.C) if stats else None), (nan(d.S, d.C) if stats else None)
    mx = d.max if max_rows is None else max_rows
    nb = l.gmp_bn_workspace_bytes(d.rows, d.C, d.S, min(mx, d.rows))
    ws = torch.full((nb,), 255, dtype=torch.uint8, device=DEV)
    rc = l.gmp_bn_fwd(ops._ptr(d.x), ops._ptr(d.res), ops._ptr(d.seg), ops._ptr(d.table), d.S, mx, d.rows,
                      d.C if Cc is None else Cc, ops._ptr(d.gamma), ops._ptr(d.beta), ops._ptr(rm), ops._ptr(rv), ops._ptr(sm), ops._ptr(sr),
                      ops._ptr(y), C.byref(cfg), ops._ptr(ws), nb - ws_short, ops._stream(d.x))
    return rc, y, sm, sr


def raw_bwd(d, cfg, rm, rv, sm, sr, groups, num_groups=None):
    """gmp_bn_bwd likewise.  Returns (rc, g_u, g_gamma, g_beta, workspace)."""
    l = L.lib()
    G = len(groups) - 1 if num_groups is None else num_groups
    gu, gg, gb = nan(d.rows, d.C), nan(max(G, 1), d.C), nan(max(G, 1), d.C)
    nb = l.gmp_bn_workspace_bytes(d.rows, d.C, d.S, d.max)
    ws = torch.full((nb,), 255, dtype=torch.uint8, device=DEV)
    arr = (C.c_int32 * len(groups))(*groups)
    rc = l.gmp_bn_bwd(ops._ptr(d.gy), ops._ptr(d.x), ops._ptr(d.res), ops._ptr(d.seg), ops._ptr(d.table), d.S, d.max, d.rows, d.C,
                      ops._ptr(d.gamma), ops._ptr(d.beta), ops._ptr(rm), ops._ptr(rv), ops._ptr(sm), ops._ptr(sr), ops._ptr(gu),
                      ops._ptr(gg) if G else None, ops._ptr(gb) if G else None, C.cast(arr, P), None, None, G, C.byref(cfg), ops._ptr(ws), nb,
                      ops._stream(d.x))
    return rc, gu, gg, gb, ws


def step(d, cfg, rm, rv, groups, fold=True):
    """Forward then backward through the raw ABI; rm / rv are updated in place by a training forward (fold=False: not handed to it).
    Everything a comparison needs, on the CPU."""
    rc, y, sm, sr = raw_fwd(d, cfg, rm if fold or not cfg.training else None, rv if fold or not cfg.training else None, stats=bool(cfg.training))
    assert rc == 0, L.lib().gmp_last_error_string()
    rc, gu, gg, gb, ws = raw_bwd(d, cfg, rm, rv, sm, sr, groups)
    assert rc == 0, L.lib().gmp_last_error_string()
    cpu = lambda t: None if t is None else t.cpu()
    return {"y": cpu(y), "mean": cpu(sm), "rstd": cpu(sr), "rm": rm.cpu(), "rv": rv.cpu(), "g_u": cpu(gu), "g_gamma": cpu(gg), "g_beta": cpu(gb), "ws": ws}


def hold(err, what, failures):
    for k, v in err.items():
        MEASURED[k] = max(MEASURED.get(k, 0.0), v)
        print(f"[measured] {k}: {v:.3e} ({what}); largest so far {MEASURED[k]:.3e}; bar {TOL[k]:.3e}")
        if not v <= TOL[k]:
            failures.append(f"{what}: {k} error {v:.3e} > {TOL[k]:.3e}")


def written(out, c, training, what):
    """Every row of y and g_u and the parameter gradients written (they were NaN-filled, the workspace too); statistics rows of live
    segments written, those of empty segments left alone."""
    assert bool(torch.isfinite(out["y"]).all()) and bool(torch.isfinite(out["g_u"]).all()), f"{what}: rows of y / g_u left unwritten"
    assert bool(torch.isfinite(out["g_gamma"]).all()) and bool(torch.isfinite(out["g_beta"]).all()), f"{what}: parameter gradients"
    if training:
        live = torch.tensor([n > 0 for n in c["sizes"]])
        for k in ("mean", "rstd"):
            assert bool(torch.isfinite(out[k][live]).all()), f"{what}: {k} of a live segment unwritten"
            assert bool(torch.isnan(out[k][~live]).all()), f"{what}: {k} row of an empty segment was written"


def gate_agrees(out, ref, what):
    sure = ref["pre"].abs() > R.delta_of(ref["y"])
    wrong = ((out["y"] != 0) != (ref["pre"] > 0)) & sure
    assert int(wrong.sum()) == 0, f"{what}: {int(wrong.sum())} ReLU decisions differ beyond delta"


def sync_state(sy, generations, what):
    h = sy[:3].tolist()
    assert h[0] == 0 and h[2] == 0 and h[1] == generations, f"{what}: sync header {h} (error, generation, departures), {generations} generations expected"


# ------------------------------------------------------------------------------------------------ regime and boundary sweep
@gpu
@pytest.mark.parametrize("C_", R.SWEEP_C)
@pytest.mark.parametrize("L_,sync", R.SWEEP)
def test_every_regime_and_switch_point_against_fp64(L_, sync, C_):
    c = R.sweep_case(L_, sync, C_)
    d = Dev(c)
    sy = sync_words(C_, d.S) if sync else None
    what, failures = f"L={L_} C={C_} sync={sync}", []
    rm, rv = d.rm.clone(), d.rv.clone()
    out = step(d, ops.make_bn_config(True, True, sync=sy), rm, rv, R.SWEEP_GROUPS)
    written(out, c, True, what + " train")
    err, ref = R.errors_against_ref(c, out, True)
    hold(err, what + " train", failures)
    gate_agrees(out, ref, what + " train")
    rm_in, rv_in = rm.cpu(), rv.cpu()
    assert not torch.equal(rm_in, c["rm"]) and not torch.equal(rv_in, c["rv"])
    oute = step(d, ops.make_bn_config(False, True, sync=sy), rm, rv, R.SWEEP_GROUPS)          # eval, on the updated running pair
    written(oute, c, False, what + " eval")
    assert torch.equal(oute["rm"], rm_in) and torch.equal(oute["rv"], rv_in), "eval mode moved the running pair"
    erre, refe = R.errors_against_ref(c, oute, False, rm_in=rm_in, rv_in=rv_in)
    hold(erre, what + " eval", failures)
    gate_agrees(oute, refe, what + " eval")
    if sync:                                    # training forward, backward, eval backward advance the generation; 4,097 rows run chunked
        sync_state(sy, 3 if L_ <= 4096 else 0, what)
        if L_ > 4096:
            assert not bool(sy.any())
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ seg_group
@gpu
@pytest.mark.parametrize("L_,sync", R.REGIME_ROWS)
def test_seg_group_selects_parameters_and_running_rows(L_, sync):
    """Through ops.bn_fwd / ops.bn_bwd: gamma, beta and the running pair are [3, C]; segment s reads and updates row seg_group[s], in
    segment order (group 0: the one-row segment, then the 64-row one); eval reads the same row; the split running update (single and
    batched) with the table equals the inline one bit for bit."""
    c, table = R.group_case(L_, sync)
    d = Dev(c, table)
    groups, what, failures = [0, 1, 3, 5], f"seg_group L={L_} sync={sync}", []
    sy = sync_words(d.C, d.S) if sync else None
    cfg = ops.make_bn_config(True, True, sync=sy)
    rm, rv = d.rm.clone(), d.rv.clone()
    y, sm, sr = ops.bn_fwd(d.x, d.res, d.seg, d.max, d.gamma, d.beta, rm, rv, cfg, seg_group=d.table)
    gu, gg, gb = ops.bn_bwd(d.gy, d.x, d.res, d.seg, d.max, d.gamma, d.beta, rm, rv, sm, sr, cfg, groups, seg_group=d.table)
    out = {"y": y.cpu(), "mean": sm.cpu(), "rstd": sr.cpu(), "rm": rm.cpu(), "rv": rv.cpu(), "g_u": gu.cpu(), "g_gamma": gg.cpu(), "g_beta": gb.cpu()}
    err, ref = R.errors_against_ref(c, out, True, groups=groups, seg_group=table)
    hold(err, what + " train", failures)
    gate_agrees(out, ref, what + " train")
    # the same launch without the running pair, then the two split updates with the table
    y2, sm2, sr2 = ops.bn_fwd(d.x, d.res, d.seg, d.max, d.gamma, d.beta, None, None, cfg, seg_group=d.table)
    live = torch.tensor([n > 0 for n in c["sizes"]], device=DEV)
    assert torch.equal(y, y2) and torch.equal(sm[live], sm2[live]) and torch.equal(sr[live], sr2[live])
    l, st = L.lib(), ops._stream(d.x)
    rm_b, rv_b, rm_c, rv_c = d.rm.clone(), d.rv.clone(), d.rm.clone(), d.rv.clone()
    L.check(l.gmp_bn_running_update(ops._ptr(d.seg), ops._ptr(d.table), d.S, d.C, ops._ptr(rm_b), ops._ptr(rv_b), ops._ptr(sm2), ops._ptr(sr2),
                                    C.byref(cfg), st), "gmp_bn_running_update")
    L.check(l.gmp_bn_running_update_batch(1, ops._ptr(d.seg), d.S, (P * 1)(d.table.data_ptr()), (C.c_int32 * 1)(d.C), (P * 1)(rm_c.data_ptr()),
                                          (P * 1)(rv_c.data_ptr()), (P * 1)(sm2.data_ptr()), (P * 1)(sr2.data_ptr()), C.byref(cfg), st),
            "gmp_bn_running_update_batch")
    assert torch.equal(rm, rm_b) and torch.equal(rv, rv_b), "gmp_bn_running_update with a seg_group table differs from the inline update"
    assert torch.equal(rm, rm_c) and torch.equal(rv, rv_c), "gmp_bn_running_update_batch with a seg_group table differs from the inline update"
    for k in range(3):
        assert not torch.equal(rm[k], d.rm[k]), f"group {k}: running mean untouched"
    # eval mode on the updated rows
    cfge = ops.make_bn_config(False, True, sync=sy)
    ye, _, _ = ops.bn_fwd(d.x, d.res, d.seg, d.max, d.gamma, d.beta, rm, rv, cfge, seg_group=d.table)
    gue, gge, gbe = ops.bn_bwd(d.gy, d.x, d.res, d.seg, d.max, d.gamma, d.beta, rm, rv, None, None, cfge, groups, seg_group=d.table)
    oute = {"y": ye.cpu(), "g_u": gue.cpu(), "g_gamma": gge.cpu(), "g_beta": gbe.cpu()}
    erre, refe = R.errors_against_ref(c, oute, False, groups=groups, seg_group=table, rm_in=rm.cpu(), rv_in=rv.cpu())
    hold(erre, what + " eval", failures)
    gate_agrees(oute, refe, what + " eval")
    if sync:
        sync_state(sy, 4, what)                 # two training forwards, two backwards (the eval forward does not rendezvous)
    assert not failures, "\n".join(failures)


@gpu
def test_ops_checks_the_grouped_parameter_shapes():
    c, table = R.group_case(300, False)
    d = Dev(c, table)
    cfg = ops.make_bn_config(True, True)
    with pytest.raises(L.GnnmpError):
        ops.bn_fwd(d.x, d.res, d.seg, d.max, d.gamma[0], d.beta[0], None, None, cfg, seg_group=d.table)          # [C] with a table
    with pytest.raises(L.GnnmpError):
        ops.bn_fwd(d.x, d.res, d.seg, d.max, d.gamma, d.beta, None, None, cfg, seg_group=d.table[:4].contiguous())   # S - 1 entries
    with pytest.raises(L.GnnmpError):
        ops.bn_fwd(d.x, d.res, d.seg, d.max, d.gamma, d.beta, d.rm[:2].contiguous(), d.rv, cfg, seg_group=d.table)   # running rows != groups
    with pytest.raises(L.GnnmpError):
        ops.bn_fwd(d.x, d.res, d.seg, d.max, d.gamma, d.beta, None, None, cfg)                                       # [3, C] without a table
    with pytest.raises(L.GnnmpError):
        ops.bn_bwd(d.gy, d.x, d.res, d.seg, d.max, d.gamma, d.beta[:, :64].contiguous(), None, None, d.rm, d.rv, cfg, seg_group=d.table)


# ------------------------------------------------------------------------------------------------ dropout gate
@gpu
@pytest.mark.parametrize("L_,sync", R.REGIME_ROWS)
def test_backward_regenerates_the_forward_dropout_gate(L_, sync):
    """p = 0.2 in every regime: the forward mask drops 17-23 % of the positive elements, kept elements are y_nodrop / 0.8, and the backward
    (gate_of in the short, medium and slab kernels, bwd_elem in the chunked ones) agrees with bn_ref_bwd given the gate read off the
    forward output -- so it regenerated that gate."""
    c = R.dropout_case(L_, sync)
    d = Dev(c)
    what, failures = f"dropout L={L_} sync={sync}", []
    sy = sync_words(d.C, d.S) if sync else None
    rm, rv = d.rm.clone(), d.rv.clone()
    out0 = step(d, ops.make_bn_config(True, True, sync=sy), rm, rv, R.SWEEP_GROUPS, fold=False)
    cfg = ops.make_bn_config(True, True, dropout_p=0.2, seed=4242, stream_id=7, sync=sy)
    out = step(d, cfg, rm, rv, R.SWEEP_GROUPS, fold=False)
    written(out, c, True, what)
    y64, pre, *_ = R.bn_ref_fwd(c["x"], c["res"], c["seg"], None, c["gamma"], c["beta"], None, None, True, True)
    pos = pre > R.delta_of(y64)
    kept = out["y"] != 0
    assert not bool((kept & (pre < -R.delta_of(y64))).any()), "an element the ReLU zeroes came through"
    dropped = 1.0 - (kept & pos).sum().item() / pos.sum().item()
    print(f"[measured] {what}: dropped share {dropped:.4f}")
    assert 0.17 <= dropped <= 0.23, f"{what}: dropped share {dropped:.4f}"
    want = out0["y"].double() / 0.8
    e = (out["y"].double() - want)[kept].abs().max().item() / want.abs().max().item()
    print(f"[measured] {what}: kept elements against y_nodrop / 0.8: {e:.3e}; bar {TOL['y_live']:.3e}")
    assert e <= TOL["y_live"]                   # (the tighter of the two forward bars: one rounded multiplication)
    err, _ = R.errors_against_ref(c, out, True, drop=1.25)
    del err["rm"], err["rv"]                    # (the running pair was kept out of these launches)
    hold(err, what, failures)
    if sync:
        sync_state(sy, 4, what)
    assert not failures, "\n".join(failures)


# ------------------------------------------------------------------------------------------------ slab regime
@gpu
@pytest.mark.parametrize("C_", [64, 192])
@pytest.mark.parametrize("rows", [1025, 4096])
def test_slab_kernels_fold_running_and_write_parameter_gradients_like_the_split_calls(rows, C_):
    """S == 1, one gradient group: the forward slab kernel folds the running pair itself and the backward one writes g_gamma / g_beta
    itself.  Both must equal, bit for bit, the split forms: a forward without the running pair plus gmp_bn_running_update, a backward with
    0 groups plus gmp_bn_param_grads on its workspace."""
    c = R.make_case([rows], C_, seed=19 * rows + C_)
    d = Dev(c)
    sy = sync_words(C_, 1)
    cfg = ops.make_bn_config(True, True, sync=sy)
    rm, rv = d.rm.clone(), d.rv.clone()
    a = step(d, cfg, rm, rv, [0, 1])                                         # fold_running, pg_gamma / pg_beta
    written(a, c, True, "slab S=1")
    l, st = L.lib(), ops._stream(d.x)
    rc, y, sm, sr = raw_fwd(d, cfg, None, None)
    assert rc == 0
    rm_b, rv_b = d.rm.clone(), d.rv.clone()
    L.check(l.gmp_bn_running_update(ops._ptr(d.seg), None, 1, C_, ops._ptr(rm_b), ops._ptr(rv_b), ops._ptr(sm), ops._ptr(sr), C.byref(cfg), st), "ru")
    assert torch.equal(a["y"], y.cpu()) and torch.equal(a["mean"], sm.cpu()) and torch.equal(a["rstd"], sr.cpu())
    assert torch.equal(rm, rm_b), f"running mean folded by the slab kernel differs in {int((rm != rm_b).sum())} columns from bn_running_kernel's"
    assert torch.equal(rv, rv_b), f"running var folded by the slab kernel differs in {int((rv != rv_b).sum())} columns from bn_running_kernel's"
    assert not torch.equal(rm, d.rm)
    rc, gu, _, _, ws = raw_bwd(d, cfg, None, None, sm, sr, [0, 1], num_groups=0)
    assert rc == 0
    gg, gb = nan(1, C_), nan(1, C_)
    L.check(l.gmp_bn_param_grads(ops._ptr(ws), 1, C_, ops._ptr(gg), ops._ptr(gb), C.cast((C.c_int32 * 2)(0, 1), P), None, None, 1, st), "pg")
    assert torch.equal(a["g_u"], gu.cpu()) and torch.equal(a["g_gamma"], gg.cpu()) and torch.equal(a["g_beta"], gb.cpu())
    failures = []
    err, ref = R.errors_against_ref(c, a, True, groups=[0, 1])
    hold(err, f"slab S=1 rows={rows} C={C_}", failures)
    sync_state(sy, 4, "slab S=1")
    assert not failures, "\n".join(failures)


@gpu
def test_one_sync_tensor_serves_slab_launches_of_changing_shapes():
    """Granules of earlier launches never carry the current tag, whatever their shapes: a sequence of slab-regime launches that changes
    (S, C, rows) on ONE sync tensor gives, launch by launch, the bits of the same call on freshly zeroed words.  Every training forward and
    every backward advances the generation (slab_depart); the waits are bounded by the kernel's own 2 s clock."""
    shapes = [([4096], 192), ([1100, 300, 1050], 64), ([1025], 64), ([2000, 1500], 192), ([4096], 192)]
    shared = torch.zeros(max(ops.bn_sync_words(C_, len(sizes)) for sizes, C_ in shapes), dtype=torch.int32, device=DEV)
    launches = 0
    for i, (sizes, C_) in enumerate(shapes):
        c = R.make_case(sizes, C_, seed=23 + i)
        d = Dev(c)
        groups = [0, len(sizes)]
        outs = []
        for sy in (shared, sync_words(C_, len(sizes))):
            rm, rv = d.rm.clone(), d.rv.clone()
            outs.append(step(d, ops.make_bn_config(True, True, dropout_p=0.2, seed=5, stream_id=i, sync=sy), rm, rv, groups))
        launches += 2
        for k in ("y", "mean", "rstd", "rm", "rv", "g_u", "g_gamma", "g_beta"):
            assert torch.equal(outs[0][k], outs[1][k]), f"launch {i} {sizes} x {C_}: {k} differs on the reused sync words"
        written(outs[0], c, True, f"launch {i}")
        sync_state(shared, launches, f"after launch {i}")
    assert launches == 10


@gpu
@pytest.mark.parametrize("rows", [1100, 4000])
def test_too_few_sync_words_fall_back_to_the_form_without_them(rows):
    """One word fewer than bn_sync_words(C, S): the strip (1,100 rows) or chunked (4,000 rows) form runs, bit-identical to sync=None, and
    no word is touched."""
    c = R.make_case([rows, 1, 0, 37], 192, seed=29 + rows)
    d = Dev(c)
    few = sync_words(192, 4, short=1)
    outs = []
    for sy in (None, few):
        rm, rv = d.rm.clone(), d.rv.clone()
        outs.append(step(d, ops.make_bn_config(True, True, dropout_p=0.2, seed=5, stream_id=2, sync=sy), rm, rv, R.SWEEP_GROUPS))
    live = torch.tensor([n > 0 for n in c["sizes"]])
    for k in ("y", "rm", "rv", "g_u", "g_gamma", "g_beta"):
        assert torch.equal(outs[0][k], outs[1][k]), f"{k} differs"
    assert torch.equal(outs[0]["mean"][live], outs[1]["mean"][live]) and torch.equal(outs[0]["rstd"][live], outs[1]["rstd"][live])
    assert not bool(few.any()), "the fallback wrote to the sync words"
    full = sync_words(192, 4)                                                # (and with the full count the slab form does run: the words move)
    rm, rv = d.rm.clone(), d.rv.clone()
    step(d, ops.make_bn_config(True, True, dropout_p=0.2, seed=5, stream_id=2, sync=full), rm, rv, R.SWEEP_GROUPS)
    sync_state(full, 2, "full sync words")


# ------------------------------------------------------------------------------------------------ argument errors
@gpu
def test_argument_errors_come_back_as_codes_and_nothing_is_launched():
    c = R.make_case([300, 1, 0, 37], 192, seed=31)
    d = Dev(c)
    train, evalc = ops.make_bn_config(True, True), ops.make_bn_config(False, True)
    rm, rv = d.rm.clone(), d.rv.clone()
    untouched = lambda *ts: all(bool(torch.isnan(t).all()) for t in ts if t is not None)

    def fwd_fails(code, cfg, **kw):
        rm_, rv_ = kw.pop("rm", rm), kw.pop("rv", rv)
        rc, y, sm, sr = raw_fwd(d, cfg, rm_, rv_, **kw)
        torch.cuda.synchronize()
        assert rc == code, f"{kw}: code {rc}, {code} expected ({L.lib().gmp_last_error_string()})"
        assert untouched(y, sm, sr) and torch.equal(rm, d.rm) and torch.equal(rv, d.rv), f"{kw}: something was written"

    fwd_fails(ERR_ARG, train, Cc=96)                                         # C must be a multiple of 64
    fwd_fails(ERR_ARG, ops.make_bn_config(True, True, dropout_p=1.0))
    fwd_fails(ERR_ARG, ops.make_bn_config(True, True, dropout_p=-0.1))
    fwd_fails(ERR_ARG, train, max_rows=d.rows + 1)                           # max_seg_rows > rows
    fwd_fails(ERR_ARG, train, stats=False)                                   # training without save_mean / save_rstd
    fwd_fails(ERR_ARG, evalc, rm=None, rv=None)                              # eval without the running pair
    fwd_fails(ERR_WORKSPACE, train, ws_short=1)                              # workspace one byte short
    rc, y, sm, sr = raw_fwd(d, train, rm, rv)
    assert rc == 0                                                           # (the same call, complete, runs)

    def bwd_fails(code, groups, **kw):
        rc, gu, gg, gb, _ = raw_bwd(d, train, None, None, sm, sr, groups, **kw)
        torch.cuda.synchronize()
        assert rc == code, f"groups {groups}: code {rc}, {code} expected ({L.lib().gmp_last_error_string()})"
        assert untouched(gu, gg, gb), f"groups {groups}: something was written"

    bwd_fails(ERR_ARG, list(range(MAX_GROUPS + 2)), num_groups=MAX_GROUPS + 1)      # G > GMP_MAX_GROUPS
    bwd_fails(ERR_ARG, [0, 2, d.S + 1])                                      # a group table running past S
    bwd_fails(ERR_ARG, [0, 3, 2])                                            # ... or backwards
    l = L.lib()
    nb = l.gmp_bn_workspace_bytes(d.rows, d.C, d.S, d.max)
    ws, gu, gg, gb = torch.empty(nb, dtype=torch.uint8, device=DEV), nan(d.rows, d.C), nan(2, d.C), nan(2, d.C)
    arr = (C.c_int32 * 3)(0, 2, 4)
    bwd = lambda ws_bytes, cfg, sm_: l.gmp_bn_bwd(ops._ptr(d.gy), ops._ptr(d.x), ops._ptr(d.res), ops._ptr(d.seg), None, d.S, d.max, d.rows, d.C, ops._ptr(d.gamma),
                                                  ops._ptr(d.beta), None, None, ops._ptr(sm_), ops._ptr(sr), ops._ptr(gu), ops._ptr(gg), ops._ptr(gb), C.cast(arr, P),
                                                  None, None, 2, C.byref(cfg), ops._ptr(ws), ws_bytes, ops._stream(d.x))
    assert bwd(nb - 1, train, sm) == ERR_WORKSPACE
    assert bwd(nb, train, None) == ERR_ARG                                   # training without the saved statistics
    assert bwd(nb, evalc, sm) == ERR_ARG                                     # eval without the running pair
    torch.cuda.synchronize()
    assert untouched(gu, gg, gb)
    assert bwd(nb, train, sm) == 0 and bool(torch.isfinite(gu).all())


@gpu
def test_no_rows_zero_both_gradient_groups():
    l = L.lib()
    Cc = 64
    gg, gb = nan(2, Cc), nan(2, Cc)
    seg = torch.zeros(3, dtype=torch.int32, device=DEV)                      # two empty segments
    cfg = ops.make_bn_config(True, True)
    arr = (C.c_int32 * 3)(0, 1, 2)
    rc = l.gmp_bn_bwd(None, None, None, ops._ptr(seg), None, 2, 0, 0, Cc, None, None, None, None, None, None, None, ops._ptr(gg), ops._ptr(gb),
                      C.cast(arr, P), None, None, 2, C.byref(cfg), None, 0, ops._stream(seg))
    assert rc == 0
    assert torch.equal(gg, torch.zeros(2, Cc, device=DEV)) and torch.equal(gb, torch.zeros(2, Cc, device=DEV))
    y = nan(1, Cc)
    rc = l.gmp_bn_fwd(None, None, ops._ptr(seg), None, 2, 0, 0, Cc, None, None, None, None, None, None, ops._ptr(y), C.byref(cfg), None, 0, ops._stream(seg))
    assert rc == 0 and bool(torch.isnan(y).all())
