"""The gradient-surgery rules of the optimisation step's tail (csrc/optim.hip through gmp_mt_surgery_clip_adamw) against their float64
restatement (tests/surgery_ref.py), direct calls with apply_update=0, and one engine step under the published PCGrad.

The problems are built here without a GPU; tests/test_surgery_host.py checks on the CPU that each of them keeps every decision a walk
takes (the sign of a dot product, a norm that is zero or not) at least MARGIN away from flipping, so the float32 Gram matrices of the
kernel decide as the restatement does and the two counts can be compared exactly.  The seeds were chosen there, from the restatement
alone.  Bars: those of check_pcgrad in tests/test_gpu_optim.py -- final_grad within 1e-5 of the tensor's input scale, normsq within
1e-5 of its own final_grad and 1e-4 of the restatement's.
"""
import ctypes as C
import random

import numpy as np
import pytest
import torch

import surgery_ref as SR
from test_gpu_optim import (BETA1, BETA2, C_MAX_NORM, DEV, EPS, MARGIN, MAXT, RANGES, Kernel, Layout, assert_same_bits, b_state,  # noqa: F401
                            make_grads, many_tensors_problem)

gpu = pytest.mark.gpu
RULES = {"reference": 0, "pcgrad": 1, "mean": 2}
SCOPES = {"tensor": 0, "model": 1}
MODES = (("pcgrad", "tensor"), ("pcgrad", "model"), ("mean", "tensor"))

SMALL_LENS = (1, 3, 4, 5, 4095, 4096, 4097)      # one chunk and its boundary
LONG_LENS = (8193, 131076)                        # three chunks / the 32-chunk cap with chunks past 4,096 floats


def holder_rows(rs, T, order, extra_task, lens_small, lens_long):
    """(lens, has, zero): every small length under every holder pattern -- all tasks of the order, exactly one holder at each order position,
    two holders, none, all with one exactly-zero gradient -- and the long ones under `all` and `two`; extra_task (when there is one) holds
    every other tensor, so it lands on flagged and on otherwise unflagged tensors."""
    n = len(order)
    pats = ["all", "two", "none", "zero"] + [("one", p) for p in range(n)]
    lens, rows, zero = [], [], []
    for g, (ln, plist) in enumerate([(l, pats) for l in lens_small] + [(l, ["all", "two"]) for l in lens_long]):
        for i, p in enumerate(plist):
            row = np.zeros(MAXT, np.uint8)
            if p in ("all", "zero"):
                row[order] = 1
            elif p == "two":
                row[[order[i] for i in rs.choice(n, 2, replace=False)]] = 1
            elif p != "none":
                row[order[p[1]]] = 1
            if p == "zero":
                zero.append((len(rows), order[int(rs.randint(n))]))
            if extra_task >= 0 and (g + i) % 2:
                row[extra_task] = 1
            lens.append(ln)
            rows.append(row)
    return lens, np.stack(rows), zero


def rule_problem(T, n_order, extra, long, seed, lone=False):
    """-> lay, T, has, tg, order, perm, extra_task.  lone: the task at the last order position holds no tensor another task holds
    (a task head's owner that shares nothing: model scope leaves it out of the one walk)."""
    rs = np.random.RandomState(seed)
    extra_task = T - 1 if extra else -1
    main = [t for t in range(T) if t != extra_task]
    order = [int(t) for t in rs.permutation(main)[:n_order]]
    lens, has, zero = holder_rows(rs, T, order, extra_task, SMALL_LENS, LONG_LENS if long else ())
    if lone:
        shared = has[:, order].sum(1) >= 2
        has[shared, order[-1]] = 0
        zero = [(k, t) for k, t in zero if t != order[-1]]
    lay = Layout(lens)
    perm = SR.draw_perm(random.Random(seed), n_order)
    return lay, T, has, make_grads(seed, lay, T, has, zero=zero), order, perm, extra_task


def many_rule_problem(seed):
    """300 short tensors under random patterns: five solve blocks, more tensors than the fold's 64-tensor tile and the norm pass's block"""
    rs = np.random.RandomState(seed)
    T, order, extra_task, K = 5, [2, 0, 3, 1], 4, 300
    has, zero = np.zeros((K, MAXT), np.uint8), []
    for k in range(K):
        p = rs.randint(5)
        if p in (0, 4):
            has[k, order] = 1
        elif p == 1:
            has[k, [order[i] for i in rs.choice(4, 2, replace=False)]] = 1
        elif p == 2:
            has[k, order[rs.randint(4)]] = 1
        if p == 4:
            zero.append((k, order[rs.randint(4)]))
        has[k, extra_task] = rs.rand() < 0.3
    lay = Layout(list(rs.randint(16, 700, K)))
    return lay, T, has, make_grads(seed, lay, T, has, zero=zero), order, SR.draw_perm(random.Random(seed), 4), extra_task


CASES = {    # T, n_order, extra task outside the order, long tensors, lone last task, seed
    "T2": (2, 2, False, True, False, 201),
    "T3_order2_extra": (3, 2, True, False, False, 202),
    "T3": (3, 3, False, False, False, 203),
    "T5_order4_extra": (5, 4, True, True, False, 204),
    "T5": (5, 5, False, False, False, 205),
    "T5_lone": (5, 5, False, False, True, 206),
    "T8_order7_extra": (8, 7, True, False, False, 207),
    "T8": (8, 8, False, True, False, 208),
}
MANY_SEED = 17


def case_problem(case):
    if case == "many":
        return many_rule_problem(MANY_SEED)
    T, n_order, extra, long, lone, seed = CASES[case]
    return rule_problem(T, n_order, extra, long, seed, lone)


# ------------------------------------------------------------------------------------------------ the C ABI
class RuleKernel(Kernel):
    """test_gpu_optim.Kernel's buffers under gmp_mt_surgery_clip_adamw"""

    def call_rule(self, rule, scope, perm, order, extra_task, *, last_task=-1, max_norm=0.0, apply_update=0, k_begin=0, k_end=None, phases=None):
        from gnn_pretraining_amd import ops
        ptr = ops._ptr
        if phases is None:
            phases = 26 if (rule, scope) == (RULES["pcgrad"], SCOPES["model"]) else 3
        o = (C.c_int32 * MAXT)(*(list(order) + [0] * (MAXT - len(order))))
        flat = [j for row in perm for j in row] if perm is not None else []
        pp = (C.c_int32 * max(len(flat), 1))(*flat) if perm is not None else None
        return self.lib.gmp_mt_surgery_clip_adamw(
            rule, scope, pp, ptr(self.tg), self.lay.P, self.T, self.lay.K, ptr(self.off), ptr(self.len), ptr(self.has),
            o, len(order), last_task, extra_task, ptr(self.params), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self.steps),
            ptr(self.lr), ptr(self.wd), BETA1, BETA2, EPS, max_norm, ptr(self.final), ptr(self.normsq), ptr(self.metrics), ptr(self.flags),
            ptr(self.ws), self.ws_bytes, apply_update, k_begin, self.lay.K if k_end is None else k_end, phases, None, ops._stream(self.final))

    def run_rule(self, mode, *args, **kw):
        rule, scope = mode
        self.L.check(self.call_rule(RULES[rule], SCOPES[scope], *args, **kw), "gmp_mt_surgery_clip_adamw")
        torch.cuda.synchronize()


_REF = {}


def restatement(case, mode):
    """computed once per (case, mode), shared, never changed"""
    if (case, mode) not in _REF:
        lay, T, has, tg, order, perm, extra_task = case_problem(case)
        _REF[case, mode] = SR.surgery(tg, lay, has, order, perm, mode[0], mode[1], -1, extra_task)
    return _REF[case, mode]


def check_rule(case, mode):
    lay, T, has, tg, order, perm, extra_task = case_problem(case)
    ref, (conf, proj), margin = restatement(case, mode)
    assert margin >= MARGIN, "the data sits too close to a decision of a walk"
    kern = RuleKernel(lay, T, has, tg)
    kern.final.fill_(float("nan"))                 # whatever is flagged is written
    kern.run_rule(mode, perm, order, extra_task)
    out = kern.outputs()
    flags = out["flags"].numpy()
    assert flags.tolist() == [int(g is not None) for g in ref], "flags"
    assert out["metrics"].tolist() == [conf, proj], f"conflicts / projections {out['metrics'].tolist()} vs {[conf, proj]}"
    fin = out["final"].double()
    worst = 0.0
    for k in range(lay.K):
        if ref[k] is None:
            continue
        scale = max(tg[t, lay.slot(k)].abs().max().item() for t in range(T) if has[k, t])
        err = (fin[lay.slot(k)] - ref[k]).abs().max().item()
        worst = max(worst, err / scale if scale else 0.0)
        assert err <= 1e-5 * scale, f"final_grad of tensor {k} (len {lay.lens[k]}): {err:.3e} > 1e-5 x {scale:.3e}"
    own = sum(float((fin[lay.slot(k)] ** 2).sum()) for k in range(lay.K) if flags[k])
    want = sum(float((g ** 2).sum()) for g in ref if g is not None)
    got = float(out["normsq"])
    print(f"{case} {mode}: counts {conf}/{proj}, margin {margin:.2e}, worst final_grad error {worst:.2e} of scale, "
          f"normsq {abs(got - own) / own:.2e} own / {abs(got - want) / want:.2e} ref")
    assert abs(got - own) <= 1e-5 * own, f"normsq {got} vs its own final_grad {own}"
    assert abs(got - want) <= 1e-4 * want, f"normsq {got} vs the restatement {want}"
    if mode == ("pcgrad", "tensor"):
        assert conf > 0, "the problem has no conflict"


@gpu
@pytest.mark.parametrize("mode", MODES, ids=["-".join(m) for m in MODES])
@pytest.mark.parametrize("case", list(CASES) + ["many"])
def test_rules_match_float64(case, mode):
    check_rule(case, mode)


# ------------------------------------------------------------------------------------------------ bitwise identities
def state_problem():
    lay, T, has, tg, order, perm, extra_task = many_rule_problem(MANY_SEED)
    return lay, T, has, tg, order, perm, extra_task, b_state(41, lay)


@gpu
def test_reference_rule_through_the_new_entry_has_the_bits_of_the_existing_call():
    lay, T, has, tg, order, last_task, extra_task = many_tensors_problem(7)
    state = b_state(41, lay)
    old = RuleKernel(lay, T, has, tg, *state)
    old.run(order, last_task, extra_task, max_norm=C_MAX_NORM, apply_update=1)
    assert old.metrics[1] > 0
    for scope, perm in (("tensor", None), ("model", SR.identity_perm(len(order)))):      # neither is read under this rule
        new = RuleKernel(lay, T, has, tg, *state)
        new.run_rule(("reference", scope), perm, order, extra_task, last_task=last_task, max_norm=C_MAX_NORM, apply_update=1, phases=3)
        assert_same_bits(old.outputs(), new.outputs(), f"reference rule, scope {scope}")
    # ... in pieces and with the foreign pass too
    parts = RuleKernel(lay, T, has, tg, *state)
    kw = dict(last_task=last_task, max_norm=C_MAX_NORM, apply_update=1)
    a, b = RANGES[1]
    parts.final[lay.off[a]:lay.off[b]] = old.final[lay.off[a]:lay.off[b]]
    parts.run_rule(("reference", "tensor"), None, order, extra_task, k_begin=a, k_end=b, phases=4, **kw)
    parts.run_rule(("reference", "tensor"), None, order, extra_task, k_begin=0, k_end=a, phases=1, **kw)
    parts.run_rule(("reference", "tensor"), None, order, extra_task, k_begin=b, k_end=lay.K, phases=1, **kw)
    parts.run_rule(("reference", "tensor"), None, order, extra_task, phases=2, **kw)
    want, got = dict(old.outputs(), metrics=None), dict(parts.outputs(), metrics=None)
    assert_same_bits(want, got, "reference rule in pieces")


@gpu
@pytest.mark.parametrize("mode", MODES, ids=["-".join(m) for m in MODES])
def test_ranges_have_the_bits_of_the_one_shot_call(mode):
    """tensor scope: phase 1 over ranges, then 2.  Model scope: phase 8 (Gram only) over ranges, then 16 | 2."""
    lay, T, has, tg, order, perm, extra_task, state = state_problem()
    kw = dict(max_norm=C_MAX_NORM, apply_update=1)
    one = RuleKernel(lay, T, has, tg, *state)
    one.run_rule(mode, perm, order, extra_task, **kw)
    want = one.outputs()
    assert int(want["flags"].sum()) < lay.K and (mode[0] == "mean" or want["metrics"][0] > 0)
    assert not torch.equal(want["params"], torch.as_tensor(state[0])), "no update"
    model = mode == ("pcgrad", "model")
    parts = RuleKernel(lay, T, has, tg, *state)
    for a, b in RANGES:
        parts.run_rule(mode, perm, order, extra_task, k_begin=a, k_end=b, phases=8 if model else 1, **kw)
    parts.run_rule(mode, perm, order, extra_task, phases=16 | 2 if model else 2, **kw)
    assert_same_bits(want, parts.outputs(), f"{mode} in ranges")


# ------------------------------------------------------------------------------------------------ argument validation
def _dup(perm):
    bad = [list(r) for r in perm]
    bad[1][0] = bad[1][1]
    return bad


def _own(perm):
    bad = [list(r) for r in perm]
    bad[2][0] = 2
    return bad


BAD = {     # -> rule, scope, perm (None = the good one; a callable changes it), phases
    "rule_3": (3, 0, None, 3),
    "rule_negative": (-1, 0, None, 3),
    "scope_2": (1, 2, None, 3),
    "perm_row_repeats_a_position": (1, 0, _dup, 3),
    "perm_row_holds_its_own_position": (1, 0, _own, 3),
    "perm_out_of_range": (1, 0, lambda p: [[len(p)] + list(p[0][1:])] + p[1:], 3),
    "perm_missing": (1, 0, lambda p: None, 3),
    "foreign_pass_with_pcgrad": (1, 0, None, 4),
    "foreign_pass_with_mean": (2, 0, None, 4 | 2),
    "bit_0_with_model_scope": (1, 1, None, 1 | 2),
    "gram_only_phase_with_tensor_scope": (1, 0, None, 8),
    "phases_0": (1, 1, None, 0),
}


@gpu
@pytest.mark.parametrize("case", list(BAD))
def test_bad_arguments_are_refused_and_launch_nothing(case):
    GMP_ERR_ARG = -1                  # include/gnnmp.h
    lay, T, order = Layout([5, 4097, 64]), 4, [2, 0, 3, 1]
    has = np.zeros((lay.K, MAXT), np.uint8)
    has[:, :T] = 1
    kern = RuleKernel(lay, T, has, make_grads(5, lay, T, has), *b_state(5, lay)[:3], np.zeros(lay.K, np.float32), *b_state(5, lay)[4:])
    kern.final.fill_(7.0)
    kern.normsq.fill_(-3.0)
    kern.metrics.fill_(-5)
    kern.flags.fill_(-9)
    before = kern.outputs()
    rule, scope, change, phases = BAD[case]
    perm = SR.draw_perm(random.Random(3), len(order))
    if change is not None:
        perm = change(perm)
    rc = kern.call_rule(rule, scope, perm, order, -1, max_norm=C_MAX_NORM, apply_update=1, phases=phases)
    torch.cuda.synchronize()
    assert rc == GMP_ERR_ARG, rc
    assert_same_bits(before, kern.outputs(), case)


# ------------------------------------------------------------------------------------------------ the engine
@gpu
@pytest.mark.parametrize("overlap", ["1", "0"], ids=["parts", "one_shot"])
@pytest.mark.parametrize("scope", ["tensor", "model"])
def test_engine_step_under_pcgrad_trains_every_head(monkeypatch, scope, overlap):
    """One s4 step: every tensor gets a gradient (under the reference rule the link-prediction head and, unless node_feat_mask is shuffled
    first, mask_token get none), and final_grad has the bits of a direct call on the engine's own per-task gradients, availability table
    and permutation table -- with the optimizer's parts beside the backward (model scope: Gram per part, one fold + solve + combine at
    the end) and as one call behind it."""
    from test_gpu_engine import build
    monkeypatch.setenv("GMP_OPT_OVERLAP", overlap)
    rng = random.Random(9)
    _, hm, eng, host, inp, gen, tasks, domains = build("s4", 61, shuffle_rng=rng, surgery="pcgrad", surgery_scope=scope)
    assert eng.parts_beside_backward == (overlap == "1" and eng.use_gates)
    eng.lr.mul_(1000)
    before = {k: v.detach().cpu().clone() for k, v in hm.state_dict().items()}
    eng.step(inp, gen, art=eng.draw(inp, gen))
    torch.cuda.synchronize()
    eng.check_gates()
    assert eng.last_order == [t for t in tasks if t != "domain_adv"]
    n = len(eng.last_order)
    twin = random.Random(9)                        # for each task in turn, one shuffle of the others
    assert eng.last_perm == SR.draw_perm(twin, n) and rng.getstate() == twin.getstate()
    assert eng.flags.cpu().tolist() == [1] * eng.K
    assert eng.steps.cpu().tolist() == [1.0] * eng.K
    after = hm.state_dict()
    for name in ("heads.link_pred.predictor.mlp.0.weight", "mask_token", "heads.node_contrast.NCI1.mlp.3.weight", "heads.graph_prop.MUTAG.mlp.0.weight",
                 "gnn_backbone.layers.0.gin_conv.nn.0.weight"):
        assert not torch.equal(before[name], after[name].cpu()), f"{name} did not move"
    conf, proj = eng.metrics.cpu().tolist()
    assert 0 < conf <= proj
    lay = Layout(eng.t_len.tolist(), eng.t_off.tolist(), eng.P)
    kern = RuleKernel(lay, eng.T, eng.has.cpu().numpy(), eng.task_grads)
    kern.run_rule(("pcgrad", scope), eng.last_perm, list(range(n)), -1)
    assert torch.equal(kern.final.view(torch.int32), eng.final_grad.view(torch.int32)), "final_grad"
    assert torch.equal(kern.flags, eng.flags) and kern.metrics.cpu().tolist() == [conf, proj]
    assert float(kern.normsq) == float(eng.normsq)


@gpu
def test_engine_under_the_reference_rule_draws_and_leaves_what_it_always_did():
    """the default engine: one shuffle of the task list per step from the seeded stream, no permutation table, and the link-prediction
    head without a gradient whenever link_pred is neither shuffled first nor the last task"""
    from test_gpu_engine import build
    rng = random.Random(9)
    _, hm, eng, host, inp, gen, tasks, domains = build("s4", 61, shuffle_rng=rng)
    assert (eng.surgery, eng.surgery_scope) == ("reference", "tensor")
    eng.step(inp, gen, art=eng.draw(inp, gen))
    torch.cuda.synchronize()
    twin, order = random.Random(9), [t for t in tasks if t != "domain_adv"]
    twin.shuffle(order)
    assert eng.last_order == order and eng.last_perm is None and rng.getstate() == twin.getstate()
    assert order[0] != "link_pred" and tasks[-1] != "link_pred"
    assert eng.flags[eng.name_index["heads.link_pred.predictor.mlp.0.weight"]].item() == 0


@gpu
def test_engine_refuses_what_the_rules_do_not_cover():
    from test_gpu_engine import build
    for kw in (dict(surgery="pcgrad", dp_mode="sharded"), dict(surgery="mean", dp_mode="sharded"), dict(surgery="nope"),
               dict(surgery="pcgrad", surgery_scope="nope"), dict(surgery="reference", surgery_scope="model")):
        with pytest.raises(ValueError):
            build("b2", 1, **kw)
