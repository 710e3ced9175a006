"""The gradient-surgery rules without a GPU: the float64 restatement (tests/surgery_ref.py) against answers worked by hand and against
the existing reference of the reference rule; control.GradientSurgery (the module path's host Gram solve) against the restatement for
every rule and scope; the random stream each rule consumes; the margins of the problems tests/test_gpu_surgery.py runs on the device;
the command line and the C ABI's declaration."""
import random

import numpy as np
import pytest
import torch

import surgery_ref as SR
import test_gpu_surgery as G
from gnn_pretraining_amd.pretrain import control as Cn
from test_gpu_optim import MARGIN, MAXT, TOY_TASKS, Layout, Toy, edge_problem, many_tensors_problem, pcgrad_min_margin, ref_pcgrad

ALL_MODES = (("reference", "tensor"),) + G.MODES


def tiny(vectors):
    """one tensor, task t's gradient = vectors[t] (None = the task lacks it)"""
    T, n = len(vectors), max(len(v) for v in vectors if v is not None)
    lay = Layout([n])
    tg, has = torch.zeros(T, lay.P, dtype=torch.float64), np.zeros((1, MAXT), np.uint8)
    for t, v in enumerate(vectors):
        if v is not None:
            tg[t, :n] = torch.tensor(v, dtype=torch.float64)
            has[0, t] = 1
    return tg, lay, has


@pytest.mark.parametrize("scope", ["tensor", "model"])
def test_known_answers_by_hand(scope):
    run = lambda vecs, perm=None: SR.surgery(*tiny(vecs), list(range(len(vecs))), perm or SR.identity_perm(len(vecs)), "pcgrad", scope)
    # v1 = g1 + 1/2 g2 = (.5, .5), v2 = g2 + g1 = (0, 1)
    final, counts, margin = run([(1.0, 0.0), (-1.0, 1.0)])
    assert torch.allclose(final[0], torch.tensor([0.25, 0.75], dtype=torch.float64), rtol=0, atol=1e-15) and counts == (2, 2)
    assert abs(margin - 2 ** -0.5) < 1e-12                       # |cos| of the pair
    final, counts, _ = run([(2.0, 0.0), (0.0, 4.0)])             # orthogonal: the plain mean, two pairs met, no conflict
    assert torch.equal(final[0], torch.tensor([1.0, 2.0], dtype=torch.float64)) and counts == (0, 2)
    final, counts, _ = run([(1.0, -2.0, 0.5), (-1.0, 2.0, -0.5)])          # g2 = -g1: each is projected onto nothing
    assert torch.equal(final[0], torch.zeros(3, dtype=torch.float64)) and counts == (2, 2)
    # three tasks: task 0 conflicts with both others, and the order it meets them in changes what is left of it
    g = [(1.0, 0.0), (-1.0, 1.0), (-1.0, -0.5)]
    a, ca, _ = run(g, [[1, 2], [0, 2], [0, 1]])
    b, cb, _ = run(g, [[2, 1], [0, 2], [0, 1]])
    # row 0 = [1, 2]: v = (.5, .5) after g1, <v, g2> = -.75 -> v + .6 g2 = (-.1, .2).  Row 0 = [2, 1]: v = (.2, -.4) after g2,
    # <v, g1> = -.6 -> v + .3 g1 = (-.1, -.1).  Task 1: <g1, g0> = -1 -> (0, 1), then <., g2> = -.5 -> (-.4, .8).  Task 2: (0, -.5), then
    # <., g1> = -.5 -> (-.25, -.25).
    want_a = (torch.tensor([-0.1, 0.2]) + torch.tensor([-0.4, 0.8]) + torch.tensor([-0.25, -0.25])).double() / 3
    want_b = (torch.tensor([-0.1, -0.1]) + torch.tensor([-0.4, 0.8]) + torch.tensor([-0.25, -0.25])).double() / 3
    assert torch.allclose(a[0], want_a, rtol=0, atol=1e-7) and torch.allclose(b[0], want_b, rtol=0, atol=1e-7)
    assert not torch.allclose(a[0], b[0], atol=1e-3), "the permutation table is not honoured"
    assert ca == cb == (6, 6)


def test_one_holder_and_mean_and_extra_task():
    tg, lay, has = tiny([(1.0, 2.0), None, (3.0, -1.0)])
    for rule, scope in G.MODES:
        final, counts, _ = SR.surgery(tg, lay, has, [1, 0], [[1], [0]], rule, scope)          # task 2 is outside the order
        assert torch.equal(final[0], torch.tensor([1.0, 2.0], dtype=torch.float64)) and counts == (0, 0)
        final, _, _ = SR.surgery(tg, lay, has, [1, 0], [[1], [0]], rule, scope, extra_task=2)
        assert torch.equal(final[0], torch.tensor([4.0, 1.0], dtype=torch.float64))
        final, _, _ = SR.surgery(tg, lay, has, [1], [[]], rule, scope, extra_task=-1)          # no holder in the order
        assert final[0] is None
    final, counts, margin = SR.surgery(tg, lay, has, [0, 2], None, "mean")
    assert torch.equal(final[0], torch.tensor([2.0, 0.5], dtype=torch.float64)) and counts == (0, 0) and margin == float("inf")


def test_model_scope_projects_whole_vectors():
    """two tensors both tasks hold: the whole vectors (1, 0 | 1) and (-1, 1 | 1) do not conflict although the first tensor's parts do;
    a third tensor one task holds alone stays out of the vectors"""
    lay = Layout([2, 1, 3])
    tg = torch.zeros(2, lay.P, dtype=torch.float64)
    tg[0, lay.slot(0)], tg[0, lay.slot(1)] = torch.tensor([1.0, 0.0]).double(), torch.tensor([1.0]).double()
    tg[1, lay.slot(0)], tg[1, lay.slot(1)] = torch.tensor([-1.0, 1.0]).double(), torch.tensor([1.0]).double()
    tg[1, lay.slot(2)] = torch.tensor([5.0, 6.0, 7.0]).double()
    has = np.zeros((3, MAXT), np.uint8)
    has[:2, :2] = 1
    has[2, 1] = 1
    final, counts, _ = SR.surgery(tg, lay, has, [0, 1], [[1], [0]], "pcgrad", "model")
    assert counts == (0, 2) and torch.equal(final[0], torch.tensor([0.0, 0.5], dtype=torch.float64))
    assert torch.equal(final[2], tg[1, lay.slot(2)])
    final, counts, _ = SR.surgery(tg, lay, has, [0, 1], [[1], [0]], "pcgrad", "tensor")
    assert counts == (2, 4) and torch.allclose(final[0], torch.tensor([0.25, 0.75], dtype=torch.float64))


@pytest.mark.parametrize("problem", ["T5_order4_extra", "T8", "many"])
def test_reference_rule_equals_the_existing_reference(problem):
    if problem == "many":
        lay, T, has, tg, order, last_task, extra_task = many_tensors_problem(7)
    else:
        T, n_order, extra = {"T5_order4_extra": (5, 4, True), "T8": (8, 8, False)}[problem]
        lay, T, has, tg, order, last_task, extra_task = edge_problem(T, n_order, extra, False, False, seed=100)
    want, counts = ref_pcgrad(tg, lay, has, order, last_task, extra_task)
    got, got_counts, margin = SR.surgery(tg, lay, has, order, None, "reference", "tensor", last_task, extra_task)
    assert got_counts == counts and counts[0] > 0
    for k in range(lay.K):
        assert (got[k] is None) == (want[k] is None), k
        if want[k] is not None:
            assert torch.allclose(got[k], want[k], rtol=0, atol=1e-12 * float(want[k].abs().max() + 1)), k
    assert margin <= pcgrad_min_margin(tg, lay, has, order) * (1 + 1e-9)       # the same bound, and the zero-norm decisions on top


# ------------------------------------------------------------------------------------------------ control.GradientSurgery
def toy_problem(seed=0):
    torch.manual_seed(seed)
    model = Toy().double()
    gen = torch.Generator().manual_seed(seed + 1)
    x = torch.randn(16, 4, generator=gen, dtype=torch.float64)
    y = 3 * torch.randn(len(TOY_TASKS), 16, 1, generator=gen, dtype=torch.float64)
    return model, x, y


def toy_task_grads(model, losses, tasks):
    params = dict(model.named_parameters())
    names = list(params)
    lay = Layout([p.numel() for p in params.values()])
    tg, has = torch.zeros(len(tasks), lay.P, dtype=torch.float64), np.zeros((lay.K, MAXT), np.uint8)
    for t, task in enumerate(tasks):
        model.zero_grad(set_to_none=True)
        losses[task].backward(retain_graph=True)
        for k, n in enumerate(names):
            if params[n].grad is not None:
                has[k, t] = 1
                tg[t, lay.slot(k)] = params[n].grad.flatten()
    model.zero_grad(set_to_none=True)
    return names, lay, tg, has


@pytest.mark.parametrize("mode", ALL_MODES, ids=["-".join(m) for m in ALL_MODES])
def test_module_path_matches_the_restatement(mode):
    rule, scope = mode
    model, x, y = toy_problem()
    main = TOY_TASKS[:-1]
    losses = model.losses(x, y)
    names, lay, tg, has = toy_task_grads(model, losses, main)
    params = dict(model.named_parameters())
    for trial in range(3):
        rng = random.Random(trial)
        order = list(main)
        if rule == "reference":
            rng.shuffle(order)
        perm = SR.draw_perm(rng, len(main)) if rule == "pcgrad" else None
        want, counts, margin = SR.surgery(tg, lay, has, [main.index(t) for t in order], perm, rule, scope, last_task=len(main) - 1)
        assert margin > 1e-6
        gs = Cn.GradientSurgery(torch.device("cpu"), rule=rule, scope=scope)
        metrics = gs.apply_gradient_surgery(model, {t: losses[t] for t in main}, list(main), order=order if rule == "reference" else None, perm=perm)
        assert (metrics["gradient_surgery/total_conflicts"], metrics["gradient_surgery/total_projections"]) == counts
        assert metrics["gradient_surgery/conflict_ratio"] == counts[0] / max(counts[1], 1)
        assert rule != "pcgrad" or counts[0] > 0
        for k, n in enumerate(names):
            g = params[n].grad
            assert (g is None) == (want[k] is None), (n, trial)
            if g is not None:
                assert torch.allclose(g.flatten(), want[k], rtol=0, atol=1e-12), (n, trial, (g.flatten() - want[k]).abs().max().item())


@pytest.mark.parametrize("mode", G.MODES, ids=["-".join(m) for m in G.MODES])
def test_every_parameter_some_task_reaches_gets_a_gradient(mode):
    model, x, y = toy_problem(3)
    main = TOY_TASKS[:-1]
    losses = model.losses(x, y)
    names, lay, tg, has = toy_task_grads(model, losses, main)
    gs = Cn.GradientSurgery(torch.device("cpu"), rule=mode[0], scope=mode[1], shuffle_rng=random.Random(1))
    gs.apply_gradient_surgery(model, {t: losses[t] for t in main}, list(main))
    params = dict(model.named_parameters())
    reached = {n for k, n in enumerate(names) if has[k].any()}
    assert {"heads.link_pred.weight", "heads.node_contrast.bias", "mask_token", "encoder.weight"} <= reached and "unused" not in reached
    assert {n for n in names if params[n].grad is not None} == reached
    # ... which the reference rule does not do, whatever it shuffles first
    ref = Cn.GradientSurgery(torch.device("cpu"), shuffle_rng=random.Random(1))
    ref.apply_gradient_surgery(model, {t: losses[t] for t in main}, list(main))
    assert {n for n in names if params[n].grad is not None} < reached


def test_rules_and_scopes_are_validated():
    for kw in (dict(rule="nope"), dict(scope="nope"), dict(rule="reference", scope="model")):
        with pytest.raises(ValueError):
            Cn.GradientSurgery(torch.device("cpu"), **kw)
    model, x, y = toy_problem()
    losses = model.losses(x, y)
    gs = Cn.GradientSurgery(torch.device("cpu"), rule="pcgrad")
    with pytest.raises(ValueError):
        gs.apply_gradient_surgery(model, {t: losses[t] for t in TOY_TASKS[:3]}, TOY_TASKS[:3], perm=[[1, 1], [0, 2], [0, 1]])
    assert gs.apply_gradient_surgery(model, {"link_pred": losses["link_pred"]}, ["link_pred"]) == {}      # one task: the caller's plain backward


def test_random_stream_of_each_rule():
    """reference: one shuffle of the task list, as before.  pcgrad: for each task in turn one shuffle of the others.  mean: nothing."""
    model, x, y = toy_problem()
    main = TOY_TASKS[:-1]
    losses = {t: l for t, l in model.losses(x, y).items() if t in main}
    after = {}
    for rule in ("reference", "pcgrad", "mean"):
        rng = random.Random(7)
        gs = Cn.GradientSurgery(torch.device("cpu"), shuffle_rng=rng, rule=rule)
        gs.apply_gradient_surgery(model, losses, list(main))
        after[rule] = (rng.getstate(), gs.last_perm)
    twin = random.Random(7)
    order = list(main)
    twin.shuffle(order)
    assert after["reference"][0] == twin.getstate() and after["reference"][1] is None
    twin = random.Random(7)
    perm = SR.draw_perm(twin, len(main))
    assert after["pcgrad"] == (twin.getstate(), perm)
    assert after["mean"] == (random.Random(7).getstate(), None)


# ------------------------------------------------------------------------------------------------ the device problems
@pytest.mark.parametrize("case", list(G.CASES) + ["many"])
def test_device_problems_keep_their_distance_from_every_decision(case):
    lay, T, has, tg, order, perm, extra_task = G.case_problem(case)
    n = len(order)
    assert T in (2, 3, 5, 8) and [sorted(r) for r in perm] == [[j for j in range(n) if j != i] for i in range(n)]
    held = has[:, order].sum(1)
    if case != "many":
        assert set(G.SMALL_LENS) <= set(lay.lens) and set(held.tolist()) >= {0, 1, min(2, n), n - ("lone" in case)}
        for p in order[:-1] if "lone" in case else order:
            assert ((held == 1) & (has[:, p] == 1)).any(), f"no tensor held by task {p} alone"
        if "lone" in case:
            assert not ((held >= 2) & (has[:, order[-1]] == 1)).any()
        if extra_task >= 0:
            assert has[held == 0, extra_task].any() and has[held > 0, extra_task].any() and not has[:, extra_task].all()
    zero = [(k, t) for k in range(lay.K) for t in order if has[k, t] and not tg[t, lay.slot(k)].any()]
    assert zero, "no holder with an exactly zero gradient"
    for mode in G.MODES:
        final, (conf, proj), margin = G.restatement(case, mode)
        print(f"{case} {mode}: K {lay.K}, conflicts {conf}, projections {proj}, margin {margin:.3e}")
        assert margin >= MARGIN, (mode, margin)
        if mode[0] == "pcgrad":                    # conflicts to resolve, and pairs that do not conflict (the one walk of model scope
            assert 0 < proj and conf < proj        # has few pairs and may meet no conflict: T5, T8 and `many` do)
            assert conf > 0 or (mode[1] == "model" and case not in ("T5", "T8", "many")), (mode, conf)
    t_conf = G.restatement(case, ("pcgrad", "tensor"))[1]
    m_conf = G.restatement(case, ("pcgrad", "model"))[1]
    assert t_conf != m_conf or n == 1, "model scope is not told apart from tensor scope by its counts"


# ------------------------------------------------------------------------------------------------ surface
def test_entry_point_is_declared_bound_and_exported():
    from gnn_pretraining_amd import _lib as L
    name = "gmp_mt_surgery_clip_adamw"
    assert L._SIGS[name][1] == [L.i32, L.i32, L.p] + L._SIGS["gmp_mt_pcgrad_clip_adamw_ex"][1]
    assert L.SURGERY_RULES == G.RULES and L.SURGERY_SCOPES == G.SCOPES
    header = open(L.HEADER_PATH).read()
    for key, val in list(G.RULES.items()) + [("scope_" + k, v) for k, v in G.SCOPES.items()]:
        assert f"#define GMP_SURGERY_{key.upper()} {val}\n" in header, key


def test_command_line_switch():
    from gnn_pretraining_amd.pretrain import pretrain as PT
    base = ["--exp_name", "s4", "--seed", "1"]
    a = PT.parse_args(base)
    assert (a.surgery, a.surgery_scope) == ("reference", "tensor")
    a = PT.parse_args(base + ["--module-path", "--surgery", "pcgrad", "--surgery-scope", "model"])
    assert (a.surgery, a.surgery_scope, a.module_path) == ("pcgrad", "model", True)
    assert PT.parse_args(base + ["--surgery", "mean"]).surgery == "mean"
    for bad in (["--surgery", "nope"], ["--surgery-scope", "model"], ["--surgery-scope", "nope"]):
        with pytest.raises(SystemExit):
            PT.parse_args(base + bad)
