"""The optimisation step's tail (csrc/optim.hip: Gram, PCGrad solve, combine, clip norm, AdamW, the sharded path's foreign pass) and
the gradient exchange's slice pack / unpack (csrc/segments.hip), called through the C ABI and checked against a float64 reference.

The reference of one step is the reference's own composition, run in float64 on the kernel's float32 inputs:
  1. oracle.train.pcgrad_combine over per-task dicts holding only the tensors whose `has` bit is set;
  2. tensors PCGrad does not emit keep the LAST task's raw gradient (gradient_surgery.py:61 via _set_gradients);
  3. the `extra_task` gradient (domain_adv in s5) is added on top;
  4. torch.nn.utils.clip_grad_norm_ over the tensors that end up with a gradient;
  5. torch.optim.AdamW, one param group per tensor (its lr and wd), grad=None where there is no gradient.
test_reference_composition_matches_the_oracle_training_step (CPU) checks that composition against oracle.train's
apply_gradient_surgery + make_optimizer on a toy module, so the reference itself models the quirks.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn

from oracle import train as OTr

DEV = "cuda:0"
MAXT = 8
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8
gpu = pytest.mark.gpu


def pad4(n):
    return (n + 3) // 4 * 4


class Layout:
    """K tensors in one flat buffer as the engines lay them out: offsets multiples of 4 floats (16 bytes), each slot zero-padded to a
    multiple of 4 floats."""

    def __init__(self, lens, off=None, P=None):
        self.lens = [int(n) for n in lens]
        self.K = len(self.lens)
        if off is None:
            off, o = [], 0
            for n in self.lens:
                off.append(o)
                o += pad4(n)
            P = o
        self.off, self.P = [int(o) for o in off], int(P)
        assert all(o % 4 == 0 for o in self.off) and self.P % 4 == 0

    def slot(self, k):
        return slice(self.off[k], self.off[k] + self.lens[k])

    def padding(self):
        m = torch.zeros(self.P, dtype=torch.bool)
        for k in range(self.K):
            m[self.off[k] + self.lens[k]:self.off[k] + pad4(self.lens[k])] = True
        return m


# ------------------------------------------------------------------------------------------------ float64 reference
def ref_pcgrad(tg, lay, has, order, last_task, extra_task):
    """Steps 1-3: the gradient every tensor ends up with (None = no gradient) and PCGrad's (conflicts, projections)."""
    per = {t: {k: tg[t, lay.slot(k)].double() for k in range(lay.K) if has[k, t]} for t in order}
    final, met = OTr.pcgrad_combine(per, list(order))
    out = []
    for k in range(lay.K):
        g = final.get(k)
        if g is None and last_task >= 0 and has[k, last_task]:
            g = tg[last_task, lay.slot(k)].double()           # not emitted: the last backward's .grad stays
        if extra_task >= 0 and has[k, extra_task]:
            ge = tg[extra_task, lay.slot(k)].double()         # accumulated by a later backward
            g = ge if g is None else g + ge
        out.append(g)
    return out, (met["gradient_surgery/total_conflicts"], met["gradient_surgery/total_projections"])


def ref_clip_adamw(lay, grads, params, exp_avg, exp_avg_sq, steps, lr, wd, max_norm):
    """Steps 4-5 from the given state: (params, exp_avg, exp_avg_sq, steps) per tensor after one clip_grad_norm_ + AdamW.step()."""
    ps = [nn.Parameter(params[lay.slot(k)].double().clone()) for k in range(lay.K)]
    for p, g in zip(ps, grads):
        p.grad = None if g is None else g.double().clone()
    if max_norm > 0:
        torch.nn.utils.clip_grad_norm_([p for p in ps if p.grad is not None], max_norm)
    opt = torch.optim.AdamW([{"params": [p], "lr": float(lr[k]), "weight_decay": float(wd[k])} for k, p in enumerate(ps)],
                            betas=(BETA1, BETA2), eps=EPS, foreach=False)
    for k, p in enumerate(ps):
        opt.state[p] = {"step": torch.tensor(float(steps[k]), dtype=torch.float64),
                        "exp_avg": exp_avg[lay.slot(k)].double().clone(), "exp_avg_sq": exp_avg_sq[lay.slot(k)].double().clone()}
    opt.step()
    st = [opt.state[p] for p in ps]
    return ([p.detach() for p in ps], [s["exp_avg"] for s in st], [s["exp_avg_sq"] for s in st], [float(s["step"]) for s in st])


def pcgrad_min_margin(tg, lay, has, order):
    """The smallest |<g_i', g_j>| / (B_i ||g_j||) over the pairs PCGrad evaluates (float64), where g_i' is task i's gradient as
    projected so far and B_i = ||g_i|| + sum of the projections' lengths bounds sum_p |alpha_ip| ||g_p||, the scale of the kernel's
    Gram-space rounding of that dot product.  It bounds |cos| from below, and keeps sign decisions away from nearly cancelled g_i'."""
    worst = float("inf")
    per = {t: {k: tg[t, lay.slot(k)].double() for k in range(lay.K) if has[k, t]} for t in order}
    for i, ti in enumerate(order):
        mod = dict(per[ti])
        bound = {k: g.norm().item() for k, g in mod.items()}
        for tj in order[:i]:
            for k in mod:
                if k not in per[tj]:
                    continue
                gi, gj = mod[k], per[tj][k]
                if gi.norm() == 0 or gj.norm() == 0:
                    continue
                dot = torch.dot(gi, gj)
                worst = min(worst, abs(dot.item()) / (bound[k] * gj.norm().item()))
                if dot < 0:
                    mod[k] = gi - (dot / gj.norm() ** 2) * gj
                    bound[k] += abs(dot.item()) / gj.norm().item()
    return worst


# ------------------------------------------------------------------------------------------------ problem generation
def make_grads(seed, lay, T, has, zero=(), mags=None):
    """float32 [T, P]: tensor k of task t = m_t (c u_k + s n) with u_k, n random unit directions and c = +-U(0.4, 1): a tensor's
    task gradients share one direction, so PCGrad meets real conflicts, at cosines far from zero.  Tensors shorter than 4 floats
    get positive c and little noise (s = 0.1; else 0.6): in one or two dimensions a projection leaves a (nearly) zero vector."""
    gen = torch.Generator().manual_seed(seed)
    rs = np.random.RandomState(seed)
    tg = torch.zeros(T, lay.P)
    mags = 10.0 ** rs.uniform(-1, 1, T) if mags is None else mags
    for k, n in enumerate(lay.lens):
        u = torch.randn(n, generator=gen, dtype=torch.float64)
        u /= u.norm()
        for t in range(T):
            if not has[k, t] or (k, t) in zero:
                continue
            c = rs.uniform(0.4, 1.0) * (1 if n < 4 or rs.rand() < 0.5 else -1)
            e = torch.randn(n, generator=gen, dtype=torch.float64)
            g = c * u + (0.1 if n < 4 else 0.6) * e / e.norm()
            tg[t, lay.slot(k)] = (mags[t] * g).float()
    return tg


PATTERNS = ("all", "no_first", "absent", "only_extra", "zero", "random")


def has_rows(rs, patterns, T, order, last_task, extra_task):
    """one `has` row per pattern:
       all        every task holds the tensor
       no_first   absent from the first-shuffled task, held by last_task (PCGrad emits nothing: the last task's raw gradient stays)
       absent     absent from the first-shuffled task, from last_task and from extra_task: no gradient at all (flag 0)
       only_extra held by extra_task alone
       zero       every task holds it, one task of the order with an exactly zero gradient (its pairs are skipped, it counts in the mean)
       random     a random subset"""
    has, zero = np.zeros((len(patterns), MAXT), np.uint8), []
    for k, p in enumerate(patterns):
        if p in ("all", "zero"):
            has[k, :T] = 1
        elif p in ("no_first", "absent", "random"):
            has[k, :T] = rs.rand(T) < 0.6
        if p == "no_first":
            has[k, order[0]] = 0
            has[k, last_task] = 1
        elif p == "absent":
            has[k, order[0]] = has[k, last_task] = 0
            if extra_task >= 0:
                has[k, extra_task] = 0
        elif p == "only_extra" and extra_task >= 0:
            has[k, extra_task] = 1
        elif p == "zero":
            zero.append((k, order[min(1, len(order) - 1)]))
    return has, zero


# ------------------------------------------------------------------------------------------------ the C ABI
class Kernel:
    """Device buffers of one problem and gmp_mt_pcgrad_clip_adamw_ex over them."""

    def __init__(self, lay, T, has, tg, params=None, exp_avg=None, exp_avg_sq=None, steps=None, lr=None, wd=None):
        from gnn_pretraining_amd import _lib as L
        self.L, self.lib, self.lay, self.T = L, L.lib(), lay, T
        self.tg = tg.to(DEV).contiguous()
        self.off = torch.tensor(lay.off, dtype=torch.int64, device=DEV)
        self.len = torch.tensor(lay.lens, dtype=torch.int32, device=DEV)
        self.has = torch.from_numpy(np.ascontiguousarray(has, dtype=np.uint8)).to(DEV)
        self.final = torch.zeros(lay.P, device=DEV)
        self.normsq = torch.zeros(1, device=DEV)
        self.metrics = torch.zeros(2, dtype=torch.int32, device=DEV)
        self.flags = torch.zeros(lay.K, dtype=torch.int32, device=DEV)
        self.ws_bytes = int(self.lib.gmp_mt_workspace_bytes(lay.K))
        self.ws = torch.zeros(self.ws_bytes, dtype=torch.uint8, device=DEV)
        to = lambda x, dt=torch.float32: None if x is None else torch.as_tensor(x, dtype=dt).to(DEV).contiguous()
        self.params, self.exp_avg, self.exp_avg_sq = to(params), to(exp_avg), to(exp_avg_sq)
        self.steps, self.lr, self.wd = to(steps), to(lr), to(wd)

    def call(self, order, last_task, extra_task, *, max_norm=0.0, apply_update=0, k_begin=0, k_end=None, phases=3, abort=None,
             num_tasks=None, n_order=None, ws_bytes=None, with_steps=True, with_params=True):
        """the return code (no check, no sync)"""
        from gnn_pretraining_amd import ops
        ptr = ops._ptr
        o = (C.c_int32 * MAXT)(*(list(order) + [0] * (MAXT - len(order))))
        return self.lib.gmp_mt_pcgrad_clip_adamw_ex(
            ptr(self.tg), self.lay.P, self.T if num_tasks is None else num_tasks, self.lay.K, ptr(self.off), ptr(self.len), ptr(self.has),
            o, len(order) if n_order is None else n_order, last_task, extra_task,
            ptr(self.params if with_params else None), ptr(self.exp_avg), ptr(self.exp_avg_sq), ptr(self.steps if with_steps else None),
            ptr(self.lr), ptr(self.wd), BETA1, BETA2, EPS, max_norm, ptr(self.final), ptr(self.normsq), ptr(self.metrics), ptr(self.flags),
            ptr(self.ws), self.ws_bytes if ws_bytes is None else ws_bytes, apply_update, k_begin, self.lay.K if k_end is None else k_end,
            phases, ptr(abort), ops._stream(self.final))

    def run(self, *args, **kw):
        self.L.check(self.call(*args, **kw), "gmp_mt_pcgrad_clip_adamw_ex")
        torch.cuda.synchronize()

    def gram(self):
        K = self.lay.K
        return self.ws[:K * MAXT * MAXT * 8].view(torch.float64).view(K, MAXT, MAXT).cpu()

    def outputs(self):
        """everything a call can change, on the host"""
        cpu = lambda x: None if x is None else x.cpu().clone()
        return {"final": cpu(self.final), "normsq": cpu(self.normsq), "metrics": cpu(self.metrics), "flags": cpu(self.flags),
                "params": cpu(self.params), "exp_avg": cpu(self.exp_avg), "exp_avg_sq": cpu(self.exp_avg_sq), "steps": cpu(self.steps)}


def assert_same_bits(a, b, what=""):
    for key in a:
        if a[key] is None:
            assert b[key] is None, (what, key)
            continue
        assert torch.equal(a[key].view(torch.int32) if a[key].dtype == torch.float32 else a[key],
                           b[key].view(torch.int32) if b[key].dtype == torch.float32 else b[key]), f"{what}: {key} differs"


# ------------------------------------------------------------------------------------------------ A. Gram, PCGrad, combine
EDGE_LENS = (1, 2, 3, 4, 5, 4095, 4096, 4097)
BIG_LENS = (131071, 131072, 131073)
HUGE_LEN = 1_000_003
MARGIN = 1e-4


def edge_problem(T, n_order, extra, big, huge, seed):
    """every (edge length, has pattern) pair, the long tensors present everywhere / absent from the first task"""
    rs = np.random.RandomState(seed)
    main = [t for t in range(T) if not (extra and t == T - 1)]
    order = [int(t) for t in rs.permutation(main)[:n_order]]
    extra_task = T - 1 if extra else -1
    last_task = max(order)                                            # last in dict order
    if n_order > 1 and order[0] == last_task:
        order[0], order[1] = order[1], order[0]
    pats = [p for n in EDGE_LENS for p in PATTERNS]
    lens = [n for n in EDGE_LENS for _ in PATTERNS]
    if big:
        pats += ["all", "no_first"] * len(BIG_LENS)
        lens += [n for n in BIG_LENS for _ in range(2)]
    if huge:
        pats.append("all")
        lens.append(HUGE_LEN)
    has, zero = has_rows(rs, pats, T, order, last_task, extra_task)
    lay = Layout(lens)
    return lay, T, has, make_grads(seed, lay, T, has, zero=zero), order, last_task, extra_task


def many_tensors_problem(seed):
    """~300 tensors of random lengths and patterns: more than 256 tensors (the norm pass's thread loop) and five solve blocks"""
    rs = np.random.RandomState(seed)
    T, order, last_task, extra_task = 5, [2, 0, 3, 1], 3, 4
    K = 300
    pats = [PATTERNS[i] for i in rs.randint(0, len(PATTERNS), K)]
    lens = list(rs.randint(16, 700, K))
    has, zero = has_rows(rs, pats, T, order, last_task, extra_task)
    lay = Layout(lens)
    return lay, T, has, make_grads(seed, lay, T, has, zero=zero), order, last_task, extra_task


A_CASES = {    # T, n_order, extra task outside the order, 131k tensors, the ~1M tensor
    "T1_finetune": (1, 1, False, True, False),
    "T2": (2, 2, False, True, True),
    "T3_order2_extra": (3, 2, True, False, False),
    "T5_order4_extra": (5, 4, True, True, False),
    "T5": (5, 5, False, False, False),
    "T6_order3": (6, 3, False, False, False),
    "T7": (7, 7, False, False, False),
    "T8_order7_extra": (8, 7, True, False, False),
    "T8": (8, 8, False, True, True),
}


def check_pcgrad(kern, tg, lay, T, has, order, last_task, extra_task):
    ref, (conf, proj) = ref_pcgrad(tg, lay, has, order, last_task, extra_task)
    assert pcgrad_min_margin(tg, lay, has, order) >= MARGIN, "the data sits too close to a PCGrad sign decision"
    kern.run(order, last_task, extra_task)
    out = kern.outputs()
    flags = out["flags"].numpy()
    assert flags.tolist() == [int(g is not None) for g in ref], "flags"
    assert out["metrics"].tolist() == [conf, proj], f"conflicts / projections {out['metrics'].tolist()} vs {[conf, proj]}"
    # Gram: per-thread fp32 sums of <= 4 x 4 x ceil(chunk / 4,096) products, a 64-lane fp32 fold, waves and chunks in fp64; the
    # largest chunk (31,252 floats of the ~1M tensor) gives <= 128 + 6 fp32 roundings per term: |error| <= 134 u sum|x y| <= 8e-6 |x||y|
    if len(order) > 1:
        G = kern.gram()
        for k in range(lay.K):
            held = [t for t in range(T) if has[k, t]]
            if len(held) < 2:
                continue
            g = {t: tg[t, lay.slot(k)].double() for t in held}
            for i, x in enumerate(held):
                for y in held[i:]:
                    want = torch.dot(g[x], g[y]).item()
                    bar = 1e-5 * g[x].norm().item() * g[y].norm().item()
                    assert abs(G[k, x, y].item() - want) <= bar and G[k, y, x].item() == G[k, x, y].item(), (k, lay.lens[k], x, y)
    fin = out["final"].double()
    for k in range(lay.K):
        if ref[k] is None:
            continue
        scale = max(tg[t, lay.slot(k)].abs().max().item() for t in range(T) if has[k, t])
        err = (fin[lay.slot(k)] - ref[k]).abs().max().item()
        # a projection can cancel most of a gradient: the scale is the inputs'
        assert err <= 1e-5 * scale, f"final_grad of tensor {k} (len {lay.lens[k]}): {err:.3e} > 1e-5 x {scale:.3e}"
    own = sum(float((fin[lay.slot(k)] ** 2).sum()) for k in range(lay.K) if flags[k])
    want = sum(float((g ** 2).sum()) for g in ref if g is not None)
    got = float(out["normsq"])
    assert abs(got - own) <= 1e-5 * own, f"normsq {got} vs its own final_grad {own}"        # fp32 chunk sums of squares (<= 130 u)
    assert abs(got - want) <= 1e-4 * want, f"normsq {got} vs the reference {want}"          # unclipped
    return out, ref


@gpu
@pytest.mark.parametrize("case", list(A_CASES))
def test_pcgrad_gram_and_combine_match_float64(case):
    T, n_order, extra, big, huge = A_CASES[case]
    lay, T, has, tg, order, last_task, extra_task = edge_problem(T, n_order, extra, big, huge, seed=100 + list(A_CASES).index(case))
    kern = Kernel(lay, T, has, tg)
    out, ref = check_pcgrad(kern, tg, lay, T, has, order, last_task, extra_task)
    if T == 1:
        # the fine-tune call: one task, no PCGrad -- the gradient goes through untouched
        for k in range(lay.K):
            if has[k, 0]:
                assert torch.equal(out["final"][lay.slot(k)], tg[0, lay.slot(k)]), k


@gpu
def test_pcgrad_over_more_than_256_tensors_matches_float64():
    lay, T, has, tg, order, last_task, extra_task = many_tensors_problem(7)
    check_pcgrad(Kernel(lay, T, has, tg), tg, lay, T, has, order, last_task, extra_task)


@gpu
@pytest.mark.parametrize("scheme", ["s4", "s5"])
def test_pcgrad_on_the_model_layouts_matches_float64(scheme):
    """the engine's own tables (offsets, lengths, availability, last task, extra task), filled with synthetic gradients"""
    from test_gpu_engine import build
    _, _, eng, *_ = build(scheme, 3)
    names = list(eng.tasks)
    main = [t for t in names if t != "domain_adv"]
    extra_task = names.index("domain_adv") if "domain_adv" in names else -1
    last_task = names.index(main[-1])
    lay = Layout(eng.t_len.tolist(), eng.t_off.tolist(), eng.P)
    has = eng.has_static.copy()
    T = eng.T
    del eng
    torch.cuda.empty_cache()
    for seed, order in ((11, [names.index(t) for t in main]), (12, [names.index(t) for t in reversed(main)])):
        tg = make_grads(seed, lay, T, has)
        check_pcgrad(Kernel(lay, T, has, tg), tg, lay, T, has, order, last_task, extra_task)


# ------------------------------------------------------------------------------------------------ B. clip + AdamW over several steps
B_LENS = (1, 3, 4, 5, 17, 64, 257, 2000, 4097, 131073, 9, 33)
EPS_K, ZERO_K, NEVER_K = 10, 11, 6          # gradients ~1e-9 (eps dominates) / flagged with an exactly zero gradient / never a gradient


def b_state(seed, lay):
    rs = np.random.RandomState(seed)
    gen = torch.Generator().manual_seed(seed)
    K, P = lay.K, lay.P
    params, m, v = torch.zeros(P), torch.zeros(P), torch.zeros(P)
    steps = np.array([(0.0, 7.0, 999.0)[k % 3] for k in range(K)], np.float32)
    if EPS_K < K:
        steps[EPS_K] = 0.0
    for k in range(K):
        n = lay.lens[k]
        params[lay.slot(k)] = torch.rand(n, generator=gen) * 2 - 1
        if steps[k] > 0:                                   # moments of a tensor that has taken steps before
            m[lay.slot(k)] = torch.randn(n, generator=gen) * 1e-2
            v[lay.slot(k)] = torch.rand(n, generator=gen) * 1e-4
    lr = rs.uniform(1e-3, 1e-2, K).astype(np.float32)
    wd = rs.uniform(0.01, 0.1, K).astype(np.float32)
    return params, m, v, steps, lr, wd


def b_step_problem(lay, T, order, last_task, extra_task, step, target_norm):
    """has pattern and gradients of one step: the pattern changes every step, so the tensors' step counts drift apart"""
    rs = np.random.RandomState(1000 + step)
    has = np.zeros((lay.K, MAXT), np.uint8)
    has[:, :T] = rs.rand(lay.K, T) < 0.6
    has[ZERO_K, :T] = 1
    has[EPS_K, order[0]] = has[EPS_K, last_task] = 1
    has[NEVER_K] = 0
    if step % 2:
        has[NEVER_K, order[-1]] = 1                          # held by a task that is neither first-shuffled nor last: no gradient all the same
    tg = make_grads(2000 + step, lay, T, has, zero=[(ZERO_K, t) for t in range(T)], mags=np.ones(T))
    tg *= target_norm / np.sqrt(lay.K)                       # a tensor's task gradients have norms ~1: the total lands near target_norm
    tg[:, lay.slot(EPS_K)] *= 3e-9 / (target_norm / np.sqrt(lay.K))     # norm ~3e-9, elements ~1e-9: sqrt(v) stays far below eps
    return has, tg


B_CASES = {"clip_hard": (1e-4, 1e-3), "clip_loose": (1e3, 1.0), "clip_off": (0.0, 1.0)}     # max_norm, target total norm


@gpu
@pytest.mark.parametrize("case", list(B_CASES))
def test_clip_and_adamw_over_several_steps_match_float64(case):
    max_norm, target = B_CASES[case]
    lay = Layout(B_LENS)
    T, order, last_task, extra_task = 4, [1, 2, 0], 2, 3
    params, m, v, steps, lr, wd = b_state(31, lay)
    has, tg = b_step_problem(lay, T, order, last_task, extra_task, 0, target)
    kern = Kernel(lay, T, has, tg, params, m, v, steps, lr, wd)
    pad = lay.padding()
    steps0 = kern.steps.cpu().clone()
    for step in range(5):
        if step:
            has, tg = b_step_problem(lay, T, order, last_task, extra_task, step, target)
            kern.has.copy_(torch.from_numpy(has))
            kern.tg.copy_(tg)
        before = kern.outputs()
        kern.run(order, last_task, extra_task, max_norm=max_norm, apply_update=1)
        after = kern.outputs()
        flags = after["flags"].numpy()
        norm = float(after["normsq"]) ** 0.5
        if case == "clip_hard":
            assert 2e-4 < norm < 5e-3, norm                      # clipping by ~10x: torch's + 1e-6 moves the coefficient by ~1e-3
        elif case == "clip_loose":
            assert norm < max_norm
        assert flags[NEVER_K] == 0 and flags[ZERO_K] == 1 and flags[EPS_K] == 1
        assert float(after["final"][lay.slot(ZERO_K)].abs().max()) == 0.0
        grads = [after["final"][lay.slot(k)] if flags[k] else None for k in range(lay.K)]
        rp, rm, rv, rs_ = ref_clip_adamw(lay, grads, before["params"], before["exp_avg"], before["exp_avg_sq"], before["steps"].numpy(),
                                          lr, wd, max_norm)
        assert after["steps"].tolist() == [float(s) for s in rs_], "step counts"
        for k in range(lay.K):
            sl = lay.slot(k)
            if not flags[k]:
                # grad=None: torch skips the parameter, weight decay included
                for key in ("params", "exp_avg", "exp_avg_sq"):
                    assert torch.equal(after[key][sl], before[key][sl]), (step, k, key)
                continue
            m_err = (after["exp_avg"][sl].double() - rm[k]).abs().max().item()
            assert m_err <= 1e-5 * rm[k].abs().max().item(), (step, k, "exp_avg", m_err)
            # the kernel forms 1 - beta2 in fp32 from the fp32 beta2: 1 - 0.999f = 0.00099998713, 1.3e-5 from torch's 0.001; at step 1 this
            # cancels against the bias correction, later only partly
            v_err = (after["exp_avg_sq"][sl].double() - rv[k]).abs().max().item()
            assert v_err <= 5e-5 * rv[k].abs().max().item(), (step, k, "exp_avg_sq", v_err)
            p_ref = rp[k]
            dp = (p_ref - before["params"][sl].double()).abs().max().item()
            ulp = torch.from_numpy(np.spacing(np.abs(p_ref.float().numpy()))).double()
            p_err = (after["params"][sl].double() - p_ref).abs()
            assert bool((p_err <= 1e-4 * dp + 2 * ulp).all()), (step, k, "params", p_err.max().item(), dp)
        for key in ("params", "exp_avg", "exp_avg_sq", "final"):
            assert float(after[key][pad].abs().max()) == 0.0, (step, key, "padding")
    taken = (kern.steps.cpu() - steps0).tolist()
    assert taken[NEVER_K] == 0 and len(set(taken)) > 2, taken              # the step counts drifted apart


# ------------------------------------------------------------------------------------------------ C. bitwise identities and guards
RANGES = ((0, 37), (37, 200), (200, 300))         # none aligned to the 64-tensor solve blocks
C_MAX_NORM = 0.5


def c_problem():
    lay, T, has, tg, order, last_task, extra_task = many_tensors_problem(7)
    return lay, T, has, tg, order, last_task, extra_task, b_state(41, lay)


@gpu
def test_ranges_and_the_foreign_pass_equal_the_one_shot_call():
    lay, T, has, tg, order, last_task, extra_task, state = c_problem()
    call = lambda kern, **kw: kern.run(order, last_task, extra_task, max_norm=C_MAX_NORM, apply_update=1, **kw)
    one = Kernel(lay, T, has, tg, *state)
    call(one)
    want = one.outputs()
    assert want["metrics"][1] > 0 and want["flags"].sum() < lay.K
    parts = Kernel(lay, T, has, tg, *state)
    for a, b in RANGES:
        call(parts, k_begin=a, k_end=b, phases=1)
    call(parts, phases=2)
    assert_same_bits(want, parts.outputs(), "three ranges")
    # the sharded path without two processes: the middle range's combined gradient arrives from its "owner", the rest is computed here
    fo = Kernel(lay, T, has, tg, *state)
    a, b = RANGES[1]
    fo.final[lay.off[a]:lay.off[b]] = one.final[lay.off[a]:lay.off[b]]
    call(fo, k_begin=a, k_end=b, phases=4)
    call(fo, k_begin=0, k_end=a, phases=1)
    call(fo, k_begin=b, k_end=lay.K, phases=1)
    call(fo, phases=2)
    got = fo.outputs()
    want_fo = dict(want, metrics=None)        # the owner counts its tensors' conflicts / projections, not this rank
    got["metrics"] = None
    assert_same_bits(want_fo, got, "foreign pass")


@gpu
def test_abort_flag_and_apply_update_0_leave_the_state_alone():
    lay, T, has, tg, order, last_task, extra_task, state = c_problem()
    one = Kernel(lay, T, has, tg, *state)
    one.run(order, last_task, extra_task, max_norm=C_MAX_NORM, apply_update=1)
    want = one.outputs()
    kern = Kernel(lay, T, has, tg, *state)
    s0 = kern.outputs()
    abort = torch.ones(1, dtype=torch.int32, device=DEV)
    kern.run(order, last_task, extra_task, max_norm=C_MAX_NORM, apply_update=1, abort=abort)
    s1 = kern.outputs()
    for key in ("params", "exp_avg", "exp_avg_sq", "steps"):
        assert torch.equal(s1[key], s0[key]), f"abort set: {key} changed"
    assert torch.equal(s1["final"], want["final"])
    abort.zero_()
    kern.run(order, last_task, extra_task, max_norm=C_MAX_NORM, apply_update=1, abort=abort)
    assert_same_bits(want, kern.outputs(), "abort cleared")
    kern = Kernel(lay, T, has, tg, *state)
    kern.run(order, last_task, extra_task, max_norm=C_MAX_NORM, apply_update=0, with_steps=False)
    s2 = kern.outputs()
    for key in ("params", "exp_avg", "exp_avg_sq", "steps"):
        assert torch.equal(s2[key], s0[key]), f"apply_update=0: {key} changed"
    for key in ("final", "normsq", "metrics", "flags"):
        assert torch.equal(s2[key], want[key]), key


@gpu
def test_slots_of_tasks_without_the_tensor_and_columns_beyond_T_are_never_read():
    lay, T, has, tg, order, last_task, extra_task, state = c_problem()
    clean = Kernel(lay, T, has, tg, *state)
    clean.run(order, last_task, extra_task, max_norm=C_MAX_NORM, apply_update=1)
    poisoned_tg, poisoned_has = tg.clone(), has.copy()
    for k in range(lay.K):
        for t in range(T):
            if not has[k, t]:
                poisoned_tg[t, lay.slot(k)] = float("nan")       # the slot only: the contract wants the padding zero
    poisoned_has[:, T:] = 1
    dirty = Kernel(lay, T, poisoned_has, poisoned_tg, *state)
    dirty.run(order, last_task, extra_task, max_norm=C_MAX_NORM, apply_update=1)
    assert_same_bits(clean.outputs(), dirty.outputs(), "poisoned")


# ------------------------------------------------------------------------------------------------ D. argument validation
D_CASES = {     # (T, K) -> the arguments of a call that must be refused
    "phases_0": lambda T, K: dict(phases=0),
    "k_end_past_K": lambda T, K: dict(k_end=K + 1),
    "k_begin_after_k_end": lambda T, K: dict(k_begin=2, k_end=1),
    "nine_tasks": lambda T, K: dict(num_tasks=9),
    "n_order_above_T": lambda T, K: dict(n_order=T + 1),
    "order_out_of_range": lambda T, K: dict(order=[0, T]),
    "last_task_not_below_T": lambda T, K: dict(last_task=T),
    "workspace_one_byte_short": lambda T, K: dict(ws_bytes=-1),
    "apply_without_optimizer_state": lambda T, K: dict(with_params=False),
}


@gpu
@pytest.mark.parametrize("case", list(D_CASES))
def test_bad_arguments_raise_and_launch_nothing(case):
    from gnn_pretraining_amd._lib import GnnmpError
    lay, T, order, last_task = Layout([5, 4097, 64]), 3, [1, 0, 2], 2
    has = np.zeros((lay.K, MAXT), np.uint8)
    has[:, :T] = 1
    kern = Kernel(lay, T, has, make_grads(5, lay, T, has), *b_state(5, lay)[:3], np.zeros(lay.K, np.float32),
                  *b_state(5, lay)[4:])
    kern.final.fill_(7.0)
    before = kern.outputs()
    kw = D_CASES[case](T, lay.K)
    order = kw.pop("order", order)
    last_task = kw.pop("last_task", last_task)
    if kw.get("ws_bytes") == -1:
        kw["ws_bytes"] = kern.ws_bytes - 1
    with pytest.raises(GnnmpError):
        kern.L.check(kern.call(order, last_task, -1, max_norm=C_MAX_NORM, apply_update=1, **kw), case)
    torch.cuda.synchronize()
    assert_same_bits(before, kern.outputs(), case)


# ------------------------------------------------------------------------------------------------ E. segment pack / unpack
SEG_CASES = {"n1": (1, False), "n7": (7, False), "n256": (256, False), "n7_over_2M_floats": (7, True)}


def seg_table(rs, n, big):
    """n slices of one buffer: offsets and lengths multiples of 4, some empty, laid out in a random order with gaps between them"""
    lens = 4 * rs.randint(1, 300, n).astype(np.int64)
    lens[rs.rand(n) < 0.25] = 0
    lens[rs.randint(n)] = 4 * rs.randint(1, 300)
    if big:                                          # > 2,097,152 floats: the grid-stride loop (2,048 x 256 threads x 4) makes three trips
        lens[0], lens[n // 2] = 3_000_000, 2_000_004
    offs, o = np.zeros(n, np.int64), 4 * rs.randint(0, 4)
    for i in rs.permutation(n):
        o += 4 * rs.randint(0, 5)
        offs[i] = o
        o += lens[i]
    pre = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    return offs, lens, pre, int(o) + 8


def bits(x):
    return x.cpu().view(torch.int32)


@gpu
@pytest.mark.parametrize("case", list(SEG_CASES))
def test_segments_pack_and_unpack_are_exact(case):
    from gnn_pretraining_amd import _lib as L, ops
    n, big = SEG_CASES[case]
    rs = np.random.RandomState(n + 1000 * big)
    gen = torch.Generator().manual_seed(n)
    offs, lens, pre, size = seg_table(rs, n, big)
    total = int(pre[-1])
    lib = L.lib()
    table = torch.from_numpy(np.concatenate([offs, pre])).to(DEV)
    base = torch.randn(size, generator=gen)
    packed = torch.full((total + 4,), -3.0, device=DEV)
    base_d = base.to(DEV)
    L.check(lib.gmp_segments_pack(ops._ptr(base_d), ops._ptr(packed), ops._ptr(table), n, total, ops._stream(base_d)), "pack")
    torch.cuda.synchronize()
    want = torch.cat([base[o:o + l] for o, l in zip(offs.tolist(), lens.tolist())])
    assert torch.equal(bits(packed[:total]), bits(want)), "pack"
    assert torch.equal(bits(packed[total:]), bits(torch.full((4,), -3.0))), "pack wrote past the total"
    src = torch.randn(total, generator=gen)
    scale = np.float32(0.37)
    dst, src_d = torch.full((size,), 1234.5, device=DEV), src.to(DEV)
    L.check(lib.gmp_segments_unpack(ops._ptr(dst), ops._ptr(src_d), ops._ptr(table), n, total, float(scale), ops._stream(dst)), "unpack")
    torch.cuda.synchronize()
    want = torch.full((size,), 1234.5)
    for i in range(n):
        want[offs[i]:offs[i] + lens[i]] = src[pre[i]:pre[i + 1]] * torch.tensor(scale)      # one fp32 product per float
    assert torch.equal(bits(dst), bits(want)), "unpack"


@gpu
def test_segments_refuse_bad_counts_and_do_nothing_for_total_0():
    from gnn_pretraining_amd import _lib as L, ops
    lib = L.lib()
    table = torch.zeros(2 * 257 + 1, dtype=torch.int64, device=DEV)
    base = torch.full((64,), 5.0, device=DEV)
    packed = torch.full((64,), -3.0, device=DEV)
    st = ops._stream(base)
    for n in (0, 257):
        with pytest.raises(L.GnnmpError):
            L.check(lib.gmp_segments_pack(ops._ptr(base), ops._ptr(packed), ops._ptr(table), n, 16, st), "pack")
        with pytest.raises(L.GnnmpError):
            L.check(lib.gmp_segments_unpack(ops._ptr(base), ops._ptr(packed), ops._ptr(table), n, 16, 1.0, st), "unpack")
    L.check(lib.gmp_segments_pack(ops._ptr(base), ops._ptr(packed), ops._ptr(table), 3, 0, st), "pack, total 0")
    L.check(lib.gmp_segments_unpack(ops._ptr(base), ops._ptr(packed), ops._ptr(table), 3, 0, 0.5, st), "unpack, total 0")
    torch.cuda.synchronize()
    assert bool((base == 5.0).all()) and bool((packed == -3.0).all())


# ------------------------------------------------------------------------------------------------ the reference itself (CPU)
TOY_TASKS = ["node_feat_mask", "link_pred", "node_contrast", "graph_prop", "domain_adv"]


class Toy(nn.Module):
    """parameters held by some tasks only, as in the real model"""

    def __init__(self):
        super().__init__()
        self.encoder = nn.Linear(4, 6)                         # every task but node_feat_mask (it runs the encoder under no_grad)
        self.mask_token = nn.Parameter(torch.randn(6))        # node_feat_mask only
        self.backbone = nn.Linear(6, 5)                        # every task
        self.heads = nn.ModuleDict({t: nn.Linear(5, 1) for t in TOY_TASKS})
        self.unused = nn.Parameter(torch.randn(3))            # no task

    def losses(self, x, y):
        out = {}
        for i, t in enumerate(TOY_TASKS):
            if t == "node_feat_mask":
                with torch.no_grad():
                    e = self.encoder(x)
                e = e + self.mask_token
            else:
                e = self.encoder(x * (i + 1))
            out[t] = ((self.heads[t](torch.tanh(self.backbone(torch.tanh(e)))) - y[i]) ** 2).mean()
        return out


def test_reference_composition_matches_the_oracle_training_step():
    """ref_pcgrad + ref_clip_adamw on each task's own gradients == the oracle's apply_gradient_surgery, domain_adv backward,
    clip_grad_norm_ and make_optimizer's AdamW on the module, two steps, float64 throughout"""
    torch.manual_seed(0)
    model = Toy().double()
    gen = torch.Generator().manual_seed(1)
    x = torch.randn(16, 4, generator=gen, dtype=torch.float64)
    y = 3 * torch.randn(len(TOY_TASKS), 16, 1, generator=gen, dtype=torch.float64)
    params = dict(model.named_parameters())
    names = list(params)
    lay = Layout([p.numel() for p in params.values()])
    opt = OTr.make_optimizer(model, TOY_TASKS)
    group = {}
    for g in opt.param_groups:
        g["lr"] *= 1000                     # a visible update and a visible decay
        g["weight_decay"] = 0.05
        group.update({id(p): g for p in g["params"]})
    lr = [group[id(params[n])]["lr"] for n in names]
    wd = [group[id(params[n])]["weight_decay"] for n in names]
    main, extra_task = TOY_TASKS[:-1], len(TOY_TASKS) - 1
    flat = torch.zeros(lay.P, dtype=torch.float64)
    for k, n in enumerate(names):
        flat[lay.slot(k)] = params[n].detach().flatten()
    m, v, steps = torch.zeros(lay.P, dtype=torch.float64), torch.zeros(lay.P, dtype=torch.float64), [0.0] * lay.K
    clipped = []
    for order_names in (["node_feat_mask", "graph_prop", "link_pred", "node_contrast"],
                        ["link_pred", "node_contrast", "node_feat_mask", "graph_prop"]):
        losses = model.losses(x, y)
        tg, has = torch.zeros(len(TOY_TASKS), lay.P, dtype=torch.float64), np.zeros((lay.K, MAXT), np.uint8)
        for t, task in enumerate(TOY_TASKS):
            model.zero_grad(set_to_none=True)
            losses[task].backward(retain_graph=True)
            for k, n in enumerate(names):
                if params[n].grad is not None:
                    has[k, t] = 1
                    tg[t, lay.slot(k)] = params[n].grad.flatten()
        order = [TOY_TASKS.index(t) for t in order_names]
        grads, _ = ref_pcgrad(tg, lay, has, order, TOY_TASKS.index(main[-1]), extra_task)
        clipped.append(sum(float((g ** 2).sum()) for g in grads if g is not None) ** 0.5 > OTr.MAX_GRAD_NORM)
        rp, rm, rv, rsteps = ref_clip_adamw(lay, grads, flat, m, v, steps, lr, wd, OTr.MAX_GRAD_NORM)
        # the oracle's step on the module itself (pretrain.py:137-153)
        opt.zero_grad(set_to_none=True)
        OTr.apply_gradient_surgery(model, {t: losses[t] for t in main}, order_names)
        losses["domain_adv"].backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm=OTr.MAX_GRAD_NORM)
        opt.step()
        for k, n in enumerate(names):
            assert torch.allclose(params[n].detach().flatten(), rp[k], rtol=0, atol=1e-13), n
            st = opt.state.get(params[n], {})
            if st:
                assert float(st["step"]) == rsteps[k], n
                assert torch.allclose(st["exp_avg"].flatten(), rm[k], rtol=0, atol=1e-13), n
                assert torch.allclose(st["exp_avg_sq"].flatten(), rv[k], rtol=0, atol=1e-13), n
            else:
                assert rsteps[k] == 0.0, n                    # never had a gradient
            flat[lay.slot(k)], m[lay.slot(k)], v[lay.slot(k)] = rp[k], rm[k], rv[k]
        steps = rsteps
        if order_names[0] == "node_feat_mask":
            # the quirks are in play: the encoder is not emitted (absent from the first task) and keeps graph_prop's raw gradient plus
            # domain_adv's; link_pred's head is neither in the first task nor the last, so it gets no gradient and no step at all
            k_enc, k_lp = names.index("encoder.weight"), names.index("heads.link_pred.weight")
            assert rsteps[k_enc] == 1.0 and rsteps[k_lp] == 0.0 and rsteps[names.index("unused")] == 0.0
    assert any(clipped)
