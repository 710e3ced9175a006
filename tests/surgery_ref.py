"""Float64 restatement of the gradient-surgery rules (csrc/optim.hip, gmp_mt_surgery_clip_adamw; pretrain/control.py GradientSurgery).

It works on the vectors themselves, never on a Gram matrix, so it shares no arithmetic with the code it checks.

    P      the tasks of `order` (task indices); position i of the order <-> task order[i]
    H_k    the tasks of P whose has[k][t] is set
    perm   perm[i] = the order POSITIONS task i walks, a permutation of the positions other than i

One walk (`_walk`): task i starts from v = g_i and meets the tasks of its row that hold a vector; a pair with ||v|| == 0 or ||g_j|| == 0 is
skipped; every other pair counts one projection; where <v, g_j> < 0 it counts one conflict and v -= <v, g_j> / ||g_j||^2 g_j.

    reference  the walk of position i over the positions before it, per tensor; only tensors the first-shuffled task holds get the mean over
               their holders, the others keep last_task's raw gradient (or none).
    pcgrad     tensor scope: the walk per tensor over perm, final = mean over H_k.  model scope: one walk on the tasks' vectors over
               S = {k : |H_k| >= 2} (zero where a task lacks a tensor) over the tasks P_S that hold any tensor of S; with
               v_i = sum_b alpha[i][b] g_b, tensor k of S gets sum_{b in H_k} (sum_{i in P_S} alpha[i][b]) / |H_k| g_b[k]; the other tensors
               as in tensor scope.
    mean       the mean over H_k, nothing counted.
extra_task's gradient is added on top under every rule.

The MARGIN of a problem: the smallest, over every decision a walk took, of
    sign of <v, g_j>:     |<v, g_j>| / (B ||g_j||)
    ||v|| == 0 ?:         ||v|| / B            (not taken where g_i or g_j is exactly zero: that zero is exact in any arithmetic)
with B = ||g_i|| + the lengths of the projections taken so far >= ||v||, the scale of a Gram-space evaluation's rounding (the bound
pcgrad_min_margin of tests/test_gpu_optim.py uses; it is never above the plain cosine).  Data whose margin is far above the rounding of
the code under test takes the same decisions there.
"""
import math

import torch


class Stats:
    def __init__(self):
        self.conflicts = self.projections = 0
        self.margin = math.inf


def _walk(vecs, rows, stats):
    """vecs {position: float64 vector}, rows {position: positions to walk} -> alpha {i: {b: coefficient}} with v_i = sum_b alpha[i][b] g_b"""
    norms = {p: v.norm().item() for p, v in vecs.items()}
    alpha = {}
    for i in sorted(vecs):
        v, al, bound = vecs[i].clone(), {i: 1.0}, norms[i]
        for j in rows[i]:
            if j not in vecs:
                continue
            gj, nj = vecs[j], norms[j]
            nv = v.norm().item()
            if norms[i] > 0 and nj > 0:
                stats.margin = min(stats.margin, nv / bound)
            if nv == 0 or nj == 0:
                continue
            stats.projections += 1
            dot = torch.dot(v, gj).item()
            stats.margin = min(stats.margin, abs(dot) / (bound * nj))
            if dot < 0:
                stats.conflicts += 1
                c = dot / nj ** 2
                v = v - c * gj
                al[j] = al.get(j, 0.0) - c
                bound += abs(dot) / nj
        alpha[i] = al
    return alpha


def _mix(alpha, vecs, walkers):
    """(1 / |vecs|) sum_{i in walkers} v_i, as a combination of the holders' original vectors"""
    out = None
    for b in sorted(vecs):
        w = sum(alpha[i].get(b, 0.0) for i in walkers) / len(vecs)
        out = w * vecs[b] if out is None else out + w * vecs[b]
    return out


def surgery(tg, lay, has, order, perm=None, rule="reference", scope="tensor", last_task=-1, extra_task=-1):
    """-> (per-tensor final gradient or None, (conflicts, projections), margin).  tg [T, P]; lay has K and slot(k); has [K, >= T]."""
    assert rule in ("reference", "pcgrad", "mean") and scope in ("tensor", "model")
    n = len(order)
    g = lambda pos, k: tg[order[pos], lay.slot(k)].double()
    held = [[pos for pos in range(n) if has[k, order[pos]]] for k in range(lay.K)]
    stats = Stats()
    final = [None] * lay.K
    if rule == "reference":
        rows = {i: list(range(i)) for i in range(n)}
        for k in range(lay.K):
            vecs = {pos: g(pos, k) for pos in held[k]}
            alpha = _walk(vecs, rows, stats)                      # counted for every tensor, emitted or not
            if 0 in vecs:
                final[k] = _mix(alpha, vecs, held[k])
            elif last_task >= 0 and has[k, last_task]:
                final[k] = tg[last_task, lay.slot(k)].double()
    elif rule == "mean":
        for k in range(lay.K):
            if held[k]:
                final[k] = sum(g(pos, k) for pos in held[k]) / len(held[k])
    else:
        rows = {i: [int(j) for j in perm[i]] for i in range(n)} if n > 1 else {0: []}
        for i in range(n):
            assert sorted(rows[i]) == [j for j in range(n) if j != i], "perm row is no permutation of the other positions"
        shared = [k for k in range(lay.K) if len(held[k]) >= 2] if scope == "model" else []
        for k in range(lay.K):
            if held[k] and k not in shared:
                vecs = {pos: g(pos, k) for pos in held[k]}
                final[k] = _mix(_walk(vecs, rows, stats), vecs, held[k])
        if shared:
            walkers = sorted({pos for k in shared for pos in held[k]})
            whole = {pos: torch.cat([g(pos, k) if pos in held[k] else torch.zeros(lay.lens[k], dtype=torch.float64) for k in shared])
                     for pos in walkers}
            alpha = _walk(whole, rows, stats)
            for k in shared:
                final[k] = _mix(alpha, {pos: g(pos, k) for pos in held[k]}, walkers)
    if extra_task >= 0:
        for k in range(lay.K):
            if has[k, extra_task]:
                ge = tg[extra_task, lay.slot(k)].double()
                final[k] = ge if final[k] is None else final[k] + ge
    return final, (stats.conflicts, stats.projections), stats.margin


def identity_perm(n):
    return [[j for j in range(n) if j != i] for i in range(n)]


def draw_perm(rng, n):
    """as the engine draws it: for each position in turn, one shuffle of the others (rng: random.Random or the random module)"""
    out = []
    for i in range(n):
        row = [j for j in range(n) if j != i]
        rng.shuffle(row)
        out.append(row)
    return out
