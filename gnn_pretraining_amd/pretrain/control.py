"""The callers that shape gradients around the hot path, with the
reference's class names and methods: TemperatureScheduler / GRLScheduler (schedulers.py),
AdaptiveLossBalancer (adaptive_loss_balancer.py), GradientSurgery (gradient_surgery.py),
TaskSpecificOptimizer (optimizers.py).  Numerics are pinned to the reference by the golden
vectors in tests/golden/reference_callers.json (tests/test_control.py).

GradientSurgery differs from the reference in mechanics only: the reference takes ~3 host syncs
per (tensor, task pair) -- about 1,900 per s4 step -- to evaluate ``norm() == 0`` and ``dot < 0``.
Here every per-tensor Gram entry <g_i, g_j> of a step is computed in ONE batched device pass, read
back in ONE transfer, and the projection coefficients are then solved on the host in the
reference's order; the projected gradients are formed with a single fused multiply-add per tensor.
"""
from __future__ import annotations

import math
import random
from typing import Dict, List, Optional

import torch
import torch.nn as nn
from torch import Tensor

FINAL_TEMP, INITIAL_TEMP = 0.2, 0.5
GAMMA, MAX_LAMBDA, START_ADVERSARIAL_EPOCH_FRACTION = 10.0, 0.01, 0.4
EPSILON, MIN_TOTAL_LOSS, WARMUP_STEPS = 1e-8, 1e-6, 100
DEFAULT_LR = DEFAULT_WEIGHT_DECAY = 1e-5
TASK_SPECIFIC_LR = {"link_pred": 5e-7, "node_feat_mask": 1e-5, "node_contrast": 1e-5, "graph_contrast": 1e-5,
                    "graph_prop": 1e-5, "domain_adv": 5e-6}


class TemperatureScheduler:
    def __init__(self, total_steps: int) -> None:
        self.total_steps, self.current_step = total_steps, 0

    def __call__(self) -> float:
        frac = min(1.0, self.current_step / self.total_steps)
        return float(INITIAL_TEMP * (FINAL_TEMP / INITIAL_TEMP) ** frac)

    def step(self) -> None:
        self.current_step += 1


class GRLScheduler:
    def __init__(self, total_epochs: int, steps_per_epoch: int) -> None:
        self.total_steps = total_epochs * steps_per_epoch
        self.start_steps = START_ADVERSARIAL_EPOCH_FRACTION * total_epochs * steps_per_epoch
        self.current_step = 0

    def __call__(self) -> float:
        if self.current_step < self.start_steps:
            return 0.0
        p = float(self.current_step - self.start_steps) / float(self.total_steps - self.start_steps)
        return float((2.0 / (1.0 + math.exp(-GAMMA * p)) - 1.0) * MAX_LAMBDA)

    def step(self) -> None:
        self.current_step += 1


class AdaptiveLossBalancer:
    def __init__(self) -> None:
        self.step_count, self.current_weights = 0, {}

    def balance_losses(self, task_losses: Dict[str, Tensor], domain_adv_lambda: float) -> Tensor:
        if len(task_losses) == 1:
            return next(iter(task_losses.values()))
        self.step_count += 1
        work = dict(task_losses)
        if "domain_adv" in work:
            others = sum(v for k, v in work.items() if k != "domain_adv")
            work["domain_adv"] = torch.clamp(-domain_adv_lambda * work["domain_adv"], min=-max(others * 0.5, 1.0))
        names = list(work)
        if self.step_count > WARMUP_STEPS:
            vals = torch.stack([work[k].detach() for k in names]).tolist()      # one transfer for all tasks
            mag = sum(abs(v) for v in vals)
            raw = [(1.0 / (abs(v) + EPSILON)) if mag > 0 else 1.0 for v in vals]
            z = sum(raw)
            weights = {k: r / z for k, r in zip(names, raw)}
        else:
            weights = {k: 1.0 / len(names) for k in names}
        self.current_weights = dict(weights)
        return torch.clamp(torch.stack([weights[k] * work[k] for k in names]).sum(), min=MIN_TOTAL_LOSS)

    def get_current_weights(self) -> Dict[str, float]:
        return self.current_weights

    def tick(self) -> None:
        """What a training step's balance_losses call leaves behind when its value is not needed (the stacked engine runs
        PCGrad on the per-task losses and never forms the total): the call counter that ends the warm-up.  The weights
        themselves are a function of the current losses only."""
        self.step_count += 1


class GradientSurgery:
    """PCGrad with the reference's exact semantics, including its gradient-setting quirk
    (gradient_surgery.py:61): only tensors present in the FIRST shuffled task's gradient set
    receive the PCGrad mean; the others keep whatever the LAST task's backward left in .grad."""

    RULES, SCOPES = ("reference", "pcgrad", "mean"), ("tensor", "model")

    def __init__(self, device: torch.device, grad_sync=None, shuffle_rng: Optional[random.Random] = None,
                 rule: str = "reference", scope: str = "tensor") -> None:
        """rule "reference": the class docstring's.  "pcgrad": PCGrad as published (Yu et al. 2020, Alg. 1) -- every holder of a tensor
        walks the other tasks in an order of its own (`perm`), the tensor gets the mean over its holders, so every parameter some task
        reaches is trained in every step; scope "tensor" projects tensor by tensor, "model" once over the whole shared vector (the
        tensors two or more tasks hold).  "mean": the plain mean over the holders (scope unused).  The same rules as the engine's
        (include/gnnmp.h gmp_mt_surgery_clip_adamw)."""
        if rule not in self.RULES or scope not in self.SCOPES:
            raise ValueError(f"rule must be one of {self.RULES}, scope one of {self.SCOPES}")
        if rule == "reference" and scope != "tensor":
            raise ValueError("the reference rule is per tensor: scope='model' needs rule='pcgrad'")
        self.device = device
        self.grad_sync = grad_sync          # dist.FlatGradSync: per-task gradients are averaged over ranks BEFORE PCGrad
        self.shuffle_rng = shuffle_rng      # data-parallel runs need the same task order on every rank
        self.rule, self.scope = rule, scope
        self.last_perm: Optional[List[List[int]]] = None

    def apply_gradient_surgery(self, model: nn.Module, task_losses: Dict[str, Tensor], task_names: List[str],
                               order: Optional[List[str]] = None, perm: Optional[List[List[int]]] = None) -> Dict[str, float]:
        if len(task_losses) <= 1:
            return {}
        if self.rule != "reference":
            return self._apply_rule(model, task_losses, perm)
        named = list(model.named_parameters())
        grads: Dict[str, Dict[str, Tensor]] = {}
        for t, loss in task_losses.items():
            model.zero_grad(set_to_none=True)
            loss.backward(retain_graph=True)
            grads[t] = {n: p.grad for n, p in named if p.grad is not None}      # fresh tensors: no clone needed
        if self.grad_sync is not None:
            self.grad_sync.average_task_grads_(grads)
        if order is None:
            order = list(task_names)
            if self.shuffle_rng is not None:
                self.shuffle_rng.shuffle(order)
            else:
                random.shuffle(order)                   # unseeded global RNG, as in the reference (:43)
        final, metrics = self._pcgrad(grads, order)
        for n, p in named:
            if n in final:
                p.grad = final[n]
        return metrics

    @staticmethod
    def _gram(grads: Dict[str, Dict[str, Tensor]], tasks: List[str], names: List[str]) -> torch.Tensor:
        """G[k, i, j] = <g_i, g_j> for tensor k (0 where a task lacks the tensor) -- one host transfer."""
        T = len(tasks)
        out = []
        for n in names:
            have = [t for t in tasks if n in grads[t]]
            M = torch.stack([grads[t][n].reshape(-1) for t in have])
            G = M @ M.t()
            full = torch.zeros(T, T, dtype=G.dtype, device=G.device)
            idx = torch.tensor([tasks.index(t) for t in have], device=G.device)
            full[idx.unsqueeze(1), idx.unsqueeze(0)] = G
            out.append(full)
        return torch.stack(out).double().cpu()

    def _pcgrad(self, grads, order: List[str]):
        tasks = list(order)
        names = sorted({n for t in tasks for n in grads[t]}, key=lambda n: n)
        gram = self._gram(grads, tasks, names)           # [K, T, T] on the host
        T = len(tasks)
        conflicts = projections = 0
        coeff: Dict[str, List[List[float]]] = {}
        for k, n in enumerate(names):
            G = gram[k]
            has = [n in grads[t] for t in tasks]
            alpha = [[1.0 if a == b else 0.0 for b in range(T)] for a in range(T)]   # g_i' = sum_b alpha[i][b] g_b
            for i in range(T):
                if not has[i]:
                    continue
                for j in range(i):
                    if not has[j]:
                        continue
                    a = alpha[i]
                    norm_i_sq = sum(a[p] * a[q] * float(G[p, q]) for p in range(T) for q in range(T))
                    norm_j_sq = float(G[j, j])
                    if norm_i_sq <= 0.0 or norm_j_sq <= 0.0:
                        continue
                    projections += 1
                    dot = sum(a[p] * float(G[p, j]) for p in range(T))
                    if dot < 0:
                        conflicts += 1
                        a[j] -= dot / norm_j_sq
            coeff[n] = alpha
        final = {}
        first = tasks[0]
        for n in grads[first]:
            alpha = coeff[n]
            holders = [i for i, t in enumerate(tasks) if n in grads[t]]
            w = [sum(alpha[i][b] for i in holders) / len(holders) for b in range(T)]
            acc = None
            for b in holders:
                if w[b] != 0.0:
                    term = grads[tasks[b]][n] * w[b]
                    acc = term if acc is None else acc.add_(term)
            final[n] = acc if acc is not None else torch.zeros_like(grads[first][n])
        metrics = {"gradient_surgery/total_conflicts": conflicts, "gradient_surgery/total_projections": projections,
                   "gradient_surgery/conflict_ratio": conflicts / max(projections, 1)}
        return final, metrics

    # ---- the rules beside the reference's ------------------------------------------------------------
    def draw_perm(self, n: int) -> List[List[int]]:
        """For each task in turn, one shuffle of the other tasks' positions (the engine's _optimizer draws the same way)."""
        perm = []
        for i in range(n):
            row = [j for j in range(n) if j != i]
            (self.shuffle_rng or random).shuffle(row)
            perm.append(row)
        return perm

    def _apply_rule(self, model: nn.Module, task_losses: Dict[str, Tensor], perm: Optional[List[List[int]]]) -> Dict[str, float]:
        named = list(model.named_parameters())
        tasks = list(task_losses)                       # no first-shuffled task here: positions are the dict order
        grads: Dict[str, Dict[str, Tensor]] = {}
        for t, loss in task_losses.items():
            model.zero_grad(set_to_none=True)
            loss.backward(retain_graph=True)
            grads[t] = {n: p.grad for n, p in named if p.grad is not None}
        if self.grad_sync is not None:
            self.grad_sync.average_task_grads_(grads)
        if self.rule == "pcgrad":
            if perm is None:
                perm = self.draw_perm(len(tasks))
            for i, row in enumerate(perm):
                if sorted(row) != [j for j in range(len(tasks)) if j != i]:
                    raise ValueError(f"perm[{i}] = {row} is no permutation of the other tasks' positions")
        else:
            perm = None
        self.last_perm = perm
        final, metrics = self._combine_rule(grads, tasks, perm)
        for n, p in named:
            if n in final:
                p.grad = final[n]
        return metrics

    def _combine_rule(self, grads, tasks: List[str], perm):
        T = len(tasks)
        names = sorted({n for t in tasks for n in grads[t]})
        holders = {n: [i for i, t in enumerate(tasks) if n in grads[t]] for n in names}
        count = {"conflicts": 0, "projections": 0}

        def walk(G: List[List[float]], held: List[int]) -> List[float]:
            """every holder's walk on one Gram matrix -> sum over the holders i of alpha[i][b] (v_i = sum_b alpha[i][b] g_b)"""
            col = [0.0] * T
            for i in held:
                a = [1.0 if b == i else 0.0 for b in range(T)]
                for j in perm[i]:
                    if j not in held:
                        continue
                    u = [sum(a[q] * G[q][p] for q in range(T)) for p in range(T)]        # <v, g_p>
                    norm_i_sq, norm_j_sq = sum(a[p] * u[p] for p in range(T)), G[j][j]
                    if norm_i_sq <= 0.0 or norm_j_sq <= 0.0:
                        continue
                    count["projections"] += 1
                    if u[j] < 0:
                        count["conflicts"] += 1
                        a[j] -= u[j] / norm_j_sq
                col = [c + x for c, x in zip(col, a)]
            return col

        weight: Dict[str, List[float]] = {n: [1.0 if b in holders[n] else 0.0 for b in range(T)] for n in names}    # the plain sum
        shared = [n for n in names if len(holders[n]) >= 2]
        if self.rule == "pcgrad" and shared:
            gram = self._gram(grads, tasks, shared)
            if self.scope == "model":
                col = walk(gram.sum(0).tolist(), sorted({i for n in shared for i in holders[n]}))
                for n in shared:
                    weight[n] = [col[b] if b in holders[n] else 0.0 for b in range(T)]
            else:
                for k, n in enumerate(shared):
                    weight[n] = walk(gram[k].tolist(), holders[n])
        final = {}
        for n in names:
            acc = None
            for b in holders[n]:
                w = weight[n][b] / len(holders[n])
                if w != 0.0:
                    term = grads[tasks[b]][n] * w
                    acc = term if acc is None else acc.add_(term)
            final[n] = acc if acc is not None else torch.zeros_like(grads[tasks[holders[n][0]]][n])
        conflicts, projections = count["conflicts"], count["projections"]
        metrics = {"gradient_surgery/total_conflicts": conflicts, "gradient_surgery/total_projections": projections,
                   "gradient_surgery/conflict_ratio": conflicts / max(projections, 1)}
        return final, metrics


class TaskSpecificOptimizer:
    def __init__(self, model: nn.Module, active_tasks: List[str]) -> None:
        self.model = model
        claimed, groups = set(), []
        for t in active_tasks:
            ps = []
            for n, p in model.named_parameters():
                if f"heads.{t}" in n:
                    ps.append(p)
                    claimed.add(n)
            if ps:
                groups.append({"params": ps, "lr": TASK_SPECIFIC_LR[t], "weight_decay": DEFAULT_WEIGHT_DECAY, "name": t})
        rest = [p for n, p in model.named_parameters() if n not in claimed]
        if rest:
            groups.append({"params": rest, "lr": DEFAULT_LR, "weight_decay": DEFAULT_WEIGHT_DECAY, "name": "default"})
        self.param_groups = groups
        self.optimizer = torch.optim.AdamW(self.param_groups)

    def zero_grad(self, set_to_none: bool = True) -> None:
        self.optimizer.zero_grad(set_to_none=set_to_none)

    def step(self) -> None:
        self.optimizer.step()
