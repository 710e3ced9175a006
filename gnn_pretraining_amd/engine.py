"""Stacked-step engine: one whole pre-training step (all tasks x all domains) as ~250 launches.

The reference runs 28 separate encoder+backbone forwards per s4 step (7 per domain: NFM 1, LP 1, NC 2,
GC 2, GP 1 -- src/pretrain/pretrain.py:124-129 over tasks.py), then 5 full backwards for PCGrad.
All 28 share the backbone weights, so here they are STACKED into one block-diagonal pass:

  * every reference forward() call becomes a *segment* of rows; BatchNorm statistics are taken per
    segment (gmp_bn_fwd seg_ptr), so the stacked pass computes exactly what the 28 calls compute,
    running statistics included (segments are applied in the reference's call order);
  * segments are laid out task-major, so each task owns one contiguous row range: ONE backward pass
    produces all per-task weight gradients PCGrad needs (grouped TN GEMMs / grouped reductions that
    write straight into a [tasks, params] gradient buffer) instead of five backward passes;
  * per-domain heads run as grouped GEMMs (one group per domain);
  * PCGrad + clip + AdamW are five multi-tensor launches over flat buffers, with the reference's
    "which tensors receive a gradient" rule (gradient_surgery.py:61) reproduced exactly.

Host work per step is index bookkeeping only (augmentation / masks / negatives with the reference's CPU
RNG contract) and ships to the device in two packed copies; nothing in the step reads back from the GPU.
No autograd: forward and backward are explicit kernel sequences over a preallocated arena.
"""
from __future__ import annotations

import ctypes as C
import os
import random
import time as _t
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from . import _lib as L
from .constants import DOMAIN_DIMENSIONS, GRAPH_PROPERTY_DIM
from .models.gnn import DROPOUT_RATE, GNN_HIDDEN_DIM, GNN_NUM_LAYERS
from .models.pretrain_model import PretrainableGNN
from .pretrain.control import DEFAULT_LR, DEFAULT_WEIGHT_DECAY, TASK_SPECIFIC_LR
from .step_host import StepInputs, StepPlan, ViewArrays, Artefacts, hostdraw, merge_mirrored_pairs, L_view_sizes      # noqa: F401  (re-exported)
from .step_host import SUPPORTED_TASKS, StepHost, _EMPTY_ART      # noqa: F401

H = GNN_HIDDEN_DIM
NT, NN, TN = 0, 1, 2
MAXT = 8
SEG_CSR_MAX_ROWS, SEG_CSR_MAX_EDGES = 8192, 24576        # gmp_csr_build_segmented: what one workgroup's LDS holds

# rough length (us) of each head's kernel chain at the s4 workload, used only to balance heads over the four streams
HEAD_CHAIN_US = {"node_contrast": 350.0, "link_pred": 330.0, "graph_contrast": 250.0, "node_feat_mask": 130.0, "graph_prop": 100.0,
                 "domain_adv": 100.0}
DA_HIDDEN, DA_DROPOUT = 128, 0.5          # heads.py:11-12


_ARR_CACHE: Dict[Tuple, "C.Array"] = {}


def _memo_array(ctype):
    """xs -> ctypes array of ctype; memoised by content (offset/row tables repeat every step)."""
    def make(xs) -> "C.Array":
        key = (ctype,) + tuple(xs)
        a = _ARR_CACHE.get(key)
        if a is None:
            if len(_ARR_CACHE) > 20000:
                _ARR_CACHE.clear()
            a = _ARR_CACHE[key] = (ctype * len(xs))(*[int(v) for v in xs])
        return a
    return make


_i32, _i64 = _memo_array(C.c_int32), _memo_array(C.c_int64)


def _merge_runs(ranges):
    """[k0, k1) tensor-index ranges -> the fewest contiguous runs covering them (one PCGrad launch set per run)."""
    out = []
    for a, b in sorted(r for r in ranges if r[1] > r[0]):
        if out and out[-1][1] == a:
            out[-1][1] = b
        else:
            out.append([a, b])
    return out


def device_views_to_host(dv) -> Tuple["ViewArrays", "ViewArrays"]:
    """ops.DeviceViews (gmp_aug_two_views outputs, on the device) -> the two ViewArrays the planner takes.  One small read-back:
    the counts say how much of the edge / common arrays is valid."""
    tot = dv.totals.cpu().tolist()
    out = []
    for v in range(2):
        rm = dv.rowmask[v].cpu().numpy().view(np.uint64) if tot[3 + v] else None
        out.append(ViewArrays(dv.rows[v].cpu().numpy(), dv.edges[v][:, :tot[v]].cpu().numpy(), np.asarray(dv.view_ptr, dtype=np.int64),
                              rm, dv.common[v][:tot[2]].cpu().numpy()))
    return out[0], out[1]


class DrawTicket:
    """One step's device-side draws in flight: the pinned slot they land in, where each (task, domain) piece sits, the flag value
    that says they have landed (StepEngine.enqueue_draws / collect_draws)."""
    __slots__ = ("slot", "layout", "epoch")

    def __init__(self, slot, layout, epoch) -> None:
        self.slot, self.layout, self.epoch = slot, layout, epoch


class StepEngine(StepHost):
    """The device half of a step on top of StepHost's draws and layout: the parameter arena, streams and gates, the native executor
    (csrc/step.hip through _fill_desc), the optimizer, the data-parallel exchange, the device draws.  The same step launched kernel by
    kernel from Python (native=False) is step_sequence.LaunchSequence, built on first use by sequence()."""

    def __init__(self, model: PretrainableGNN, tasks: Sequence[str], domains: Sequence[str], device,
                 max_rows: int = 16384, max_edges: int = 131072, seed: int = 0, shuffle_rng: Optional[random.Random] = None,
                 grad_sync=None, rng_mode: str = "reference", native: bool = True, neg_rng: Optional[random.Random] = None,
                 dp_mode: Optional[str] = None, device_negatives: bool = False, surgery: str = "reference",
                 surgery_scope: str = "tensor") -> None:
        super().__init__(tasks, domains, seed=seed, rng_mode=rng_mode, neg_rng=neg_rng, max_rows=max_rows, max_edges=max_edges)
        self.native = native       # True: csrc/step.hip enqueues the step; False: the same launches one by one from Python
        # data-parallel exchange: "allreduce" (every rank all-reduces all per-task gradients and runs the whole PCGrad: dist.OverlappedGradSync)
        # or "sharded" (reduce-scatter to the owner of each tensor, PCGrad on the owned tensors, all-gather of the combined gradient:
        # dist.ShardedGradSync -- 30 % fewer bytes, PCGrad 1/W per rank; needs the native executor)
        self.dp_mode = dp_mode or os.environ.get("GMP_DP_MODE", "allreduce")
        if self.dp_mode not in ("allreduce", "sharded"):
            raise ValueError("dp_mode must be 'allreduce' or 'sharded'")
        # gradient-surgery rule (include/gnnmp.h gmp_mt_surgery_clip_adamw): "reference" = the reference's PCGrad, quirk included (only
        # tensors of the first-shuffled task get the PCGrad mean, the last task keeps its raw gradient, the other heads get none);
        # "pcgrad" = PCGrad as published, per tensor or over the whole shared vector ("model"); "mean" = the plain mean (scope unused)
        if surgery not in L.SURGERY_RULES or surgery_scope not in L.SURGERY_SCOPES:
            raise ValueError(f"surgery must be one of {sorted(L.SURGERY_RULES)}, surgery_scope one of {sorted(L.SURGERY_SCOPES)}")
        if surgery == "reference" and surgery_scope != "tensor":
            raise ValueError("the reference rule is per tensor: surgery_scope='model' needs surgery='pcgrad'")
        if surgery != "reference" and self.dp_mode == "sharded":
            raise ValueError("dp_mode='sharded' needs surgery='reference': its foreign pass encodes the reference's emission rule")
        self.surgery, self.surgery_scope = surgery, surgery_scope
        self.last_order, self.last_perm = None, None
        self._shard_sync_obj = None
        # link-prediction negatives drawn on the device too (csrc/augment.hip gmp_aug_negative_edges), riding the draw ticket: opt-in
        if device_negatives and rng_mode != "device":
            raise ValueError("device_negatives needs rng_mode='device'")
        self.device_negatives = bool(device_negatives)
        self.model, self.device = model, torch.device(device)
        self.T, self.D = len(self.tasks), len(self.domains)
        self._bn_calls_dom = [0] * self.D
        self.lib = L.lib()
        self.dpad = 40 if max(DOMAIN_DIMENSIONS[d] for d in domains) <= 40 else 64
        self.step_count = 0
        self.shuffle_rng = shuffle_rng
        self.grad_sync = grad_sync
        self._packed_sync = None
        self._bn_calls = 0
        self.temperature = 0.5
        self.da_dropout = DA_DROPOUT
        self.grl_lambda = 0.0              # gradient-reversal strength of the domain-adversarial task (GRLScheduler)
        self._p_cache, self._sequence = {}, None
        self.host_ms = {"draw": 0.0, "plan": 0.0, "upload": 0.0, "launch": 0.0, "steps": 0}   # host time per phase (upload includes ring waits)
        self.dropout_p = DROPOUT_RATE
        self.max_grad_norm = 0.5
        self._desc, self.gates_mismatch = None, None       # the native executor's step descriptor (_init_desc); what verify_gates saw differ
        self._lead: Dict[int, "torch.cuda.Event"] = {}       # rng_mode 'device': end-of-step events the launcher waits on (step())
        self._has_dirty = False            # the device copy of the gradient-availability table differs from has_static (_upload)
        # device draws: ring of pinned result slots, ticket counter, workspace, outgrown buffers still in use, sequence number per mode
        self._draw_slots, self._draw_count, self._draw_ws, self._draw_graveyard = [None] * self.DRAW_SLOTS, 0, None, []
        self._draw_seq = {True: 0, False: 0}
        self._flatten_parameters()
        self._build_tables()
        self._alloc()

    @property
    def upload_on_aux(self) -> bool:
        """Native executor with gates: the step's index arrays go up on the aux stream (16 us of PCIe reads off the main stream)."""
        return bool(self.use_gates and self.native and os.environ.get("GMP_UPLOAD_ON_AUX", "1") != "0")

    @property
    def parts_beside_backward(self) -> bool:
        """(self.native may be flipped after construction -- the tests do: only the native executor publishes the part flags)"""
        return bool(self._parts_ok and self.native)

    # ------------------------------------------------------------------ parameters
    def _flatten_parameters(self) -> None:
        m, dev = self.model, self.device
        named = dict(m.named_parameters())
        enc = [m.input_encoders[d] for d in self.domains]
        order: List[Tuple[str, Tensor]] = []
        for d, e in zip(self.domains, enc):
            order.append((f"input_encoders.{d}.linear.weight", e.linear.weight))
        for key in ("linear.bias", "batch_norm.weight", "batch_norm.bias"):      # [D][256] blocks (grouped BN layout)
            for d in self.domains:
                order.append((f"input_encoders.{d}.{key}", named[f"input_encoders.{d}.{key}"]))
        seen = {n for n, _ in order}
        for n, p in named.items():
            if n not in seen:
                order.append((n, p))
        al4 = lambda v: (v + 3) // 4 * 4           # every tensor starts 16-byte aligned (float4 / MFMA tile loads)
        self.off: Dict[str, int] = {}
        o = 0
        for n, p in order:
            self.off[n] = o
            o += al4(p.numel())
        self.P = o
        self.P_shared = min(self.off[n] for n, _ in order if n.startswith("heads.")) if any(n.startswith("heads.") for n, _ in order) else o
        self.flat = torch.zeros(self.P, device=dev)
        for n, p in order:
            o = self.off[n]
            self.flat[o:o + p.numel()].copy_(p.data.reshape(-1))
            p.data = self.flat[o:o + p.numel()].view_as(p)
        self.names = [n for n, _ in order]
        self.numel = {n: p.numel() for n, p in order}
        # encoder running statistics as [D][256] blocks
        self.enc_rm = torch.zeros(self.D, H, device=dev)
        self.enc_rv = torch.ones(self.D, H, device=dev)
        for i, e in enumerate(enc):
            self.enc_rm[i].copy_(e.batch_norm.running_mean)
            self.enc_rv[i].copy_(e.batch_norm.running_var)
            e.batch_norm.running_mean.data = self.enc_rm[i]
            e.batch_norm.running_var.data = self.enc_rv[i]
        self.exp_avg = torch.zeros(self.P, device=dev)
        self.exp_avg_sq = torch.zeros(self.P, device=dev)

    def _build_tables(self) -> None:
        dev, T = self.device, self.T
        K = len(self.names)
        self.K = K
        self.t_off = torch.tensor([self.off[n] for n in self.names], dtype=torch.int64, device=dev)
        self.t_len = torch.tensor([self.numel[n] for n in self.names], dtype=torch.int32, device=dev)
        has = np.zeros((K, MAXT), dtype=np.uint8)
        lr = np.zeros(K, dtype=np.float32)
        for k, n in enumerate(self.names):
            lr[k] = DEFAULT_LR
            if n.startswith("input_encoders."):
                for t, task in enumerate(self.tasks):
                    has[k, t] = task != "node_feat_mask"        # NFM runs the encoder under no_grad
            elif n == "mask_token":
                for t, task in enumerate(self.tasks):
                    has[k, t] = task == "node_feat_mask"
            elif n.startswith("gnn_backbone."):
                has[k, :T] = 1
            elif n.startswith("heads."):
                for t, task in enumerate(self.tasks):
                    if f"heads.{task}" in n:
                        has[k, t] = 1
                        lr[k] = TASK_SPECIFIC_LR[task]
        self.has_static = has
        self.has = torch.from_numpy(has.copy()).to(dev)
        self.lr = torch.from_numpy(lr).to(dev)
        self.wd = torch.full((K,), DEFAULT_WEIGHT_DECAY, dtype=torch.float32, device=dev)
        self.steps = torch.zeros(K, dtype=torch.float32, device=dev)
        self.name_index = {n: k for k, n in enumerate(self.names)}

    def _alloc(self) -> None:
        dev, R = self.device, self.max_rows
        f = lambda *shape: torch.empty(*shape, device=dev)
        self.task_grads = torch.zeros(self.T, self.P, device=dev)
        self.final_grad = torch.zeros(self.P, device=dev)
        self.normsq = torch.zeros(1, device=dev)
        self.metrics = torch.zeros(2, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(self.K, dtype=torch.int32, device=dev)
        self.mt_ws = torch.empty(self.lib.gmp_mt_workspace_bytes(self.K), dtype=torch.uint8, device=dev)
        Lr = GNN_NUM_LAYERS
        self.z0 = f(R, H)
        self.h = [f(R, H) for _ in range(Lr + 1)]
        self.a = [f(R, H) for _ in range(Lr)]
        self.z1 = [f(R, 2 * H) for _ in range(Lr)]
        self.r1 = [f(R, 2 * H) for _ in range(Lr)]
        self.z2 = [f(R, H) for _ in range(Lr)]
        self.stat = {k: f(Lr, self.S_MAX, c) for k, c in (("m1", 2 * H), ("s1", 2 * H), ("m2", H), ("s2", H))}
        self.enc_mean, self.enc_rstd = f(self.S_MAX, H), f(self.S_MAX, H)
        self.gA, self.gB = f(R, H), f(R, H)                  # ping-pong [R,256] gradients
        self.ga = f(R, H)                                    # gradient w.r.t. a layer's aggregated input (own buffer: activations stay intact)
        self.gW = f(R, 2 * H)                                # [R,512] gradients
        # per-layer g_u / g_z1 of the native executor's backward: aux never holds main back (gnnmp_step.h)
        self.gu_l, self.gz1_l = [f(R, H) for _ in range(Lr)], [f(R, 2 * H) for _ in range(Lr)]
        self.rowdot = f(Lr * R)                              # one slice per backward layer for the native executor (gnnmp_step.h)
        self.gemm_ws = torch.empty(48 << 20, dtype=torch.uint8, device=dev)     # slice partials of the grouped weight-gradient GEMMs (aux | second weight-gradient stream) | encoder backward (main)
        # the task heads are independent of each other: each has its own scratch and they share four streams
        # The runtime multiplexes HIP streams onto 4 hardware queues (GPU_MAX_HW_QUEUES; raising it made the step 2.4x
        # slower), and a per-task stream layout left three task heads serialised on one queue (profiles/README.md).  So:
        # exactly four streams -- main, aux and two more -- and the heads are packed onto them by estimated chain length
        # (longest first onto the least-loaded stream; main and aux are idle while the heads run).
        # ... and which hardware queue a stream lands on is measured, not assumed (streams.py): a kernel trace showed two of the
        # four streams sharing the main stream's queue, their heads running behind main's instead of beside them.
        from . import streams as ST
        self.aux_stream, *extra = ST.concurrent_streams(dev, 3)
        # Cross-stream dependencies inside the native step are carried by GATES (a sleeping wave on a flag word, csrc/streams.hip)
        # instead of events when all four streams were measured on hardware queues of their own: a queue parked on an event wait
        # costs every running queue ~2 us per kernel boundary, and with the host several steps ahead two or three queues were
        # parked most of the time (scripts/diag_blocked_queues.py).  In one in-order queue a gate ahead of its opener would never
        # open, hence the condition.  GMP_STEP_GATES=0 keeps the events (needed under tools that serialise kernels, e.g. --pmc).
        self.sync_flags = torch.zeros(64, dtype=torch.int32, device=dev)
        self._epoch = 0
        self.use_gates = bool(ST.last_report.get("calibrated") and ST.last_report.get("own_queue") == 3
                              and os.environ.get("GMP_STEP_GATES", "1") != "0")
        # PCGrad (and the data-parallel exchange) part by part beside the backward: needs the gates and the native executor
        # (opt-in, GMP_OPT_OVERLAP=1: measured 1.58 against 1.54 ms/step on one GPU -- 28 small launches on the exchange stream beside
        # the backward and a longer hand-over chain at the end cost more than the 58 us of Gram / solve / combine they take off it)
        self._parts_ok = (self.use_gates and os.environ.get("GMP_DP_OVERLAP", "1") != "0" and os.environ.get("GMP_OPT_OVERLAP", "0") == "1")
        self.comm_stream = extra[1]        # data-parallel exchange beside the backward (the head streams are idle by then)
        bins = [[0.0, extra[0]], [0.0, extra[1]], [0.0, self.aux_stream], [0.0, None]]      # None = the main stream
        self.task_streams = [None] * self.T
        for ti in sorted(range(self.T), key=lambda i: -HEAD_CHAIN_US.get(self.tasks[i], 100.0)):
            b = min(bins, key=lambda x: x[0])
            b[0] += HEAD_CHAIN_US.get(self.tasks[ti], 100.0)
            self.task_streams[ti] = b[1]
        self.task_gemm_ws = [torch.empty(24 << 20, dtype=torch.uint8, device=dev) for _ in range(self.T)]
        self.task_loss_ws = [torch.empty(self.lib.gmp_loss_workspace_bytes(R * H), dtype=torch.uint8, device=dev) for _ in range(self.T)]
        # one slice per BatchNorm (11) + spare, each large enough for the long-segment regime (segments up to R rows): the
        # native executor keeps every BN backward's per-segment sums until the aux stream has reduced them per task
        self.bn_ws = torch.empty(12 * self.lib.gmp_bn_workspace_bytes(R, 2 * H, self.S_MAX, R), dtype=torch.uint8, device=dev)
        self.csr_ws = torch.empty(self.lib.gmp_csr_build_workspace_bytes(R, self.max_edges), dtype=torch.uint8, device=dev)
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
        self.csr = [i32(R + 1), i32(self.max_edges), i32(self.max_edges), i32(R + 1), i32(self.max_edges), i32(self.max_edges)]
        self.csr_status = i32(1)
        self.lp_csr_status = i32(1)
        self.lp_csr_ws = torch.empty(self.lib.gmp_csr_build_workspace_bytes(R, self.max_edges), dtype=torch.uint8, device=dev)
        self.lp_csr = [i32(R + 1), i32(self.max_edges), i32(self.max_edges), i32(R + 1), i32(self.max_edges), i32(self.max_edges)]
        self.loss_sums = torch.zeros(MAXT, device=dev)       # per-task loss SUMS of the last step
        # head workspaces (rows bounded by max_rows / edges)
        self.hd = {k: f(n, c) for k, (n, c) in {
            "nfm_in": (R, H), "nfm_y1": (R, H), "nfm_d1": (R, H), "nfm_y2": (R, H), "nfm_tgt": (R, H), "nfm_g": (R, H), "nfm_g1": (R, H), "nfm_gin": (R, H),
            "lp_feat": (self.KMAX, 3 * H), "lp_y1": (self.KMAX, H), "lp_d1": (self.KMAX, H), "lp_gy1": (self.KMAX, H),
            "lp_gfeat": (self.KMAX, 3 * H), "lp_ghs": (self.KMAX, H), "lp_ghd": (self.KMAX, H),
            "nc_in": (2 * R, H), "nc_y1": (2 * R, H), "nc_d1": (2 * R, H), "nc_z": (2 * R, 128), "nc_gz": (2 * R, 128), "nc_g1": (2 * R, H), "nc_gin": (2 * R, H),
            "gc_mean": (1024, H), "gc_max": (1024, H), "gc_in": (1024, 2 * H), "gc_y1": (1024, H), "gc_d1": (1024, H), "gc_z": (1024, 128),
            "gc_gz": (1024, 128), "gc_g1": (1024, H), "gc_gin": (1024, 2 * H), "gc_gmean": (1024, H), "gc_gmax": (1024, H),
            "da_in": (1024, H), "da_y1": (1024, DA_HIDDEN), "da_d1": (1024, DA_HIDDEN), "da_logits": (1024, 8), "da_glogits": (1024, 8),
            "da_g1": (1024, DA_HIDDEN), "da_gin": (1024, H),
            "gp_in": (1024, H), "gp_y1": (1024, 2 * H), "gp_d1": (1024, 2 * H), "gp_y2": (1024, 16), "gp_g2": (1024, 16), "gp_g1": (1024, 2 * H), "gp_gin": (1024, H),
        }.items()}
        # (lp_lab: upload set below; merged rows keep two scores each -- one per ordered row of the reference's list)
        self.lp_y2, self.lp_p, self.lp_gy2 = f(2 * self.KMAX), f(2 * self.KMAX), f(2 * self.KMAX)
        self.gp_y2 = f(1024, GRAPH_PROPERTY_DIM)
        self.gp_g2 = f(1024, GRAPH_PROPERTY_DIM)
        # one per contrastive head, keyed by the head's first scalar slot (0: node_contrast, D: graph_contrast)
        self.ntx_ws = {s: torch.empty(self.lib.gmp_nt_xent_grouped_workspace_bytes(self.D, 512, 128), dtype=torch.uint8, device=dev) for s in (0, self.D)}
        # packed per-step index uploads (pinned staging; StepHost.plan checks a step against these capacities)
        # The host runs several steps ahead of the GPU (nothing in a step syncs), so the pinned staging buffers
        # form a ring: a slot is refilled only after the copy that last read it has completed (event per slot).
        self.STAGES = 4
        self.stage = [{"pin32": torch.empty(self.i32_cap, dtype=torch.int32).pin_memory(),
                       "pin64": torch.empty(self.i64_cap, dtype=torch.int64).pin_memory(),
                       "pinf": torch.empty(64 + self.KMAX, dtype=torch.float32).pin_memory(),
                       "event": None} for _ in range(self.STAGES)]
        # Two sets of upload destinations, alternating by step: the native executor uploads step t+1's arrays on the AUX stream,
        # behind aux's last work of step t and beside main's tail / optimizer, into the set step t is not using.
        self._up_sets = [(torch.empty(self.i32_cap, dtype=torch.int32, device=dev), torch.empty(self.i64_cap, dtype=torch.int64, device=dev),
                          torch.zeros(64, device=dev), f(self.KMAX)) for _ in range(2)]
        self.dev32, self.dev64, self.scal, self.lp_lab = self._up_sets[0]

    # ------------------------------------------------------------------ draws (the host modes and plan() are StepHost's)
    def draw(self, inp: StepInputs, gen: torch.Generator) -> Dict[str, object]:
        """StepHost.draw, plus rng_mode 'device': the draws made by kernels on the aux stream (enqueue_draws / collect_draws)."""
        if self.rng_mode == "device":
            return self.collect_draws(inp, self.enqueue_draws(inp))
        return super().draw(inp, gen)

    def rng_state(self) -> Dict[str, object]:
        """StepHost's stream of negatives plus the device-draw sequence numbers and the step counter (the dropout seed)."""
        return {**super().rng_state(), "draw_seq": dict(self._draw_seq), "step_count": int(self.step_count)}

    def set_rng_state(self, st: Dict[str, object]) -> None:
        super().set_rng_state(st)
        self._draw_seq = {bool(k): int(n) for k, n in st.get("draw_seq", {}).items()} or {True: 0, False: 0}
        self.step_count = int(st.get("step_count", self.step_count))

    # ---- device draws (csrc/augment.hip): masks and views built on the GPU, one ticket per step ----------------------------
    DRAW_SLOTS = 8

    def enqueue_draws(self, inp: StepInputs) -> "DrawTicket":
        """Enqueue the device-side draws of ONE step (rng_mode 'device'): node-feature-masking indices and the two augmented views
        of every contrastive (task, domain) pair, by gmp_aug_node_masks / gmp_aug_two_views on the aux stream (with device_negatives
        also the link-prediction negatives of every domain whose graphs fit gmp_aug_negative_edges), followed by one copy
        kernel that writes the results into a pinned host slot and a one-thread kernel that raises the slot's flag.  Safe to call
        from the prefetch thread while the launcher thread enqueues steps: the kernels depend on nothing a step computes, and
        wherever they land between the aux stream's packets they run at most one step later.  Returns the ticket
        collect_draws() waits on."""
        k = self._draw_count                       # ticket number: ring slot and flag value (every enqueue, probes and evaluation included)
        self._draw_count += 1
        # The random stream is a function of (engine seed, mode, how many inputs of that mode were drawn), not of the ticket number:
        # evaluation passes and verify_gates' probe steps (which rewinds its own) leave the training sequence where it was
        mode = bool(self.model.training)
        seq = self._draw_seq[mode]
        self._draw_seq[mode] = seq + 1
        self._bury()                               # free outgrown buffers the aux stream has passed
        lay, off = [], 0

        def take(nbytes: int) -> int:
            nonlocal off
            o = off
            off += (nbytes + 15) // 16 * 16
            return o

        for t in self.tasks:
            if t not in ("node_feat_mask", "node_contrast", "graph_contrast"):
                continue
            for d in self.domains:
                hb = inp.host[d]
                G, N, E = hb.num_graphs, hb.num_nodes, hb.num_edges
                if G == 0 or (t == "graph_contrast" and G < 2):
                    continue
                _, _, _, _, _, vptr_h, moff_h = inp.dev_graph(d)
                if t == "node_feat_mask":
                    lay.append((t, d, {"idx": take(8 * int(moff_h[-1])), "m": int(moff_h[-1])}))
                else:
                    V = int(vptr_h[-1])
                    lay.append((t, d, {"rows": (take(8 * V), take(8 * V)), "mask": (take(8 * V), take(8 * V)),
                                       "edges": (take(16 * max(E, 1)), take(16 * max(E, 1))), "common": (take(8 * V), take(8 * V)),
                                       "counts": take(20 * G), "totals": take(32), "V": V, "E": E, "vptr": vptr_h}))
        nlay = []                                   # link-prediction negatives on the device: one job per domain whose graphs fit the kernel
        if self.device_negatives and "link_pred" in self.tasks:
            from .ops import NEG_MAX_GRAPH_NODES, negative_capacity
            for d in self.domains:
                hb = inp.host[d]
                if hb.num_graphs == 0:
                    continue
                meta = hb._cache.get("neg_meta")              # (largest graph, capacity): functions of the batch alone
                if meta is None:
                    nmax = max(int(b - a) for a, b in zip(hb.ptr_host[:-1], hb.ptr_host[1:]))
                    meta = hb._cache["neg_meta"] = (nmax, negative_capacity(hb.ptr_host, hb.num_edges) if nmax <= NEG_MAX_GRAPH_NODES else 0)
                if meta[0] > NEG_MAX_GRAPH_NODES:
                    continue                        # a graph over the kernel's limit: this domain's negatives stay on the host
                cap = max(meta[1], 1)
                nlay.append(("link_pred", d, {"neg": take(16 * cap), "cap": cap, "counts": take(4 * hb.num_graphs), "total": take(16), "nmax": meta[0]}))
        total = max(off, 16)
        slot_id = k % self.DRAW_SLOTS
        slot = self._draw_slots[slot_id]
        if slot is None or slot["dev"].numel() < total:
            cap = max(total * 2, 1 << 20)
            self._bury(slot)
            slot = self._draw_slots[slot_id] = {"dev": torch.empty(cap, dtype=torch.uint8, device=self.device),
                                                "pin": torch.empty(cap, dtype=torch.uint8).pin_memory(),
                                                "flag": torch.zeros(4, dtype=torch.int32).pin_memory()}
        lib, aux = self.lib, self.aux_stream.cuda_stream
        base = slot["dev"].data_ptr()
        seed = (self.seed * 1000003 + 0x5bd1e995 * (seq + 1) + (0 if mode else 0x9E3779B97F4A7C15)) & (2 ** 64 - 1)
        # every (task, domain) job of the step in three launches (masks | views | emit): on the aux stream beside a running step the
        # twenty per-job launches cost that step 0.3 ms
        mjobs, vjobs, nmax_all, emax_all, ws_need = [], [], 1, 0, 0
        for (t, d, o) in lay:
            hb = inp.host[d]
            nmax_all = max(nmax_all, max(int(b - a) for a, b in zip(hb.ptr_host[:-1], hb.ptr_host[1:])))
            if t != "node_feat_mask":
                emax_all = max([emax_all] + [int(b - a) for a, b in zip(hb.edge_ptr_host[:-1], hb.edge_ptr_host[1:])])
                o["ws_off"], o["ws_bytes"] = ws_need, (lib.gmp_aug_workspace_bytes(hb.num_nodes, o["E"], hb.num_graphs) + 255) // 256 * 256
                ws_need += o["ws_bytes"]
        neg_nmax = max([1] + [o["nmax"] for (_, _, o) in nlay])
        for (_, d, o) in nlay:
            o["ws_off"], o["ws_bytes"] = ws_need, (lib.gmp_aug_negative_edges_workspace_bytes(inp.host[d].num_nodes, neg_nmax, o["cap"]) + 255) // 256 * 256
            ws_need += o["ws_bytes"]
        if ws_need and (self._draw_ws is None or self._draw_ws.numel() < ws_need):
            # (kernels of earlier tickets may still be using the old one on the aux stream: keep it alive.  One region per JOB -- the
            # jobs of a ticket run concurrently; tickets follow each other on the aux stream and share the regions)
            self._bury(self._draw_ws)
            self._draw_ws = torch.empty(max(2 * ws_need, 4 * lib.gmp_aug_workspace_bytes(self.max_rows, self.max_edges, 1024)),
                                        dtype=torch.uint8, device=self.device)
        ws_base = self._draw_ws.data_ptr() if ws_need else 0
        for (t, d, o) in lay:
            ptr, eptr, ei, vptr, optr, _, _ = inp.dev_graph(d)
            hb = inp.host[d]
            sid = 16 * self.tasks.index(t) + 2 * self.domains.index(d) * len(self.tasks) * 16
            if t == "node_feat_mask":
                if o["m"]:
                    mjobs.append(L.AugMasksJob(ptr.data_ptr(), optr.data_ptr(), hb.num_graphs, sid, base + o["idx"]))
            else:
                vjobs.append(L.AugViewsJob(ptr.data_ptr(), eptr.data_ptr(), ei.data_ptr(), hb.num_nodes, o["E"], vptr.data_ptr(), hb.num_graphs,
                                           int(hb.x.size(1)), sid, base + o["rows"][0], base + o["rows"][1], base + o["mask"][0], base + o["mask"][1],
                                           base + o["edges"][0], base + o["edges"][1], max(o["E"], 1), base + o["common"][0], base + o["common"][1],
                                           base + o["counts"], base + o["totals"], ws_base + o["ws_off"], o["ws_bytes"]))
        if mjobs:
            self._chk(lib.gmp_aug_node_masks_batch((L.AugMasksJob * len(mjobs))(*mjobs), len(mjobs), nmax_all, seed, aux), "aug_node_masks_batch")
        if vjobs:
            self._chk(lib.gmp_aug_two_views_batch((L.AugViewsJob * len(vjobs))(*vjobs), len(vjobs), nmax_all, emax_all, seed, aux), "aug_two_views_batch")
        if nlay:
            njobs = []
            for (t, d, o) in nlay:
                ptr, eptr, ei, _, _, _, _ = inp.dev_graph(d)
                hb = inp.host[d]
                sid = 16 * self.tasks.index(t) + 2 * self.domains.index(d) * len(self.tasks) * 16
                njobs.append(L.AugNegJob(ptr.data_ptr(), eptr.data_ptr(), ei.data_ptr() if hb.num_edges else None, hb.num_nodes, hb.num_edges,
                                         hb.num_graphs, sid, hb.num_edges, base + o["neg"], o["cap"], base + o["counts"], base + o["total"],
                                         ws_base + o["ws_off"], o["ws_bytes"]))
            self._chk(lib.gmp_aug_negative_edges_batch((L.AugNegJob * len(njobs))(*njobs), len(njobs), neg_nmax, seed, aux), "aug_negative_edges_batch")
        src = (C.c_void_p * 1)(base)
        dst = (C.c_void_p * 1)(slot["pin"].data_ptr())
        self._chk(lib.gmp_upload(1, src, dst, (C.c_int64 * 1)((total + 15) // 16 * 16), aux), "draw results -> pinned host")
        self._chk(lib.gmp_gate_open(slot["flag"].data_ptr(), k + 1, aux), "draw flag")
        return DrawTicket(slot, lay + nlay, k + 1)

    def _bury(self, obj=None) -> None:
        """Outgrown draw slots / workspaces may still be in use by tickets already on the aux stream: each is kept with an event recorded
        there and dropped once the stream has passed it (they used to live as long as the engine)."""
        if obj is not None:
            ev = torch.cuda.Event()
            ev.record(self.aux_stream)
            self._draw_graveyard.append((obj, ev))
        self._draw_graveyard = [(o, e) for o, e in self._draw_graveyard if not e.query()]

    def collect_draws(self, inp: StepInputs, ticket: "DrawTicket") -> Dict[str, object]:
        """Wait for a ticket's flag (a word in pinned host memory the GPU sets behind its copy: no HIP call, no stream sync) and wrap
        the slot's arrays as the step's artefacts.  Link-prediction negatives come from the host sampler (mostly "every non-edge", no draw)
        unless the engine was built with device_negatives: then the ticket carries them too, and only a domain batch with a graph over the
        kernel's 1,024-node limit still asks the host."""
        flag = ticket.slot["flag"].numpy()
        t_end = _t.time() + 120.0
        while int(flag[0]) < ticket.epoch:
            if _t.time() > t_end:
                raise L.GnnmpError("engine: device draws did not arrive within two minutes")
            _t.sleep(2e-5)
        buf = ticket.slot["pin"].numpy()
        art: Dict[str, object] = {}
        for t in self.tasks:
            if t == "link_pred":
                on_ticket = {d for (tt, d, _) in ticket.layout if tt == "link_pred"}
                art[t] = {d: (None if d in on_ticket else _EMPTY_ART[t]() if not inp.host[d].num_graphs else self._negatives(inp.host[d]))
                          for d in self.domains}
            elif t in ("node_feat_mask", "node_contrast", "graph_contrast"):
                art[t] = {d: _EMPTY_ART[t]() for d in self.domains}        # domains without a drawn piece (no graphs / too few)
        for (t, d, o) in ticket.layout:
            if t == "node_feat_mask":
                art[t][d] = buf[o["idx"]:o["idx"] + 8 * o["m"]].view(np.int64).copy()
            elif t == "link_pred":
                k = int(buf[o["total"]:o["total"] + 4].view(np.int32)[0])
                art[t][d] = buf[o["neg"]:o["neg"] + 16 * o["cap"]].view(np.int64).reshape(2, -1)[:, :k].copy()
            else:
                tot = buf[o["totals"]:o["totals"] + 20].view(np.int32)
                views = []
                for v in range(2):
                    V, e = o["V"], int(tot[v])
                    rows = buf[o["rows"][v]:o["rows"][v] + 8 * V].view(np.int64).copy()
                    ed = buf[o["edges"][v]:o["edges"][v] + 16 * max(o["E"], 1)].view(np.int64).reshape(2, -1)[:, :e].copy()
                    rm = buf[o["mask"][v]:o["mask"][v] + 8 * V].view(np.uint64).copy() if tot[3 + v] else None
                    cm = buf[o["common"][v]:o["common"][v] + 8 * int(tot[2])].view(np.int64).copy()
                    views.append(ViewArrays(rows, ed, o["vptr"], rm, cm))
                art[t][d] = (views[0], views[1])
        return art

    # ------------------------------------------------------------------ one step
    def prepare(self, inp: StepInputs, gen: torch.Generator, ticket: Optional[DrawTicket] = None):
        """Host half of a step (all RNG draws + the segment layout); may run on another thread ahead of time.  `ticket`: the
        device-side draws of this input, enqueued earlier (rng_mode 'device'; StepPrefetcher keeps a few inputs' tickets in flight)."""
        art = self.collect_draws(inp, ticket) if ticket is not None else self.draw(inp, gen)
        return art, self.plan(inp, art)

    def step(self, inp: StepInputs, gen: torch.Generator, art: Optional[Dict[str, object]] = None,
             order: Optional[List[str]] = None, apply_update: bool = True, prepared=None) -> None:
        """Forward, backward, PCGrad, clip, AdamW for one step.  Nothing is read back: losses stay in
        self.loss_sums / self.plan_sizes until someone asks (losses())."""
        main_h = torch.cuda.current_stream(self.device).cuda_stream
        if self.rng_mode == "device":
            # Device draws ride the aux stream, i.e. they run behind whatever the launcher has already enqueued there: the launcher
            # therefore keeps at most two steps in front of the GPU (enough to keep it fed: enqueueing a step takes half a step), so a
            # ticket is served within two steps and the prefetcher's three tickets in flight cover it
            ev = self._lead.pop(self.step_count - int(os.environ.get("GMP_DEVICE_LEAD", "2")), None)
            if ev is not None:
                ev.synchronize()
        t0 = _t.perf_counter()
        if prepared is not None:
            art, p = prepared
            t1 = t2 = _t.perf_counter()
        else:
            if art is None:
                art = self.draw(inp, gen)
            t1 = _t.perf_counter()
            p = self.plan(inp, art)
            t2 = _t.perf_counter()
        self._upload(p, inp, art)
        t3 = _t.perf_counter()
        if self.native:
            self._forward_backward_native(p, inp)        # one C call enqueues the whole forward/heads/backward
        else:
            self.sequence().run(p, inp)                  # the same launches one by one (step_sequence.py)
        self._optimizer(p, order, apply_update, main_h)
        t4 = _t.perf_counter()
        h = self.host_ms
        h["draw"] += (t1 - t0) * 1e3; h["plan"] += (t2 - t1) * 1e3; h["upload"] += (t3 - t2) * 1e3; h["launch"] += (t4 - t3) * 1e3
        h["steps"] += 1
        if self.rng_mode == "device":
            e = torch.cuda.Event()
            e.record(torch.cuda.current_stream(self.device))
            self._lead[self.step_count] = e
        self.step_count += 1
        self.last_plan, self.last_inputs = p, inp
        if self.model.training:                      # BatchNorm call counters (one per forward() the reference would have made)
            lens = np.diff(p.a32["seg_ptr"])
            dom = p.a32["seg_dom"]
            self._bn_calls += int((lens > 0).sum())
            for di in range(self.D):
                self._bn_calls_dom[di] += int(((lens > 0) & (dom == di)).sum())

    def sequence(self):
        """The Python launch sequence over this engine's arena (native=False; scripts time its forward)."""
        if self._sequence is None:
            from .step_sequence import LaunchSequence
            self._sequence = LaunchSequence(self)
        return self._sequence

    @property
    def dropout_seed(self) -> int:
        """Seed of every dropout mask of the step about to run: both executors draw the same masks from it."""
        return (self.seed * 1000003 + self.step_count) & (2 ** 64 - 1)

    def flush_counters(self) -> None:
        """Bring every BatchNorm's num_batches_tracked up to date (it only matters for the saved state_dict -- momentum is
        fixed -- so the engine counts calls on the host and writes them when asked: pretrain() does before a checkpoint)."""
        if self._bn_calls:
            for l in self.model.gnn_backbone.layers:
                l.batch_norm.num_batches_tracked += self._bn_calls
                l.gin_conv.nn[1].num_batches_tracked += self._bn_calls
            self._bn_calls = 0
        for di, d in enumerate(self.domains):
            if self._bn_calls_dom[di]:
                self.model.input_encoders[d].batch_norm.num_batches_tracked += self._bn_calls_dom[di]
                self._bn_calls_dom[di] = 0

    # ---- upload ------------------------------------------------------------------------------------
    def _upload(self, p: StepPlan, inp: StepInputs, art) -> None:
        slot = self.stage[self.step_count % self.STAGES]
        if slot["event"] is not None:
            slot["event"].synchronize()                  # the copy that read this slot STAGES steps ago is done
        # device scalars (scal: [0:8) 1/size per task, [16:48) per-domain NT-Xent sums), LP labels and the index arrays of THIS step
        self.dev32, self.dev64, self.scal, self.lp_lab = self._up_sets[self.step_count & 1]
        on_aux = self.upload_on_aux
        up_stream = self.aux_stream if on_aux else torch.cuda.current_stream(self.device)
        pin32, pin64, pinf = slot["pin32"], slot["pin64"], slot["pinf"]
        o32, o64, lay32, lay64 = p.cat32.size, p.cat64.size, p.lay32, p.lay64
        pin32.numpy()[:o32] = p.cat32
        pin64.numpy()[:o64] = p.cat64
        nf = pinf.numpy()
        nf[:64] = 0.0
        for ti, t in enumerate(self.tasks):
            nf[ti] = 1.0 / max(p.sizes[t], 1)            # [0:8) = 1/size per task, [16:48) = per-domain NT-Xent sums (zeroed)
        nlab = 0
        if "link_pred" in self.tasks:
            nf[64:64 + p.lp_K] = p.lp_labels
            nlab = (p.lp_K + 3) // 4 * 4
        # one kernel reads the four pinned pieces over PCIe (gmp_upload) instead of four hand-overs to the copy engine
        src = (C.c_void_p * 4)(pin32.data_ptr(), pin64.data_ptr(), pinf.data_ptr(), pinf.data_ptr() + 256)
        dst = (C.c_void_p * 4)(self.dev32.data_ptr(), self.dev64.data_ptr(), self.scal.data_ptr(), self.lp_lab.data_ptr())
        nbytes = (C.c_int64 * 4)(4 * o32, 8 * o64, 256, 4 * nlab)
        self._chk(self.lib.gmp_upload(4, src, dst, nbytes, up_stream.cuda_stream), "gmp_upload")
        ev = torch.cuda.Event()
        ev.record(up_stream)
        slot["event"] = ev
        b32, b64 = self.dev32.data_ptr(), self.dev64.data_ptr()
        p.d32 = {k: b32 + 4 * o for k, o in lay32.items()}
        p.d64 = {k: b64 + 8 * o for k, o in lay64.items()}
        # per-step gradient-availability table (static unless a (task, domain) pair dropped out)
        if p.skipped:
            has = self.has_static.copy()
            for ti, d in p.skipped:
                t = self.tasks[ti]
                k = [self.name_index[n] for n in self.names if n.startswith(f"heads.{t}.{d}.")]
                has[k, ti] = 0
            self.has.copy_(torch.from_numpy(has).to(self.device))
            self._has_dirty = True
        elif self._has_dirty:
            self.has.copy_(torch.from_numpy(self.has_static).to(self.device))
            self._has_dirty = False

    # ---- what both executors read: error check, addresses in the arena, plan helpers (more beside _fill_desc) ------------
    def _chk(self, rc: int, what: str) -> None:
        if rc:
            L.check(rc, what)

    def _P(self, name: str) -> int:
        v = self._p_cache.get(name)
        if v is None:
            v = self._p_cache[name] = self.flat.data_ptr() + 4 * self.off[name]
        return v

    def _TG(self, t: int, name: str) -> int:
        """Float offset of (task t, tensor) inside the [T, P] per-task gradient buffer."""
        return t * self.P + self.off[name]

    def head_offsets(self, ti: int, prefix: str):
        """(field suffix, offset in flat, offset in task_grads) of the four tensors of the two-layer head `prefix`"""
        return [(a, self.off[prefix + n], self._TG(ti, prefix + n))
                for a, n in (("w0", "mlp.0.weight"), ("b0", "mlp.0.bias"), ("w3", "mlp.3.weight"), ("b3", "mlp.3.bias"))]

    @staticmethod
    def _lp_segmented(p: StepPlan) -> bool:
        return p.lp_S > 0 and p.lp_max_rows <= SEG_CSR_MAX_ROWS and p.lp_max_edges <= SEG_CSR_MAX_EDGES

    def _ntx_workspace(self, slot0: int, ns) -> Tensor:
        """One grouped workspace per contrastive task (slot0 = 0 node level, D graph level), grown on demand."""
        need = self.lib.gmp_nt_xent_grouped_workspace_bytes(len(ns), max(max(ns), 1), 128)
        if need > self.ntx_ws[slot0].numel():
            self.ntx_ws[slot0] = torch.empty(need, dtype=torch.uint8, device=self.device)
        return self.ntx_ws[slot0]

    # ---- optimizer ---------------------------------------------------------------------------------
    def _optimizer(self, p: StepPlan, order: Optional[List[str]], apply_update: bool, main_h: int) -> None:
        """PCGrad, clip and AdamW behind the step's backward; main_h: the main stream's handle (hipStream_t)."""
        names = list(self.tasks)
        main_tasks = [t for t in names if t != "domain_adv"]     # pretrain.py:137-150: PCGrad over the main tasks, then
        extra = names.index("domain_adv") if "domain_adv" in names else -1   # domain_adv_loss.backward() accumulates on top
        rule, model_scope = L.SURGERY_RULES[self.surgery], self.surgery == "pcgrad" and self.surgery_scope == "model"
        perm = None
        if self.surgery == "reference":
            if order is None:
                order = list(main_tasks)
                if len(order) > 1:
                    (self.shuffle_rng or random).shuffle(order)       # reference: unseeded random.shuffle (gradient_surgery.py:43)
        else:
            # the other rules have no first-shuffled task: the order is the dict order (whatever `order` says), and PCGrad as published
            # draws, for each task in turn, the order in which it meets the others -- positions of `order`
            order = list(main_tasks)
            if self.surgery == "pcgrad":
                perm = []
                for i in range(len(order)):
                    row = [j for j in range(len(order)) if j != i]
                    (self.shuffle_rng or random).shuffle(row)
                    perm.append(row)
        idx = [names.index(t) for t in order]
        self.last_order, self.last_perm = order, perm
        oidx = _i32(idx)
        pidx = _i32([j for row in perm for j in row]) if perm and len(order) > 1 else None
        gram_only, all_tensors = (8, 16) if model_scope else (1, 0)     # model scope: Gram per part, one fold + solve + combine at the end

        def pcgrad(k0: int, k1: int, phases: int, stream: int) -> None:
            args = (self.task_grads.data_ptr(), self.P, self.T, self.K, self.t_off.data_ptr(), self.t_len.data_ptr(), self.has.data_ptr(),
                    oidx, len(idx), names.index(main_tasks[-1]), extra, self.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                    self.steps.data_ptr() if apply_update else None, self.lr.data_ptr(), self.wd.data_ptr(), 0.9, 0.999, 1e-8, self.max_grad_norm,
                    self.final_grad.data_ptr(), self.normsq.data_ptr(), self.metrics.data_ptr(), self.flags.data_ptr(), self.mt_ws.data_ptr(),
                    self.mt_ws.numel(), int(apply_update), k0, k1, phases,
                    (self.sync_flags.data_ptr() + 4 * 63) if self.use_gates else None,      # a timed-out gate: no update from this step on
                    stream)
            if rule == 0:
                self._chk(self.lib.gmp_mt_pcgrad_clip_adamw_ex(*args), "mt_pcgrad_clip_adamw")
            else:
                self._chk(self.lib.gmp_mt_surgery_clip_adamw(rule, L.SURGERY_SCOPES[self.surgery_scope], pidx, *args), "mt_surgery_clip_adamw")

        if self.grad_sync is not None and self.dp_mode == "sharded" and self.native:
            from . import dist as D
            if D.world_size() > 1:
                sync = self._shard_sync()
                sync.average_(self.lib, torch.cuda.current_stream(self.device),
                              gate=(self.sync_flags.data_ptr(), self._epoch) if self.use_gates else None,
                              own_pass=lambda a, b, st: pcgrad(a, b, 1, st), foreign_pass=lambda a, b, st: pcgrad(a, b, 4, st))
                pcgrad(0, self.K, 2, main_h)
                return
        if self.parts_beside_backward:
            # PCGrad follows the backward part by part on the exchange stream (Gram / solve / combine of a part as soon as its
            # gradients are final -- and, data parallel, averaged); only the total norm, the clip and AdamW wait for the last part
            sync = self._part_sync()
            k_of = self._part_tensors
            sync.average_(self.lib, torch.cuda.current_stream(self.device), gate=(self.sync_flags.data_ptr(), self._epoch),
                          exchange=self.grad_sync is not None,
                          after_message=lambda parts, st: [pcgrad(a, b, gram_only, st) for a, b in _merge_runs([k_of[q] for q in parts])])
            pcgrad(0, self.K, all_tensors | 2, main_h)
            return
        if self.grad_sync is not None:
            self._sync_task_grads()
        pcgrad(0, self.K, gram_only | all_tensors | 2, main_h)

    def _head_slices(self):
        out = []
        for k, n in enumerate(self.names):
            if n.startswith("heads."):
                t = int(np.argmax(self.has_static[k]))
                out.append((t * self.P + self.off[n], -(-self.numel[n] // 4) * 4))       # tensors are 4-float aligned
        return out

    def _part_sync(self):
        """The per-task gradient matrix cut into the parts the step finishes one after the other (gmp_step_wait_grads): part 0
        the task heads, part 1 + k backbone layer L-1-k, last part mask token + encoders -- as message slices for the exchange
        (dist.OverlappedGradSync) and as tensor-index ranges for PCGrad (self._part_tensors)."""
        if self._packed_sync is None:
            from .dist import OverlappedGradSync
            ranges: List[List[List[int]]] = [[] for _ in range(GNN_NUM_LAYERS + 2)]
            krange: List[List[int]] = [[self.K, 0] for _ in range(GNN_NUM_LAYERS + 2)]
            shared = [n for n in self.names if self.off[n] < self.P_shared]
            for i, n in enumerate(shared):
                part = GNN_NUM_LAYERS + 1
                if n.startswith("gnn_backbone.layers."):
                    part = GNN_NUM_LAYERS - int(n.split(".")[2])
                end = self.off[shared[i + 1]] if i + 1 < len(shared) else self.P_shared
                r = ranges[part]
                if r and r[-1][1] == self.off[n]:
                    r[-1][1] = end                                   # contiguous with the previous tensor of this part
                else:
                    r.append([self.off[n], end])
                k = self.name_index[n]
                krange[part] = [min(krange[part][0], k), max(krange[part][1], k + 1)]
            hk = [k for k, n in enumerate(self.names) if n.startswith("heads.")]
            krange[0] = [min(hk), max(hk) + 1] if hk else [0, 0]
            for b, (k0, k1) in enumerate(krange):                    # every part must be one run of tensor indices
                if k1 > k0 and sorted(self._part_of(n) for n in self.names[k0:k1]) != [b] * (k1 - k0):
                    raise L.GnnmpError("engine: the tensors of a backward part are not contiguous in the flat layout")
            self._part_tensors = [(k0, k1) if k1 > k0 else (0, 0) for k0, k1 in krange]
            parts = [self._head_slices()] + [[(t * self.P + lo, hi - lo) for t in range(self.T) for lo, hi in ranges[b]]
                                             for b in range(1, GNN_NUM_LAYERS + 2)]
            self._packed_sync = OverlappedGradSync(self.task_grads.view(-1), parts, self.comm_stream)
        return self._packed_sync

    def _shard_sync(self):
        """dist.ShardedGradSync over the same parts as _part_sync: tensor k's message slices = one copy per task that has it (static table),
        its combined gradient = its slot of final_grad."""
        if self._shard_sync_obj is None:
            from .dist import ShardedGradSync
            self._part_sync()                                  # builds self._part_tensors (and checks the parts are runs of tensor indices)
            al4 = lambda v: -(-v // 4) * 4

            def msg(k: int):
                n = self.names[k]
                return [(t * self.P + self.off[n], al4(self.numel[n])) for t in range(self.T) if self.has_static[k][t]]

            fin = lambda k: (self.off[self.names[k]], al4(self.numel[self.names[k]]))
            self._shard_sync_obj = ShardedGradSync(self.task_grads.view(-1), self.final_grad, self._part_tensors, msg, fin, self.comm_stream)
        return self._shard_sync_obj

    @staticmethod
    def _part_of(name: str) -> int:
        if name.startswith("heads."):
            return 0
        if name.startswith("gnn_backbone.layers."):
            return GNN_NUM_LAYERS - int(name.split(".")[2])
        return GNN_NUM_LAYERS + 1

    def _sync_task_grads(self) -> None:
        """Data parallel: average the per-task gradients over ranks BEFORE PCGrad -- shared tensors once per task,
        every head once (only its own task's row is meaningful).  Native executor: in parts beside the backward
        (dist.OverlappedGradSync; GMP_DP_OVERLAP=0 falls back to one flat all-reduce after it)."""
        head_slices = self._head_slices() if self._packed_sync is None else []
        if self.native and os.environ.get("GMP_DP_OVERLAP", "1") != "0":
            self._part_sync().average_(self.lib, torch.cuda.current_stream(self.device),
                                       gate=(self.sync_flags.data_ptr(), self._epoch) if self.use_gates else None)
            return
        if self._packed_sync is None:
            from .dist import PackedGradSync
            slices = [(t * self.P, self.P_shared) for t in range(self.T)] + head_slices
            self._packed_sync = PackedGradSync(self.task_grads.view(-1), slices)
        self._packed_sync.average_()

    # ---- reporting (the only host syncs, and only on request) ---------------------------------------
    def check_gates(self) -> None:
        """A gate that timed out let its stream run ahead of a dependency: results since then are not to be trusted."""
        if self.use_gates and int(self.sync_flags[63].item()) != 0:
            raise L.GnnmpError("engine: a cross-stream gate timed out (streams sharing a hardware queue, or a tool serialising "
                               "kernels?) -- rerun with GMP_STEP_GATES=0")

    def verify_gates(self, inp: "StepInputs", steps: int = 2, timeout_s: float = 5.0) -> bool:
        """Start-up self-check of the gates in the process as it now is (call it AFTER the process group exists: a communicator
        brings streams and queues of its own, and the stream -> hardware-queue calibration this engine was built on predates
        nothing it has not seen).  `steps` probe steps run from the current state with gates (short time-out), then -- from the
        same state, with the same draws and dropout seeds -- with events; gates stay on only when no gate timed out and
        parameters, per-task gradients, losses and running statistics are bitwise equal, on EVERY rank.  The engine's state is
        restored afterwards.  Collective: all ranks of a data-parallel job must call it together."""
        if not self.use_gates:
            return False
        import torch.distributed as tdist
        dev = self.device
        bufs = [self.flat, self.exp_avg, self.exp_avg_sq, self.steps, self.enc_rm, self.enc_rv, self.loss_sums]
        bufs += [b for n, b in self.model.named_buffers() if "running_" in n and not n.startswith("input_encoders.")]
        saved = [b.clone() for b in bufs]
        host_state = (self.step_count, self._bn_calls, list(self._bn_calls_dom), self._nprng, dict(self.host_ms))
        # the link-prediction negatives draw from a stream of their own (neg_rng / its native twin): both passes must see the same one
        neg_state = self.sync_neg_rng().getstate()
        seq_state = dict(self._draw_seq)

        def rewind_negatives() -> None:
            self._draw_seq = dict(seq_state)               # device draws: both passes (and the run after them) see the same sequence
            self.neg_rng.setstate(neg_state)
            self._neg_native = None                      # the native twin is re-created from neg_rng at its next use
        tasks = [t for t in self.tasks if t != "domain_adv"]
        self._chk(self.lib.gmp_gate_set_timeout(float(timeout_s)), "gate_set_timeout")
        outs, timed_out = [], False
        try:
            for gates in (True, False):
                self.use_gates = gates
                for b, s in zip(bufs, saved):
                    b.copy_(s)
                self.step_count = host_state[0]
                self._nprng = None
                rewind_negatives()
                g = torch.Generator().manual_seed(12345)
                for _ in range(steps):
                    self.step(inp, g, order=tasks)
                torch.cuda.synchronize(dev)
                if gates:
                    timed_out = int(self.sync_flags[63].item()) != 0
                    self.sync_flags[63] = 0
                outs.append([self.flat.clone(), self.task_grads.clone(), self.loss_sums.clone()] + [b.clone() for b in bufs[4:]])
        finally:
            for b, s in zip(bufs, saved):
                b.copy_(s)
            self.step_count, self._bn_calls, self._bn_calls_dom, self._nprng = host_state[0], host_state[1], host_state[2], host_state[3]
            rewind_negatives()
            self.host_ms.update(host_state[4])
            self._chk(self.lib.gmp_gate_set_timeout(float(os.environ.get("GMP_GATE_TIMEOUT_S", "120"))), "gate_set_timeout")
        ok = (not timed_out) and all(torch.equal(a, b) for a, b in zip(outs[0], outs[1]))
        if not ok and not timed_out:          # name what differed: a mismatch is a synchronisation bug, not a tuning matter
            labels = ["parameters", "per-task gradients", "loss sums"] + [f"buffer {i}" for i in range(len(outs[0]) - 3)]
            self.gates_mismatch = [(n, float((a.double() - b.double()).abs().max())) for n, a, b in zip(labels, outs[0], outs[1]) if not torch.equal(a, b)]
        if tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
            t = torch.tensor([1 if ok else 0], device=dev, dtype=torch.int32)
            tdist.all_reduce(t, op=tdist.ReduceOp.MIN)
            ok = bool(t.item())
        self.use_gates = ok
        self.gates_verified = {"ok": ok, "timed_out": timed_out, "steps": steps}
        if self.gates_mismatch:
            self.gates_verified["mismatch"] = self.gates_mismatch
        torch.cuda.synchronize(dev)
        return ok

    def losses(self) -> Dict[str, float]:
        self.check_gates()
        sums = self.loss_sums[:self.T].tolist()
        return {t: sums[i] / max(self.last_plan.sizes[t], 1) for i, t in enumerate(self.tasks)}

    def task_gradient(self, task: str, name: str) -> Tensor:
        t = self.tasks.index(task)
        o = self.off[name]
        return self.task_grads[t, o:o + self.numel[name]].view_as(dict(self.model.named_parameters())[name])

    def final_gradient(self, name: str) -> Tensor:
        o = self.off[name]
        return self.final_grad[o:o + self.numel[name]].view_as(dict(self.model.named_parameters())[name])

    # ---- native executor: the same sequence enqueued by one C call (csrc/step.hip) ---------------------
    def _init_desc(self):
        from ._step_desc import StepDesc, TASK_KIND
        d = StepDesc()
        D, T = self.domains, self.T
        ptr = lambda t: t.data_ptr()
        d.num_tasks, d.num_domains, d.dpad, d.hidden = T, len(D), self.dpad, H
        d.flat, d.P, d.task_grads = ptr(self.flat), self.P, ptr(self.task_grads)
        for i in range(6):
            d.csr[i], d.lp_csr[i] = ptr(self.csr[i]), ptr(self.lp_csr[i])
        d.csr_status, d.csr_ws, d.csr_ws_bytes = ptr(self.csr_status), ptr(self.csr_ws), self.csr_ws.numel()
        d.lp_csr_status, d.lp_csr_ws, d.lp_csr_ws_bytes = ptr(self.lp_csr_status), ptr(self.lp_csr_ws), self.lp_csr_ws.numel()
        for i, dom in enumerate(D):
            d.enc_off_w[i] = self.off[f"input_encoders.{dom}.linear.weight"]
            d.enc_off_b[i] = self.off[f"input_encoders.{dom}.linear.bias"]
            d.enc_d_in[i] = DOMAIN_DIMENSIONS[dom]
        d.enc_off_gamma0 = self.off[f"input_encoders.{D[0]}.batch_norm.weight"]
        d.enc_off_beta0 = self.off[f"input_encoders.{D[0]}.batch_norm.bias"]
        d.enc_rm, d.enc_rv, d.enc_mean, d.enc_rstd, d.z0 = ptr(self.enc_rm), ptr(self.enc_rv), ptr(self.enc_mean), ptr(self.enc_rstd), ptr(self.z0)
        d.nfm_task = self.tasks.index("node_feat_mask") if "node_feat_mask" in self.tasks else -1
        if d.nfm_task >= 0:
            d.off_mask_token, d.tg_mask_token = self.off["mask_token"], self._TG(d.nfm_task, "mask_token")
        for l in range(GNN_NUM_LAYERS + 1):
            d.h[l] = ptr(self.h[l])
        names = {"eps": "gin_conv.eps", "w1": "gin_conv.nn.0.weight", "b1": "gin_conv.nn.0.bias", "g1": "gin_conv.nn.1.weight",
                 "be1": "gin_conv.nn.1.bias", "w2": "gin_conv.nn.3.weight", "b2": "gin_conv.nn.3.bias", "g2": "batch_norm.weight", "be2": "batch_norm.bias"}
        for l in range(GNN_NUM_LAYERS):
            Ld, pre, layer = d.layer[l], f"gnn_backbone.layers.{l}.", self.model.gnn_backbone.layers[l]
            for k, n in names.items():
                setattr(Ld, "off_" + k, self.off[pre + n])
                arr = getattr(Ld, "tg_" + k)
                for t in range(T):
                    arr[t] = self._TG(t, pre + n)
            bn1, bn2 = layer.gin_conv.nn[1], layer.batch_norm
            Ld.rm1, Ld.rv1, Ld.rm2, Ld.rv2 = ptr(bn1.running_mean), ptr(bn1.running_var), ptr(bn2.running_mean), ptr(bn2.running_var)
            Ld.a, Ld.z1, Ld.r1, Ld.z2 = ptr(self.a[l]), ptr(self.z1[l]), ptr(self.r1[l]), ptr(self.z2[l])
            Ld.m1, Ld.s1, Ld.m2, Ld.s2 = ptr(self.stat["m1"][l]), ptr(self.stat["s1"][l]), ptr(self.stat["m2"][l]), ptr(self.stat["s2"][l])
        d.gA, d.gB, d.gW, d.rowdot, d.ga = ptr(self.gA), ptr(self.gB), ptr(self.gW), ptr(self.rowdot), ptr(self.ga)
        for l in range(GNN_NUM_LAYERS):
            d.gu_l[l], d.gz1_l[l] = ptr(self.gu_l[l]), ptr(self.gz1_l[l])
        d.bn_ws, d.bn_ws_bytes = ptr(self.bn_ws), self.bn_ws.numel()
        d.gemm_ws, d.gemm_ws_bytes = ptr(self.gemm_ws), self.gemm_ws.numel()
        hd = self.hd
        mlp_cfg = {"node_feat_mask": (H, H, H, "nfm_in", "nfm_y1", "nfm_d1", "nfm_y2", "nfm_g", "nfm_g1", "nfm_gin"),   # (y2 is read again by the deferred loss sum)
                   "node_contrast": (H, H, 128, "nc_in", "nc_y1", "nc_d1", "nc_z", "nc_gz", "nc_g1", "nc_gin"),
                   "graph_contrast": (2 * H, H, 128, "gc_in", "gc_y1", "gc_d1", "gc_z", "gc_gz", "gc_g1", "gc_gin"),
                   "graph_prop": (H, 2 * H, GRAPH_PROPERTY_DIM, "gp_in", "gp_y1", "gp_d1", None, None, "gp_g1", "gp_gin")}
        sc = ptr(self.scal)

        for ti, t in enumerate(self.tasks):
            td = d.task[ti]
            td.kind = TASK_KIND[t]
            td.g_scale, td.loss_sum = sc + 4 * ti, ptr(self.loss_sums) + 4 * ti
            td.gemm_ws, td.gemm_ws_bytes = ptr(self.task_gemm_ws[ti]), self.task_gemm_ws[ti].numel()
            td.loss_ws, td.loss_ws_bytes = ptr(self.task_loss_ws[ti]), self.task_loss_ws[ti].numel()
            if t in mlp_cfg:
                k_in, k_hid, k_out, x, y1, d1, y2, g_out, g_hid, g_in = mlp_cfg[t]
                m = td.mlp
                m.k_in, m.k_hid, m.k_out, m.site = k_in, k_hid, k_out, 100 + ti
                for i, dom in enumerate(D):
                    for a, off, tg in self.head_offsets(ti, f"heads.{t}.{dom}."):
                        getattr(m, "off_" + a)[i], getattr(m, "tg_" + a)[i] = off, tg
                m.x, m.y1, m.d1, m.g_hid, m.g_in = ptr(hd[x]), ptr(hd[y1]), ptr(hd[d1]), ptr(hd[g_hid]), ptr(hd[g_in])
                m.y2 = ptr(self.gp_y2) if t == "graph_prop" else ptr(hd[y2])
                m.g_out = ptr(self.gp_g2) if t == "graph_prop" else ptr(hd[g_out])
            if t == "node_feat_mask":
                td.nfm_target = ptr(hd["nfm_tgt"])
            if t in ("node_contrast", "graph_contrast"):
                td.ntx_sums = sc + 4 * (16 + (0 if t == "node_contrast" else self.D))
            if t == "graph_contrast":
                td.pool_mean, td.pool_max, td.g_mean, td.g_max = ptr(hd["gc_mean"]), ptr(hd["gc_max"]), ptr(hd["gc_gmean"]), ptr(hd["gc_gmax"])
            if t == "domain_adv":
                m = td.mlp
                m.x, m.y1, m.d1, m.y2, m.g_out, m.g_hid, m.g_in = (ptr(hd[k]) for k in ("da_in", "da_y1", "da_d1", "da_logits", "da_glogits", "da_g1", "da_gin"))
                td.da_classes, td.da_hidden, td.da_dropout = len(D), DA_HIDDEN, DA_DROPOUT
            if t == "link_pred":
                td.lp_labels = ptr(self.lp_lab)
                for a in ("feat", "y1", "d1", "gy1", "gfeat", "ghs", "ghd"):
                    setattr(td, "lp_" + a, ptr(hd["lp_" + a]))
                td.lp_y2, td.lp_p, td.lp_gy2 = ptr(self.lp_y2), ptr(self.lp_p), ptr(self.lp_gy2)
            if t in ("domain_adv", "link_pred"):      # one head shared by all domains
                for a, off, tg in self.head_offsets(ti, "heads.domain_adv.classifier." if t == "domain_adv" else "heads.link_pred.predictor."):
                    setattr(td, "one_off_" + a, off)
                    setattr(td, "one_tg_" + a, tg)
                td.one_site = 100 + ti
        self._desc = d
        main_h = torch.cuda.current_stream(self.device).cuda_stream
        self._stream_arr = (C.c_void_p * self.T)(*[(s.cuda_stream if s is not None else main_h) for s in self.task_streams])
        return d

    def _fill_desc(self, p: StepPlan, inp: StepInputs):
        d = self._desc or self._init_desc()
        D = self.domains
        d.N, d.E, d.S, d.max_seg, d.num_tiles = p.N, p.E, p.S, p.max_seg, p.num_tiles
        d.max_seg_edges, d.seg_eptr = p.max_seg_edges, p.d32["seg_eptr"]
        for k in range(2):
            d.fwd_cut_seg[k], d.fwd_cut_row[k] = p.fwd_cuts[k] if k < len(p.fwd_cuts) else (0, 0)
        d.training, d.dropout_p = int(self.model.training), float(self.dropout_p)
        d.dp_exchange = int(self.grad_sync is not None or self.parts_beside_backward)     # publish when each part's gradients are final
        d.upload_on_aux = int(self.upload_on_aux)
        sc = self.scal.data_ptr()                    # this step's upload set
        for ti, t in enumerate(self.tasks):
            td = d.task[ti]
            td.g_scale = sc + 4 * ti
            if t in ("node_contrast", "graph_contrast"):
                td.ntx_sums = sc + 4 * (16 + (0 if t == "node_contrast" else self.D))
            if t == "link_pred":
                td.lp_labels = self.lp_lab.data_ptr()
        self._epoch += 1
        d.epoch, d.sync_flags = self._epoch, (self.sync_flags.data_ptr() if self.use_gates else None)
        d.seed = self.dropout_seed
        d.seg_ptr, d.seg_dom, d.src_row, d.tiles = p.d32["seg_ptr"], p.d32["seg_dom"], p.d32["src_row"], p.d32["tiles"]
        d.edge_index, d.rowmask = p.d64["edge_index"], p.d64.get("rowmask")
        for i, v in enumerate(p.task_row):
            d.task_row[i] = v
        for i, v in enumerate(self._task_segments(p)):
            d.task_seg[i] = v
        d.x_all, d.x_rows = inp.x_all.data_ptr(), inp.x_all.size(0)
        groups = self._encoder_groups(p)
        d.enc_groups = len(groups)
        if groups:
            d.enc_gseg[0] = groups[0][2]
            for g, (ti, dom, lo, hi) in enumerate(groups):
                d.enc_gseg[g + 1] = hi
                d.enc_tg_w[g], d.enc_tg_b[g] = self._TG(ti, f"input_encoders.{dom}.linear.weight"), self._TG(ti, f"input_encoders.{dom}.linear.bias")
                d.enc_tg_gamma[g], d.enc_tg_beta[g] = self._TG(ti, f"input_encoders.{dom}.batch_norm.weight"), self._TG(ti, f"input_encoders.{dom}.batch_norm.bias")
        T_ = float(self.temperature)
        for ti, t in enumerate(self.tasks):
            td = d.task[ti]
            td.row0, td.row1 = p.task_row[ti], p.task_row[ti + 1]
            rows = {"node_feat_mask": getattr(p, "nfm_rows", None), "node_contrast": getattr(p, "nc_rows", None),
                    "graph_contrast": getattr(p, "gc_rows", None), "graph_prop": getattr(p, "gp_rows", None)}.get(t)
            if rows is not None:
                for i, v in enumerate(rows):
                    td.mlp.rows[i] = v
            if t == "node_feat_mask":
                td.idx, td.num_idx = p.d64["nfm_idx"], p.nfm_rows[-1]
            elif t == "node_contrast":
                td.idx, td.num_idx = p.d64["nc_idx"], p.nc_rows[-1]
            if t in ("node_contrast", "graph_contrast"):
                ns, slot0 = (p.nc_n, 0) if t == "node_contrast" else (p.gc_n, self.D)
                td.temperature = T_
                for di, n in enumerate(ns):
                    td.ntx_n[di] = n
                ws = self._ntx_workspace(slot0, ns)
                td.ntx_ws, td.ntx_ws_bytes = ws.data_ptr(), ws.numel()
            if t == "graph_contrast":
                td.pool_ptr, td.pool_gid, td.pool_B, td.pool_r0, td.pool_M = p.d32["gc_ptr"], p.d64["gc_gid"], p.gc_B, p.gc_r0, p.gc_M
            if t == "graph_prop":
                td.pool_ptr, td.pool_gid, td.pool_B, td.pool_r0, td.pool_M = p.d32["gp_ptr"], p.d64["gp_gid"], p.gp_B, p.gp_r0, p.gp_M
                td.labels = inp.graph_props.data_ptr()
            if t == "domain_adv":
                td.pool_ptr, td.pool_gid, td.pool_B, td.pool_r0, td.pool_M = p.d32["da_ptr"], p.d64["da_gid"], p.da_B, p.da_r0, p.da_M
                td.da_labels, td.da_lambda, td.da_dropout = p.d64["da_labels"], float(self.grl_lambda), float(self.da_dropout)
            if t == "link_pred":
                td.lp_K, td.lp_edges = p.lp_K, p.d64["lp_edges"]
                td.lp_pos = p.d32.get("lp_pos")
                if self._lp_segmented(p):
                    d.lp_seg_ptr, d.lp_seg_eptr, d.lp_S = p.d32["lp_seg_ptr"], p.d32["lp_seg_eptr"], p.lp_S
                    d.lp_max_seg_rows, d.lp_max_seg_edges, d.lp_rows_end = p.lp_max_rows, p.lp_max_edges, p.lp_rows_end
                else:
                    d.lp_S = 0
        return d

    def _task_segments(self, p: StepPlan) -> List[int]:
        """Exclusive scan of the per-task segment counts (segments are task-major): task t owns segments [out[t], out[t + 1])."""
        return [sum(1 for s in p.seg_task if s < ti) for ti in range(self.T + 1)]

    def _encoder_groups(self, p: StepPlan):
        """(task index, domain, first segment, one-past-last segment) for every (task, domain) pair whose encoder receives a
        gradient this step; pairs that dropped out get their gradient slots zeroed."""
        seg_of: Dict[Tuple[int, int], List[int]] = {}
        for si, (tt, dd) in enumerate(zip(p.seg_task, p.seg_dom)):
            seg_of.setdefault((tt, dd), []).append(si)
        groups = []
        for ti, t in enumerate(self.tasks):
            if t == "node_feat_mask":
                continue
            for di, dom in enumerate(self.domains):
                segs = seg_of.get((ti, di), [])
                if not segs:
                    for key in ("linear.weight", "linear.bias", "batch_norm.weight", "batch_norm.bias"):
                        n = f"input_encoders.{dom}.{key}"
                        self.task_grads[ti, self.off[n]:self.off[n] + self.numel[n]].zero_()
                    continue
                groups.append((ti, dom, segs[0], segs[-1] + 1))
        for a, b in zip(groups[:-1], groups[1:]):
            if a[3] != b[2]:
                raise L.GnnmpError("engine: encoder gradient groups are not contiguous (segments must be task-major)")
        return groups

    def _forward_backward_native(self, p: StepPlan, inp: StepInputs) -> None:
        d = self._fill_desc(p, inp)
        main = torch.cuda.current_stream(self.device)
        self._chk(self.lib.gmp_pretrain_step_fwd_bwd(C.byref(d), main.cuda_stream, self._stream_arr, self.aux_stream.cuda_stream),
                  "gmp_pretrain_step_fwd_bwd")


class StepPrefetcher:
    """Runs engine.prepare() for upcoming steps on a background thread.  The device half of a step is one long C call
    (gmp_pretrain_step_fwd_bwd) that releases the GIL, so index drawing for step t+1 overlaps the launches of step t.
    The RNG stream is unchanged: only this thread draws, in step order."""

    def __init__(self, engine: StepEngine, inputs, gen: torch.Generator, depth: int = 3) -> None:
        import queue
        import threading
        self.q: "queue.Queue" = queue.Queue(maxsize=depth)
        self._err = None

        # producer time in prepare() (host-order draws: in plan(), with draw() on its own thread in draw_s), consumer time blocked in get()
        self.busy_s, self.draw_s, self.wait_s, self.items = 0.0, 0.0, 0.0, 0

        def work() -> None:
            try:
                if engine.rng_mode == "device":
                    # the draws of the next LOOK inputs are in flight on the GPU while this thread plans the current one: a ticket
                    # enqueued on the aux stream runs within one step, and this thread is `depth` steps ahead of the launcher
                    from collections import deque
                    LOOK, ahead, it = 3, deque(), iter(inputs)
                    done = False
                    while True:
                        while not done and len(ahead) < LOOK:
                            try:
                                nxt = next(it)
                            except StopIteration:
                                done = True
                                break
                            ahead.append((nxt, engine.enqueue_draws(nxt)))
                        if not ahead:
                            break
                        inp, ticket = ahead.popleft()
                        t0 = _t.perf_counter()
                        item = (inp, engine.prepare(inp, gen, ticket))
                        self.busy_s += _t.perf_counter() - t0
                        self.q.put(item)
                    self.q.put(None)
                    return
                for inp in inputs:
                    t0 = _t.perf_counter()
                    art = engine.draw(inp, gen)
                    self.draw_s += _t.perf_counter() - t0
                    t0 = _t.perf_counter()
                    item = (inp, (art, engine.plan(inp, art)))
                    self.busy_s += _t.perf_counter() - t0
                    self.q.put(item)
            except BaseException as e:           # surfaced on the consumer side
                self._err = e
            self.q.put(None)

        # (One thread draws and lays out.  A second, layout-only stage and shorter CPython switch intervals measured equal or worse in round 2
        # -- three Python threads on one GIL -- and were removed in round 3.)
        self.thread = threading.Thread(target=work, daemon=True)
        self.thread.start()

    def __iter__(self):
        while True:
            t0 = _t.perf_counter()
            item = self.q.get()
            self.wait_s += _t.perf_counter() - t0
            self.items += 1
            if item is None:
                if self._err is not None:
                    raise self._err
                return
            yield item
