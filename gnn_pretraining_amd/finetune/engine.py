"""One full-graph node-classification fine-tune step as an explicit kernel sequence (BASELINE.json configs[4]: Cora_NC).

The reference's epoch on Cora_NC is ONE optimisation step over the whole graph (src/finetune/finetune.py:162-179, batch_size -1):
`model(data)` = InputEncoder (Linear 1433 -> 256, BN, ReLU, dropout) -> 5 GIN layers on all 2,708 nodes -> Linear 256 -> 7,
cross-entropy (mean) on the 140 training nodes, `loss.backward()`, `AdamW(model.param_groups).step()`
(src/models/finetune_model.py:38-64: encoder / head lr 1e-3, backbone 1e-4, AdamW's default weight decay 0.01, no clipping).
The module path (models/finetune_model.py on autograd Functions) runs that in 3.4 ms, nearly all of it host time in ~200 small
autograd nodes.  Here the same step is ~60 launches with no autograd and no host synchronisation: the graph's CSR is built once,
the encoder's K = 1,433 is padded to 1,440 (a multiple of the GEMM's 32-deep K-step; the weight's padded columns stay zero), and
the optimizer is the pre-training engine's multi-tensor AdamW over one flat buffer.

Structure: BackboneEngine holds what every fine-tune step shares (flat buffer, streams and gates, the backbone forward, backward and AdamW)
and is built from the model alone; a leaf supplies N, csr, seg_ptr[1] = N and the encoder input (dense `x` with leading dimension dpad, or
`xs` / `x_csc` with `sparse` set), sizes the row buffers with _alloc_rows, stores its step's inputs on itself, calls _enqueue, and implements
its one hook, _head_backward.  FullGraphEngine adds a graph fixed at construction; on it sit NodeClassificationEngine (logits, CE head,
the hipGraph capture) and LinkPredictionEngine; GraphClassificationEngine sits on the base directly (capacities, a batch per step).

`FinetuneGNN` stays the owner of the parameters (its tensors become views into the flat buffer, `state_dict()` keys unchanged),
so checkpoints, evaluation and the reference-shaped loop around it are untouched.

Round 3: shapes, pointers and the training rows are the same every step, so the whole step is captured ONCE in a hipGraph
(torch.cuda.CUDAGraph over the ctypes launches) and replayed: ~65 ctypes crossings + launches per step (1.35 ms, host-bound) become
one replay.  What changed per step -- the dropout seed -- is read from a device word the graph's last node increments
(gmp_bn_config.seed_dev, gmp_counter_add), so replay k draws exactly the masks the eager step k draws (tests/test_gpu_modules.py).
The encoder GEMM (172 output tiles for 256 CUs) ran as three K-slices (38 us; unsliced since: 33), and the one-segment BatchNorms (2,708 rows) take the medium
regime of csrc/batchnorm.hip (one launch instead of four).  Measured (MI355X, profiles/README.md round 3): the step was NOT host-bound as
round 2 believed -- its kernels add up to 1.43 ms (BatchNorm 0.58, GEMMs 0.56) -- so the replay (host 0.76 ms) runs at the GPU's 1.38 ms;
a parallel graph branch for the weight-gradient GEMMs (GMP_FINETUNE_FORK=1) makes the replay itself cost 1.45 ms of host time.
Second half of round 3: BatchNorm as slabs over the whole chip in one launch (gmp_bn_config.sync: 34 -> 12 us per backward launch) brought the
kernels to 1.0 ms; the eager step with the weight-gradient GEMMs on the side stream then beats the replay (0.88 against 0.95 ms) and is the
default; the capture stays available (GMP_FINETUNE_GRAPH=1) and tested.

Sparse features (opt-in, `x` a graph.SparseFeatures): the encoder GEMM becomes gmp_sparse_linear_fwd (W transposed into a workspace, one wave
per node gathering the rows of W^T its non-zeros name) and its weight gradient gmp_sparse_linear_wgrad over the CSC form built once here, plus
gmp_colsum for the bias.  The flat-buffer layout, the padded [256, dpad] slot and every other launch are the dense path's.

Inference (embed / predict on all three engines): always eval mode, whatever model.training is.  With running statistics BatchNorm is a
per-channel affine map, so one gmp_bn_fold turns the eleven BatchNorms into (scale, shift) rows as the parameters and running statistics
stand at the call, and every Linear + BatchNorm (+ residual) + ReLU of the backbone is ONE gmp_linear_affine_fwd: a GIN layer is three
launches (aggregate, GEMM, GEMM) instead of the five forward() runs under model.eval().  One stream, no gates, no capture, no dropout, no
saved statistics; it writes activation buffers only, which every training step rewrites before it reads them, so a step after a predict is
bitwise the step without it."""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from .. import _lib as L, operators as OP, ops
from ..graph import SparseFeatures
from ..models.finetune_model import LR_BACKBONE, LR_FINETUNE, FinetuneGNN
from ..models.gnn import DROPOUT_RATE, GNN_HIDDEN_DIM, GNN_NUM_LAYERS

H = GNN_HIDDEN_DIM
NT, NN, TN = 0, 1, 2
ADAMW_WEIGHT_DECAY = 0.01           # torch.optim.AdamW default: the reference passes none (finetune.py:363)


def _i32(xs):
    return (C.c_int32 * len(xs))(*[int(v) for v in xs])


def _i64(xs):
    return (C.c_int64 * len(xs))(*[int(v) for v in xs])


def _ptr(t: Optional[Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


class BackboneEngine:
    """Everything the three engines share, and nothing else; built from the model alone (the structure paragraph of the module docstring)."""
    def __init__(self, model: FinetuneGNN, d_in: int, device, seed: int = 0) -> None:
        self.model, self.device, self.lib = model, torch.device(device), L.lib()
        self.seed, self.step_count, self.dropout_p = seed, 0, DROPOUT_RATE
        dev = self.device
        self.d_in, self.dpad = int(d_in), (int(d_in) + 31) // 32 * 32
        self.N, self.csr, self.sparse, self.x, self.num_targets = 0, None, False, None, 0
        self._flatten()
        f = lambda *s: torch.empty(*s, device=dev)
        self.stat = {k: f(GNN_NUM_LAYERS, c) for k, c in (("m1", 2 * H), ("s1", 2 * H), ("m2", H), ("s2", H))}
        self.enc_mean, self.enc_rstd = f(H), f(H)
        # the side stream must sit on a hardware queue of its own: in a process whose queues are taken (bench.py after the pre-training engine) a fresh
        # pool stream shared the main stream's queue and the forked step took 3.98 ms instead of 0.88 -- measured, not assumed (streams.py)
        if dev.type == "cuda":
            from .. import streams as ST
            self.side = ST.concurrent_streams(dev, 1)[0]
            # main <-> side dependencies by gates (a sleeping wave on a flag word, csrc/streams.hip) instead of events where the two streams
            # were measured on different hardware queues: a queue parked on an event wait costs the running one ~2 us per kernel boundary
            own_queue = not ST.share_queue(torch.cuda.current_stream(dev).cuda_stream, self.side.cuda_stream)
            self._gates_ok = own_queue and os.environ.get("GMP_FINETUNE_GATES", "1") != "0"
        else:
            self.side, self._gates_ok, own_queue = None, False, False
        self.sync_flags, self._epoch = torch.zeros(64, dtype=torch.int32, device=dev), 0
        self.side_ws = torch.empty(32 << 20, dtype=torch.uint8, device=dev)
        # Default since the slab BatchNorm: launch by launch, the weight-gradient GEMMs on the side stream (0.88 ms per Cora_NC step; the host needs
        # 0.55-0.68 ms for the 120 ctypes launches and keeps up).  Not without a queue of its own for the side stream (every hardware queue of the
        # process taken): the fork would run behind main's kernels in the same in-order queue, slower than the plain chain
        self.fork_wgrads = os.environ.get("GMP_FINETUNE_FORK", "1" if own_queue else "0") == "1"
        self.seg_ptr = torch.zeros(2, dtype=torch.int32, device=dev)                # the one BatchNorm segment [0, N)
        # rendezvous words of the BatchNorm slab form (gmp_bn_config.sync: the graph's 2,708 rows as 128-row slabs over the whole chip, one
        # launch); every BatchNorm of the step runs on the main stream, so one buffer serves them all.  GMP_BN_SLABS=0: one workgroup per strip
        self.bn_sync = (torch.zeros(self.lib.gmp_bn_sync_bytes(2 * H, 1) // 4, dtype=torch.int32, device=dev)
                        if os.environ.get("GMP_BN_SLABS", "1") != "0" else None)
        self.gemm_ws = torch.empty(32 << 20, dtype=torch.uint8, device=dev)
        self.loss_sum, self.g_scale = torch.zeros(1, device=dev), torch.ones(1, device=dev)
        self.mt_ws = torch.empty(self.lib.gmp_mt_workspace_bytes(self.K), dtype=torch.uint8, device=dev)
        self.normsq, self.metrics, self.flags = torch.zeros(1, device=dev), torch.zeros(2, dtype=torch.int32, device=dev), torch.zeros(self.K, dtype=torch.int32, device=dev)
        self._bn_calls = 0
        # inference path: the (scale, shift) table of the 11 BatchNorms (encoder, then inner / outer of each layer), refilled per pass
        self._fold_ch = [H] + [2 * H, H] * GNN_NUM_LAYERS
        self._fold_off = [2 * sum(self._fold_ch[:i]) for i in range(len(self._fold_ch))]
        self._fold_table = torch.empty(2 * sum(self._fold_ch), device=dev)
        self._infer_loss: Optional[Tuple[Tensor, int]] = None     # (loss sum, count) of the last predict with targets; a step clears it
        self._fwd_gen, self._embed_gen = 0, -1                    # forwards that wrote h[] so far / the one whose output embed() last returned

    def _alloc_rows(self, cap_n: int) -> None:
        """Every [rows, 256 / 512] activation and gradient buffer and the BatchNorm workspace, for up to cap_n rows."""
        f, Lr = (lambda *s: torch.empty(*s, device=self.device)), GNN_NUM_LAYERS
        self.z0, self.h = f(cap_n, H), [f(cap_n, H) for _ in range(Lr + 1)]
        self.a, self.z1 = [f(cap_n, H) for _ in range(Lr)], [f(cap_n, 2 * H) for _ in range(Lr)]
        self.r1, self.z2 = [f(cap_n, 2 * H) for _ in range(Lr)], [f(cap_n, H) for _ in range(Lr)]
        self.gA, self.ga, self.gW = f(cap_n, H), f(cap_n, H), f(cap_n, 2 * H)
        # per-layer g_u / g_z1 (+ one g_u for the encoder): the weight-gradient GEMMs read them on the side stream while the chain moves on
        self.gu_l, self.gz1_l = [f(cap_n, H) for _ in range(Lr + 1)], [f(cap_n, 2 * H) for _ in range(Lr)]
        self.rowdot = f(Lr, cap_n)
        self.bn_ws = torch.empty(max(self.lib.gmp_bn_workspace_bytes(cap_n, 2 * H, 1, cap_n), 16), dtype=torch.uint8, device=self.device)

    # ------------------------------------------------------------------ parameters: one flat buffer, the module's tensors view into it
    def _flatten(self) -> None:
        m, dev = self.model, self.device
        named = [(n, p) for n, p in m.named_parameters()]
        al4 = lambda v: (v + 3) // 4 * 4
        self.off: Dict[str, int] = {}
        self.numel: Dict[str, int] = {}
        o = 0
        for n, p in named:
            cnt = H * self.dpad if n == "input_encoder.linear.weight" else p.numel()      # encoder weight: rows padded to dpad columns
            self.off[n], self.numel[n] = o, cnt
            o += al4(cnt)
        self.P = o
        self.flat = torch.zeros(self.P, device=dev)
        for n, p in named:
            a = self.off[n]
            if n == "input_encoder.linear.weight":
                view = self.flat[a:a + H * self.dpad].view(H, self.dpad)
                view[:, :self.d_in].copy_(p.data)
                p.data = view[:, :self.d_in]                      # strided view: the padded columns are outside the parameter
            else:
                self.flat[a:a + p.numel()].copy_(p.data.reshape(-1))
                p.data = self.flat[a:a + p.numel()].view_as(p)
        self.names = [n for n, _ in named]
        self.K = len(self.names)
        self.grad = torch.zeros(1, self.P, device=dev)            # [tasks = 1, P]
        self.final_grad = torch.zeros(self.P, device=dev)
        self.exp_avg, self.exp_avg_sq = torch.zeros(self.P, device=dev), torch.zeros(self.P, device=dev)
        self.t_off = torch.tensor([self.off[n] for n in self.names], dtype=torch.int64, device=dev)
        self.t_len = torch.tensor([self.numel[n] for n in self.names], dtype=torch.int32, device=dev)
        trainable = {n: p.requires_grad for n, p in named}
        has = torch.zeros(self.K, 8, dtype=torch.uint8)
        lr = torch.zeros(self.K)
        for k, n in enumerate(self.names):
            has[k, 0] = 1 if trainable[n] else 0
            lr[k] = LR_BACKBONE if n.startswith("gnn_backbone.") else LR_FINETUNE
        self.has, self.lr = has.to(dev), lr.to(dev)
        self.wd = torch.full((self.K,), ADAMW_WEIGHT_DECAY, device=dev)
        self.steps = torch.zeros(self.K, device=dev)

    def _P(self, n: str) -> int:
        return self.flat.data_ptr() + 4 * self.off[n]

    def _G(self, n: str) -> int:
        return self.off[n]

    def _chk(self, rc: int, what: str) -> None:
        if rc:
            L.check(rc, what)

    def _cfg(self, relu: bool, dropout: bool, site: int) -> L.BnConfig:
        """Dropout seed of a launch = seed * 1000003 + step number; in a captured step the step number comes from the device word."""
        p = self.dropout_p if (dropout and self.model.training) else 0.0
        base = self.seed * 1000003
        sync = (self.bn_sync.data_ptr(), self.bn_sync.numel()) if self.bn_sync is not None else (None, 0)
        step = 0 if self._seed_dev else self.step_count
        return L.BnConfig(int(self.model.training), int(relu), 1e-5, 0.1, p, (base + step) & (2 ** 64 - 1), site + self._site_base, self._seed_dev, *sync)

    _seed_dev = None                    # the device word a captured step reads its step number from (NodeClassificationEngine.step)
    _site_base = 0                      # added to every dropout site of a forward (LinkPredictionEngine.mining_forward: a second pass per step)

    # ------------------------------------------------------------------ the launches that recur; pointers are resolved at every launch
    def _gemm(self, st, mode, A, B, bias, Cc, M, N, K, lda, ldb, ldc, ws: Optional[Tensor] = None):
        self._chk(self.lib.gmp_gemm_f32(mode, A, B, bias, Cc, M, N, K, lda, ldb, ldc, 1.0, 0, 0, None if ws is None else ws.data_ptr(),
                                        0 if ws is None else ws.numel(), st), "gemm")

    def _wgrad(self, st, G, X, w_name: str, b_name: str, M_tn: int, N_out: int, ldx: int, ws: Optional[Tensor] = None):
        """dW = G^T X and db = colsum(G) over all rows (one group), straight into the gradient buffer."""
        g, ws = self.grad.data_ptr(), (self.gemm_ws if ws is None else ws)
        self._chk(self.lib.gmp_gemm_f32_grouped(TN, G, X, None, g, 1, _i32([0, self.N]), None, None, _i64([self._G(w_name)]), g, _i64([self._G(b_name)]),
                                                M_tn, N_out, 0, M_tn, ldx, N_out, 1.0, 0, 0, ws.data_ptr(), ws.numel(), st), "wgrad")

    def _bn_fwd(self, st, z: Tensor, resid: Optional[Tensor], pre: str, bn, mean: Optional[Tensor], rstd: Optional[Tensor], out: Tensor, cfg: L.BnConfig):
        """out = act(BatchNorm(z) [+ resid]) over the one segment [0, N): `pre` names the affine pair in the flat buffer, `bn` the module
        whose running statistics it reads (and in training updates), mean / rstd the rows the backward reads (None in eval mode)."""
        N, P = self.N, self._P
        self._chk(self.lib.gmp_bn_fwd(z.data_ptr(), _ptr(resid), self.seg_ptr.data_ptr(), None, 1, N, N, z.size(1), P(pre + "weight"), P(pre + "bias"),
                                      bn.running_mean.data_ptr(), bn.running_var.data_ptr(), _ptr(mean), _ptr(rstd), out.data_ptr(), C.byref(cfg),
                                      self.bn_ws.data_ptr(), self.bn_ws.numel(), st), "bn " + pre)

    def _bn_bwd(self, st, gy: Tensor, z: Tensor, resid: Optional[Tensor], pre: str, bn, mean: Tensor, rstd: Tensor, gz: Tensor, cfg: L.BnConfig):
        """gz = d loss / d z of _bn_fwd's launch from gy = d loss / d out; the affine pair's gradients go straight into the gradient buffer."""
        N, P, g = self.N, self._P, self.grad.data_ptr()
        self._chk(self.lib.gmp_bn_bwd(gy.data_ptr(), z.data_ptr(), _ptr(resid), self.seg_ptr.data_ptr(), None, 1, N, N, z.size(1), P(pre + "weight"),
                                      P(pre + "bias"), bn.running_mean.data_ptr(), bn.running_var.data_ptr(), mean.data_ptr(), rstd.data_ptr(),
                                      gz.data_ptr(), g, g, _i32([0, 1]), _i64([self._G(pre + "weight")]), _i64([self._G(pre + "bias")]), 1,
                                      C.byref(cfg), self.bn_ws.data_ptr(), self.bn_ws.numel(), st), "bn bwd " + pre)

    def _sparse_encoder(self, st) -> None:
        """z0 = xs W^T + b (gmp_sparse_linear_fwd on the [256, dpad] weight slot)."""
        xs, P = self.xs, self._P
        self._chk(self.lib.gmp_sparse_linear_fwd(xs.rowptr.data_ptr(), xs.col.data_ptr(), xs.val.data_ptr(), self.N, self.d_in, P("input_encoder.linear.weight"),
                                                 self.dpad, P("input_encoder.linear.bias"), self.z0.data_ptr(), H, H, self.sp_status.data_ptr(),
                                                 self.sp_wt.data_ptr(), self.sp_wt.numel(), st), "sparse encoder")

    # ------------------------------------------------------------------ forward (finetune_model.py:68-80, message passing on the full graph)
    def forward(self) -> Tensor:
        """Encoder + backbone in the model's mode (the leaf's head runs behind it).  The engine's own buffer: the next forward overwrites it."""
        self._backbone_forward()
        if self.model.training:
            self._bn_calls += 1             # num_batches_tracked only matters for a saved state_dict (momentum is fixed): flush_counters()
        return self.h[GNN_NUM_LAYERS]

    def _backbone_forward(self) -> None:
        """Encoder + the GIN layers into h[GNN_NUM_LAYERS]; every activation the backward reads stays in the engine's buffers."""
        lib, N, P, c = self.lib, self.N, self._P, self.csr
        self._fwd_gen += 1
        st = torch.cuda.current_stream(self.device).cuda_stream
        # 2,708 x 1,440 -> 256 is 172 output tiles for 256 CUs; unsliced since round 3 (three K-slices + their reduction: 38 us, one launch: 33 --
        # gmp_gemm_f32_workspace_bytes now slices NT / NN only below ~100 tiles)
        if self.sparse:
            self._sparse_encoder(st)
        else:
            self._gemm(st, NT, self.x.data_ptr(), P("input_encoder.linear.weight"), P("input_encoder.linear.bias"), self.z0.data_ptr(), N, H, self.dpad,
                       self.dpad, self.dpad, H, ws=self.gemm_ws)
        self._bn_fwd(st, self.z0, None, "input_encoder.batch_norm.", self.model.input_encoder.batch_norm, self.enc_mean, self.enc_rstd, self.h[0], self._cfg(True, True, 1))
        for l in range(GNN_NUM_LAYERS):
            pre, layer = f"gnn_backbone.layers.{l}.", self.model.gnn_backbone.layers[l]
            self._chk(lib.gmp_gin_aggregate_fwd(self.h[l].data_ptr(), c.rowptr.data_ptr(), c.col.data_ptr(), P(pre + "gin_conv.eps"), self.a[l].data_ptr(), N, H, st), "aggregate")
            self._gemm(st, NT, self.a[l].data_ptr(), P(pre + "gin_conv.nn.0.weight"), P(pre + "gin_conv.nn.0.bias"), self.z1[l].data_ptr(), N, 2 * H, H, H, H, 2 * H)
            self._bn_fwd(st, self.z1[l], None, pre + "gin_conv.nn.1.", layer.gin_conv.nn[1], self.stat["m1"][l], self.stat["s1"][l], self.r1[l], self._cfg(True, False, 0))
            self._gemm(st, NT, self.r1[l].data_ptr(), P(pre + "gin_conv.nn.3.weight"), P(pre + "gin_conv.nn.3.bias"), self.z2[l].data_ptr(), N, H, 2 * H, 2 * H, 2 * H, H)
            self._bn_fwd(st, self.z2[l], self.h[l], pre + "batch_norm.", layer.batch_norm, self.stat["m2"][l], self.stat["s2"][l], self.h[l + 1], self._cfg(True, True, 10 + l))

    # ------------------------------------------------------------------ inference: eval mode, BatchNorm folded into the GEMM epilogues
    def _bn_modules(self):
        return [self.model.input_encoder.batch_norm] + [b for l in self.model.gnn_backbone.layers for b in (l.gin_conv.nn[1], l.batch_norm)]

    def _bn_names(self) -> List[str]:
        return ["input_encoder.batch_norm."] + [f"gnn_backbone.layers.{l}.{n}" for l in range(GNN_NUM_LAYERS) for n in ("gin_conv.nn.1.", "batch_norm.")]

    def _infer_forward(self) -> Tensor:
        """Encoder + the GIN layers in eval mode into h[GNN_NUM_LAYERS], on the current stream: gmp_bn_fold, the encoder as one
        gmp_linear_affine_fwd (sparse features: gmp_sparse_linear_fwd + the eval-mode gmp_bn_fwd), then aggregate, GEMM, GEMM per layer."""
        lib, N, P, c = self.lib, self.N, self._P, self.csr
        self._fwd_gen += 1
        st = torch.cuda.current_stream(self.device).cuda_stream
        bns, names = self._bn_modules(), self._bn_names()
        tbl = lambda xs: (C.c_void_p * len(xs))(*xs)
        self._chk(lib.gmp_bn_fold(len(bns), tbl([P(n + "weight") for n in names]), tbl([P(n + "bias") for n in names]),
                                  tbl([b.running_mean.data_ptr() for b in bns]), tbl([b.running_var.data_ptr() for b in bns]),
                                  _i32(self._fold_ch), 1e-5, self._fold_table.data_ptr(), st), "bn fold")
        sc = lambda i: self._fold_table.data_ptr() + 4 * self._fold_off[i]
        sh = lambda i: sc(i) + 4 * self._fold_ch[i]
        ws = self.gemm_ws

        def lin(A, w_name, b_name, resid, i, out, M, Nout, K, lda, ldw):
            self._chk(lib.gmp_linear_affine_fwd(A, P(w_name), P(b_name), resid, sc(i), sh(i), out, M, Nout, K, lda, ldw, Nout if resid else 0, Nout, 1,
                                                ws.data_ptr(), ws.numel(), st), "linear affine")

        if self.sparse:
            self._sparse_encoder(st)
            self._bn_fwd(st, self.z0, None, "input_encoder.batch_norm.", bns[0], None, None, self.h[0], L.BnConfig(0, 1, 1e-5, 0.1, 0.0, 0, 0, None, None, 0))
        else:
            lin(self.x.data_ptr(), "input_encoder.linear.weight", "input_encoder.linear.bias", None, 0, self.h[0].data_ptr(), N, H, self.dpad, self.dpad, self.dpad)
        for l in range(GNN_NUM_LAYERS):
            pre = f"gnn_backbone.layers.{l}."
            self._chk(lib.gmp_gin_aggregate_fwd(self.h[l].data_ptr(), c.rowptr.data_ptr(), c.col.data_ptr(), P(pre + "gin_conv.eps"), self.a[l].data_ptr(), N, H, st), "aggregate")
            lin(self.a[l].data_ptr(), pre + "gin_conv.nn.0.weight", pre + "gin_conv.nn.0.bias", None, 1 + 2 * l, self.r1[l].data_ptr(), N, 2 * H, H, H, H)
            lin(self.r1[l].data_ptr(), pre + "gin_conv.nn.3.weight", pre + "gin_conv.nn.3.bias", self.h[l].data_ptr(), 2 + 2 * l, self.h[l + 1].data_ptr(), N, H, 2 * H, 2 * H, 2 * H)
        return self.h[GNN_NUM_LAYERS]

    def embed(self) -> Tensor:
        """The backbone's output rows [N, 256] in eval mode (whatever model.training is), from the parameters and running statistics as
        they stand now.  The engine's own buffer: the next forward, step, embed or predict overwrites it."""
        out = self._infer_forward()[:self.N]
        self._embed_gen = self._fwd_gen
        return out

    def flush_counters(self) -> None:
        if self._bn_calls:
            for bn in self._bn_modules():
                bn.num_batches_tracked += self._bn_calls
            self._bn_calls = 0

    # ------------------------------------------------------------------ one optimisation step (finetune.py:162-179 + 318-320)
    def _enqueue(self, apply_update: bool, forked: bool = False) -> None:
        """The step's launches on the current stream, for the inputs the leaf's step() has stored on the engine.  forked: the weight-gradient
        GEMMs (they only feed the gradient buffer) go to the side stream behind an event of the main one -- inside a capture a parallel
        branch of the graph -- and are joined before AdamW."""
        lib, N, P, c = self.lib, self.N, self._P, self.csr
        main = torch.cuda.current_stream(self.device)
        st = main.cuda_stream
        side = self.side if (forked and self.side is not None) else None
        sst = side.cuda_stream if side is not None else st
        wws = self.side_ws if side is not None else self.gemm_ws

        gates = side is not None and self._gates_ok and not torch.cuda.is_current_stream_capturing()
        if gates:
            self._epoch += 1
        flags, epoch, nfork = self.sync_flags.data_ptr(), self._epoch, [0]

        def fork() -> None:
            """The side stream may read what main has produced so far.  The caller launches a GEMM on MAIN next; with gates that GEMM carries
            the signal as it starts (gmp_gate_open_by_next_gemm) -- no one-thread launch on the chain."""
            if side is None:
                return
            if gates:
                k = nfork[0]
                nfork[0] = k + 1
                self._chk(lib.gmp_gate_open_by_next_gemm(flags + 4 * k, epoch), "gate open by gemm")
                self._chk(lib.gmp_gate_wait(flags, 1 << k, epoch, flags + 4 * 63, sst), "gate wait")
            else:
                side.wait_stream(main)

        def flush() -> None:                                        # the GEMM that was to carry the signal launched nothing: open the gate by hand
            if gates and lib.gmp_gate_open_pending():
                self._chk(lib.gmp_gate_open_by_next_gemm(None, 0), "cancel")
                self._chk(lib.gmp_gate_open(flags + 4 * (nfork[0] - 1), epoch, st), "gate open")

        self.forward()
        self._head_backward(st)
        g, gcur, ga, pending_eps = self.grad.data_ptr(), self.gA, self.ga, None
        for l in reversed(range(GNN_NUM_LAYERS)):
            pre, layer = f"gnn_backbone.layers.{l}.", self.model.gnn_backbone.layers[l]
            gu, gz1 = self.gu_l[l], self.gz1_l[l]
            self._bn_bwd(st, gcur, self.z2[l], self.h[l], pre + "batch_norm.", layer.batch_norm, self.stat["m2"][l], self.stat["s2"][l], gu, self._cfg(True, True, 10 + l))
            fork()
            self._gemm(st, NN, gu.data_ptr(), P(pre + "gin_conv.nn.3.weight"), None, self.gW.data_ptr(), N, 2 * H, H, H, 2 * H, 2 * H)
            flush()
            if pending_eps is not None:                             # (the previous layer's aggregation backward is behind this fork too)
                self._eps_grad(sst, pending_eps)
                pending_eps = None
            self._wgrad(sst, gu.data_ptr(), self.r1[l].data_ptr(), pre + "gin_conv.nn.3.weight", pre + "gin_conv.nn.3.bias", H, 2 * H, 2 * H, wws)
            self._bn_bwd(st, self.gW, self.z1[l], None, pre + "gin_conv.nn.1.", layer.gin_conv.nn[1], self.stat["m1"][l], self.stat["s1"][l], gz1, self._cfg(True, False, 0))
            fork()
            self._gemm(st, NN, gz1.data_ptr(), P(pre + "gin_conv.nn.0.weight"), None, ga.data_ptr(), N, H, 2 * H, 2 * H, H, H)
            flush()
            self._wgrad(sst, gz1.data_ptr(), self.a[l].data_ptr(), pre + "gin_conv.nn.0.weight", pre + "gin_conv.nn.0.bias", 2 * H, H, H, wws)
            self._chk(lib.gmp_gin_aggregate_bwd_ex(ga.data_ptr(), c.rowptr_t.data_ptr(), c.col_t.data_ptr(), P(pre + "gin_conv.eps"), self.h[l].data_ptr(),
                                                   gu.data_ptr(), gcur.data_ptr(), self.rowdot[l].data_ptr(), N, H, st), "aggregate bwd")
            pending_eps = l                                          # eps gradient: a 5 us sum that only feeds the gradient buffer -- with the next fork
        self._eps_grad(st, pending_eps)                             # layer 0's: on main, in front of the encoder backward
        gu = self.gu_l[GNN_NUM_LAYERS]
        self._bn_bwd(st, gcur, self.z0, None, "input_encoder.batch_norm.", self.model.input_encoder.batch_norm, self.enc_mean, self.enc_rstd, gu, self._cfg(True, True, 1))
        if self.sparse:                                             # dW over the whole [256, dpad] slot (padding columns 0.0), db = colsum
            colptr, row, val_t = self.x_csc
            self._chk(lib.gmp_sparse_linear_wgrad(colptr.data_ptr(), row.data_ptr(), val_t.data_ptr(), N, self.d_in, gu.data_ptr(), H,
                                                  g + 4 * self._G("input_encoder.linear.weight"), self.dpad, self.sp_status.data_ptr(), st), "sparse wgrad")
            self._chk(lib.gmp_colsum(gu.data_ptr(), g + 4 * self._G("input_encoder.linear.bias"), N, H, H, 0, self.colsum_ws.data_ptr(),
                                     self.colsum_ws.numel(), st), "encoder bias grad")
        else:
            self._wgrad(st, gu.data_ptr(), self.x.data_ptr(), "input_encoder.linear.weight", "input_encoder.linear.bias", H, self.dpad, self.dpad)
        if side is not None:                                        # every weight gradient is in the buffer
            if gates:
                self._chk(lib.gmp_gate_open(flags + 4 * 40, epoch, sst), "gate open")
                self._chk(lib.gmp_gate_wait(flags, 1 << 40, epoch, flags + 4 * 63, st), "gate wait")
            else:
                main.wait_stream(side)
        # AdamW over the flat buffer (the pre-training engine's multi-tensor kernels with one task: no projection, no clipping)
        self._chk(lib.gmp_mt_pcgrad_clip_adamw(g, self.P, 1, self.K, self.t_off.data_ptr(), self.t_len.data_ptr(), self.has.data_ptr(), _i32([0]), 1, 0, -1,
                                               self.flat.data_ptr(), self.exp_avg.data_ptr(), self.exp_avg_sq.data_ptr(),
                                               self.steps.data_ptr() if apply_update else None, self.lr.data_ptr(), self.wd.data_ptr(), 0.9, 0.999, 1e-8, 0.0,
                                               self.final_grad.data_ptr(), self.normsq.data_ptr(), self.metrics.data_ptr(), self.flags.data_ptr(),
                                               self.mt_ws.data_ptr(), self.mt_ws.numel(), int(apply_update), st), "adamw")

    def _head_backward(self, st: int) -> None:
        """The leaf's: loss and head after forward(), from the inputs its step() stored; d loss / d h[GNN_NUM_LAYERS] into gA."""
        raise NotImplementedError

    def _eps_grad(self, stream: int, l: int) -> None:
        self._chk(self.lib.gmp_group_sum_1d(self.rowdot[l].data_ptr(), 1, _i32([0, self.N]), _i64([self._G(f"gnn_backbone.layers.{l}.gin_conv.eps")]),
                                            self.grad.data_ptr(), stream), "eps grad")

    def loss(self) -> float:
        """Mean loss of the last step, or of the last predict with targets (a read-back: the one place the loop synchronises, so the gates'
        time-out word and the slab BatchNorm's are looked at here too)."""
        infer = self._infer_loss
        v = float((self.loss_sum if infer is None else infer[0]).item())
        if self.sparse and int(self.sp_status.item()) != 0:
            raise L.GnnmpError(f"fine-tune engine: the sparse encoder skipped {int(self.sp_status.item())} out-of-range feature indices")
        if int(self.sync_flags[63].item()) != 0 or (self.bn_sync is not None and int(self.bn_sync[0].item()) != 0):
            raise L.GnnmpError("fine-tune engine: a cross-stream gate or a BatchNorm slab wait timed out (streams sharing a hardware queue, "
                               "a tool serialising kernels, or a sync buffer shared between streams): results since then are not to be trusted")
        return v / max(self.num_targets if infer is None else infer[1], 1)

    def gradient(self, name: str) -> Tensor:
        o = self.off[name]
        if name == "input_encoder.linear.weight":
            return self.final_grad[o:o + H * self.dpad].view(H, self.dpad)[:, :self.d_in]
        p = dict(self.model.named_parameters())[name]
        return self.final_grad[o:o + p.numel()].view_as(p)


class FullGraphEngine(BackboneEngine):
    """A fixed graph given at construction: its features (dense, or a graph.SparseFeatures) and its CSR are set up once, here."""

    def __init__(self, model: FinetuneGNN, x: Tensor, edge_index: Tensor, device, seed: int = 0) -> None:
        super().__init__(model, int(x.size(1)), device, seed)
        dev, self.N = self.device, int(x.size(0))
        # sparse (CSR) features: the encoder is gmp_sparse_linear_fwd / _wgrad on the same [256, dpad] weight slot; the CSC form the
        # weight gradient reads is built here, once (the features never change)
        self.sparse = isinstance(x, SparseFeatures)
        if self.sparse:
            self.xs = x.to(dev)
            self.x_csc = self.xs.csc()
            self.sp_wt = torch.empty(self.lib.gmp_sparse_linear_workspace_bytes(self.d_in, H), dtype=torch.uint8, device=dev)
            self.sp_status = torch.zeros(1, dtype=torch.int32, device=dev)          # skipped indices (none once csc() has passed): loss()
            self.colsum_ws = torch.empty(max(self.lib.gmp_colsum_workspace_bytes(self.N, H), 16), dtype=torch.uint8, device=dev)
        else:
            self.x = torch.zeros(self.N, self.dpad, device=dev)
            self.x[:, :self.d_in] = x.to(dev)
        self.csr = ops.csr_build(edge_index.to(dev).contiguous(), self.N)
        self.seg_ptr[1:].fill_(self.N)
        self._alloc_rows(self.N)


class NodeClassificationEngine(FullGraphEngine):
    def __init__(self, model: FinetuneGNN, x: Tensor, edge_index: Tensor, device, seed: int = 0) -> None:
        super().__init__(model, x, edge_index, device, seed)
        dev = self.device
        self.classes = int(model.classification_head.mlp[0].weight.size(0))
        self.logits = torch.empty(self.N, self.classes, device=dev)
        self.loss_ws = torch.empty(self.lib.gmp_loss_workspace_bytes(self.N * H), dtype=torch.uint8, device=dev)
        self.seed_word = torch.zeros(1, dtype=torch.int64, device=dev)        # device copy of step_count for captured steps (gmp_bn_config.seed_dev)
        # GMP_FINETUNE_GRAPH=1: the step captured once and replayed (bitwise the numbers of the eager default, host 0.43 ms per replay,
        # 0.95 ms per step on ONE chain: replaying a graph with a second branch costs the host 1.45 ms on this runtime -- ROCm 7.2,
        # profiles/README.md round 3 -- so a captured step keeps its weight gradients in the chain unless GMP_FINETUNE_FORK says otherwise).
        self.use_graph = dev.type == "cuda" and os.environ.get("GMP_FINETUNE_GRAPH", "0") == "1"
        if self.use_graph and "GMP_FINETUNE_FORK" not in os.environ:
            self.fork_wgrads = False
        self._graph, self._graph_key, self._graph_step, self._graph_seen = None, None, -1, None
        self._train_idx: Optional[Tensor] = None
        self._step_args: Optional[Tuple[Tensor, Tensor]] = None  # (node_indices, targets) of the step being enqueued: _head_backward

    def forward(self) -> Tensor:
        self._head_logits(super().forward())
        return self.logits

    def _head_logits(self, hL: Tensor) -> None:
        self._gemm(torch.cuda.current_stream(self.device).cuda_stream, NT, hL.data_ptr(), self._P("classification_head.mlp.0.weight"),
                   self._P("classification_head.mlp.0.bias"), self.logits.data_ptr(), self.N, self.classes, H, H, H, self.classes)

    def predict(self, node_indices: Tensor, targets: Optional[Tensor] = None) -> Tensor:
        """Eval-mode logits [len(node_indices), C] of the given nodes; with targets, loss() then returns their mean cross-entropy.
        Changes nothing a training step reads: parameters, optimizer state, running statistics, counters and the captured step stay as they are."""
        self._head_logits(self._infer_forward())
        with torch.no_grad():
            rows = OP.take_rows(self.logits, node_indices)
            self._infer_loss = None
            if targets is not None:
                self._infer_loss = (ops.cross_entropy_sum_fwd(rows, targets.contiguous()), int(node_indices.numel()))
        return rows

    # ------------------------------------------------------------------ one optimisation step (finetune.py:162-179 + 318-320)
    def step(self, node_indices: Tensor, targets: Tensor, apply_update: bool = True) -> None:
        """loss = cross_entropy(model(data)[node_indices], targets) (mean); backward; AdamW.  Nothing is read back: loss().
        Training steps with an update are replayed from a hipGraph captured at the first such call for these index tensors."""
        self._infer_loss, self._step_args = None, (node_indices, targets)
        if not (self.use_graph and apply_update and self.model.training):
            self._enqueue(apply_update, forked=self.fork_wgrads)
            self.step_count += 1
            return
        key = (node_indices.data_ptr(), targets.data_ptr(), int(node_indices.numel()))
        if self._graph_key != key:
            # an eager step first (it IS this call's step): code objects loaded, LDS attributes set, row buffers allocated -- nothing of
            # that may happen inside a capture.  The capture itself (tens of ms) waits for the SECOND call with the same index tensors:
            # a caller that builds fresh tensors per call never pays for it.
            self._enqueue(True)
            self.step_count += 1
            if self._graph_seen != key:
                self._graph_seen, self._graph_keep = key, (node_indices, targets)
                return
            torch.cuda.current_stream(self.device).synchronize()
            graph = torch.cuda.CUDAGraph()
            self._seed_dev = self.seed_word.data_ptr()
            try:
                with torch.cuda.graph(graph):
                    self._enqueue(True, forked=self.fork_wgrads)
                    self._chk(self.lib.gmp_counter_add(self.seed_word.data_ptr(), 1, torch.cuda.current_stream(self.device).cuda_stream), "seed word")
            finally:
                self._seed_dev = None
            self._bn_calls -= 1                                     # (forward() counted the capture pass, which ran nothing)
            self._graph, self._graph_key, self._graph_step = graph, key, -1
            self._graph_keep = (node_indices, targets)             # the captured launches hold these pointers
            return
        if self._graph_step != self.step_count:                    # eager steps ran in between (evaluation does not count): resynchronise
            self.seed_word.fill_(self.step_count)
        self._graph.replay()
        self._fwd_gen += 1
        self.step_count += 1
        self._graph_step = self.step_count
        self._bn_calls += 1

    def _head_backward(self, st: int) -> None:
        """Loss and head of the step after forward(): d loss / d h[GNN_NUM_LAYERS] into gA (the backbone backward starts from it)."""
        lib, N, P, Cn = self.lib, self.N, self._P, self.classes
        node_indices, targets = self._step_args
        M = int(node_indices.numel())
        if self._train_idx is None or self._train_idx.numel() != M:
            f = lambda *s: torch.empty(*s, device=self.device)
            self._rows_logits, self._rows_g, self._rows_h, self._rows_gh = f(M, Cn), f(M, Cn), f(M, H), f(M, H)
        self._train_idx, self.num_targets = node_indices, M
        self.g_scale.fill_(1.0 / M)
        idx, tgt, g = node_indices.data_ptr(), targets.data_ptr(), self.grad.data_ptr()
        hL = self.h[GNN_NUM_LAYERS]
        self._chk(lib.gmp_row_gather(self.logits.data_ptr(), idx, None, self._rows_logits.data_ptr(), M, N, Cn, st), "logit rows")
        self._chk(lib.gmp_cross_entropy_sum_fwd(self._rows_logits.data_ptr(), tgt, M, Cn, self.loss_sum.data_ptr(), self.loss_ws.data_ptr(), self.loss_ws.numel(), st), "ce")
        self._chk(lib.gmp_cross_entropy_sum_bwd(self._rows_logits.data_ptr(), tgt, M, Cn, self.g_scale.data_ptr(), self._rows_g.data_ptr(), st), "ce bwd")
        # head: dW = g^T h[idx], db = colsum(g), g_h[idx] = g W  (only the M training rows carry a gradient)
        self._chk(lib.gmp_row_gather(hL.data_ptr(), idx, None, self._rows_h.data_ptr(), M, N, H, st), "h rows")
        self._chk(lib.gmp_gemm_f32_grouped(TN, self._rows_g.data_ptr(), self._rows_h.data_ptr(), None, g, 1, _i32([0, M]), None, None,
                                           _i64([self._G("classification_head.mlp.0.weight")]), g, _i64([self._G("classification_head.mlp.0.bias")]),
                                           Cn, H, 0, Cn, H, H, 1.0, 0, 0, None, 0, st), "head wgrad")
        self._gemm(st, NN, self._rows_g.data_ptr(), P("classification_head.mlp.0.weight"), None, self._rows_gh.data_ptr(), M, H, Cn, Cn, H, H)
        self.gA.zero_()
        self._chk(lib.gmp_row_fill(self.gA.data_ptr(), idx, self._rows_gh.data_ptr(), M, N, H, 0, st), "scatter g_h")

    def logits_of_step(self) -> Tensor:
        """The last step's logits [len(node_indices), C] of its training rows (the engine's buffer: the next step overwrites it)."""
        return self._rows_logits


LP_SCORER_SITE = 40                 # dropout site of the scorer's hidden layer (the backbone's: 1 and 10-14)
MINING_SITE_BASE = 100              # added to the backbone's sites in the mining pass: masks independent of the training forward's
_LP_HEAD = "classification_head.predictor.mlp."


class LinkRanks(NamedTuple):
    """LinkPredictionEngine.rank(): per true pair, over its filtered candidates."""
    n_greater: Tensor   # [Q] int32: candidates scoring above the true pair
    n_equal: Tensor     # [Q] int32: candidates scoring exactly the true pair's logit
    rank: Tensor        # [Q] float32: 1 + n_greater + n_equal / 2
    logit: Tensor       # [Q] the true pair's logit (sigmoid of it is predict()'s probability)

    @classmethod
    def from_counts(cls, n_greater: Tensor, n_equal: Tensor, logit: Tensor) -> "LinkRanks":
        """A tie sits at the mean over its orders."""
        return cls(n_greater, n_equal, 1.0 + n_greater.to(torch.float32) + 0.5 * n_equal.to(torch.float32), logit)


class LinkPredictionEngine(FullGraphEngine):
    """One link-prediction fine-tune step (Cora_LP / CiteSeer_LP, src/finetune/finetune.py:181-211) as an explicit kernel sequence.

    The reference's training batch is: a no-grad train-mode embedding pass over the message-passing graph (train_pos) to mine hard
    negatives, a second full forward, the MLPLinkPredictor over [pos | neg], BCE (mean), backward, AdamW.  Here:
      mining_forward()   the first pass -- the shared encoder + backbone launches with dropout sites MINING_SITE_BASE higher,
                         BatchNorm in batch statistics updating the running ones, counted in num_batches_tracked (twice per step, as on
                         the module path); LinkPredictionHardNegativeMiner runs on its output unchanged
      step(pos, neg)     the pairs into a preallocated buffer, the training forward, the fused scorer (gmp_lp_score_fwd: the [K, 768]
                         features never leave LDS), gmp_sigmoid_bce_sum_fwd_bwd, gmp_lp_score_bwd (head gradients straight into the flat
                         buffer, per-pair g_hs / g_hd), csr_build + two segment_sums onto the nodes, then the shared backbone
                         backward (side-stream fork, gates) and AdamW with the reference's groups.  Nothing is read back.
    The module stays the owner of the parameters (views into the flat buffer), so evaluation and checkpoints go through it."""

    def __init__(self, model: FinetuneGNN, x: Tensor, message_passing_edges: Tensor, device, seed: int = 0, max_pairs: int = 512) -> None:
        super().__init__(model, x, message_passing_edges, device, seed)
        self._pairs: Optional[Tensor] = None
        self._grow(max_pairs)

    def _grow(self, kmax: int) -> None:
        dev, lib, N = self.device, self.lib, self.N
        ws = lambda n: torch.empty(max(int(n), 16), dtype=torch.uint8, device=dev)
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
        self.kmax = kmax
        self.pair_buf = torch.empty(2 * kmax, dtype=torch.int64, device=dev)      # step k's pairs: the first 2 K words, viewed [2, K]
        self.labels = torch.empty(kmax, device=dev)
        self.act = torch.empty(kmax, H, device=dev)
        self.logit, self.probs, self.g_logit = (torch.empty(kmax, device=dev) for _ in range(3))
        self.g_hs, self.g_hd = torch.empty(kmax, H, device=dev), torch.empty(kmax, H, device=dev)
        self.score_fwd_ws = ws(lib.gmp_lp_score_fwd_workspace_bytes(kmax))
        self.score_bwd_ws = ws(lib.gmp_lp_score_bwd_workspace_bytes(kmax))
        self.pair_loss_ws = ws(lib.gmp_loss_workspace_bytes(kmax))
        self.pair_csr = [i32(N + 1), i32(kmax), i32(kmax), i32(N + 1), i32(kmax), i32(kmax), i32(1)]
        self.pair_csr_ws = ws(lib.gmp_csr_build_workspace_bytes(N, kmax))

    # ------------------------------------------------------------------ forward: the base's, encoder + backbone only (the scorer runs in the step)
    def mining_forward(self) -> Tensor:
        """The reference's no-grad embedding pass (finetune.py:181-190) in the model's mode.  Returns the engine's own [N, 256] buffer: the
        next forward overwrites it."""
        self._site_base = MINING_SITE_BASE
        try:
            return self.forward()
        finally:
            self._site_base = 0

    # ------------------------------------------------------------------ one optimisation step
    def step(self, pos_edges: Tensor, neg_edges: Tensor, apply_update: bool = True) -> None:
        """loss = BCE(scorer(h, [pos | neg]), [1 | 0]) (mean); backward; AdamW.  pos / neg int64 [2, *] on the device."""
        P_, Q = int(pos_edges.size(1)), int(neg_edges.size(1))
        K = P_ + Q
        self._infer_loss = None
        if K == 0:
            raise ValueError("LinkPredictionEngine.step: no pairs")
        if K > self.kmax:
            self._grow(max(K, 2 * self.kmax))
        pairs = self.pair_buf[:2 * K].view(2, K)
        pairs[:, :P_].copy_(pos_edges)
        if Q:
            pairs[:, P_:].copy_(neg_edges)
        self.labels[:P_].fill_(1.0)
        if Q:
            self.labels[P_:K].fill_(0.0)
        self._pairs, self.num_targets = pairs, K
        self._enqueue(apply_update, forked=self.fork_wgrads)
        self.step_count += 1

    def _head_backward(self, st: int) -> None:
        """Scorer, loss and their backward after forward(): d loss / d h[GNN_NUM_LAYERS] into gA."""
        lib, N, P, g = self.lib, self.N, self._P, self.grad.data_ptr()
        pairs, labels = self._pairs, self.labels
        K = int(pairs.size(1))
        src, dst = pairs.data_ptr(), pairs.data_ptr() + 8 * K
        p = self.dropout_p if self.model.training else 0.0
        seed = (self.seed * 1000003 + self.step_count) & (2 ** 64 - 1)
        hL = self.h[GNN_NUM_LAYERS].data_ptr()
        self.g_scale.fill_(1.0 / K)
        self._chk(lib.gmp_lp_score_fwd(hL, src, dst, N, K, H, H, P(_LP_HEAD + "0.weight"), P(_LP_HEAD + "0.bias"), P(_LP_HEAD + "3.weight"),
                                       P(_LP_HEAD + "3.bias"), self.act.data_ptr(), self.logit.data_ptr(), p, seed, LP_SCORER_SITE,
                                       self.score_fwd_ws.data_ptr(), self.score_fwd_ws.numel(), st), "lp score")
        self._chk(lib.gmp_sigmoid_bce_sum_fwd_bwd(self.logit.data_ptr(), labels.data_ptr(), K, self.g_scale.data_ptr(), self.loss_sum.data_ptr(),
                                                  self.probs.data_ptr(), self.g_logit.data_ptr(), self.pair_loss_ws.data_ptr(), self.pair_loss_ws.numel(), st),
                  "lp bce")
        self._chk(lib.gmp_lp_score_bwd(hL, src, dst, N, K, H, H, P(_LP_HEAD + "0.weight"), P(_LP_HEAD + "3.weight"), self.act.data_ptr(),
                                       self.g_logit.data_ptr(), p, seed, LP_SCORER_SITE, g + 4 * self._G(_LP_HEAD + "0.weight"),
                                       g + 4 * self._G(_LP_HEAD + "0.bias"), g + 4 * self._G(_LP_HEAD + "3.weight"), g + 4 * self._G(_LP_HEAD + "3.bias"),
                                       0, self.g_hs.data_ptr(), self.g_hd.data_ptr(), self.score_bwd_ws.data_ptr(), self.score_bwd_ws.numel(), st),
                  "lp score bwd")
        # the pair scatter: g_h[i] = sum of g_hs over pairs from i + sum of g_hd over pairs to i (fixed order, operators.lp_edge_features)
        rowptr, col, perm, rowptr_t, col_t, perm_t, status = (t.data_ptr() for t in self.pair_csr)
        self._chk(lib.gmp_csr_build(pairs.data_ptr(), N, K, rowptr, col, perm, rowptr_t, col_t, perm_t, status, self.pair_csr_ws.data_ptr(),
                                    self.pair_csr_ws.numel(), st), "pair csr")
        self._chk(lib.gmp_segment_sum(self.g_hs.data_ptr(), rowptr_t, perm_t, self.gA.data_ptr(), N, H, 0, 0, st), "g_h from sources")
        self._chk(lib.gmp_segment_sum(self.g_hd.data_ptr(), rowptr, perm, self.gA.data_ptr(), N, H, 0, 1, st), "g_h from destinations")

    # ------------------------------------------------------------------ inference
    def predict(self, edges: Tensor, labels: Optional[Tensor] = None, embeddings: Optional[Tensor] = None) -> Tensor:
        """Eval-mode probabilities [K] of the pairs edges [2, K] (int64, on the device): the fused scorer with p = 0 over the backbone's
        eval-mode output.  embeddings: the result of an embed() no forward has overwritten since -- an evaluation pass embeds once and scores
        every batch of pairs against it (the parameters do not change within a pass); an embedding that a later forward or step has overwritten
        is refused.  None: embed() first.  With labels, loss() then returns the mean BCE.  Changes nothing a training step reads."""
        K = int(edges.size(1))
        if K == 0:
            raise ValueError("LinkPredictionEngine.predict: no pairs")
        hL = self._embeddings("predict", embeddings)
        if K > self.kmax:
            self._grow(max(K, 2 * self.kmax))
        lib, P, st = self.lib, self._P, torch.cuda.current_stream(self.device).cuda_stream
        pairs = edges.contiguous()
        self._chk(lib.gmp_lp_score_fwd(hL.data_ptr(), pairs.data_ptr(), pairs.data_ptr() + 8 * K, self.N, K, H, H, P(_LP_HEAD + "0.weight"),
                                       P(_LP_HEAD + "0.bias"), P(_LP_HEAD + "3.weight"), P(_LP_HEAD + "3.bias"), self.act.data_ptr(), self.logit.data_ptr(),
                                       0.0, 0, LP_SCORER_SITE, self.score_fwd_ws.data_ptr(), self.score_fwd_ws.numel(), st), "lp score (eval)")
        self._infer_loss = None
        if labels is None:
            return ops.sigmoid_fwd(self.logit[:K])
        probs, loss_sum, g_scale = torch.empty(K, device=self.device), torch.zeros(1, device=self.device), torch.ones(1, device=self.device)
        lab = labels.to(torch.float32).contiguous()
        self._chk(lib.gmp_sigmoid_bce_sum_fwd_bwd(self.logit.data_ptr(), lab.data_ptr(), K, g_scale.data_ptr(), loss_sum.data_ptr(), probs.data_ptr(),
                                                  self.g_logit.data_ptr(), self.pair_loss_ws.data_ptr(), self.pair_loss_ws.numel(), st), "lp bce (eval)")
        self._infer_loss = (loss_sum, K)
        return probs

    def _embeddings(self, who: str, embeddings: Optional[Tensor]) -> Tensor:
        """embed() if none are given; given ones must be this engine's, and no forward may have overwritten them since."""
        hL = self.embed() if embeddings is None else embeddings
        if hL.data_ptr() != self.h[GNN_NUM_LAYERS].data_ptr() or hL.size(0) != self.N:
            raise ValueError(f"LinkPredictionEngine.{who}: embeddings must be the result of this engine's embed()")
        if self._embed_gen != self._fwd_gen:
            raise ValueError(f"LinkPredictionEngine.{who}: a forward or a step has overwritten these embeddings since embed() returned them")
        return hL

    def _ranking_inputs(self, who: str, embeddings: Optional[Tensor], filter_edges: Optional[Tensor]):
        """The embeddings under predict()'s rules, the scorer's weights and the filter's source-major CSR (cached per tensor)."""
        hL, mlp = self._embeddings(who, embeddings), self.model.classification_head.predictor.mlp
        return hL, (mlp[0].weight, mlp[0].bias, mlp[3].weight, mlp[3].bias), None if filter_edges is None else filter_edges.to(self.device)

    def rank(self, edges: Tensor, filter_edges: Optional[Tensor] = None, embeddings: Optional[Tensor] = None) -> "LinkRanks":
        """Every true pair of edges [2, Q] (int64, on the device) ranked against all N nodes as destinations (gmp_lp_rank: no pair list,
        no per-candidate logit in memory).  Left out of a pair's candidates: its source, its destination, and every c with (source, c) in
        filter_edges [2, E] (the known positives; its CSR is built once per tensor).  embeddings: as for predict().  Eval mode; changes
        nothing a training step reads."""
        if int(edges.size(1)) == 0:
            raise ValueError("LinkPredictionEngine.rank: no pairs")
        hL, weights, filt = self._ranking_inputs("rank", embeddings, filter_edges)
        logit, n_greater, n_equal = OP.lp_rank(hL, edges, *weights, filter_edges=filt)
        return LinkRanks.from_counts(n_greater, n_equal, logit)

    def top_k(self, sources: Tensor, k: int, filter_edges: Optional[Tensor] = None, embeddings: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
        """The k (1 <= k <= 64) most probable destinations of every node of sources [Q] (int64, on the device) among all N nodes
        (gmp_lp_topk): (idx [Q, k] int64, probability [Q, k]), best first, ties to the lower index, the source itself and its
        filter_edges destinations left out; -1 / probability 0 where a source has fewer than k candidates.  Otherwise as rank()."""
        if int(sources.numel()) == 0:
            raise ValueError("LinkPredictionEngine.top_k: no sources")
        hL, weights, filt = self._ranking_inputs("top_k", embeddings, filter_edges)
        idx, logit = OP.lp_topk(hL, sources, k, *weights, filter_edges=filt)
        return idx, ops.sigmoid_fwd(logit.view(-1)).view_as(logit)

    # ------------------------------------------------------------------ read-backs
    def probabilities(self) -> Tensor:
        """sigmoid(logit) of the last step's pairs, [pos | neg] order."""
        return self.probs[:self.num_targets]

    def labels_of_step(self) -> Tensor:
        return self.labels[:self.num_targets]


GC_HEAD_SITE = 41                   # dropout site of the graph-classification head's hidden layer (the backbone's: 1 and 10-14, the scorer's: 40)
_GC_HEAD = "classification_head.mlp."


class GraphClassificationEngine(BackboneEngine):
    """One graph-classification fine-tune step (ENZYMES / PTC_MR, src/finetune/finetune.py:136-158 + 283-331) as an explicit kernel sequence.

    The reference's training batch is 32 graphs (about 1,000 rows for ENZYMES, 450 for PTC_MR): forward, global_mean_pool, the
    256 -> 128 -> C head, cross-entropy (C > 2) or BCE-with-logits on logits[:, 1] (C == 2), backward, AdamW.  The batch -- and with it the
    number of rows, edges and graphs -- changes every step, so unlike the full-graph engines this one works on CAPACITIES:
      buffers            activations, gradients, the CSR and the workspaces are sized for max_nodes / max_edges / max_graphs and regrown by
                         doubling when a batch exceeds them (_alloc); every row-major buffer has leading dimension 256 / 512, so a step
                         uses its first N rows and rows a larger previous batch left behind are never read
      step(batch)        the batch's x into the padded [N, dpad] input (the padding columns stay zero), gmp_csr_build on the device into the
                         preallocated CSR, seg_ptr = [0, N], the shared backbone forward, the fused head (gmp_gc_head_fwd: pooling,
                         both layers, the loss and d loss / d logits in one kernel + the loss sum), gmp_gc_head_bwd (head gradients straight
                         into the flat buffer, every row of d loss / d h written), then the shared backbone backward (side-stream
                         fork, gates) and AdamW.  Nothing is read back; no captured replay (shapes change every step).
    Which tensors train comes from the model (requires_grad as FinetuneGNN set it: the encoder is frozen for ENZYMES, the backbone for
    linear_probe), the learning rates are those of FinetuneGNN.param_groups.  A frozen tensor is never touched by the optimizer -- no update,
    no weight decay -- and stays bitwise what it was.  The backward still runs through frozen layers (no launch is skipped);
    gradient(name) of a frozen tensor returns zeros.
    The module stays the owner of the parameters (views into the flat buffer), so evaluation and checkpoints go through it.
    Measured (MI355X, scripts/bench_gc_finetune.py, profiles/README.md GC fine-tune): 0.80 ms per 32-graph ENZYMES-shaped step against 3.28 on the
    module path, 0.88 against 2.98 at the PTC_MR shape; about 120 launches per step, host-bound."""

    def __init__(self, model: FinetuneGNN, device, seed: int = 0, max_nodes: int = 2048, max_edges: int = 8192, max_graphs: int = 64) -> None:
        super().__init__(model, int(model.input_encoder.linear.weight.size(1)), device, seed)
        self.classes = int(model.classification_head.mlp[3].weight.size(0))
        self.B, self._unlabelled = 0, False
        self._ptr32: Optional[Tensor] = None                     # the loaded batch's graph offsets; None: no batch loaded yet
        self._y: Optional[Tensor] = None
        self._alloc(max(int(max_nodes), 1), max(int(max_edges), 1), max(int(max_graphs), 1))

    def _alloc(self, cap_n: int, cap_e: int, cap_b: int) -> None:
        dev, lib = self.device, self.lib
        f = lambda *s: torch.empty(*s, device=dev)
        i32 = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
        ws = lambda n: torch.empty(max(int(n), 16), dtype=torch.uint8, device=dev)
        self.cap_n, self.cap_e, self.cap_b = cap_n, cap_e, cap_b
        self.x = torch.zeros(cap_n, self.dpad, device=dev)
        self._alloc_rows(cap_n)
        self.csr = ops.CSR(i32(cap_n + 1), i32(cap_e), i32(cap_e), i32(cap_n + 1), i32(cap_e), i32(cap_e), cap_n, torch.zeros(1, dtype=torch.int32, device=dev))
        self.csr_ws = ws(lib.gmp_csr_build_workspace_bytes(cap_n, cap_e))
        self.pooled, self.act = f(cap_b, H), f(cap_b, self.model.classification_head.mlp[0].weight.size(0))
        self.logits_b, self.g_logits = f(cap_b, self.classes), f(cap_b, self.classes)
        self.head_ws = ws(lib.gmp_gc_head_fwd_workspace_bytes(cap_b))

    # ------------------------------------------------------------------ this step's batch into the engine's buffers
    def _load(self, batch, need_y: bool = True) -> None:
        if batch.x.device.type != self.device.type:
            batch = batch.to(self.device)
        N, E, B = batch.num_nodes, batch.num_edges, batch.num_graphs
        if N < 1 or B < 1:
            raise ValueError("GraphClassificationEngine: an empty batch")
        if batch.x.size(1) != self.d_in:
            raise ValueError(f"GraphClassificationEngine: the batch has {batch.x.size(1)} features, the encoder {self.d_in}")
        if need_y and (batch.y is None or batch.y.numel() != B):
            raise ValueError("GraphClassificationEngine: the batch needs one label per graph")
        if N > self.cap_n or E > self.cap_e or B > self.cap_b:
            grown = lambda need, cap: max(need, 2 * cap) if need > cap else cap
            self._alloc(grown(N, self.cap_n), grown(E, self.cap_e), grown(B, self.cap_b))
        self.N, self.B, self.num_targets = N, B, B
        self._unlabelled = False
        self.seg_ptr[1:].fill_(N)                                # the one BatchNorm segment [0, N)
        self.x[:N, :self.d_in].copy_(batch.x)
        ei, c = batch.edge_index.contiguous(), self.csr
        st = torch.cuda.current_stream(self.device).cuda_stream
        self._chk(self.lib.gmp_csr_build(ei.data_ptr() if E else None, N, E, c.rowptr.data_ptr(), c.col.data_ptr(), c.perm.data_ptr(),
                                         c.rowptr_t.data_ptr(), c.col_t.data_ptr(), c.perm_t.data_ptr(), c.status.data_ptr(),
                                         self.csr_ws.data_ptr(), self.csr_ws.numel(), st), "batch csr")
        # (a cast on the device: Batch.ptr32 would upload the host offsets again, one blocking copy per step)
        self._ptr32 = batch.ptr.to(torch.int32)
        self._y = batch.y.to(torch.int64).contiguous() if (need_y or (batch.y is not None and batch.y.numel() == B)) else None

    # ------------------------------------------------------------------ forward: encoder + backbone (the head runs in the step)
    def forward(self, batch=None) -> Tensor:
        """The backbone's output for `batch` (or for the batch already loaded) in the model's mode: the first N rows of the engine's own
        buffer, which the next forward overwrites."""
        self._load_or_keep(batch)
        return super().forward()[:self.N]

    def _load_or_keep(self, batch, need_y: bool = True) -> None:
        if batch is not None:
            self._load(batch, need_y)
        elif self._ptr32 is None:
            raise ValueError("GraphClassificationEngine: no batch has been loaded yet")

    def evaluate(self, batch=None) -> Tensor:
        """logits [B, C] of `batch` (or of the batch already loaded) in the model's mode (forward + the fused head; loss() then holds the batch's mean loss)."""
        self.forward(batch)
        self._head_forward(torch.cuda.current_stream(self.device).cuda_stream)
        return self.logits()

    # ------------------------------------------------------------------ inference
    def embed(self, batch=None) -> Tensor:
        """The backbone's eval-mode output rows [N, 256] for `batch` (or for the batch already loaded), whatever model.training is.  Loads the
        batch and regrows the capacities as step does; labels are not needed.  The engine's own buffer: the next forward overwrites it."""
        self._load_or_keep(batch, need_y=False)
        return super().embed()

    def predict(self, batch) -> Tensor:
        """Eval-mode logits [B, C] of `batch` (the folded backbone + the fused head with p = 0).  With labels (batch.y) loss() then holds the
        batch's mean loss; without, the fused head runs against zero labels and loss() raises until a labelled batch has been loaded.  Like evaluate(), it replaces the loaded
        batch (N, B, the CSR: forward() / embed() without an argument then act on this one) and the last loss; parameters, optimizer state,
        running statistics and counters stay as they are, and a step reloads its own batch, so training is unaffected."""
        self._load(batch, need_y=False)
        if self._y is None:
            self._y, self._unlabelled = torch.zeros(self.B, dtype=torch.int64, device=self.device), True
        self._infer_forward()
        self._head_forward(torch.cuda.current_stream(self.device).cuda_stream, p=0.0)
        return self.logits()

    # ------------------------------------------------------------------ one optimisation step
    def step(self, batch, apply_update: bool = True) -> None:
        """loss = classification_loss(model(batch), batch.y) (mean over the batch's graphs); backward; AdamW.  `batch` is the loader's Batch
        (x, edge_index, ptr32, y), moved to the device if it is not there yet."""
        self._load(batch)
        self._enqueue(apply_update, forked=self.fork_wgrads)
        self.step_count += 1

    def _head_args(self):
        p = self.dropout_p if self.model.training else 0.0
        return p, (self.seed * 1000003 + self.step_count) & (2 ** 64 - 1)

    def _head_forward(self, st: int, p: Optional[float] = None) -> None:
        lib, P = self.lib, self._P
        p_step, seed = self._head_args()
        p = p_step if p is None else p
        self.g_scale.fill_(1.0 / self.B)
        self._chk(lib.gmp_gc_head_fwd(self.h[GNN_NUM_LAYERS].data_ptr(), H, self._ptr32.data_ptr(), self.N, self.B, H, self.act.size(1), self.classes,
                                      P(_GC_HEAD + "0.weight"), P(_GC_HEAD + "0.bias"), P(_GC_HEAD + "3.weight"), P(_GC_HEAD + "3.bias"),
                                      self._y.data_ptr(), self.g_scale.data_ptr(), self.pooled.data_ptr(), self.act.data_ptr(),
                                      self.logits_b.data_ptr(), self.loss_sum.data_ptr(), self.g_logits.data_ptr(), p, seed, GC_HEAD_SITE,
                                      self.head_ws.data_ptr(), self.head_ws.numel(), st), "gc head")

    def _head_backward(self, st: int) -> None:
        """Head, loss and their backward after forward(): d loss / d h[GNN_NUM_LAYERS] into every row of gA."""
        lib, P, g = self.lib, self._P, self.grad.data_ptr()
        p, seed = self._head_args()
        self._head_forward(st)
        self._chk(lib.gmp_gc_head_bwd(self._ptr32.data_ptr(), self.N, self.B, H, self.act.size(1), self.classes, P(_GC_HEAD + "0.weight"),
                                      P(_GC_HEAD + "3.weight"), self.pooled.data_ptr(), self.act.data_ptr(), self.g_logits.data_ptr(), p, seed,
                                      GC_HEAD_SITE, g + 4 * self._G(_GC_HEAD + "0.weight"), g + 4 * self._G(_GC_HEAD + "0.bias"),
                                      g + 4 * self._G(_GC_HEAD + "3.weight"), g + 4 * self._G(_GC_HEAD + "3.bias"), self.gA.data_ptr(), H, st),
                  "gc head bwd")

    # ------------------------------------------------------------------ read-backs
    def loss(self) -> float:
        """Mean loss of the last step (synchronises; checks the gate and slab time-out words as every engine does, and the CSR build's
        count of edge endpoints outside the batch)."""
        if self._unlabelled:
            raise L.GnnmpError("fine-tune engine: the last predict had no labels (batch.y): there is no loss to report")
        v = super().loss()
        if int(self.csr.status.item()) != 0:
            raise L.GnnmpError(f"fine-tune engine: {int(self.csr.status.item())} edge endpoints outside the batch's nodes")
        return v

    def logits(self) -> Tensor:
        """The last step's logits [B, C] (a view of the engine's buffer: the next step overwrites it)."""
        return self.logits_b[:self.B]

    def gradient(self, name: str) -> Tensor:
        g = super().gradient(name)
        return g if dict(self.model.named_parameters())[name].requires_grad else torch.zeros_like(g)
