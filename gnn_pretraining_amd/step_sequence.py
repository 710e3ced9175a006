"""The pre-training step launched kernel by kernel from Python (StepEngine(native=False)): the readable reference of csrc/step.hip.
Same entry points, same order, same buffers, same streams and event waits as the native executor's unfused path, so the two give
bitwise the same parameters (tests/test_gpu_engine.py).  The engine owns the arena, the uploads and the plan helpers; this module
only reads them.  Nothing here keeps a "current" stream or workspace: every helper takes the Lane its launches go to."""
from __future__ import annotations

import ctypes as C
from typing import List, NamedTuple, Optional

import torch
from torch import Tensor

from . import _lib as L
from .constants import DOMAIN_DIMENSIONS, GRAPH_PROPERTY_DIM
from .engine import DA_HIDDEN, H, NN, NT, SEG_CSR_MAX_EDGES, SEG_CSR_MAX_ROWS, TN, StepEngine, _i32, _i64
from .models.gnn import GNN_NUM_LAYERS
from .step_host import StepInputs, StepPlan


class Lane(NamedTuple):
    """Where one chain of launches goes: the stream's handle and the scratch no chain on another stream is using."""
    st: int
    gemm_ws: Tensor
    loss_ws: Tensor


class LaunchSequence:
    def __init__(self, eng: StepEngine) -> None:
        self.e, self.lib, self.chk, self.hd = eng, eng.lib, eng._chk, eng.hd
        self.hL, self.gH, self.tg = eng.h[GNN_NUM_LAYERS], eng.gA, eng.task_grads.data_ptr()
        self.gW2 = torch.empty(eng.max_rows, 2 * H, device=eng.device)          # g_z1 (the native executor has gz1_l)

    def run(self, p: StepPlan, inp: StepInputs) -> None:
        """Forward, heads and backward of one uploaded step; per-task gradients and loss sums are left where the optimizer reads them."""
        self.heads(p, inp, self.forward(p, inp))
        self.backward(self._main()[1], p, inp)

    def _main(self):
        main = torch.cuda.current_stream(self.e.device)
        return main, Lane(main.cuda_stream, self.e.gemm_ws, self.e.task_loss_ws[0])

    # ---- launch helpers ----------------------------------------------------------------------------
    def _gemm(self, ln: Lane, mode, A, B, bias, Cc, M, N, K, lda, ldb, ldc, relu=False) -> None:
        self.chk(self.lib.gmp_gemm_f32(mode, A, B, bias, Cc, M, N, K, lda, ldb, ldc, 1.0, 0, int(relu), None, 0, ln.st), "gemm")

    def _gemm_g(self, ln: Lane, mode, A, B, bias, Cc, rows, boff, biasoff, coff, asum, asumoff, M_tn, N, K, lda, ldb, ldc, relu=False) -> None:
        opt = lambda xs: None if xs is None else _i64(xs)
        self.chk(self.lib.gmp_gemm_f32_grouped(mode, A, B, bias, Cc, len(rows) - 1, _i32(rows), opt(boff), opt(biasoff), opt(coff), asum, opt(asumoff),
                                               M_tn, N, K, lda, ldb, ldc, 1.0, 0, int(relu), ln.gemm_ws.data_ptr() if mode == TN else None,
                                               ln.gemm_ws.numel(), ln.st), "gemm_grouped")

    def _bn_cfg(self, relu: bool, dropout: bool, site: int) -> L.BnConfig:
        p = self.e.dropout_p if (dropout and self.e.model.training) else 0.0
        return L.BnConfig(int(self.e.model.training), int(relu), 1e-5, 0.1, p, self.e.dropout_seed, site)

    def _drop(self, ln: Lane, src: Tensor, dst: Tensor, numel: int, site: int, p: Optional[float] = None) -> Tensor:
        """dropout(src) -> dst (returns the tensor holding the result; p == 0 aliases src)."""
        p = self.e.dropout_p if p is None else p
        if not self.e.model.training or p <= 0:
            return src
        self.chk(self.lib.gmp_dropout_fwd(src.data_ptr(), dst.data_ptr(), numel, p, self.e.dropout_seed, site, ln.st), "dropout")
        return dst

    def _relu_drop_bwd(self, ln: Lane, g: Tensor, act: Tensor, out: Tensor, numel: int, site: int, p: Optional[float] = None) -> None:
        p = (self.e.dropout_p if p is None else p) if self.e.model.training else 0.0
        self.chk(self.lib.gmp_relu_dropout_bwd(g.data_ptr(), act.data_ptr(), out.data_ptr(), numel, p, self.e.dropout_seed, site, ln.st), "relu_dropout_bwd")

    def _bn_fwd(self, ln: Lane, p: StepPlan, cfg, x, res, dom, cols, gamma, beta, rm, rv, mean, rstd, out, what: str) -> None:
        """BatchNorm over the step's segments (per domain where `dom` is given); res: the residual added before the ReLU."""
        ws = self.e.bn_ws
        self.chk(self.lib.gmp_bn_fwd(x.data_ptr(), res, p.d32["seg_ptr"], dom, p.S, p.max_seg, p.N, cols, gamma, beta, rm.data_ptr(), rv.data_ptr(),
                                     mean.data_ptr(), rstd.data_ptr(), out.data_ptr(), C.byref(cfg), ws.data_ptr(), ws.numel(), ln.st), what)

    def _bn_bwd(self, ln: Lane, p: StepPlan, cfg, g, x, res, dom, cols, gamma, beta, rm, rv, mean, rstd, g_out, group_ptr, tg_gamma, tg_beta, groups, what) -> None:
        """Its backward; the weight / bias gradients of segment group k go to task_grads at float offsets tg_gamma[k] / tg_beta[k]."""
        ws = self.e.bn_ws
        self.chk(self.lib.gmp_bn_bwd(g.data_ptr(), x.data_ptr(), res, p.d32["seg_ptr"], dom, p.S, p.max_seg, p.N, cols, gamma, beta, rm.data_ptr(),
                                     rv.data_ptr(), mean.data_ptr(), rstd.data_ptr(), g_out.data_ptr(), self.tg, self.tg, group_ptr, tg_gamma, tg_beta,
                                     groups, C.byref(cfg), ws.data_ptr(), ws.numel(), ln.st), what)

    # ---- forward -----------------------------------------------------------------------------------
    def forward(self, p: StepPlan, inp: StepInputs) -> "torch.cuda.Event":
        """Encoders and the backbone on the current stream, both CSR builds beside the encoders on the aux stream.  Returns the event
        behind the link-prediction CSR: its head and the backward wait on it."""
        e, lib, chk, N, P, D, c = self.e, self.lib, self.chk, p.N, self.e._P, self.e.domains, self.e.csr
        main, ln = self._main()
        ev_csr, ev_lpcsr = self._csr_builds(p, main)
        w_off, b_off = ([e.off[f"input_encoders.{d}.linear.{k}"] for d in D] for k in ("weight", "bias"))
        chk(lib.gmp_encoder_fwd(inp.x_all.data_ptr(), inp.x_all.size(0), N, p.S, p.d32["src_row"], p.d32["seg_ptr"], p.d32["seg_dom"], p.d64.get("rowmask"),
                                p.d32["tiles"], p.num_tiles, e.flat.data_ptr(), len(D), _i64(w_off), _i64(b_off), _i32([DOMAIN_DIMENSIONS[d] for d in D]),
                                e.dpad, e.z0.data_ptr(), ln.st), "encoder_fwd")
        e0 = f"input_encoders.{D[0]}."
        self._bn_fwd(ln, p, self._bn_cfg(True, True, 1), e.z0, None, p.d32["seg_dom"], H, P(e0 + "batch_norm.weight"), P(e0 + "batch_norm.bias"),
                     e.enc_rm, e.enc_rv, e.enc_mean, e.enc_rstd, e.h[0], "bn_fwd encoders")
        if "node_feat_mask" in e.tasks and p.nfm_rows[-1]:
            M = p.nfm_rows[-1]
            chk(lib.gmp_row_gather(e.h[0].data_ptr(), p.d64["nfm_idx"], None, self.hd["nfm_tgt"].data_ptr(), M, N, H, ln.st), "nfm target")
            chk(lib.gmp_row_fill(e.h[0].data_ptr(), p.d64["nfm_idx"], P("mask_token"), M, N, H, 1, ln.st), "nfm mask")
        main.wait_event(ev_csr)
        for l in range(GNN_NUM_LAYERS):
            pre, layer = f"gnn_backbone.layers.{l}.", e.model.gnn_backbone.layers[l]
            bn1, bn2 = layer.gin_conv.nn[1], layer.batch_norm
            chk(lib.gmp_gin_aggregate_fwd(e.h[l].data_ptr(), c[0].data_ptr(), c[1].data_ptr(), P(pre + "gin_conv.eps"), e.a[l].data_ptr(), N, H, ln.st), "aggregate")
            self._gemm(ln, NT, e.a[l].data_ptr(), P(pre + "gin_conv.nn.0.weight"), P(pre + "gin_conv.nn.0.bias"), e.z1[l].data_ptr(), N, 2 * H, H, H, H, 2 * H)
            self._bn_fwd(ln, p, self._bn_cfg(True, False, 0), e.z1[l], None, None, 2 * H, P(pre + "gin_conv.nn.1.weight"), P(pre + "gin_conv.nn.1.bias"),
                         bn1.running_mean, bn1.running_var, e.stat["m1"][l], e.stat["s1"][l], e.r1[l], "bn1")
            self._gemm(ln, NT, e.r1[l].data_ptr(), P(pre + "gin_conv.nn.3.weight"), P(pre + "gin_conv.nn.3.bias"), e.z2[l].data_ptr(), N, H, 2 * H, 2 * H, 2 * H, H)
            self._bn_fwd(ln, p, self._bn_cfg(True, True, 10 + l), e.z2[l], e.h[l].data_ptr(), None, H, P(pre + "batch_norm.weight"), P(pre + "batch_norm.bias"),
                         bn2.running_mean, bn2.running_var, e.stat["m2"][l], e.stat["s2"][l], e.h[l + 1], "bn2")
        return ev_lpcsr

    def _csr_builds(self, p: StepPlan, main):
        """Both CSR builds depend only on the uploaded indices: they run on the aux stream.  Returns (event behind the stacked graph's
        CSR, event behind the link-prediction one)."""
        e, lib, chk, N = self.e, self.lib, self.chk, p.N
        ptrs = lambda bufs: [b.data_ptr() for b in bufs]
        ev_up = torch.cuda.Event(); ev_up.record(main)
        e.aux_stream.wait_event(ev_up)
        with torch.cuda.stream(e.aux_stream):
            ast = e.aux_stream.cuda_stream
            if p.max_seg <= SEG_CSR_MAX_ROWS and p.max_seg_edges <= SEG_CSR_MAX_EDGES:      # block diagonal: one workgroup per segment
                chk(lib.gmp_csr_build_segmented(p.d64["edge_index"], N, p.E, p.d32["seg_ptr"], p.d32["seg_eptr"], p.S, p.max_seg,
                                                p.max_seg_edges, *ptrs(e.csr), e.csr_status.data_ptr(), ast), "csr_build_segmented")
            else:
                chk(lib.gmp_csr_build(p.d64["edge_index"], N, p.E, *ptrs(e.csr), e.csr_status.data_ptr(), e.csr_ws.data_ptr(),
                                      e.csr_ws.numel(), ast), "csr_build")
            ev_csr = torch.cuda.Event(); ev_csr.record(e.aux_stream)
            if "link_pred" in e.tasks:
                if e._lp_segmented(p):
                    chk(lib.gmp_csr_build_segmented(p.d64["lp_edges"], p.lp_rows_end, p.lp_K, p.d32["lp_seg_ptr"], p.d32["lp_seg_eptr"], p.lp_S,
                                                    p.lp_max_rows, p.lp_max_edges, *ptrs(e.lp_csr), e.lp_csr_status.data_ptr(), ast), "lp csr (segmented)")
                else:
                    chk(lib.gmp_csr_build(p.d64["lp_edges"], N, p.lp_K, *ptrs(e.lp_csr), e.lp_csr_status.data_ptr(), e.lp_csr_ws.data_ptr(),
                                          e.lp_csr_ws.numel(), ast), "lp csr")
            ev_lpcsr = torch.cuda.Event(); ev_lpcsr.record(e.aux_stream)
        return ev_csr, ev_lpcsr

    # ---- heads -------------------------------------------------------------------------------------
    def heads(self, p: StepPlan, inp: StepInputs, ev_lpcsr) -> None:
        """Every task's head on the stream the engine packed it onto (the ones on other streams first, the ones on main last), each
        with a lane of its own; main then waits for all of them."""
        e = self.e
        self.gH[:p.N].zero_()
        main = torch.cuda.current_stream(e.device)
        ev_fwd = torch.cuda.Event(); ev_fwd.record(main)
        done = []
        for ti in sorted(range(e.T), key=lambda i: e.task_streams[i] is None):
            t, ts = e.tasks[ti], main if e.task_streams[ti] is None else e.task_streams[ti]
            if ts is not main:
                ts.wait_event(ev_fwd)
            if t == "link_pred":
                ts.wait_event(ev_lpcsr)
            with torch.cuda.stream(ts):
                # (gs: the device scalar 1/size_t = d total_t / d loss_sum; ls: the task's loss-sum slot)
                self.HEADS[t](self, Lane(ts.cuda_stream, e.task_gemm_ws[ti], e.task_loss_ws[ti]), p, inp, ti,
                              e.scal.data_ptr() + 4 * ti, e.loss_sums.data_ptr() + 4 * ti)
                if ts is not main:
                    ev = torch.cuda.Event(); ev.record(ts)
                    done.append(ev)
        for ev in done:
            main.wait_event(ev)
        main.wait_event(ev_lpcsr)

    def _head_tensors(self, ti: int, task: str):
        """A per-domain two-layer head: (w0, b0, w3, b3), each a per-domain list of offsets -- first in flat, then in task_grads."""
        per = [self.e.head_offsets(ti, f"heads.{task}.{d}.") for d in self.e.domains]
        return [[h[k][1] for h in per] for k in range(4)], [[h[k][2] for h in per] for k in range(4)]

    def _mlp2(self, ln: Lane, ti: int, task: str, x: Tensor, rows: List[int], k_in: int, k_hid: int, k_out: int, bufs) -> Tensor:
        """Per-domain two-layer MLPHead (Linear-ReLU-Dropout-Linear) over row groups; returns the tensor the second layer read."""
        y1, d1, y2 = bufs
        (w0, b0, w3, b3), _ = self._head_tensors(ti, task)
        fp = self.e.flat.data_ptr()
        self._gemm_g(ln, NT, x.data_ptr(), fp, fp, y1.data_ptr(), rows, w0, b0, None, None, None, 0, k_hid, k_in, k_in, k_in, k_hid, relu=True)
        d1 = self._drop(ln, y1, d1, rows[-1] * k_hid, 100 + ti)
        self._gemm_g(ln, NT, d1.data_ptr(), fp, fp, y2.data_ptr(), rows, w3, b3, None, None, None, 0, k_out, k_hid, k_hid, k_hid, k_out)
        return d1

    def _mlp2_bwd(self, ln: Lane, ti: int, task: str, x: Tensor, rows: List[int], k_in: int, k_hid: int, k_out: int, y1: Tensor, d1: Tensor,
                  g_out: Tensor, g_hid: Tensor, g_in: Tensor) -> None:
        """Backward of _mlp2: per-domain weight/bias gradients go straight into task_grads[ti]."""
        (w0, _, w3, _), (gw0, gb0, gw3, gb3) = self._head_tensors(ti, task)
        tg, fp = self.tg, self.e.flat.data_ptr()
        # dW3 = g_out^T d1, db3 = colsum(g_out)
        self._gemm_g(ln, TN, g_out.data_ptr(), d1.data_ptr(), None, tg, rows, None, None, gw3, tg, gb3, k_out, k_hid, 0, k_out, k_hid, k_hid)
        # g_d1 = g_out W3
        self._gemm_g(ln, NN, g_out.data_ptr(), fp, None, g_hid.data_ptr(), rows, w3, None, None, None, None, 0, k_hid, k_out, k_out, k_hid, k_hid)
        self._relu_drop_bwd(ln, g_hid, y1, g_hid, rows[-1] * k_hid, 100 + ti)
        self._gemm_g(ln, TN, g_hid.data_ptr(), x.data_ptr(), None, tg, rows, None, None, gw0, tg, gb0, k_hid, k_in, 0, k_hid, k_in, k_in)
        self._gemm_g(ln, NN, g_hid.data_ptr(), fp, None, g_in.data_ptr(), rows, w0, None, None, None, None, 0, k_in, k_hid, k_hid, k_in, k_in)

    def _nt_xent_domains(self, ln: Lane, ns: List[int], rows: List[int], z: Tensor, gz: Tensor, gs: int, ls: int, slot0: int) -> None:
        """One NT-Xent problem per domain on rows [rows[d], rows[d+1]) = [z1 ; z2]; loss sums land in scal[16+slot],
        their total in the task's loss slot."""
        ws = self.e._ntx_workspace(slot0, ns)
        self.chk(self.lib.gmp_nt_xent_grouped(z.data_ptr(), gz.data_ptr(), len(ns), _i32(list(ns)), _i64([int(r) for r in rows[:len(ns)]]), 128,
                                              float(self.e.temperature), gs, self.e.scal.data_ptr() + 4 * (16 + slot0), ls, ws.data_ptr(), ws.numel(),
                                              ln.st), "nt_xent grouped")

    # one method per task kind: head forward, loss and head backward (writes the task's rows of gH and its slots of task_grads)
    def node_feat_mask(self, ln: Lane, p: StepPlan, inp: StepInputs, ti: int, gs: int, ls: int) -> None:
        lib, chk, hd, st, N = self.lib, self.chk, self.hd, ln.st, p.N
        rows, M = p.nfm_rows, p.nfm_rows[-1]
        if M == 0:
            return
        chk(lib.gmp_row_gather(self.hL.data_ptr(), p.d64["nfm_idx"], None, hd["nfm_in"].data_ptr(), M, N, H, st), "nfm gather")
        d1 = self._mlp2(ln, ti, "node_feat_mask", hd["nfm_in"], rows, H, H, H, (hd["nfm_y1"], hd["nfm_d1"], hd["nfm_y2"]))
        chk(lib.gmp_mse_sum_fwd(hd["nfm_y2"].data_ptr(), hd["nfm_tgt"].data_ptr(), M * H, ls, ln.loss_ws.data_ptr(), ln.loss_ws.numel(), st), "mse")
        chk(lib.gmp_mse_sum_bwd(hd["nfm_y2"].data_ptr(), hd["nfm_tgt"].data_ptr(), gs, hd["nfm_g"].data_ptr(), M * H, st), "mse bwd")
        self._mlp2_bwd(ln, ti, "node_feat_mask", hd["nfm_in"], rows, H, H, H, hd["nfm_y1"], d1, hd["nfm_g"], hd["nfm_g1"], hd["nfm_y2"])
        chk(lib.gmp_row_fill(self.gH.data_ptr(), p.d64["nfm_idx"], hd["nfm_y2"].data_ptr(), M, N, H, 0, st), "nfm scatter")

    # (longer than its neighbours on purpose: the merged and the ordered arm alternate with the launches they share)
    def link_pred(self, ln: Lane, p: StepPlan, inp: StepInputs, ti: int, gs: int, ls: int) -> None:
        e, lib, chk, hd, st, N, K, tg = self.e, self.lib, self.chk, self.hd, ln.st, p.N, p.lp_K, self.tg
        hL, gH, fp = self.hL, self.gH, self.e.flat.data_ptr()
        head = e.head_offsets(ti, "heads.link_pred.predictor.")
        (w0, b0, w3, b3), (gw0, gb0, gw3, gb3) = [fp + 4 * off for _, off, _ in head], [g for _, _, g in head]
        y2, lab, gy2, gws = e.lp_y2.data_ptr(), e.lp_lab.data_ptr(), e.lp_gy2.data_ptr(), ln.gemm_ws
        chk(lib.gmp_lp_edge_features_fwd(hL.data_ptr(), p.d64["lp_edges"], hd["lp_feat"].data_ptr(), N, K, H, st), "lp feat")
        self._gemm(ln, NT, hd["lp_feat"].data_ptr(), w0, b0, hd["lp_y1"].data_ptr(), K, H, 3 * H, 3 * H, 3 * H, H, relu=True)
        # the 256 -> 1 layer as a row dot product / outer product / weighted column sum (csrc/elementwise.hip), as in csrc/step.hip
        pdrop = e.dropout_p if (e.model.training and e.dropout_p > 0) else 0.0
        dseed, site = e.dropout_seed, 100 + ti
        d1 = hd["lp_d1"] if pdrop > 0 else hd["lp_y1"]
        pos = p.d32.get("lp_pos")            # merged rows: the ordered row(s) each stands for (a dropout mask per ordered row)
        if pos is not None:
            chk(lib.gmp_lp_pair_rowdot_fwd(hd["lp_y1"].data_ptr(), w3, b3, pos, y2, K, H, pdrop, dseed, site, st), "lp pair rowdot")
            chk(lib.gmp_lp_pair_sigmoid_bce_fwd_bwd(y2, lab, pos, K, gs, ls, e.lp_p.data_ptr(), gy2, ln.loss_ws.data_ptr(), ln.loss_ws.numel(), st), "pair sigmoid+bce")
            chk(lib.gmp_lp_pair_outer_bwd(gy2, w3, hd["lp_y1"].data_ptr(), pos, hd["lp_gy1"].data_ptr(), K, H, pdrop, dseed, site, st), "lp pair outer")
        else:
            chk(lib.gmp_dropout_rowdot_fwd(hd["lp_y1"].data_ptr(), w3, b3, hd["lp_d1"].data_ptr(), y2, K, H, pdrop, dseed, site, st), "lp rowdot")
            chk(lib.gmp_sigmoid_bce_signed_sum_fwd_bwd(y2, lab, K, gs, ls, e.lp_p.data_ptr(), gy2, ln.loss_ws.data_ptr(), ln.loss_ws.numel(), st), "sigmoid+bce")
            chk(lib.gmp_outer_relu_dropout_bwd(gy2, w3, hd["lp_y1"].data_ptr(), hd["lp_gy1"].data_ptr(), K, H, pdrop, dseed, site, st), "lp outer")
        # dW0 with db0 riding along (column sums of the A tile already in LDS)
        self._gemm_g(ln, TN, hd["lp_gy1"].data_ptr(), hd["lp_feat"].data_ptr(), None, tg, [0, K], None, None, [gw0], tg, [gb0], H, 3 * H, 0, H, 3 * H, 3 * H)
        if pos is not None:
            chk(lib.gmp_lp_pair_weighted_colsum(gy2, hd["lp_y1"].data_ptr(), pos, tg + 4 * gw3, tg + 4 * gb3, K, H, pdrop, dseed, site,
                                                gws.data_ptr(), gws.numel(), st), "lp pair dW3")
        else:
            chk(lib.gmp_weighted_colsum(gy2, d1.data_ptr(), tg + 4 * gw3, tg + 4 * gb3, K, H, gws.data_ptr(), gws.numel(), st), "lp dW3")
        self._gemm(ln, NN, hd["lp_gy1"].data_ptr(), w0, None, hd["lp_gfeat"].data_ptr(), K, 3 * H, H, H, 3 * H, 3 * H)
        chk(lib.gmp_lp_edge_features_bwd(hd["lp_gfeat"].data_ptr(), hL.data_ptr(), p.d64["lp_edges"], hd["lp_ghs"].data_ptr(),
                                         hd["lp_ghd"].data_ptr(), N, K, H, st), "lp feat bwd")
        # reduce the per-edge gradients onto nodes -- only over this task's own rows (other tasks' heads are
        # writing their rows of gH concurrently on their own streams)
        c = e.lp_csr
        r0, r1 = p.task_row[ti], p.task_row[ti + 1]
        g_rows = gH.data_ptr() + 4 * H * r0
        chk(lib.gmp_segment_sum(hd["lp_ghs"].data_ptr(), c[3].data_ptr() + 4 * r0, c[5].data_ptr(), g_rows, r1 - r0, H, 0, 1, st), "lp g by src")
        chk(lib.gmp_segment_sum(hd["lp_ghd"].data_ptr(), c[0].data_ptr() + 4 * r0, c[2].data_ptr(), g_rows, r1 - r0, H, 0, 1, st), "lp g by dst")

    def node_contrast(self, ln: Lane, p: StepPlan, inp: StepInputs, ti: int, gs: int, ls: int) -> None:
        lib, chk, hd, st, N = self.lib, self.chk, self.hd, ln.st, p.N
        rows, M = p.nc_rows, p.nc_rows[-1]
        if M == 0:
            return
        chk(lib.gmp_row_gather(self.hL.data_ptr(), p.d64["nc_idx"], None, hd["nc_in"].data_ptr(), M, N, H, st), "nc gather")
        d1 = self._mlp2(ln, ti, "node_contrast", hd["nc_in"], rows, H, H, 128, (hd["nc_y1"], hd["nc_d1"], hd["nc_z"]))
        self._nt_xent_domains(ln, p.nc_n, rows, hd["nc_z"], hd["nc_gz"], gs, ls, 0)
        self._mlp2_bwd(ln, ti, "node_contrast", hd["nc_in"], rows, H, H, 128, hd["nc_y1"], d1, hd["nc_gz"], hd["nc_g1"], hd["nc_gin"])
        chk(lib.gmp_row_fill(self.gH.data_ptr(), p.d64["nc_idx"], hd["nc_gin"].data_ptr(), M, N, H, 0, st), "nc scatter")

    def graph_contrast(self, ln: Lane, p: StepPlan, inp: StepInputs, ti: int, gs: int, ls: int) -> None:
        lib, chk, hd, st, hL, gH = self.lib, self.chk, self.hd, ln.st, self.hL, self.gH
        rows, B = p.gc_rows, p.gc_B
        if B == 0:
            return
        chk(lib.gmp_segment_sum(hL.data_ptr(), p.d32["gc_ptr"], None, hd["gc_mean"].data_ptr(), B, H, 1, 0, st), "gc mean")
        chk(lib.gmp_segment_max_fwd(hL.data_ptr(), p.d32["gc_ptr"], hd["gc_max"].data_ptr(), B, H, st), "gc max")
        torch.cat([hd["gc_mean"][:B], hd["gc_max"][:B]], dim=1, out=hd["gc_in"][:B])
        d1 = self._mlp2(ln, ti, "graph_contrast", hd["gc_in"], rows, 2 * H, H, 128, (hd["gc_y1"], hd["gc_d1"], hd["gc_z"]))
        self._nt_xent_domains(ln, p.gc_n, rows, hd["gc_z"], hd["gc_gz"], gs, ls, self.e.D)
        self._mlp2_bwd(ln, ti, "graph_contrast", hd["gc_in"], rows, 2 * H, H, 128, hd["gc_y1"], d1, hd["gc_gz"], hd["gc_g1"], hd["gc_gin"])
        hd["gc_gmean"][:B].copy_(hd["gc_gin"][:B, :H])
        hd["gc_gmax"][:B].copy_(hd["gc_gin"][:B, H:])
        g_rows = gH.data_ptr() + 4 * H * p.gc_r0
        chk(lib.gmp_row_gather(hd["gc_gmean"].data_ptr(), p.d64["gc_gid"], p.d32["gc_ptr"], g_rows, p.gc_M, B, H, st), "gc mean bwd")
        chk(lib.gmp_segment_max_bwd(hd["gc_gmax"].data_ptr(), hL.data_ptr(), hd["gc_max"].data_ptr(), p.d32["gc_ptr"], gH.data_ptr(), B, H, 1, st), "gc max bwd")

    def graph_prop(self, ln: Lane, p: StepPlan, inp: StepInputs, ti: int, gs: int, ls: int) -> None:
        e, lib, chk, hd, st = self.e, self.lib, self.chk, self.hd, ln.st
        rows, B, G = p.gp_rows, p.gp_B, GRAPH_PROPERTY_DIM
        chk(lib.gmp_segment_sum(self.hL.data_ptr(), p.d32["gp_ptr"], None, hd["gp_in"].data_ptr(), B, H, 1, 0, st), "gp mean")
        d1 = self._mlp2(ln, ti, "graph_prop", hd["gp_in"], rows, H, 2 * H, G, (hd["gp_y1"], hd["gp_d1"], e.gp_y2))
        chk(lib.gmp_mse_sum_fwd(e.gp_y2.data_ptr(), inp.graph_props.data_ptr(), B * G, ls, ln.loss_ws.data_ptr(), ln.loss_ws.numel(), st), "gp mse")
        chk(lib.gmp_mse_sum_bwd(e.gp_y2.data_ptr(), inp.graph_props.data_ptr(), gs, e.gp_g2.data_ptr(), B * G, st), "gp mse bwd")
        self._mlp2_bwd(ln, ti, "graph_prop", hd["gp_in"], rows, H, 2 * H, G, hd["gp_y1"], d1, e.gp_g2, hd["gp_g1"], hd["gp_gin"])
        g_rows = self.gH.data_ptr() + 4 * H * p.gp_r0
        chk(lib.gmp_row_gather(hd["gp_gin"].data_ptr(), p.d64["gp_gid"], p.d32["gp_ptr"], g_rows, p.gp_M, B, H, st), "gp mean bwd")

    def domain_adv(self, ln: Lane, p: StepPlan, inp: StepInputs, ti: int, gs: int, ls: int) -> None:
        # mean read-out -> gradient reversal -> Linear 256->128, ReLU, Dropout(.5), Linear 128->D -> CE(sum)  (heads.py:70-82)
        e, lib, chk, hd, st, tg = self.e, self.lib, self.chk, self.hd, ln.st, self.tg
        B, Cc, lam, fp, one = p.da_B, len(e.domains), float(e.grl_lambda), e.flat.data_ptr(), _i32([0, p.da_B])
        head = e.head_offsets(ti, "heads.domain_adv.classifier.")
        (w0, b0, w3, b3), (gw0, gb0, gw3, gb3) = [fp + 4 * off for _, off, _ in head], [_i64([g]) for _, _, g in head]
        chk(lib.gmp_segment_sum(self.hL.data_ptr(), p.d32["da_ptr"], None, hd["da_in"].data_ptr(), B, H, 1, 0, st), "da mean")
        self._gemm(ln, NT, hd["da_in"].data_ptr(), w0, b0, hd["da_y1"].data_ptr(), B, DA_HIDDEN, H, H, H, DA_HIDDEN, relu=True)
        d1 = self._drop(ln, hd["da_y1"], hd["da_d1"], B * DA_HIDDEN, 100 + ti, p=e.da_dropout)
        self._gemm(ln, NT, d1.data_ptr(), w3, b3, hd["da_logits"].data_ptr(), B, Cc, DA_HIDDEN, DA_HIDDEN, DA_HIDDEN, Cc)
        chk(lib.gmp_cross_entropy_sum_fwd(hd["da_logits"].data_ptr(), p.d64["da_labels"], B, Cc, ls, ln.loss_ws.data_ptr(), ln.loss_ws.numel(), st), "da ce")
        chk(lib.gmp_cross_entropy_sum_bwd(hd["da_logits"].data_ptr(), p.d64["da_labels"], B, Cc, gs, hd["da_glogits"].data_ptr(), st), "da ce bwd")
        chk(lib.gmp_gemm_f32_grouped(TN, hd["da_glogits"].data_ptr(), d1.data_ptr(), None, tg, 1, one, None, None, gw3, tg, gb3,
                                     Cc, DA_HIDDEN, 0, Cc, DA_HIDDEN, DA_HIDDEN, 1.0, 0, 0, None, 0, st), "da dW3")
        self._gemm(ln, NN, hd["da_glogits"].data_ptr(), w3, None, hd["da_g1"].data_ptr(), B, DA_HIDDEN, Cc, Cc, DA_HIDDEN, DA_HIDDEN)
        self._relu_drop_bwd(ln, hd["da_g1"], hd["da_y1"], hd["da_g1"], B * DA_HIDDEN, 100 + ti, p=e.da_dropout)
        chk(lib.gmp_gemm_f32_grouped(TN, hd["da_g1"].data_ptr(), hd["da_in"].data_ptr(), None, tg, 1, one, None, None, gw0, tg, gb0,
                                     DA_HIDDEN, H, 0, DA_HIDDEN, H, H, 1.0, 0, 0, None, 0, st), "da dW0")
        chk(lib.gmp_gemm_f32(NN, hd["da_g1"].data_ptr(), w0, None, hd["da_gin"].data_ptr(), B, H, DA_HIDDEN, DA_HIDDEN, H, H, -lam, 0, 0, None, 0, st), "da grl")
        g_rows = self.gH.data_ptr() + 4 * H * p.da_r0
        chk(lib.gmp_row_gather(hd["da_gin"].data_ptr(), p.d64["da_gid"], p.d32["da_ptr"], g_rows, p.da_M, B, H, st), "da mean bwd")

    HEADS = {f.__name__: f for f in (node_feat_mask, link_pred, node_contrast, graph_contrast, graph_prop, domain_adv)}

    # ---- backward ----------------------------------------------------------------------------------
    def backward(self, ln: Lane, p: StepPlan, inp: StepInputs) -> None:
        """The stacked backward from gH down: every layer's per-task weight gradients (one group of rows / segments per task), then the
        mask token (NFM) and the encoders (every task but NFM; one group per (task, domain) pair)."""
        e, lib, chk, N, P, TG, T, tg, D, c = self.e, self.lib, self.chk, p.N, self.e._P, self.e._TG, self.e.T, self.tg, self.e.domains, self.e.csr
        gcur, gu, ga, gW, gW2, trow, st = e.gA, e.gB, e.ga, e.gW, self.gW2, p.task_row, ln.st
        task_seg = _i32(e._task_segments(p))
        for l in reversed(range(GNN_NUM_LAYERS)):
            pre, layer = f"gnn_backbone.layers.{l}.", e.model.gnn_backbone.layers[l]
            bn1, bn2 = layer.gin_conv.nn[1], layer.batch_norm
            per_task = lambda name: [TG(t, pre + name) for t in range(T)]
            self._bn_bwd(ln, p, self._bn_cfg(True, True, 10 + l), gcur, e.z2[l], e.h[l].data_ptr(), None, H, P(pre + "batch_norm.weight"),
                         P(pre + "batch_norm.bias"), bn2.running_mean, bn2.running_var, e.stat["m2"][l], e.stat["s2"][l], gu, task_seg,
                         _i64(per_task("batch_norm.weight")), _i64(per_task("batch_norm.bias")), T, "bn2 bwd")
            self._gemm_g(ln, TN, gu.data_ptr(), e.r1[l].data_ptr(), None, tg, trow, None, None, per_task("gin_conv.nn.3.weight"),
                         tg, per_task("gin_conv.nn.3.bias"), H, 2 * H, 0, H, 2 * H, 2 * H)
            self._gemm(ln, NN, gu.data_ptr(), P(pre + "gin_conv.nn.3.weight"), None, gW.data_ptr(), N, 2 * H, H, H, 2 * H, 2 * H)
            self._bn_bwd(ln, p, self._bn_cfg(True, False, 0), gW, e.z1[l], None, None, 2 * H, P(pre + "gin_conv.nn.1.weight"),
                         P(pre + "gin_conv.nn.1.bias"), bn1.running_mean, bn1.running_var, e.stat["m1"][l], e.stat["s1"][l], gW2, task_seg,
                         _i64(per_task("gin_conv.nn.1.weight")), _i64(per_task("gin_conv.nn.1.bias")), T, "bn1 bwd")
            self._gemm_g(ln, TN, gW2.data_ptr(), e.a[l].data_ptr(), None, tg, trow, None, None, per_task("gin_conv.nn.0.weight"),
                         tg, per_task("gin_conv.nn.0.bias"), 2 * H, H, 0, 2 * H, H, H)
            self._gemm(ln, NN, gW2.data_ptr(), P(pre + "gin_conv.nn.0.weight"), None, ga.data_ptr(), N, H, 2 * H, 2 * H, H, H)
            chk(lib.gmp_gin_aggregate_bwd_ex(ga.data_ptr(), c[3].data_ptr(), c[4].data_ptr(), P(pre + "gin_conv.eps"), e.h[l].data_ptr(),
                                             gu.data_ptr(), gcur.data_ptr(), e.rowdot.data_ptr(), N, H, st), "aggregate bwd")
            chk(lib.gmp_group_sum_1d(e.rowdot.data_ptr(), T, _i32(trow), _i64(per_task("gin_conv.eps")), tg, st), "eps grad")
        if "node_feat_mask" in e.tasks and p.nfm_rows[-1]:
            ti, M = e.tasks.index("node_feat_mask"), p.nfm_rows[-1]
            chk(lib.gmp_row_gather(gcur.data_ptr(), p.d64["nfm_idx"], None, self.hd["nfm_in"].data_ptr(), M, N, H, st), "token rows")
            chk(lib.gmp_colsum(self.hd["nfm_in"].data_ptr(), tg + 4 * TG(ti, "mask_token"), M, H, H, 0, ln.loss_ws.data_ptr(), ln.loss_ws.numel(), st), "token grad")
        groups = e._encoder_groups(p)              # (zeroes the slots of the pairs that dropped out)
        if not groups:
            return
        ptr = _i32([groups[0][2]] + [hi for (_, _, _, hi) in groups])
        enc_tg = lambda key: _i64([TG(ti, f"input_encoders.{d}.{key}") for (ti, d, _, _) in groups])
        e0 = f"input_encoders.{D[0]}."
        self._bn_bwd(ln, p, self._bn_cfg(True, True, 1), gcur, e.z0, None, p.d32["seg_dom"], H, P(e0 + "batch_norm.weight"), P(e0 + "batch_norm.bias"),
                     e.enc_rm, e.enc_rv, e.enc_mean, e.enc_rstd, gu, ptr, enc_tg("batch_norm.weight"), enc_tg("batch_norm.bias"), len(groups), "bn bwd encoders")
        chk(lib.gmp_encoder_bwd(inp.x_all.data_ptr(), inp.x_all.size(0), N, p.S, p.d32["src_row"], p.d32["seg_ptr"], p.d32["seg_dom"], p.d64.get("rowmask"),
                                gu.data_ptr(), len(D), _i32([DOMAIN_DIMENSIONS[d] for d in D]), e.dpad, len(groups), ptr,
                                enc_tg("linear.weight"), enc_tg("linear.bias"), tg, ln.gemm_ws.data_ptr(), ln.gemm_ws.numel(), st), "encoder bwd")
