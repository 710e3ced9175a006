"""Raw (non-autograd) wrappers: torch tensors in, one C-ABI call each.

These check shapes/dtypes/devices on the host before the launch (a wrong shape
must raise here, not fault on the GPU) and allocate outputs/workspaces with
torch.  Autograd lives in operators.py.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, NamedTuple, Optional, Tuple

import torch
from torch import Tensor

from . import _lib as L


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)      # the handle without building a Stream object (5 us -> 0.3 us per op)


def _stream(t: Tensor) -> C.c_void_p:
    if _raw_stream is not None:
        idx = t.device.index
        return C.c_void_p(_raw_stream(idx if idx is not None else torch.cuda.current_device()))
    return C.c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def _ptr(t: Optional[Tensor]) -> C.c_void_p:
    return C.c_void_p(0 if t is None else t.data_ptr())


def _need(t: Tensor, dtype, name: str, ndim: Optional[int] = None) -> None:
    if not t.is_cuda:
        raise L.GnnmpError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback), got {t.device}")
    if t.dtype != dtype:
        raise L.GnnmpError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise L.GnnmpError(f"{name}: must be contiguous")
    if ndim is not None and t.dim() != ndim:
        raise L.GnnmpError(f"{name}: expected {ndim} dims, got shape {tuple(t.shape)}")


def _need_rows(t: Tensor, name: str) -> None:
    """2-D fp32 GPU tensor whose rows are contiguous (stride 1 along a row, leading dimension >= the row length)."""
    if not t.is_cuda:
        raise L.GnnmpError(f"{name}: expected a GPU tensor (the HIP path has no CPU fallback), got {t.device}")
    if t.dtype != torch.float32 or t.dim() != 2:
        raise L.GnnmpError(f"{name}: expected a 2-D {torch.float32} tensor, got {t.dtype} {tuple(t.shape)}")
    if t.numel() and (t.stride(1) != 1 or (t.size(0) > 1 and t.stride(0) < t.size(1))):
        raise L.GnnmpError(f"{name}: rows must be contiguous (strides {t.stride()})")


def _ws(nbytes: int, device) -> Tensor:
    return torch.empty(max(int(nbytes), 16), dtype=torch.uint8, device=device)


class CSR(NamedTuple):
    """Both orientations of one edge_index (int32, device)."""
    rowptr: Tensor     # [N+1] grouped by target
    col: Tensor        # [E]   sources
    perm: Tensor       # [E]   COO edge id per slot
    rowptr_t: Tensor   # grouped by source (transposed graph)
    col_t: Tensor
    perm_t: Tensor
    num_nodes: int
    status: Tensor     # int32[1]: endpoints out of range (0 when well formed)


def csr_build(edge_index: Tensor, num_nodes: int) -> CSR:
    _need(edge_index, torch.int64, "edge_index", 2)
    if edge_index.size(0) != 2:
        raise L.GnnmpError(f"edge_index must be [2,E], got {tuple(edge_index.shape)}")
    E, dev = edge_index.size(1), edge_index.device
    mk = lambda n: torch.empty(n, dtype=torch.int32, device=dev)
    out = CSR(mk(num_nodes + 1), mk(E), mk(E), mk(num_nodes + 1), mk(E), mk(E), num_nodes, mk(1))
    l = L.lib()
    ws = _ws(l.gmp_csr_build_workspace_bytes(num_nodes, E), dev)
    L.check(l.gmp_csr_build(_ptr(edge_index), num_nodes, E, _ptr(out.rowptr), _ptr(out.col), _ptr(out.perm),
                            _ptr(out.rowptr_t), _ptr(out.col_t), _ptr(out.perm_t), _ptr(out.status),
                            _ptr(ws), ws.numel(), _stream(edge_index)), "gmp_csr_build")
    return out


def _feat_ok(x: Tensor, name: str) -> int:
    _need(x, torch.float32, name, 2)
    F = x.size(1)
    if F % 4 or F > 1024:
        raise L.GnnmpError(f"{name}: feature width {F} must be a multiple of 4 and <= 1024")
    return F


def gin_aggregate_fwd(x: Tensor, rowptr: Tensor, col: Tensor, eps: Tensor) -> Tensor:
    F = _feat_ok(x, "x")
    _need(rowptr, torch.int32, "rowptr", 1); _need(col, torch.int32, "col", 1); _need(eps, torch.float32, "eps")
    if rowptr.numel() != x.size(0) + 1:
        raise L.GnnmpError(f"rowptr has {rowptr.numel()} entries for {x.size(0)} rows")
    out = torch.empty_like(x)
    L.check(L.lib().gmp_gin_aggregate_fwd(_ptr(x), _ptr(rowptr), _ptr(col), _ptr(eps), _ptr(out), x.size(0), F,
                                          _stream(x)), "gmp_gin_aggregate_fwd")
    return out


def gin_aggregate_bwd(g_out: Tensor, rowptr_t: Tensor, col_t: Tensor, eps: Tensor,
                      x: Optional[Tensor]) -> Tuple[Tensor, Optional[Tensor]]:
    F = _feat_ok(g_out, "g_out")
    _need(rowptr_t, torch.int32, "rowptr_t", 1); _need(col_t, torch.int32, "col_t", 1)
    if rowptr_t.numel() != g_out.size(0) + 1:
        raise L.GnnmpError("rowptr_t / g_out row mismatch")
    g_x = torch.empty_like(g_out)
    g_eps = None
    if x is not None:
        _feat_ok(x, "x")
        if x.shape != g_out.shape:
            raise L.GnnmpError("x / g_out shape mismatch")
        g_eps = torch.empty(1, dtype=torch.float32, device=g_out.device)
    l = L.lib()
    ws = _ws(l.gmp_gin_aggregate_bwd_workspace_bytes(g_out.size(0), F), g_out.device)
    L.check(l.gmp_gin_aggregate_bwd(_ptr(g_out), _ptr(rowptr_t), _ptr(col_t), _ptr(eps), _ptr(x), _ptr(g_x),
                                    _ptr(g_eps), g_out.size(0), F, _ptr(ws), ws.numel(), _stream(g_out)),
            "gmp_gin_aggregate_bwd")
    return g_x, g_eps


def gin_aggregate_fwd_rows(x: Tensor, rowptr: Tensor, col: Tensor, eps: Tensor, out: Tensor, row0: int, row1: int) -> Tensor:
    """Rows [row0, row1) of gin_aggregate_fwd written into `out` [N, F] (the other rows are left as they are); col keeps the whole
    batch's numbering."""
    F = _feat_ok(x, "x")
    _need(rowptr, torch.int32, "rowptr", 1); _need(col, torch.int32, "col", 1); _need(eps, torch.float32, "eps")
    _need(out, torch.float32, "out", 2)
    if rowptr.numel() != x.size(0) + 1 or out.shape != x.shape:
        raise L.GnnmpError("gin_aggregate_fwd_rows: rowptr / out do not match x")
    if not 0 <= row0 <= row1 <= x.size(0):
        raise L.GnnmpError(f"gin_aggregate_fwd_rows: rows [{row0}, {row1}) of {x.size(0)}")
    L.check(L.lib().gmp_gin_aggregate_fwd_rows(_ptr(x), _ptr(rowptr), _ptr(col), _ptr(eps), _ptr(out), row0, row1, F, _stream(x)),
            "gmp_gin_aggregate_fwd_rows")
    return out


def gin_aggregate_bwd_ex(g_out: Tensor, rowptr_t: Tensor, col_t: Tensor, eps: Tensor, x: Optional[Tensor] = None,
                         addend: Optional[Tensor] = None) -> Tuple[Tensor, Optional[Tensor]]:
    """The stacked step's backward: g_x = (1 + eps) g + sum over the transposed CSR of g (+ addend), and, when x is given,
    rowdot [N] = <g[r], x[r]> per row (gmp_group_sum_1d reduces it to the eps gradient of a task)."""
    F = _feat_ok(g_out, "g_out")
    _need(rowptr_t, torch.int32, "rowptr_t", 1); _need(col_t, torch.int32, "col_t", 1); _need(eps, torch.float32, "eps")
    if rowptr_t.numel() != g_out.size(0) + 1:
        raise L.GnnmpError("rowptr_t / g_out row mismatch")
    for t, n in ((x, "x"), (addend, "addend")):
        if t is not None:
            _feat_ok(t, n)
            if t.shape != g_out.shape:
                raise L.GnnmpError(f"{n} / g_out shape mismatch")
    g_x = torch.empty_like(g_out)
    rowdot = torch.empty(g_out.size(0), dtype=torch.float32, device=g_out.device) if x is not None else None
    L.check(L.lib().gmp_gin_aggregate_bwd_ex(_ptr(g_out), _ptr(rowptr_t), _ptr(col_t), _ptr(eps), _ptr(x), _ptr(addend), _ptr(g_x),
                                             _ptr(rowdot), g_out.size(0), F, _stream(g_out)), "gmp_gin_aggregate_bwd_ex")
    return g_x, rowdot


def group_sum_1d(vals: Tensor, group_rows, out: Optional[Tensor] = None, out_off=None) -> Tensor:
    """out[out_off[g]] = sum of vals[group_rows[g] : group_rows[g + 1]] (out_off default g; group_rows / out_off: host lists).  Slots
    of `out` that no group names are left as they are."""
    _need(vals, torch.float32, "vals", 1)
    rows = [int(r) for r in group_rows]
    G = len(rows) - 1
    if G < 1 or rows[0] < 0 or rows[-1] > vals.numel() or any(a > b for a, b in zip(rows[:-1], rows[1:])):
        raise L.GnnmpError(f"group_sum_1d: group rows {rows} for {vals.numel()} values")
    off = list(range(G)) if out_off is None else [int(o) for o in out_off]
    if out is None:
        out = torch.empty(max(off) + 1 if off else 0, dtype=torch.float32, device=vals.device)
    _need(out, torch.float32, "out", 1)
    if len(off) != G or min(off) < 0 or max(off) >= out.numel():
        raise L.GnnmpError(f"group_sum_1d: output slots {off} for {out.numel()} entries")
    L.check(L.lib().gmp_group_sum_1d(_ptr(vals), G, (C.c_int32 * (G + 1))(*rows), None if out_off is None else (C.c_int64 * G)(*off),
                                     _ptr(out), _stream(vals)), "gmp_group_sum_1d")
    return out


def segment_sum(src: Tensor, ptr: Tensor, idx: Optional[Tensor], mean: bool = False,
                out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    _need(src, torch.float32, "src", 2)
    F = src.size(1)
    _need(ptr, torch.int32, "ptr", 1)
    if idx is not None:
        _need(idx, torch.int32, "idx", 1)
    nseg = ptr.numel() - 1
    if out is None:
        out = torch.empty(nseg, F, dtype=torch.float32, device=src.device)
        accumulate = False
    L.check(L.lib().gmp_segment_sum(_ptr(src), _ptr(ptr), _ptr(idx), _ptr(out), nseg, F, int(mean), int(accumulate),
                                    _stream(src)), "gmp_segment_sum")
    return out


def row_gather(src: Tensor, idx: Tensor, seg_ptr: Optional[Tensor] = None) -> Tensor:
    _need(src, torch.float32, "src", 2)
    F = src.size(1)
    _need(idx, torch.int64, "idx", 1)
    if seg_ptr is not None:
        _need(seg_ptr, torch.int32, "seg_ptr", 1)
        if seg_ptr.numel() != src.size(0) + 1:
            raise L.GnnmpError("seg_ptr must have one entry per source row + 1")
    out = torch.empty(idx.numel(), F, dtype=torch.float32, device=src.device)
    L.check(L.lib().gmp_row_gather(_ptr(src), _ptr(idx), _ptr(seg_ptr), _ptr(out), idx.numel(), src.size(0), F,
                                   _stream(src)), "gmp_row_gather")
    return out


def segment_max_fwd(x: Tensor, ptr: Tensor) -> Tensor:
    F = _feat_ok(x, "x")
    _need(ptr, torch.int32, "ptr", 1)
    out = torch.empty(ptr.numel() - 1, F, dtype=torch.float32, device=x.device)
    L.check(L.lib().gmp_segment_max_fwd(_ptr(x), _ptr(ptr), _ptr(out), ptr.numel() - 1, F, _stream(x)),
            "gmp_segment_max_fwd")
    return out


def segment_max_bwd(g_out: Tensor, x: Tensor, out: Tensor, ptr: Tensor, g_x: Optional[Tensor] = None,
                    accumulate: bool = False) -> Tensor:
    """g_x (nullable: a fresh buffer): rows of a segment are overwritten, or added to when `accumulate`; rows outside every segment
    are left as they are."""
    F = _feat_ok(x, "x")
    _need(g_out, torch.float32, "g_out", 2); _need(out, torch.float32, "out", 2); _need(ptr, torch.int32, "ptr", 1)
    if g_out.shape != out.shape or out.size(0) != ptr.numel() - 1 or out.size(1) != F:
        raise L.GnnmpError("segment_max_bwd: shape mismatch")
    if g_x is None:
        g_x = torch.empty_like(x)
        accumulate = False
    else:
        _need(g_x, torch.float32, "g_x", 2)
        if g_x.shape != x.shape:
            raise L.GnnmpError("segment_max_bwd: g_x shape")
    L.check(L.lib().gmp_segment_max_bwd(_ptr(g_out), _ptr(x), _ptr(out), _ptr(ptr), _ptr(g_x), ptr.numel() - 1, F, int(accumulate),
                                        _stream(x)), "gmp_segment_max_bwd")
    return g_x


NT, NN, TN = L.K["GMP_GEMM_NT"], L.K["GMP_GEMM_NN"], L.K["GMP_GEMM_TN"]


def gemm(mode: int, A: Tensor, B: Tensor, bias: Optional[Tensor] = None, out: Optional[Tensor] = None,
         alpha: float = 1.0, accumulate: bool = False, relu: bool = False) -> Tensor:
    """NT: A[M,K] B[N,K]^T ; NN: A[M,K] B[K,N] ; TN: A[K,M]^T B[K,N].  Operands may be row-strided views (unit stride along a row, any
    leading dimension >= the row length): the fine-tune engine keeps the encoder weight as a [256, 1433] view of its K-padded [256, 1440]
    slot, and evaluation through the module multiplies by that view."""
    _need_rows(A, "A"); _need_rows(B, "B")
    if mode == NT:
        M, K, N = A.size(0), A.size(1), B.size(0); kb = B.size(1)
    elif mode == NN:
        M, K, N = A.size(0), A.size(1), B.size(1); kb = B.size(0)
    elif mode == TN:
        M, K, N = A.size(1), A.size(0), B.size(1); kb = B.size(0)
    else:
        raise L.GnnmpError(f"gemm mode {mode}")
    if kb != K:
        raise L.GnnmpError(f"gemm: inner dims differ ({K} vs {kb}) for mode {mode}")
    if bias is not None:
        _need(bias, torch.float32, "bias", 1)
        if bias.numel() != N:
            raise L.GnnmpError("gemm: bias length")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
        accumulate = False
    else:
        _need(out, torch.float32, "out", 2)
        if tuple(out.shape) != (M, N):
            raise L.GnnmpError("gemm: out shape")
    l = L.lib()
    wsb = l.gmp_gemm_f32_workspace_bytes(mode, M, N, K)
    ws = _ws(wsb, A.device) if wsb else None
    L.check(l.gmp_gemm_f32(mode, _ptr(A), _ptr(B), _ptr(bias), _ptr(out), M, N, K, A.stride(0) if A.size(0) > 1 else A.size(1),
                           B.stride(0) if B.size(0) > 1 else B.size(1), N,
                           float(alpha), int(accumulate), int(relu), _ptr(ws), wsb, _stream(A)), "gmp_gemm_f32")
    return out


def colsum(A: Tensor, out: Optional[Tensor] = None, accumulate: bool = False) -> Tensor:
    _need(A, torch.float32, "A", 2)
    M, N = A.shape
    if out is None:
        out = torch.empty(N, dtype=torch.float32, device=A.device)
        accumulate = False
    l = L.lib()
    wsb = l.gmp_colsum_workspace_bytes(M, N)
    ws = _ws(wsb, A.device)
    L.check(l.gmp_colsum(_ptr(A), _ptr(out), M, N, N, int(accumulate), _ptr(ws), ws.numel(), _stream(A)), "gmp_colsum")
    return out


def _sparse_ok(x, K_needed: bool = True) -> None:
    from .graph import SparseFeatures
    if not isinstance(x, SparseFeatures):
        raise L.GnnmpError(f"expected SparseFeatures, got {type(x).__name__}")
    _need(x.rowptr, torch.int32, "x.rowptr", 1); _need(x.col, torch.int32, "x.col", 1); _need(x.val, torch.float32, "x.val", 1)
    if x.rowptr.numel() != x.shape[0] + 1:
        raise L.GnnmpError(f"x.rowptr has {x.rowptr.numel()} entries for {x.shape[0]} rows")


def sparse_linear_fwd(x, weight: Tensor, bias: Optional[Tensor] = None, out: Optional[Tensor] = None,
                      status: Optional[Tensor] = None) -> Tensor:
    """out[N, H] = X W^T + b with X a SparseFeatures [N, K] and W [H, >= K] (a row-strided view such as the fine-tune engine's [256, 1433]
    view of its [256, 1440] slot is read in place).  status (int32[1], nullable): skipped column indices are ADDED to it."""
    _sparse_ok(x)
    _need_rows(weight, "weight")
    N, K = x.shape
    H = weight.size(0)
    if weight.size(1) != K:
        raise L.GnnmpError(f"sparse_linear: weight has {weight.size(1)} columns for {K} features")
    ldw = weight.stride(0) if H > 1 else K
    if bias is not None:
        _need(bias, torch.float32, "bias", 1)
        if bias.numel() != H:
            raise L.GnnmpError("sparse_linear: bias length")
    if out is None:
        out = torch.empty(N, H, dtype=torch.float32, device=weight.device)
    else:
        _need(out, torch.float32, "out", 2)
        if tuple(out.shape) != (N, H):
            raise L.GnnmpError("sparse_linear: out shape")
    if status is not None:
        _need(status, torch.int32, "status", 1)
    l = L.lib()
    ws = _ws(l.gmp_sparse_linear_workspace_bytes(K, H), weight.device)
    L.check(l.gmp_sparse_linear_fwd(_ptr(x.rowptr), _ptr(x.col), _ptr(x.val), N, K, _ptr(weight), ldw, _ptr(bias), _ptr(out), H, H,
                                    _ptr(status), _ptr(ws), ws.numel(), _stream(weight)), "gmp_sparse_linear_fwd")
    return out


def sparse_csc_build(x) -> Tuple[Tensor, Tensor, Tensor, Tensor]:
    """(colptr int32 [K+1], row int32 [nnz], val_t fp32 [nnz], status int32[1]) of a SparseFeatures on the GPU; status = column
    indices outside [0, K) (left out; the first colptr[K] slots of row / val_t are valid)."""
    _sparse_ok(x)
    N, K = x.shape
    nnz, dev = x.nnz, x.device
    colptr, row = torch.empty(K + 1, dtype=torch.int32, device=dev), torch.zeros(nnz, dtype=torch.int32, device=dev)
    val_t, status = torch.zeros(nnz, dtype=torch.float32, device=dev), torch.empty(1, dtype=torch.int32, device=dev)
    l = L.lib()
    ws = _ws(l.gmp_sparse_csc_workspace_bytes(N, K, nnz), dev)
    L.check(l.gmp_sparse_csc_build(_ptr(x.rowptr), _ptr(x.col), _ptr(x.val), N, K, nnz, _ptr(colptr), _ptr(row), _ptr(val_t), _ptr(status),
                                   _ptr(ws), ws.numel(), _stream(x.val)), "gmp_sparse_csc_build")
    return colptr, row, val_t, status


def sparse_linear_wgrad(csc, num_rows: int, g: Tensor, out: Optional[Tensor] = None, status: Optional[Tensor] = None) -> Tensor:
    """dW [H, ldw] = G^T X from the CSC form (colptr, row, val_t) of X [num_rows, K]; out (nullable) may be wider than K (its padding
    columns are overwritten with 0.0, like every column without entries)."""
    colptr, row, val_t = csc
    _need(colptr, torch.int32, "colptr", 1); _need(row, torch.int32, "row", 1); _need(val_t, torch.float32, "val_t", 1)
    _need(g, torch.float32, "g", 2)
    K, H = colptr.numel() - 1, g.size(1)
    if g.size(0) != num_rows:
        raise L.GnnmpError(f"sparse_linear_wgrad: g has {g.size(0)} rows for {num_rows}")
    if out is None:
        out = torch.empty(H, K, dtype=torch.float32, device=g.device)
    else:
        _need_rows(out, "out")
        if out.size(0) != H or out.size(1) < K:
            raise L.GnnmpError(f"sparse_linear_wgrad: out {tuple(out.shape)} for [{H}, >= {K}]")
    ldw = out.stride(0) if H > 1 else out.size(1)
    if status is not None:
        _need(status, torch.int32, "status", 1)
    L.check(L.lib().gmp_sparse_linear_wgrad(_ptr(colptr), _ptr(row), _ptr(val_t), num_rows, K, _ptr(g), H, _ptr(out), ldw, _ptr(status),
                                            _stream(g)), "gmp_sparse_linear_wgrad")
    return out


def make_bn_config(training: bool, relu: bool, dropout_p: float = 0.0, seed: int = 0, stream_id: int = 0,
                   eps: float = 1e-5, momentum: float = 0.1, sync: Optional[Tensor] = None) -> L.BnConfig:
    """sync: zero-filled int32 device tensor of bn_sync_words(channels, segments) words (gmp_bn_config.sync): segments of 1,025-4,096
    rows then run as 128-row slabs over the whole chip.  The caller keeps the tensor alive while launches that got it are in flight."""
    if sync is None:
        return L.BnConfig(int(training), int(relu), eps, momentum, float(dropout_p), seed & (2 ** 64 - 1), stream_id)
    _need(sync, torch.int32, "sync", 1)
    return L.BnConfig(int(training), int(relu), eps, momentum, float(dropout_p), seed & (2 ** 64 - 1), stream_id, None, sync.data_ptr(),
                      sync.numel())


def bn_sync_words(channels: int, num_segments: int) -> int:
    return L.lib().gmp_bn_sync_bytes(channels, num_segments) // 4


def _bn_params(Cc: int, S: int, seg_group: Optional[Tensor], named) -> None:
    """gamma / beta (and the running pair, when given) are [C], or [groups, C] with a seg_group table of S entries (< groups: the caller's part)."""
    if seg_group is None:
        for n, t in named[:2]:
            _need(t, torch.float32, n, 1)
            if t.numel() != Cc:
                raise L.GnnmpError(f"bn: {n} length")
        return
    _need(seg_group, torch.int32, "seg_group", 1)
    if seg_group.numel() != S:
        raise L.GnnmpError(f"bn: seg_group has {seg_group.numel()} entries for {S} segments")
    for n, t in named:
        if t is None:
            continue
        _need(t, torch.float32, n, 2)
        if t.size(1) != Cc or t.size(0) != named[0][1].size(0):
            raise L.GnnmpError(f"bn: {n} is {tuple(t.shape)} for [groups, {Cc}]")


def bn_fwd(x: Tensor, residual: Optional[Tensor], seg_ptr: Tensor, max_seg_rows: int, gamma: Tensor, beta: Tensor,
           running_mean: Optional[Tensor], running_var: Optional[Tensor], cfg: L.BnConfig, seg_group: Optional[Tensor] = None):
    """Returns (y, save_mean, save_rstd); the saved stats are None in eval mode.  seg_group (int32 [S], device): the parameter group of
    each segment; gamma, beta and the running pair are then [groups, C]."""
    _need(x, torch.float32, "x", 2)
    rows, Cc = x.shape
    if residual is not None:
        _need(residual, torch.float32, "residual", 2)
        if residual.shape != x.shape:
            raise L.GnnmpError("bn: residual shape")
    _need(seg_ptr, torch.int32, "seg_ptr", 1)
    S = seg_ptr.numel() - 1
    _bn_params(Cc, S, seg_group, (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var)))
    y = torch.empty_like(x)
    sm = sr = None
    if cfg.training:
        sm = torch.empty(S, Cc, dtype=torch.float32, device=x.device)
        sr = torch.empty(S, Cc, dtype=torch.float32, device=x.device)
    l = L.lib()
    ws = _ws(l.gmp_bn_workspace_bytes(rows, Cc, S, max_seg_rows), x.device)
    L.check(l.gmp_bn_fwd(_ptr(x), _ptr(residual), _ptr(seg_ptr), _ptr(seg_group), S, max_seg_rows, rows, Cc, _ptr(gamma), _ptr(beta),
                         _ptr(running_mean), _ptr(running_var), _ptr(sm), _ptr(sr), _ptr(y), C.byref(cfg),
                         _ptr(ws), ws.numel(), _stream(x)), "gmp_bn_fwd")
    return y, sm, sr


def _ptr_table(ts):
    return (C.c_void_p * len(ts))(*[None if t is None else t.data_ptr() for t in ts])


def bn_fold(layers, eps: float = 1e-5, out: Optional[Tensor] = None):
    """Eval-mode BatchNorm as per-channel (scale, shift) rows, all `layers` in one launch (gmp_bn_fold).  layers: a sequence of
    (gamma, beta, running_mean, running_var) -- gamma / beta may be None (1 / 0).  Returns (table, [(scale, shift), ...]): the pairs are
    views into `table` (2 * sum of the channel counts floats; pass `out` to reuse one)."""
    layers = list(layers)
    if not 1 <= len(layers) <= 16:
        raise L.GnnmpError(f"bn_fold: {len(layers)} layers (1 .. 16)")
    chans = []
    for i, (g, b, m, v) in enumerate(layers):
        _need(m, torch.float32, f"running_mean[{i}]", 1); _need(v, torch.float32, f"running_var[{i}]", 1)
        for t, n in ((g, "gamma"), (b, "beta"), (v, "running_var")):
            if t is not None:
                _need(t, torch.float32, f"{n}[{i}]", 1)
                if t.numel() != m.numel():
                    raise L.GnnmpError(f"bn_fold: {n}[{i}] length")
        if m.numel() < 1:
            raise L.GnnmpError(f"bn_fold: layer {i} has no channels")
        chans.append(m.numel())
    total = 2 * sum(chans)
    dev = layers[0][2].device
    if out is None:
        out = torch.empty(total, dtype=torch.float32, device=dev)
    else:
        _need(out, torch.float32, "out", 1)
        if out.numel() < total:
            raise L.GnnmpError(f"bn_fold: out has {out.numel()} floats, {total} needed")
    cols = list(zip(*layers))
    L.check(L.lib().gmp_bn_fold(len(layers), _ptr_table(cols[0]), _ptr_table(cols[1]), _ptr_table(cols[2]), _ptr_table(cols[3]),
                                (C.c_int32 * len(chans))(*chans), float(eps), _ptr(out), _stream(out)), "gmp_bn_fold")
    pairs, o = [], 0
    for c in chans:
        pairs.append((out[o:o + c], out[o + c:o + 2 * c]))
        o += 2 * c
    return out, pairs


def linear_affine(A: Tensor, W: Tensor, bias: Optional[Tensor], scale: Tensor, shift: Tensor, residual: Optional[Tensor] = None,
                  relu: bool = False, out: Optional[Tensor] = None) -> Tensor:
    """act(((A W^T + bias) + residual) * scale + shift), in that order (gmp_linear_affine_fwd): a Linear with the eval-mode BatchNorm that
    follows it (ops.bn_fold) in the GEMM epilogue.  A [M, K], W [N, K], residual [M, N] and out [M, N] may be row-strided views."""
    _need_rows(A, "A"); _need_rows(W, "W")
    M, K, N = A.size(0), A.size(1), W.size(0)
    if W.size(1) != K or K < 1:
        raise L.GnnmpError(f"linear_affine: A has {K} columns, W {W.size(1)}")
    for t, n in ((bias, "bias"), (scale, "scale"), (shift, "shift")):
        if t is None and n == "bias":
            continue
        _need(t, torch.float32, n, 1)
        if t.numel() != N:
            raise L.GnnmpError(f"linear_affine: {n} length")
    ld = lambda t: t.stride(0) if t.size(0) > 1 else t.size(1)
    if residual is not None:
        _need_rows(residual, "residual")
        if tuple(residual.shape) != (M, N):
            raise L.GnnmpError("linear_affine: residual shape")
    if out is None:
        out = torch.empty(M, N, dtype=torch.float32, device=A.device)
    else:
        _need_rows(out, "out")
        if tuple(out.shape) != (M, N):
            raise L.GnnmpError("linear_affine: out shape")
    l = L.lib()
    wsb = l.gmp_linear_affine_workspace_bytes(M, N, K)
    ws = _ws(wsb, A.device) if wsb else None
    L.check(l.gmp_linear_affine_fwd(_ptr(A), _ptr(W), _ptr(bias), _ptr(residual), _ptr(scale), _ptr(shift), _ptr(out), M, N, K, ld(A), ld(W),
                                    0 if residual is None else ld(residual), ld(out), int(relu), _ptr(ws), wsb, _stream(A)),
            "gmp_linear_affine_fwd")
    return out


def bn_bwd(g_y: Tensor, x: Tensor, residual: Optional[Tensor], seg_ptr: Tensor, max_seg_rows: int, gamma: Tensor,
           beta: Tensor, running_mean, running_var, save_mean, save_rstd, cfg: L.BnConfig, group_seg_ptr=None, seg_group: Optional[Tensor] = None):
    """Returns (g_u, g_gamma [G,C], g_beta [G,C]); group_seg_ptr: python list of segment offsets (default one group).
    seg_group (int32 [S], device): the parameter group of each segment; gamma, beta and the running pair are then [groups, C]."""
    _need(g_y, torch.float32, "g_y", 2); _need(x, torch.float32, "x", 2)
    rows, Cc = x.shape
    S = seg_ptr.numel() - 1
    if seg_group is not None:
        _bn_params(Cc, S, seg_group, (("gamma", gamma), ("beta", beta), ("running_mean", running_mean), ("running_var", running_var)))
    grp = [0, S] if group_seg_ptr is None else list(group_seg_ptr)
    G = len(grp) - 1
    arr = (C.c_int32 * (G + 1))(*grp)
    g_u = torch.empty_like(x)
    gg = torch.empty(G, Cc, dtype=torch.float32, device=x.device)
    gb = torch.empty(G, Cc, dtype=torch.float32, device=x.device)
    l = L.lib()
    ws = _ws(l.gmp_bn_workspace_bytes(rows, Cc, S, max_seg_rows), x.device)
    L.check(l.gmp_bn_bwd(_ptr(g_y), _ptr(x), _ptr(residual), _ptr(seg_ptr), _ptr(seg_group), S, max_seg_rows, rows, Cc, _ptr(gamma),
                         _ptr(beta), _ptr(running_mean), _ptr(running_var), _ptr(save_mean), _ptr(save_rstd),
                         _ptr(g_u), _ptr(gg), _ptr(gb), C.cast(arr, C.c_void_p), None, None, G, C.byref(cfg), _ptr(ws), ws.numel(),
                         _stream(x)), "gmp_bn_bwd")
    return g_u, gg, gb


def lp_edge_features_fwd(h: Tensor, edges: Tensor) -> Tensor:
    F = _feat_ok(h, "h")
    _need(edges, torch.int64, "edges", 2)
    K = edges.size(1)
    feat = torch.empty(K, 3 * F, dtype=torch.float32, device=h.device)
    L.check(L.lib().gmp_lp_edge_features_fwd(_ptr(h), _ptr(edges), _ptr(feat), h.size(0), K, F, _stream(h)),
            "gmp_lp_edge_features_fwd")
    return feat


def lp_edge_features_bwd(g_feat: Tensor, h: Tensor, edges: Tensor) -> Tuple[Tensor, Tensor]:
    F = _feat_ok(h, "h")
    _need(g_feat, torch.float32, "g_feat", 2); _need(edges, torch.int64, "edges", 2)
    K = edges.size(1)
    if tuple(g_feat.shape) != (K, 3 * F):
        raise L.GnnmpError("lp_edge_features_bwd: g_feat shape")
    ghs = torch.empty(K, F, dtype=torch.float32, device=h.device)
    ghd = torch.empty_like(ghs)
    L.check(L.lib().gmp_lp_edge_features_bwd(_ptr(g_feat), _ptr(h), _ptr(edges), _ptr(ghs), _ptr(ghd), h.size(0), K, F,
                                             _stream(h)), "gmp_lp_edge_features_bwd")
    return ghs, ghd


def lp_feat_gemm_fwd(h: Tensor, edges: Tensor, w0: Tensor, b0: Tensor) -> Tensor:
    """relu(lp_edge_features(h, edges) @ w0.T + b0) [K, 256] with the features generated in the GEMM's loader (gmp_lp_feat_gemm_fwd)."""
    F = _feat_ok(h, "h")
    _need(edges, torch.int64, "edges", 2); _need(w0, torch.float32, "w0", 2); _need(b0, torch.float32, "b0", 1)
    K = edges.size(1)
    y1 = torch.empty(K, F, dtype=torch.float32, device=h.device)
    L.check(L.lib().gmp_lp_feat_gemm_fwd(_ptr(h), _ptr(edges), _ptr(w0), _ptr(b0), _ptr(y1), h.size(0), K, F, _stream(h)), "gmp_lp_feat_gemm_fwd")
    return y1


def lp_feat_gemm_wgrad(gy1: Tensor, h: Tensor, edges: Tensor, workspace: Optional[Tensor]) -> Tuple[Tensor, Tensor]:
    """dW0 [256, 768] = gy1.T @ lp_edge_features(h, edges) and db0 [256] = gy1.sum(0), features generated in the loader
    (gmp_lp_feat_gemm_wgrad); the workspace (uint8) decides the row slices as it does for gmp_gemm_f32_grouped."""
    F = _feat_ok(h, "h")
    _need(gy1, torch.float32, "gy1", 2); _need(edges, torch.int64, "edges", 2)
    K = edges.size(1)
    dW0 = torch.empty(F, 3 * F, dtype=torch.float32, device=h.device)
    db0 = torch.empty(F, dtype=torch.float32, device=h.device)
    L.check(L.lib().gmp_lp_feat_gemm_wgrad(_ptr(gy1), _ptr(h), _ptr(edges), _ptr(dW0), _ptr(db0), h.size(0), K, F, _ptr(workspace),
                                           0 if workspace is None else workspace.numel(), _stream(h)), "gmp_lp_feat_gemm_wgrad")
    return dW0, db0


def lp_feat_gemm_bwd_fold(gy1: Tensor, w0: Tensor, h: Tensor, edges: Tensor) -> Tuple[Tensor, Tensor]:
    """g_hs, g_hd [K, 256] of lp_edge_features_bwd(gy1 @ w0, h, edges) without the [K, 768] matrix (gmp_lp_feat_gemm_bwd_fold:
    K >= 1024, feature width 256; bit for bit the two-launch form)."""
    F = _feat_ok(h, "h")
    _need(gy1, torch.float32, "gy1", 2); _need(w0, torch.float32, "w0", 2); _need(edges, torch.int64, "edges", 2)
    K = edges.size(1)
    if tuple(gy1.shape) != (K, F) or tuple(w0.shape) != (F, 3 * F):
        raise L.GnnmpError("lp_feat_gemm_bwd_fold: gy1 [K, F] and w0 [F, 3 F] expected")
    ghs = torch.empty(K, F, dtype=torch.float32, device=h.device)
    ghd = torch.empty_like(ghs)
    L.check(L.lib().gmp_lp_feat_gemm_bwd_fold(_ptr(gy1), _ptr(w0), _ptr(h), _ptr(edges), _ptr(ghs), _ptr(ghd), h.size(0), K, F,
                                              _stream(h)), "gmp_lp_feat_gemm_bwd_fold")
    return ghs, ghd


def nt_xent_fwd(z1: Tensor, z2: Tensor, temperature: float) -> Tuple[Tensor, Tensor]:
    """Returns (loss_sum [1], workspace) -- the workspace feeds nt_xent_bwd."""
    _need(z1, torch.float32, "z1", 2); _need(z2, torch.float32, "z2", 2)
    if z1.shape != z2.shape:
        raise L.GnnmpError("nt_xent: z1/z2 shapes differ")
    n, d = z1.shape
    l = L.lib()
    ws = _ws(l.gmp_nt_xent_workspace_bytes(n, d), z1.device)
    loss = torch.empty(1, dtype=torch.float32, device=z1.device)
    L.check(l.gmp_nt_xent_fwd(_ptr(z1), _ptr(z2), n, d, float(temperature), _ptr(loss), _ptr(ws), ws.numel(),
                              _stream(z1)), "gmp_nt_xent_fwd")
    return loss, ws


def nt_xent_bwd(z1: Tensor, z2: Tensor, temperature: float, g_scale: Tensor, ws: Tensor) -> Tuple[Tensor, Tensor]:
    n, d = z1.shape
    _need(g_scale, torch.float32, "g_scale")
    g1, g2 = torch.empty_like(z1), torch.empty_like(z2)
    L.check(L.lib().gmp_nt_xent_bwd(_ptr(z1), _ptr(z2), n, d, float(temperature), _ptr(g_scale), _ptr(g1), _ptr(g2),
                                    _ptr(ws), ws.numel(), _stream(z1)), "gmp_nt_xent_bwd")
    return g1, g2


def nt_xent_stream_fwd(z1: Tensor, z2: Tensor, temperature: float) -> Tuple[Tensor, Tensor]:
    """The streaming form (no [2n, 2n] matrix, O(n d) workspace, any n).  Returns (loss_sum [1], workspace) -- the workspace
    feeds nt_xent_stream_bwd."""
    _need(z1, torch.float32, "z1", 2); _need(z2, torch.float32, "z2", 2)
    if z1.shape != z2.shape:
        raise L.GnnmpError("nt_xent_stream: z1/z2 shapes differ")
    n, d = z1.shape
    l = L.lib()
    ws = _ws(l.gmp_nt_xent_stream_workspace_bytes(n, d), z1.device)
    loss = torch.empty(1, dtype=torch.float32, device=z1.device)
    L.check(l.gmp_nt_xent_stream_fwd(_ptr(z1), _ptr(z2), n, d, float(temperature), _ptr(loss), _ptr(ws), ws.numel(),
                                     _stream(z1)), "gmp_nt_xent_stream_fwd")
    return loss, ws


def nt_xent_stream_bwd(z1: Tensor, z2: Tensor, temperature: float, g_scale: Tensor, ws: Tensor) -> Tuple[Tensor, Tensor]:
    n, d = z1.shape
    _need(g_scale, torch.float32, "g_scale")
    g1, g2 = torch.empty_like(z1), torch.empty_like(z2)
    L.check(L.lib().gmp_nt_xent_stream_bwd(_ptr(z1), _ptr(z2), n, d, float(temperature), _ptr(g_scale), _ptr(g1), _ptr(g2),
                                           _ptr(ws), ws.numel(), _stream(z1)), "gmp_nt_xent_stream_bwd")
    return g1, g2


MINER_IMPLS = ("matrix", "stream", "auto")
MINER_MATRIX_MAX_N = 65535          # the dense form packs the flat pair index into 32 bits


def hard_negative_topk(emb: Tensor, existing_edges: Tensor, k: int, return_scores: bool = False,
                       return_matrix: bool = False, impl: str = "matrix"):
    """Top-k cosine-similarity non-edges (finetune.py:45-75).  Returns edges [2,k] int64 (score-descending), and
    optionally the selected scores [k] and the masked n x n similarity matrix.
    impl: "matrix" (csrc/hardneg.hip: the n x n matrix in the workspace, n <= 65535), "stream" (csrc/hardneg_stream.hip: tiles
    recomputed in MFMA accumulators, workspace O(n d + E), n <= 2^20, a -1 / -inf tail when fewer than k pairs are unmasked),
    or "auto" (stream when n > 65535, matrix otherwise)."""
    if impl not in MINER_IMPLS:
        raise ValueError(f"hard_negative_topk: impl={impl!r} is not one of {MINER_IMPLS}")
    _need(emb, torch.float32, "emb", 2); _need(existing_edges, torch.int64, "existing_edges", 2)
    n, d = emb.shape
    E = existing_edges.size(1)
    l = L.lib()
    stream = impl == "stream" or (impl == "auto" and n > MINER_MATRIX_MAX_N)
    if stream:
        fn, name, nbytes = l.gmp_hard_negative_topk_stream, "gmp_hard_negative_topk_stream", l.gmp_hard_negative_stream_workspace_bytes(n, d, E)
    else:
        # beyond its limit the dense entry point refuses n before it looks at the workspace: no 4 n^2 bytes just to hear that
        fn, name, nbytes = l.gmp_hard_negative_topk, "gmp_hard_negative_topk", l.gmp_hard_negative_workspace_bytes(n, d) if n <= MINER_MATRIX_MAX_N else 0
    ws = _ws(nbytes, emb.device)
    out = torch.empty(2, k, dtype=torch.int64, device=emb.device)
    sc = torch.empty(k, dtype=torch.float32, device=emb.device) if return_scores else None
    mat = torch.empty(n, n, dtype=torch.float32, device=emb.device) if return_matrix else None
    L.check(fn(_ptr(emb), n, d, _ptr(existing_edges) if E else None, E, k, _ptr(out) if k else None,
               _ptr(sc) if sc is not None else None, _ptr(mat) if mat is not None else None,
               _ptr(ws), ws.numel(), _stream(emb)), name)
    res = (out,)
    if return_scores:
        res += (sc,)
    if return_matrix:
        res += (mat,)
    return res if len(res) > 1 else out


def nt_xent_grouped(z: Tensor, ns, row_offsets, temperature: float, g_scale: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """Several NT-Xent problems in one call: group g's rows [z1; z2] (2*ns[g] of them) start at row_offsets[g] of z.
    Returns (g_z [same shape as z; rows outside every group untouched = 0], loss_sums [G], loss_total [1])."""
    _need(z, torch.float32, "z", 2); _need(g_scale, torch.float32, "g_scale")
    G, d = len(ns), z.size(1)
    l = L.lib()
    ws = _ws(l.gmp_nt_xent_grouped_workspace_bytes(G, max(max(ns), 1), d), z.device)
    gz = torch.zeros_like(z)
    sums = torch.empty(G, dtype=torch.float32, device=z.device)
    total = torch.empty(1, dtype=torch.float32, device=z.device)
    n_arr = (C.c_int32 * G)(*[int(n) for n in ns])
    o_arr = (C.c_int64 * G)(*[int(o) for o in row_offsets])
    L.check(l.gmp_nt_xent_grouped(_ptr(z), _ptr(gz), G, n_arr, o_arr, d, float(temperature), _ptr(g_scale), _ptr(sums), _ptr(total),
                                  _ptr(ws), ws.numel(), _stream(z)), "gmp_nt_xent_grouped")
    return gz, sums, total


def dropout_fwd(x: Tensor, p: float, seed: int, stream_id: int) -> Tensor:
    _need(x, torch.float32, "x")
    if x.numel() % 4:
        raise L.GnnmpError("dropout: numel must be a multiple of 4")
    y = torch.empty_like(x)
    L.check(L.lib().gmp_dropout_fwd(_ptr(x), _ptr(y), x.numel(), float(p), seed & (2 ** 64 - 1), stream_id, _stream(x)),
            "gmp_dropout_fwd")
    return y


def relu_dropout_bwd(g: Tensor, act: Tensor, p: float, seed: int, stream_id: int) -> Tensor:
    _need(g, torch.float32, "g"); _need(act, torch.float32, "act")
    if g.shape != act.shape or g.numel() % 4:
        raise L.GnnmpError("relu_dropout_bwd: shapes")
    out = torch.empty_like(g)
    L.check(L.lib().gmp_relu_dropout_bwd(_ptr(g), _ptr(act), _ptr(out), g.numel(), float(p), seed & (2 ** 64 - 1),
                                         stream_id, _stream(g)), "gmp_relu_dropout_bwd")
    return out


def _loss_ws(n: int, device) -> Tensor:
    return _ws(L.lib().gmp_loss_workspace_bytes(n), device)


def mse_sum_fwd(a: Tensor, b: Tensor) -> Tensor:
    _need(a, torch.float32, "a"); _need(b, torch.float32, "b")
    if a.shape != b.shape:
        raise L.GnnmpError(f"mse_sum: shapes {tuple(a.shape)} vs {tuple(b.shape)}")
    loss = torch.empty(1, dtype=torch.float32, device=a.device)
    ws = _loss_ws(a.numel(), a.device)
    L.check(L.lib().gmp_mse_sum_fwd(_ptr(a), _ptr(b), a.numel(), _ptr(loss), _ptr(ws), ws.numel(), _stream(a)), "gmp_mse_sum_fwd")
    return loss


def mse_sum_bwd(a: Tensor, b: Tensor, g_scale: Tensor) -> Tensor:
    ga = torch.empty_like(a)
    L.check(L.lib().gmp_mse_sum_bwd(_ptr(a), _ptr(b), _ptr(g_scale), _ptr(ga), a.numel(), _stream(a)), "gmp_mse_sum_bwd")
    return ga


def sigmoid_fwd(x: Tensor) -> Tensor:
    _need(x, torch.float32, "x")
    y = torch.empty_like(x)
    L.check(L.lib().gmp_sigmoid_fwd(_ptr(x), _ptr(y), x.numel(), _stream(x)), "gmp_sigmoid_fwd")
    return y


def sigmoid_bwd(g: Tensor, y: Tensor) -> Tensor:
    _need(g, torch.float32, "g")
    out = torch.empty_like(y)
    L.check(L.lib().gmp_sigmoid_bwd(_ptr(g), _ptr(y), _ptr(out), y.numel(), _stream(y)), "gmp_sigmoid_bwd")
    return out


def bce_sum_fwd(p: Tensor, labels: Tensor) -> Tensor:
    _need(p, torch.float32, "p"); _need(labels, torch.float32, "labels")
    if p.shape != labels.shape:
        raise L.GnnmpError("bce_sum: shapes differ")
    loss = torch.empty(1, dtype=torch.float32, device=p.device)
    ws = _loss_ws(p.numel(), p.device)
    L.check(L.lib().gmp_bce_sum_fwd(_ptr(p), _ptr(labels), p.numel(), _ptr(loss), _ptr(ws), ws.numel(), _stream(p)), "gmp_bce_sum_fwd")
    return loss


def bce_sum_bwd(p: Tensor, labels: Tensor, g_scale: Tensor) -> Tensor:
    gp = torch.empty_like(p)
    L.check(L.lib().gmp_bce_sum_bwd(_ptr(p), _ptr(labels), _ptr(g_scale), _ptr(gp), p.numel(), _stream(p)), "gmp_bce_sum_bwd")
    return gp


def _sigmoid_bce(fn: str, x: Tensor, y: Tensor, g_scale: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    _need(x, torch.float32, "x", 1); _need(y, torch.float32, "labels", 1); _need(g_scale, torch.float32, "g_scale")
    if x.shape != y.shape:
        raise L.GnnmpError(f"{fn}: shapes {tuple(x.shape)} vs {tuple(y.shape)}")
    loss = torch.empty(1, dtype=torch.float32, device=x.device)
    p, gx = torch.empty_like(x), torch.empty_like(x)
    ws = _loss_ws(x.numel(), x.device)
    L.check(getattr(L.lib(), fn)(_ptr(x), _ptr(y), x.numel(), _ptr(g_scale), _ptr(loss), _ptr(p), _ptr(gx), _ptr(ws), ws.numel(),
                                 _stream(x)), fn)
    return loss, p, gx


def sigmoid_bce_sum_fwd_bwd(x: Tensor, labels: Tensor, g_scale: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """(loss_sum [1], sigmoid(x), d (g_scale * loss_sum) / d x) in one pass (gmp_sigmoid_bce_sum_fwd_bwd)."""
    return _sigmoid_bce("gmp_sigmoid_bce_sum_fwd_bwd", x, labels, g_scale)


def sigmoid_bce_signed_sum_fwd_bwd(x: Tensor, signed_weight: Tensor, g_scale: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """The same pass with signed_weight[i] = +w (positive pair) / -w (negative pair): loss term and gradient scaled by w."""
    return _sigmoid_bce("gmp_sigmoid_bce_signed_sum_fwd_bwd", x, signed_weight, g_scale)


def cross_entropy_sum_fwd(logits: Tensor, target: Tensor) -> Tensor:
    _need(logits, torch.float32, "logits", 2); _need(target, torch.int64, "target", 1)
    if target.numel() != logits.size(0):
        raise L.GnnmpError("cross_entropy: target length")
    loss = torch.empty(1, dtype=torch.float32, device=logits.device)
    ws = _loss_ws(logits.size(0), logits.device)
    L.check(L.lib().gmp_cross_entropy_sum_fwd(_ptr(logits), _ptr(target), logits.size(0), logits.size(1), _ptr(loss),
                                              _ptr(ws), ws.numel(), _stream(logits)), "gmp_cross_entropy_sum_fwd")
    return loss


def cross_entropy_sum_bwd(logits: Tensor, target: Tensor, g_scale: Tensor) -> Tensor:
    gl = torch.empty_like(logits)
    L.check(L.lib().gmp_cross_entropy_sum_bwd(_ptr(logits), _ptr(target), logits.size(0), logits.size(1), _ptr(g_scale),
                                              _ptr(gl), _stream(logits)), "gmp_cross_entropy_sum_bwd")
    return gl


def row_fill_(dst: Tensor, idx: Tensor, src: Tensor, broadcast: bool) -> Tensor:
    F = _feat_ok(dst, "dst")
    _need(idx, torch.int64, "idx", 1); _need(src, torch.float32, "src")
    if broadcast:
        if src.numel() != F:
            raise L.GnnmpError("row_fill: broadcast source must have F elements")
    elif tuple(src.shape) != (idx.numel(), F):
        raise L.GnnmpError("row_fill: source shape")
    L.check(L.lib().gmp_row_fill(_ptr(dst), _ptr(idx), _ptr(src), idx.numel(), dst.size(0), F, int(broadcast), _stream(dst)),
            "gmp_row_fill")
    return dst


# ---- device-side augmentation and masking (csrc/augment.hip) ---------------------------------------------
def view_sizes(ptr_host) -> Tuple[list, list]:
    """Per-graph kept-node counts of an augmented view and masked-node counts of node-feature masking: functions of the graph
    sizes alone (augmentations.py:49-50, pretrain_model.py:75-76), so the host lays out offsets without asking the device."""
    n = [int(b - a) for a, b in zip(ptr_host[:-1], ptr_host[1:])]
    kept = [v - max(1, int(v * 0.2)) if v >= 3 else v for v in n]
    masked = [max(1, int(v * 0.15)) if v >= 3 else 0 for v in n]
    return kept, masked


class DeviceViews(NamedTuple):
    """gmp_aug_two_views outputs of one domain batch (all on the device): per view rows / rowmask / edges [2, ecap] / common, plus
    counts [3G] (edges view 1, edges view 2, common, per graph) and totals [5] (E1, E2, common, mask flag 1, mask flag 2)."""
    rows: Tuple[Tensor, Tensor]
    rowmask: Tuple[Tensor, Tensor]
    edges: Tuple[Tensor, Tensor]
    common: Tuple[Tensor, Tensor]
    counts: Tensor
    totals: Tensor
    view_ptr: list


def aug_node_masks(ptr: Tensor, ptr_host, seed: int, stream_id: int) -> Tensor:
    """Node-feature-masking indices of a domain batch, drawn on the device (pretrain_model.py:71-80's per-graph loop)."""
    _need(ptr, torch.int64, "ptr", 1)
    _, masked = view_sizes(ptr_host)
    off = [0]
    for m in masked:
        off.append(off[-1] + m)
    out = torch.empty(off[-1], dtype=torch.int64, device=ptr.device)
    if off[-1] == 0:
        return out
    out_ptr = torch.tensor(off, dtype=torch.int64).to(ptr.device)
    G = len(ptr_host) - 1
    L.check(L.lib().gmp_aug_node_masks(_ptr(ptr), _ptr(out_ptr), G, max(int(b - a) for a, b in zip(ptr_host[:-1], ptr_host[1:])),
                                       seed & (2 ** 64 - 1), stream_id & 0xffffffff, _ptr(out), _stream(ptr)), "gmp_aug_node_masks")
    return out


def aug_two_views(ptr: Tensor, eptr: Tensor, edge_index: Tensor, ptr_host, eptr_host, num_features: int, seed: int,
                  stream_id: int) -> DeviceViews:
    """GraphAugmentor.create_two_views (augmentations.py:88-111) of a domain batch on the device."""
    _need(ptr, torch.int64, "ptr", 1); _need(eptr, torch.int64, "eptr", 1); _need(edge_index, torch.int64, "edge_index", 2)
    dev, G = ptr.device, len(ptr_host) - 1
    N, E = int(ptr_host[-1]), int(edge_index.size(1))
    kept, _ = view_sizes(ptr_host)
    vp = [0]
    for k in kept:
        vp.append(vp[-1] + k)
    vptr = torch.tensor(vp, dtype=torch.int64).to(dev)
    mk = lambda n, dt=torch.int64: torch.empty(n, dtype=dt, device=dev)
    rows, masks = (mk(vp[-1]), mk(vp[-1])), (mk(vp[-1]), mk(vp[-1]))
    edges, common = (mk(2 * max(E, 1)).view(2, -1), mk(2 * max(E, 1)).view(2, -1)), (mk(vp[-1]), mk(vp[-1]))
    counts, totals = mk(5 * max(G, 1), torch.int32), mk(5, torch.int32)
    l = L.lib()
    ws = _ws(l.gmp_aug_workspace_bytes(N, E, G), dev)
    L.check(l.gmp_aug_two_views(_ptr(ptr), _ptr(eptr), _ptr(edge_index.contiguous()), N, E, _ptr(vptr), G,
                                max([int(b - a) for a, b in zip(ptr_host[:-1], ptr_host[1:])] + [0]),
                                max([int(b - a) for a, b in zip(eptr_host[:-1], eptr_host[1:])] + [0]), num_features,
                                seed & (2 ** 64 - 1), stream_id & 0xffffffff, _ptr(rows[0]), _ptr(rows[1]), _ptr(masks[0]), _ptr(masks[1]),
                                _ptr(edges[0]), _ptr(edges[1]), max(E, 1), _ptr(common[0]), _ptr(common[1]), _ptr(counts), _ptr(totals),
                                _ptr(ws), ws.numel(), _stream(ptr)), "gmp_aug_two_views")
    return DeviceViews(rows, masks, edges, common, counts, totals, vp)


def aug_node_masks_batch(jobs, seed: int):
    """gmp_aug_node_masks for several domain batches in ONE launch.  jobs: [(ptr, ptr_host, stream_id)]; returns a list of index tensors
    identical to aug_node_masks(ptr, ptr_host, seed, stream_id) per job."""
    outs, cjobs, keep, nmax = [], [], [], 1
    for ptr, ptr_host, sid in jobs:
        _need(ptr, torch.int64, "ptr", 1)
        _, masked = view_sizes(ptr_host)
        off = [0]
        for m in masked:
            off.append(off[-1] + m)
        out = torch.empty(off[-1], dtype=torch.int64, device=ptr.device)
        outs.append(out)
        if off[-1] == 0:
            continue
        out_ptr = torch.tensor(off, dtype=torch.int64).to(ptr.device)
        keep.append(out_ptr)
        nmax = max(nmax, max(int(b - a) for a, b in zip(ptr_host[:-1], ptr_host[1:])))
        cjobs.append(L.AugMasksJob(_ptr(ptr), _ptr(out_ptr), len(ptr_host) - 1, sid & 0xffffffff, _ptr(out)))
    if cjobs:
        L.check(L.lib().gmp_aug_node_masks_batch((L.AugMasksJob * len(cjobs))(*cjobs), len(cjobs), nmax, seed & (2 ** 64 - 1), _stream(jobs[0][0])),
                "gmp_aug_node_masks_batch")
    return outs


def aug_two_views_batch(jobs, seed: int):
    """gmp_aug_two_views for several domain batches in TWO launches.  jobs: [(ptr, eptr, edge_index, ptr_host, eptr_host, num_features,
    stream_id)]; returns a list of DeviceViews identical to aug_two_views(..., seed, stream_id) per job."""
    res, cjobs, keep, nmax, emax = [], [], [], 1, 0
    l = L.lib()
    for ptr, eptr, edge_index, ptr_host, eptr_host, F, sid in jobs:
        dev, G = ptr.device, len(ptr_host) - 1
        N, E = int(ptr_host[-1]), int(edge_index.size(1))
        kept, _ = view_sizes(ptr_host)
        vp = [0]
        for k in kept:
            vp.append(vp[-1] + k)
        vptr = torch.tensor(vp, dtype=torch.int64).to(dev)
        mk = lambda n, dt=torch.int64: torch.empty(n, dtype=dt, device=dev)
        rows, masks = (mk(vp[-1]), mk(vp[-1])), (mk(vp[-1]), mk(vp[-1]))
        edges, common = (mk(2 * max(E, 1)).view(2, -1), mk(2 * max(E, 1)).view(2, -1)), (mk(vp[-1]), mk(vp[-1]))
        counts, totals = mk(5 * max(G, 1), torch.int32), mk(5, torch.int32)
        ws = _ws(l.gmp_aug_workspace_bytes(N, E, G), dev).clone()          # (one region per job: the jobs of a launch run concurrently)
        ei = edge_index.contiguous()
        keep += [vptr, ws, ei]
        nmax = max([nmax] + [int(b - a) for a, b in zip(ptr_host[:-1], ptr_host[1:])])
        emax = max([emax] + [int(b - a) for a, b in zip(eptr_host[:-1], eptr_host[1:])])
        cjobs.append(L.AugViewsJob(_ptr(ptr), _ptr(eptr), _ptr(ei), N, E, _ptr(vptr), G, F, sid & 0xffffffff, _ptr(rows[0]), _ptr(rows[1]),
                                   _ptr(masks[0]), _ptr(masks[1]), _ptr(edges[0]), _ptr(edges[1]), max(E, 1), _ptr(common[0]), _ptr(common[1]),
                                   _ptr(counts), _ptr(totals), _ptr(ws), ws.numel()))
        res.append(DeviceViews(rows, masks, edges, common, counts, totals, vp))
    if cjobs:
        L.check(l.gmp_aug_two_views_batch((L.AugViewsJob * len(cjobs))(*cjobs), len(cjobs), nmax, emax, seed & (2 ** 64 - 1), _stream(jobs[0][0])),
                "gmp_aug_two_views_batch")
        torch.cuda.current_stream(jobs[0][0].device).synchronize()          # (the per-job scratch above dies with this frame)
    return res


NEG_MAX_GRAPH_NODES = 1024          # gmp_aug_negative_edges: nodes per graph


def negative_capacity(ptr_host, num_neg: int) -> int:
    """sum_g min(num_neg, n_g (n_g - 1)): the host-known bound on a batch's negatives that sizes gmp_aug_negative_edges' output."""
    return sum(min(int(num_neg), int(b - a) * (int(b - a) - 1)) for a, b in zip(ptr_host[:-1], ptr_host[1:]) if b - a >= 2)


def batched_negative_sampling(edge_index: Tensor, ptr: Tensor, eptr: Tensor, num_neg: int, seed: int,
                              stream_id: int = 0) -> Tuple[Tensor, Tensor]:
    """batched_negative_sampling(to_undirected(edge_index), batch, num_neg) of a domain batch on the device (gmp_aug_negative_edges;
    the rule and its two departures from PyG: include/gnnmp.h).  edge_index [2, E], ptr / eptr [G + 1]: int64 on the device, batch
    numbering.  Returns (neg [2, K] int64 on the device, counts [G] int32): graph g's counts[g] pairs in ascending code order, graphs
    in batch order.  Synchronises (K is read back)."""
    _need(ptr, torch.int64, "ptr", 1); _need(eptr, torch.int64, "eptr", 1); _need(edge_index, torch.int64, "edge_index", 2)
    if ptr.numel() != eptr.numel() or edge_index.size(0) != 2 or num_neg < 0:
        raise L.GnnmpError("batched_negative_sampling: ptr / eptr / edge_index [2, E] / num_neg >= 0 do not fit together")
    dev, G = ptr.device, ptr.numel() - 1
    if G <= 0:
        return torch.empty(2, 0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    ptr_host = ptr.cpu().tolist()
    N, E = int(ptr_host[-1]), int(edge_index.size(1))
    nmax = max(int(b - a) for a, b in zip(ptr_host[:-1], ptr_host[1:]))
    cap = max(negative_capacity(ptr_host, num_neg) if nmax <= NEG_MAX_GRAPH_NODES else 0, 1)
    neg = torch.empty(2, cap, dtype=torch.int64, device=dev)
    counts, total = torch.empty(G, dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    l = L.lib()
    ws = _ws(l.gmp_aug_negative_edges_workspace_bytes(N, nmax, cap), dev)
    L.check(l.gmp_aug_negative_edges(_ptr(ptr), _ptr(eptr), _ptr(edge_index) if E else None, N, E, G, nmax, int(num_neg), seed & (2 ** 64 - 1),
                                     stream_id & 0xffffffff, _ptr(neg), cap, _ptr(counts), _ptr(total), _ptr(ws), ws.numel(), _stream(ptr)),
            "gmp_aug_negative_edges")
    return neg[:, :int(total.item())], counts


def batched_negative_sampling_batch(jobs, seed: int):
    """gmp_aug_negative_edges for several domain batches in TWO launches.  jobs: [(edge_index, ptr, eptr, num_neg, stream_id)]; returns a
    list of (neg, counts) identical to batched_negative_sampling(..., seed, stream_id) per job."""
    l = L.lib()
    hosts = [ptr.cpu().tolist() for _, ptr, _, _, _ in jobs]
    nmax = max([1] + [int(b - a) for h in hosts for a, b in zip(h[:-1], h[1:])])
    res, cjobs, keep = [], [], []
    for (ei, ptr, eptr, num_neg, sid), h in zip(jobs, hosts):
        _need(ptr, torch.int64, "ptr", 1); _need(eptr, torch.int64, "eptr", 1); _need(ei, torch.int64, "edge_index", 2)
        dev, G = ptr.device, len(h) - 1
        N, E = int(h[-1]), int(ei.size(1))
        cap = max(negative_capacity(h, num_neg) if nmax <= NEG_MAX_GRAPH_NODES else 0, 1)
        neg = torch.empty(2, cap, dtype=torch.int64, device=dev)
        counts, total = torch.empty(max(G, 0), dtype=torch.int32, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
        ws = _ws(l.gmp_aug_negative_edges_workspace_bytes(N, nmax, cap), dev)          # (one region per job: the jobs of a launch run concurrently)
        keep.append(ws)
        cjobs.append(L.AugNegJob(_ptr(ptr), _ptr(eptr), _ptr(ei) if E else None, N, E, G, sid & 0xffffffff, int(num_neg), _ptr(neg), cap,
                                 _ptr(counts), _ptr(total), _ptr(ws), ws.numel()))
        res.append((neg, counts, total))
    if cjobs:
        L.check(l.gmp_aug_negative_edges_batch((L.AugNegJob * len(cjobs))(*cjobs), len(cjobs), nmax, seed & (2 ** 64 - 1), _stream(jobs[0][1])),
                "gmp_aug_negative_edges_batch")
    return [(neg[:, :int(total.item())], counts) for neg, counts, total in res]


def dropout_rowdot_fwd(x: Tensor, w: Tensor, bias: Optional[Tensor], p: float, seed: int, stream_id: int):
    """(dropout(x), dropout(x) @ w + bias) for a Linear(F, 1) (gmp_dropout_rowdot_fwd); the dropped copy is x itself when p == 0."""
    _need(x, torch.float32, "x", 2)
    rows, F = x.shape
    d = torch.empty_like(x) if p > 0 else x
    y = torch.empty(rows, dtype=torch.float32, device=x.device)
    L.check(L.lib().gmp_dropout_rowdot_fwd(_ptr(x), _ptr(w), _ptr(bias), _ptr(d), _ptr(y), rows, F, float(p), seed & (2 ** 64 - 1), stream_id,
                                           _stream(x)), "gmp_dropout_rowdot_fwd")
    return d, y


def outer_relu_dropout_bwd(g: Tensor, w: Tensor, act: Tensor, p: float, seed: int, stream_id: int) -> Tensor:
    """g[m] * w[c] pushed through the dropout mask of the forward and the ReLU whose output was `act` (gmp_outer_relu_dropout_bwd)."""
    rows, F = act.shape
    out = torch.empty_like(act)
    L.check(L.lib().gmp_outer_relu_dropout_bwd(_ptr(g), _ptr(w), _ptr(act), _ptr(out), rows, F, float(p), seed & (2 ** 64 - 1), stream_id,
                                               _stream(act)), "gmp_outer_relu_dropout_bwd")
    return out


def weighted_colsum(g: Tensor, x: Tensor):
    """(sum_m g[m] x[m, :], sum_m g[m]) -- weight and bias gradient of a Linear(F, 1) (gmp_weighted_colsum)."""
    rows, F = x.shape
    ow = torch.empty(F, dtype=torch.float32, device=x.device)
    ob = torch.empty(1, dtype=torch.float32, device=x.device)
    l = L.lib()
    ws = _ws(l.gmp_weighted_colsum_workspace_bytes(rows, F), x.device)
    L.check(l.gmp_weighted_colsum(_ptr(g), _ptr(x), _ptr(ow), _ptr(ob), rows, F, _ptr(ws), ws.numel(), _stream(x)), "gmp_weighted_colsum")
    return ow, ob


def lp_pair_head(y1: Tensor, w: Tensor, bias: Tensor, pos: Tensor, sign: Tensor, g_scale: Tensor, p: float, seed: int, stream_id: int):
    """The link-prediction scorer's tail over MERGED rows (one per unordered pair), one dropout mask / score / BCE term per ORDERED row of the
    reference's list (heads.py:44-52, tasks.py:111-120; gnnmp.h gmp_lp_pair_*).  y1 [K, F] = ReLU output of the 768 -> 256 layer, pos [2, K] int32
    ordered positions (second -1 = none), sign [K] (> 0: positive pair).  Returns (y2 [2, K], loss_sum [1], g_y2 [2, K], g_y1 [K, F], g_w [F], g_b [1])."""
    _need(y1, torch.float32, "y1", 2)
    _need(pos, torch.int32, "pos", 2)
    K, F = y1.shape
    l, dev, st, sd = L.lib(), y1.device, _stream(y1), seed & (2 ** 64 - 1)
    y2, g_y2, prob = (torch.empty(2, K, dtype=torch.float32, device=dev) for _ in range(3))
    loss, g_w, g_b, g_y1 = torch.zeros(1, device=dev), torch.empty(F, device=dev), torch.empty(1, device=dev), torch.empty_like(y1)
    lws = _ws(l.gmp_loss_workspace_bytes(2 * K), dev)
    L.check(l.gmp_lp_pair_rowdot_fwd(_ptr(y1), _ptr(w), _ptr(bias), _ptr(pos), _ptr(y2), K, F, float(p), sd, stream_id, st), "gmp_lp_pair_rowdot_fwd")
    L.check(l.gmp_lp_pair_sigmoid_bce_fwd_bwd(_ptr(y2), _ptr(sign), _ptr(pos), K, _ptr(g_scale), _ptr(loss), _ptr(prob), _ptr(g_y2), _ptr(lws), lws.numel(), st),
            "gmp_lp_pair_sigmoid_bce_fwd_bwd")
    L.check(l.gmp_lp_pair_outer_bwd(_ptr(g_y2), _ptr(w), _ptr(y1), _ptr(pos), _ptr(g_y1), K, F, float(p), sd, stream_id, st), "gmp_lp_pair_outer_bwd")
    ws = _ws(l.gmp_lp_pair_colsum_workspace_bytes(K, F), dev).clone()
    L.check(l.gmp_lp_pair_weighted_colsum(_ptr(g_y2), _ptr(y1), _ptr(pos), _ptr(g_w), _ptr(g_b), K, F, float(p), sd, stream_id, _ptr(ws), ws.numel(), st),
            "gmp_lp_pair_weighted_colsum")
    return y2, loss, g_y2, g_y1, g_w, g_b


def lp_score_fwd(h: Tensor, src: Tensor, dst: Tensor, w0: Tensor, b0: Tensor, w3: Tensor, b3: Tensor, p: float = 0.0, seed: int = 0,
                 site: int = 0) -> Tuple[Tensor, Tensor]:
    """The fused link-prediction scorer up to the logit (gnnmp.h gmp_lp_score_fwd): h [N, 256], src / dst int64 [K], w0 [256, 768],
    b0 [256], w3 [1, 256] or [256], b3 [1].  Returns (act [K, 256] = the pre-dropout ReLU output, logit [K])."""
    _need(h, torch.float32, "h", 2)
    _need(src, torch.int64, "src", 1); _need(dst, torch.int64, "dst", 1)
    for t, n in ((w0, "w0"), (b0, "b0"), (w3, "w3"), (b3, "b3")):
        _need(t, torch.float32, n)
    K, dev, l = src.numel(), h.device, L.lib()
    if dst.numel() != K:
        raise L.GnnmpError("lp_score_fwd: src and dst differ in length")
    act, logit = torch.empty(K, w0.size(0), device=dev), torch.empty(K, device=dev)
    ws = _ws(l.gmp_lp_score_fwd_workspace_bytes(K), dev)
    L.check(l.gmp_lp_score_fwd(_ptr(h), _ptr(src), _ptr(dst), h.size(0), K, h.size(1), w0.size(0), _ptr(w0), _ptr(b0), _ptr(w3), _ptr(b3),
                               _ptr(act), _ptr(logit), float(p), seed & (2 ** 64 - 1), site, _ptr(ws), ws.numel(), _stream(h)), "gmp_lp_score_fwd")
    return act, logit


def lp_score_bwd(h: Tensor, src: Tensor, dst: Tensor, w0: Tensor, w3: Tensor, act: Tensor, g_logit: Tensor, p: float = 0.0, seed: int = 0,
                 site: int = 0) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Backward of lp_score_fwd from d loss / d logit (gnnmp.h gmp_lp_score_bwd).  Returns (g_w0 [256, 768], g_b0 [256], g_w3 [256],
    g_b3 [1], g_hs [K, 256], g_hd [K, 256]); lp_score_node_grad reduces the last two onto nodes."""
    _need(act, torch.float32, "act", 2); _need(g_logit, torch.float32, "g_logit", 1)
    K, dev, l = src.numel(), h.device, L.lib()
    Hd, F = w0.size(0), h.size(1)
    g_w0, g_b0, g_w3, g_b3 = torch.empty_like(w0), torch.empty(Hd, device=dev), torch.empty(Hd, device=dev), torch.empty(1, device=dev)
    g_hs, g_hd = torch.empty(K, F, device=dev), torch.empty(K, F, device=dev)
    ws = _ws(l.gmp_lp_score_bwd_workspace_bytes(K), dev)
    L.check(l.gmp_lp_score_bwd(_ptr(h), _ptr(src), _ptr(dst), h.size(0), K, F, Hd, _ptr(w0), _ptr(w3), _ptr(act), _ptr(g_logit), float(p),
                               seed & (2 ** 64 - 1), site, _ptr(g_w0), _ptr(g_b0), _ptr(g_w3), _ptr(g_b3), 0, _ptr(g_hs), _ptr(g_hd),
                               _ptr(ws), ws.numel(), _stream(h)), "gmp_lp_score_bwd")
    return g_w0, g_b0, g_w3, g_b3, g_hs, g_hd


def lp_score_node_grad(g_hs: Tensor, g_hd: Tensor, pairs: Tensor, num_nodes: int) -> Tensor:
    """g_h[i] = sum of g_hs over the pairs whose source is i + sum of g_hd over those whose destination is i (fixed order: csr_build +
    two segment_sums, the backward of operators.lp_edge_features).  pairs int64 [2, K] contiguous; a pair with an endpoint outside
    [0, num_nodes) is dropped by csr_build and gives no node gradient."""
    csr = csr_build(pairs, num_nodes)
    gh = segment_sum(g_hs, csr.rowptr_t, csr.perm_t)
    return segment_sum(g_hd, csr.rowptr, csr.perm, out=gh, accumulate=True)


def _lp_filter_args(who: str, num_nodes: int, filter_rowptr: Optional[Tensor], filter_col: Optional[Tensor]) -> int:
    """The entry count of a ranker's optional filter CSR (int32 rowptr [num_nodes + 1] / col), 0 without one."""
    if (filter_rowptr is None) != (filter_col is None):
        raise L.GnnmpError(f"{who}: filter_rowptr and filter_col go together")
    if filter_rowptr is None:
        return 0
    _need(filter_rowptr, torch.int32, "filter_rowptr", 1); _need(filter_col, torch.int32, "filter_col", 1)
    if filter_rowptr.numel() != num_nodes + 1:
        raise L.GnnmpError(f"{who}: filter_rowptr has {filter_rowptr.numel()} entries for {num_nodes} nodes")
    return filter_col.numel()


def _lp_rank_args(who: str, h: Tensor, w0: Tensor, b0: Tensor, w3: Tensor, b3: Tensor, filter_rowptr: Optional[Tensor],
                  filter_col: Optional[Tensor]) -> int:
    _need(h, torch.float32, "h", 2)
    for t, n in ((w0, "w0"), (b0, "b0"), (w3, "w3"), (b3, "b3")):
        _need(t, torch.float32, n)
    return _lp_filter_args(who, h.size(0), filter_rowptr, filter_col)


def _rank_call(who: str, fn, lead, workspace_bytes, src: Tensor, dst: Tensor, num_nodes: int, filter_rowptr: Optional[Tensor],
               filter_col: Optional[Tensor], anchor: Tensor, extra: tuple = ()) -> Tuple[Tensor, Tensor, Tensor]:
    """The call of the all-candidate ranker fn = gmp_{who} behind its scorer's own checks: the pairs and the filter CSR checked, the three
    outputs and the workspace (workspace_bytes(Q)) allocated where `anchor` lives.  lead(src, dst, Q) gives the C arguments up to the
    filter, `extra` those between n_equal and the workspace.  Returns (score_true [Q], n_greater [Q] int32, n_equal [Q] int32)."""
    fnnz = _lp_filter_args(who, num_nodes, filter_rowptr, filter_col)
    _need(src, torch.int64, "src", 1); _need(dst, torch.int64, "dst", 1)
    Q, dev = src.numel(), anchor.device
    if dst.numel() != Q:
        raise L.GnnmpError(f"{who}: src and dst differ in length")
    score = torch.empty(Q, device=dev)
    n_greater, n_equal = torch.empty(Q, dtype=torch.int32, device=dev), torch.empty(Q, dtype=torch.int32, device=dev)
    ws = _ws(workspace_bytes(Q), dev)
    L.check(fn(*lead(_ptr(src), _ptr(dst), Q), _ptr(filter_rowptr), _ptr(filter_col), fnnz, _ptr(score), _ptr(n_greater),
                                           _ptr(n_equal), *extra, _ptr(ws), ws.numel(), _stream(anchor)), f"gmp_{who}")
    return score, n_greater, n_equal


def _score_call(who: str, fn, lead, workspace_bytes, src: Tensor, dst: Tensor, anchor: Tensor) -> Tensor:
    """_rank_call for the pair scorer fn = gmp_{who}: score [P] of the pairs (src[p], dst[p]).  workspace_bytes None: it takes no workspace."""
    _need(src, torch.int64, "src", 1); _need(dst, torch.int64, "dst", 1)
    P, dev = src.numel(), anchor.device
    if dst.numel() != P:
        raise L.GnnmpError(f"{who}: src and dst differ in length")
    score = torch.empty(P, device=dev)
    ws = None if workspace_bytes is None else _ws(workspace_bytes(P), dev)
    L.check(fn(*lead(_ptr(src), _ptr(dst), P), _ptr(score), *(() if ws is None else (_ptr(ws), ws.numel())),
                                           _stream(anchor)), f"gmp_{who}")
    return score


def lp_rank(h: Tensor, src: Tensor, dst: Tensor, w0: Tensor, b0: Tensor, w3: Tensor, b3: Tensor, filter_rowptr: Optional[Tensor] = None,
            filter_col: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Every true pair (src[q], dst[q]) ranked against all nodes of h [N, 256] (gnnmp.h gmp_lp_rank): returns (logit_true [Q],
    n_greater [Q] int32, n_equal [Q] int32) over the candidates c other than src[q], dst[q] and the entries of src[q]'s row of the
    optional filter CSR (int32 rowptr [N + 1] / col, row = source).  Logits are those of lp_score_fwd with p = 0, bit for bit."""
    _lp_rank_args("lp_rank", h, w0, b0, w3, b3, filter_rowptr, filter_col)
    N = h.size(0)
    return _rank_call("lp_rank", L.lib().gmp_lp_rank, lambda s, d, Q: (_ptr(h), s, d, N, Q, h.size(1), w0.size(0), _ptr(w0), _ptr(b0), _ptr(w3), _ptr(b3)),
                      lambda Q: L.lib().gmp_lp_rank_workspace_bytes(Q, N), src, dst, N, filter_rowptr, filter_col, h)


def lp_topk(h: Tensor, src: Tensor, k: int, w0: Tensor, b0: Tensor, w3: Tensor, b3: Tensor, filter_rowptr: Optional[Tensor] = None,
            filter_col: Optional[Tensor] = None) -> Tuple[Tensor, Tensor]:
    """The k (1 <= k <= 64) best destinations of every source over all nodes of h [N, 256] (gnnmp.h gmp_lp_topk): returns (idx [Q, k]
    int64, logit [Q, k]), logit descending, ties to the lower node index, the source itself and its filter row left out; a row with
    fewer than k candidates is padded with -1 / -inf."""
    nnz = _lp_rank_args("lp_topk", h, w0, b0, w3, b3, filter_rowptr, filter_col)
    _need(src, torch.int64, "src", 1)
    if not 1 <= int(k) <= 64:
        raise L.GnnmpError(f"lp_topk: k={k} (1 <= k <= 64)")
    Q, N, dev, l = src.numel(), h.size(0), h.device, L.lib()
    idx, logit = torch.empty(Q, k, dtype=torch.int64, device=dev), torch.empty(Q, k, device=dev)
    ws = _ws(l.gmp_lp_topk_workspace_bytes(Q, N), dev)
    L.check(l.gmp_lp_topk(_ptr(h), _ptr(src), N, Q, int(k), h.size(1), w0.size(0), _ptr(w0), _ptr(b0), _ptr(w3), _ptr(b3), _ptr(filter_rowptr),
                          _ptr(filter_col), nnz, _ptr(idx), _ptr(logit), _ptr(ws), ws.numel(), _stream(h)), "gmp_lp_topk")
    return idx, logit


LP_CN_MODES = {"sum": 0, "jaccard": 1}                      # gmp_lp_cn_score / gmp_lp_cn_rank (gnnmp.h)


def _simple_graph_args(who: str, rowptr: Tensor, col: Tensor, mode: str, modes: Dict[str, int]) -> Tuple[int, int, int]:
    """(num_nodes, nnz, mode code) of a simple-graph CSR and its scorer's mode out of `modes` (gnnmp.h gmp_lp_cn_score, gmp_lp_walk_score)."""
    _need(rowptr, torch.int32, "rowptr", 1); _need(col, torch.int32, "col", 1)
    if rowptr.numel() < 1:
        raise L.GnnmpError(f"{who}: rowptr is empty (it has num_nodes + 1 entries)")
    if mode not in modes:
        raise L.GnnmpError(f"{who}: mode={mode!r} is not one of {tuple(modes)}")
    return rowptr.numel() - 1, col.numel(), modes[mode]


def _node_weight_arg(who: str, weight: Optional[Tensor], num_nodes: int, refusal: Optional[str]) -> None:      # refusal: of a mode that takes none
    if weight is not None:
        _need(weight, torch.float32, "weight", 1)
        if refusal:
            raise L.GnnmpError(f"{who}: {refusal}")
        if weight.numel() != num_nodes:
            raise L.GnnmpError(f"{who}: weight has {weight.numel()} entries for {num_nodes} nodes")


def lp_cn_score(rowptr: Tensor, col: Tensor, src: Tensor, dst: Tensor, weight: Optional[Tensor] = None, mode: str = "sum") -> Tensor:
    """The neighbourhood score of every pair (src[p], dst[p]) on the simple undirected graph (rowptr, col) (int32 CSR: symmetric, no
    loops, rows strictly ascending; gnnmp.h gmp_lp_cn_score): mode "sum" the fp32 sum of weight[z] over the common neighbours z in
    ascending z (weight None: 1, the common-neighbour count), mode "jaccard" CN / (deg s + deg d - CN).  A pair with an endpoint outside
    the graph scores 0."""
    N, nnz, code = _simple_graph_args("lp_cn_score", rowptr, col, mode, LP_CN_MODES)
    _node_weight_arg("lp_cn_score", weight, N, "Jaccard takes no weight array" if mode == "jaccard" else None)
    return _score_call("lp_cn_score", L.lib().gmp_lp_cn_score, lambda s, d, P: (_ptr(rowptr), _ptr(col), N, nnz, s, d, P, _ptr(weight), code), None, src, dst, rowptr)


def lp_cn_rank(rowptr: Tensor, col: Tensor, src: Tensor, dst: Tensor, weight: Optional[Tensor] = None, mode: str = "sum",
               filter_rowptr: Optional[Tensor] = None, filter_col: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Every true pair (src[q], dst[q]) ranked against all nodes with lp_cn_score's scorer (gnnmp.h gmp_lp_cn_rank): returns
    (score_true [Q], n_greater [Q] int32, n_equal [Q] int32) over the candidates c other than src[q], dst[q] and the entries of
    src[q]'s row of the optional filter CSR (lp_rank's).  A candidate's score has the bits lp_cn_score gives the pair; Jaccard is
    compared exactly in integers.  Nothing of size Q x N is allocated."""
    N, nnz, code = _simple_graph_args("lp_cn_rank", rowptr, col, mode, LP_CN_MODES)
    _node_weight_arg("lp_cn_rank", weight, N, "Jaccard takes no weight array" if mode == "jaccard" else None)
    return _rank_call("lp_cn_rank", L.lib().gmp_lp_cn_rank, lambda s, d, Q: (_ptr(rowptr), _ptr(col), N, nnz, s, d, Q, _ptr(weight), code),
                      lambda Q: L.lib().gmp_lp_cn_rank_workspace_bytes(Q, N), src, dst, N, filter_rowptr, filter_col, rowptr)


LP_WALK_MODES = {"sum": 0, "hops": 1}                       # gmp_lp_walk_score / gmp_lp_walk_rank (gnnmp.h)
LP_WALK_MAX_ROUNDS = 64


def _lp_walk_args(who: str, rowptr: Tensor, col: Tensor, rounds: int, damping: float, weight: Optional[Tensor], mode: str):
    """_simple_graph_args and the walk's own two, as a function of (src, dst, count) that gives the C arguments up to the scorer's end."""
    N, nnz, code = _simple_graph_args(who, rowptr, col, mode, LP_WALK_MODES)
    if not 1 <= int(rounds) <= LP_WALK_MAX_ROUNDS:
        raise L.GnnmpError(f"{who}: rounds={rounds} (1 <= rounds <= {LP_WALK_MAX_ROUNDS})")
    if mode == "sum" and not 0.0 < float(damping) <= 1.0:
        raise L.GnnmpError(f"{who}: damping={damping} (0 < damping <= 1)")
    _node_weight_arg(who, weight, N, "hops take no weight array" if mode == "hops" else None)
    return (N, lambda s, d, n: (_ptr(rowptr), _ptr(col), N, nnz, s, d, n, _ptr(weight), float(damping), int(rounds), code),
            lambda n: L.lib().gmp_lp_walk_workspace_bytes(n, N))


def lp_walk_score(rowptr: Tensor, col: Tensor, src: Tensor, dst: Tensor, rounds: int, damping: float = 1.0, weight: Optional[Tensor] = None,
                  mode: str = "sum") -> Tensor:
    """The walk score of every pair (src[p], dst[p]) on the simple undirected graph (rowptr, col) (int32 CSR, lp_cn_score's contract;
    gnnmp.h gmp_lp_walk_score): mode "sum" the fp32 sum over l <= rounds of y_l[dst], y_l = damping * A diag(weight) y_{l-1} from y_0 =
    e_src, every row folded in ascending neighbour order (weight None: 1); mode "hops" minus the BFS distance, -(rounds + 1) beyond
    `rounds` hops.  An endpoint outside the graph scores 0 / -(rounds + 1).  Pairs with equal sources next to each other share one
    propagation."""
    _, lead, workspace_bytes = _lp_walk_args("lp_walk_score", rowptr, col, rounds, damping, weight, mode)
    return _score_call("lp_walk_score", L.lib().gmp_lp_walk_score, lead, workspace_bytes, src, dst, rowptr)


def lp_walk_rank(rowptr: Tensor, col: Tensor, src: Tensor, dst: Tensor, rounds: int, damping: float = 1.0, weight: Optional[Tensor] = None,
                 mode: str = "sum", filter_rowptr: Optional[Tensor] = None, filter_col: Optional[Tensor] = None) -> Tuple[Tensor, Tensor, Tensor]:
    """Every true pair (src[q], dst[q]) ranked against all nodes with lp_walk_score's scorer (gnnmp.h gmp_lp_walk_rank): returns
    (score_true [Q], n_greater [Q] int32, n_equal [Q] int32) over the candidates c other than src[q], dst[q] and the entries of
    src[q]'s row of the optional filter CSR (lp_rank's).  A candidate's score has the bits lp_walk_score gives the pair.  One workgroup
    per query keeps its vectors in LDS (num_nodes <= gmp_lp_walk_lds_nodes()) or in a bounded workspace: nothing of size Q x N."""
    N, lead, workspace_bytes = _lp_walk_args("lp_walk_rank", rowptr, col, rounds, damping, weight, mode)
    return _rank_call("lp_walk_rank", L.lib().gmp_lp_walk_rank, lead, workspace_bytes, src, dst, N, filter_rowptr, filter_col, rowptr)


EMB_LINK_MODES = {"cos": 0, "dot": 1}                       # gmp_emb_link_score / gmp_emb_link_rank (gnnmp.h)
EMB_LINK_MAX_DIM = 256


def _emb_link_args(who: str, h: Tensor, src: Tensor, dst: Tensor, mode: str) -> Tuple[int, int, int]:
    """(num_nodes, number of pairs, mode code) of an embedding matrix and its pairs (gnnmp.h gmp_emb_link_score)."""
    if mode not in EMB_LINK_MODES:
        raise L.GnnmpError(f"{who}: mode={mode!r} is not one of {tuple(EMB_LINK_MODES)}")
    _need(h, torch.float32, "h", 2)
    _need(src, torch.int64, "src", 1); _need(dst, torch.int64, "dst", 1)
    if not 1 <= h.size(1) <= EMB_LINK_MAX_DIM:
        raise L.GnnmpError(f"{who}: dim={h.size(1)} (1 <= dim <= {EMB_LINK_MAX_DIM})")
    if dst.numel() != src.numel():
        raise L.GnnmpError(f"{who}: src and dst differ in length")
    return h.size(0), src.numel(), EMB_LINK_MODES[mode]


def emb_link_score(h: Tensor, src: Tensor, dst: Tensor, mode: str = "cos") -> Tensor:
    """The score of every pair (src[p], dst[p]) from the rows of h [N, d <= 256] alone (gnnmp.h gmp_emb_link_score; csrc/emb_link.hip):
    mode "cos" the cosine of the two rows, normalised as knn_topk normalises (a zero row scores 0), mode "dot" their inner product.  An
    endpoint outside [0, N) reads as a zero row.  Returns score [P]."""
    N, _, code = _emb_link_args("emb_link_score", h, src, dst, mode)
    return _score_call("emb_link_score", L.lib().gmp_emb_link_score, lambda s, d, P: (_ptr(h), N, h.size(1), code, s, d, P),
                       lambda P: L.lib().gmp_emb_link_workspace_bytes(N, P, h.size(1)), src, dst, h)


def emb_link_rank(h: Tensor, src: Tensor, dst: Tensor, mode: str = "cos", filter_rowptr: Optional[Tensor] = None,
                  filter_col: Optional[Tensor] = None, filter_edges: Optional[Tensor] = None, return_matrix: bool = False):
    """Every true pair (src[q], dst[q]) ranked against all nodes with emb_link_score's scorer (gnnmp.h gmp_emb_link_rank): returns
    (score_true [Q], n_greater [Q] int32, n_equal [Q] int32) over the candidates c other than src[q], dst[q] and the entries of
    src[q]'s row of the optional filter -- a CSR (lp_rank's: int32 rowptr [N + 1] / col, row = source) or filter_edges int64 [2, E]
    (source, destination), turned into that CSR by csr_build.  A candidate's score has the bits emb_link_score gives the pair.  Nothing
    of size Q x N is allocated unless return_matrix asks for every score as the compare saw it (a fourth result, tests only)."""
    N, Q, code = _emb_link_args("emb_link_rank", h, src, dst, mode)
    if filter_edges is not None:
        if filter_rowptr is not None or filter_col is not None:
            raise L.GnnmpError("emb_link_rank: pass the filter as a CSR or as filter_edges, not both")
        csr = csr_build(filter_edges, N)
        filter_rowptr, filter_col = csr.rowptr_t, csr.col_t
    mat = torch.empty(Q, N, device=h.device) if return_matrix else None
    out = _rank_call("emb_link_rank", L.lib().gmp_emb_link_rank, lambda s, d, Q: (_ptr(h), N, h.size(1), code, s, d, Q),
                     lambda Q: L.lib().gmp_emb_link_workspace_bytes(N, Q, h.size(1)), src, dst, N, filter_rowptr, filter_col, h, extra=(_ptr(mat),))
    return (*out, mat) if return_matrix else out


def graph_simple_check(rowptr: Tensor, col: Tensor) -> Tensor:
    """int32 [1] on the device: how many entries of the int32 CSR (rowptr, col) keep it from being a simple undirected graph -- out of
    range, a self-loop, not greater than the entry before it in the row, or without the mirror entry (gnnmp.h gmp_graph_simple_check)."""
    _need(rowptr, torch.int32, "rowptr", 1); _need(col, torch.int32, "col", 1)
    if rowptr.numel() < 1:
        raise L.GnnmpError("graph_simple_check: rowptr is empty (it has num_nodes + 1 entries)")
    violations = torch.empty(1, dtype=torch.int32, device=rowptr.device)
    L.check(L.lib().gmp_graph_simple_check(_ptr(rowptr), _ptr(col), rowptr.numel() - 1, col.numel(), _ptr(violations), _stream(rowptr)),
            "gmp_graph_simple_check")
    return violations


KNN_MAX_K, KNN_MAX_DIM, KNN_MAX_CLASSES = 64, 256, 32      # gmp_knn_topk / gmp_knn_vote (gnnmp.h)


def knn_topk(queries: Tensor, database: Tensor, k: int, exclude_self: bool = False, return_matrix: bool = False):
    """The k (1 <= k <= 64) nearest database rows of every query row in cosine similarity (gnnmp.h gmp_knn_topk; csrc/knn.hip): returns
    (idx [nq, k] int64, sim [nq, k]), similarity descending, ties to the lower database index, -1 / -inf behind a query's last candidate.
    queries [nq, d] and database [ndb, d] fp32 contiguous, 1 <= d <= 256.  Nothing of size nq x ndb is allocated unless return_matrix asks
    for the similarity matrix as the selection saw it (a third result, tests only).  exclude_self: leave-one-out over one set -- queries
    and database must be the same tensor; row i never returns i."""
    _need(queries, torch.float32, "queries", 2); _need(database, torch.float32, "database", 2)
    nq, d = queries.shape
    ndb = database.size(0)
    if database.size(1) != d or database.device != queries.device:
        raise L.GnnmpError(f"knn_topk: queries {tuple(queries.shape)} on {queries.device}, database {tuple(database.shape)} on {database.device}")
    if not 1 <= int(k) <= KNN_MAX_K or not 1 <= d <= KNN_MAX_DIM:
        raise L.GnnmpError(f"knn_topk: k={k} dim={d} (1 <= k <= {KNN_MAX_K}, 1 <= dim <= {KNN_MAX_DIM})")
    if exclude_self and (queries.data_ptr() != database.data_ptr() or nq != ndb):
        raise L.GnnmpError("knn_topk: exclude_self is leave-one-out over one set: pass the same tensor as queries and as database")
    dev, l = queries.device, L.lib()
    idx, sim = torch.empty(nq, k, dtype=torch.int64, device=dev), torch.empty(nq, k, device=dev)
    mat = torch.empty(nq, ndb, device=dev) if return_matrix else None
    ws = _ws(l.gmp_knn_workspace_bytes(nq, ndb, d, int(k)), dev)
    L.check(l.gmp_knn_topk(_ptr(queries), nq, _ptr(database), ndb, d, int(k), int(bool(exclude_self)), _ptr(idx), _ptr(sim), _ptr(mat),
                           _ptr(ws), ws.numel(), _stream(queries)), "gmp_knn_topk")
    return (idx, sim, mat) if return_matrix else (idx, sim)


def knn_vote(idx: Tensor, sim: Tensor, labels: Tensor, num_classes: int, temperature: float = 0.07) -> Tuple[Tensor, Tensor]:
    """The weighted k-NN vote of Wu et al. 2018 on knn_topk's (idx, sim) (gnnmp.h gmp_knn_vote): class_scores [nq, C] with [q, c] = the
    sum over q's neighbours r, in order, of exp(sim[q, r] / temperature) where labels[idx[q, r]] == c, and pred [nq] int64 = the argmax
    (ties to the lower class, -1 for a query without neighbours).  labels int64 [ndb].  Raises when a neighbour's label lies outside
    [0, num_classes) (one read-back of the status word)."""
    _need(idx, torch.int64, "idx", 2); _need(sim, torch.float32, "sim", 2); _need(labels, torch.int64, "labels", 1)
    nq, k = idx.shape
    if tuple(sim.shape) != (nq, k) or sim.device != idx.device or labels.device != idx.device:
        raise L.GnnmpError(f"knn_vote: idx {tuple(idx.shape)} on {idx.device}, sim {tuple(sim.shape)} on {sim.device}, labels on {labels.device}")
    if not 1 <= k <= KNN_MAX_K or not 2 <= int(num_classes) <= KNN_MAX_CLASSES or not float(temperature) > 0.0:
        raise L.GnnmpError(f"knn_vote: k={k} num_classes={num_classes} temperature={temperature} "
                           f"(1 <= k <= {KNN_MAX_K}, 2 <= num_classes <= {KNN_MAX_CLASSES}, temperature > 0)")
    dev = idx.device
    scores = torch.empty(nq, int(num_classes), device=dev)
    pred = torch.empty(nq, dtype=torch.int64, device=dev)
    status = torch.empty(1, dtype=torch.int32, device=dev)
    L.check(L.lib().gmp_knn_vote(_ptr(idx), _ptr(sim), nq, k, _ptr(labels), labels.numel(), int(num_classes), float(temperature), _ptr(scores),
                                 _ptr(pred), _ptr(status), _stream(idx)), "gmp_knn_vote")
    bad = int(status.item())
    if bad:
        raise L.GnnmpError(f"knn_vote: {bad} neighbours have a label outside [0, {num_classes})")
    return scores, pred


KMEANS_MAX_CLUSTERS, KMEANS_MAX_DIM, KMEANS_MAX_ITER = 1024, 256, 10000       # gmp_kmeans_assign / gmp_kmeans_fit / gmp_contingency (gnnmp.h)

class KMeansFit(NamedTuple):
    centroids: Tensor  # [kc, d]
    labels: Tensor     # [n] int64, the last assignment pass
    sim: Tensor        # [n] the winning similarities of that pass
    n_iter: int
    converged: bool    # the last pass moved no row
    empty: int         # clusters the last update found without rows


def _kmeans_args(who: str, x: Tensor, centroids: Tensor) -> Tuple[int, int, int]:
    _need(x, torch.float32, "x", 2); _need(centroids, torch.float32, "centroids", 2)
    n, d = x.shape
    kc = centroids.size(0)
    if centroids.size(1) != d or centroids.device != x.device:
        raise L.GnnmpError(f"{who}: x {tuple(x.shape)} on {x.device}, centroids {tuple(centroids.shape)} on {centroids.device}")
    if not 1 <= kc <= KMEANS_MAX_CLUSTERS or not 1 <= d <= KMEANS_MAX_DIM:
        raise L.GnnmpError(f"{who}: clusters={kc} dim={d} (1 <= clusters <= {KMEANS_MAX_CLUSTERS}, 1 <= dim <= {KMEANS_MAX_DIM})")
    return n, kc, d


def kmeans_assign(x: Tensor, centroids: Tensor, return_matrix: bool = False):
    """Every row of x [n, d] to its centroid of greatest cosine similarity (gnnmp.h gmp_kmeans_assign; csrc/kmeans.hip): returns
    (labels [n] int64, sim [n]), ties to the lower centroid index.  x and centroids [kc, d] fp32 contiguous, 1 <= kc <= 1024,
    1 <= d <= 256; both are normalised inside (a zero row scores 0 and lands on centroid 0).  Nothing of size n x kc is allocated unless
    return_matrix asks for the similarity matrix as the selection saw it (a third result, tests only)."""
    n, kc, d = _kmeans_args("kmeans_assign", x, centroids)
    dev, l = x.device, L.lib()
    labels, sim = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, device=dev)
    mat = torch.empty(n, kc, device=dev) if return_matrix else None
    ws = _ws(l.gmp_kmeans_workspace_bytes(n, kc, d), dev)
    L.check(l.gmp_kmeans_assign(_ptr(x), n, _ptr(centroids), kc, d, _ptr(labels), _ptr(sim), _ptr(mat), _ptr(ws), ws.numel(), _stream(x)),
            "gmp_kmeans_assign")
    return (labels, sim, mat) if return_matrix else (labels, sim)


def kmeans_fit(x: Tensor, init_centroids: Tensor, max_iter: int = 100) -> KMeansFit:
    """Spherical k-means from the given centroids (gnnmp.h gmp_kmeans_fit): up to max_iter Lloyd iterations -- assign every row to its
    centroid of greatest cosine similarity, stop when no label changed, otherwise each centroid becomes the normalised sum of its rows
    (in a fixed order: bitwise repeatable; a cluster without rows keeps its centroid) -- enqueued at once, without a host round trip in
    between.  Returns (centroids [kc, d], labels [n] int64 and sim [n] of the last assignment, n_iter, converged, empty): the three
    scalars come from one host copy at the end; empty = clusters the last update found without rows."""
    n, kc, d = _kmeans_args("kmeans_fit", x, init_centroids)
    if not 1 <= int(max_iter) <= KMEANS_MAX_ITER:
        raise L.GnnmpError(f"kmeans_fit: max_iter={max_iter} (1 <= max_iter <= {KMEANS_MAX_ITER})")
    dev, l = x.device, L.lib()
    centroids = init_centroids.clone()
    labels, sim = torch.empty(n, dtype=torch.int64, device=dev), torch.empty(n, device=dev)
    info = torch.zeros(4, dtype=torch.int64, device=dev)
    ws = _ws(l.gmp_kmeans_workspace_bytes(n, kc, d), dev)
    L.check(l.gmp_kmeans_fit(_ptr(x), n, _ptr(init_centroids), kc, d, int(max_iter), _ptr(centroids), _ptr(labels), _ptr(sim), _ptr(info),
                             _ptr(ws), ws.numel(), _stream(x)), "gmp_kmeans_fit")
    n_iter, changed, empty, _ = (int(v) for v in info.tolist())                 # the one read-back
    return KMeansFit(centroids, labels, sim, n_iter, n > 0 and changed == 0, empty)


def contingency(a: Tensor, b: Tensor, na: int, nb: int) -> Tensor:
    """table [na, nb] int64 with table[a[i], b[i]] = the number of such rows (gnnmp.h gmp_contingency: integer atomics, exact), a and b
    int64 [n] on the GPU, 1 <= na, nb <= 1024.  Raises when an entry lies outside its range (one read-back of the status word)."""
    _need(a, torch.int64, "a", 1); _need(b, torch.int64, "b", 1)
    n = a.numel()
    if b.numel() != n or b.device != a.device:
        raise L.GnnmpError(f"contingency: a [{n}] on {a.device}, b [{b.numel()}] on {b.device}")
    if not 1 <= int(na) <= KMEANS_MAX_CLUSTERS or not 1 <= int(nb) <= KMEANS_MAX_CLUSTERS:
        raise L.GnnmpError(f"contingency: na={na} nb={nb} (1 <= na, nb <= {KMEANS_MAX_CLUSTERS})")
    table = torch.zeros(int(na), int(nb), dtype=torch.int64, device=a.device)
    status = torch.zeros(1, dtype=torch.int32, device=a.device)
    L.check(L.lib().gmp_contingency(_ptr(a), _ptr(b), n, int(na), int(nb), _ptr(table), _ptr(status), _stream(a)), "gmp_contingency")
    bad = int(status.item())
    if bad:
        raise L.GnnmpError(f"contingency: {bad} rows have an entry outside [0, {na}) x [0, {nb})")
    return table


LOGREG_MAX_CLASSES, LOGREG_MAX_DIM, LOGREG_MAX_ITER = 32, 256, 10000           # gmp_logreg_fit / gmp_logreg_predict (gnnmp.h)


class LogRegState(NamedTuple):
    """What a softmax-regression fit resumes from: the parameters, Adam's two moments on the block (W | b), and the number of updates."""
    weight: Tensor      # [C, d]
    bias: Tensor        # [C]
    exp_avg: Tensor     # [C, d + 1]
    exp_avg_sq: Tensor  # [C, d + 1]
    step: Tensor        # int64 [1], on the device


class LogRegFit(NamedTuple):
    state: LogRegState
    loss_history: Tensor            # [iters]: entry k = the loss at the parameters before update k of this call
    grad: Optional[Tensor] = None   # [C, d + 1]: (gW | gb) of the last iteration as the update saw it (return_grad)
    logits: Optional[Tensor] = None  # [n, C]: the logits of the last iteration (return_logits)


def logreg_init(num_classes: int, dim: int, device) -> LogRegState:
    """The defined starting point of logreg_fit: everything zero (the problem is convex; no random state is involved)."""
    c, d = int(num_classes), int(dim)
    if not 2 <= c <= LOGREG_MAX_CLASSES or not 1 <= d <= LOGREG_MAX_DIM:
        raise L.GnnmpError(f"logreg_init: num_classes={num_classes} dim={dim} (2 <= num_classes <= {LOGREG_MAX_CLASSES}, 1 <= dim <= {LOGREG_MAX_DIM})")
    return LogRegState(torch.zeros(c, d, device=device), torch.zeros(c, device=device), torch.zeros(c, d + 1, device=device),
                       torch.zeros(c, d + 1, device=device), torch.zeros(1, dtype=torch.int64, device=device))


def _logreg_enqueue(x: Tensor, labels: Tensor, num_classes: int, iters: int, lr: float, l2: float, state: Optional[LogRegState],
                    return_grad: bool, return_logits: bool) -> Tuple[LogRegFit, Tensor]:
    """logreg_fit without the read-back: (the fit, status int32 [1] still on the device) -- for callers that read it with other words."""
    _need(x, torch.float32, "x", 2); _need(labels, torch.int64, "labels", 1)
    n, d = x.shape
    c = int(num_classes)
    if labels.numel() != n or labels.device != x.device:
        raise L.GnnmpError(f"logreg_fit: x {tuple(x.shape)} on {x.device}, labels [{labels.numel()}] on {labels.device}")
    if not 2 <= c <= LOGREG_MAX_CLASSES or not 1 <= d <= LOGREG_MAX_DIM or not 1 <= int(iters) <= LOGREG_MAX_ITER:
        raise L.GnnmpError(f"logreg_fit: num_classes={num_classes} dim={d} iters={iters} (2 <= num_classes <= {LOGREG_MAX_CLASSES}, "
                           f"1 <= dim <= {LOGREG_MAX_DIM}, 1 <= iters <= {LOGREG_MAX_ITER})")
    if not float(lr) > 0.0 or not float(l2) >= 0.0:
        raise L.GnnmpError(f"logreg_fit: lr={lr} l2={l2} (lr > 0, l2 >= 0)")
    dev, l = x.device, L.lib()
    if state is None:
        state = logreg_init(c, d, dev)
    else:
        want = ((c, d), (c,), (c, d + 1), (c, d + 1), (1,))
        dtypes = (torch.float32,) * 4 + (torch.int64,)
        for t, shape, dtype, name in zip(state, want, dtypes, LogRegState._fields):
            _need(t, dtype, f"state.{name}")
            if tuple(t.shape) != shape or t.device != dev:
                raise L.GnnmpError(f"logreg_fit: state.{name} {tuple(t.shape)} on {t.device} (expected {shape} on {dev})")
        state = LogRegState(*(t.clone() for t in state))            # the caller's state is left alone
    loss = torch.zeros(int(iters), device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    grad = torch.zeros(c, d + 1, device=dev) if return_grad else None
    logits = torch.zeros(n, c, device=dev) if return_logits else None
    ws = _ws(l.gmp_logreg_workspace_bytes(n, c, d), dev)
    L.check(l.gmp_logreg_fit(_ptr(x), _ptr(labels), n, c, d, int(iters), float(lr), float(l2), _ptr(state.weight), _ptr(state.bias),
                             _ptr(state.exp_avg), _ptr(state.exp_avg_sq), _ptr(state.step), _ptr(loss), _ptr(status), _ptr(grad), _ptr(logits),
                             _ptr(ws), ws.numel(), _stream(x)), "gmp_logreg_fit")
    return LogRegFit(state, loss, grad, logits), status


def logreg_fit(x: Tensor, labels: Tensor, num_classes: int, iters: int = 100, lr: float = 0.01, l2: float = 0.0,
               state: Optional[LogRegState] = None, return_grad: bool = False, return_logits: bool = False) -> LogRegFit:
    """Softmax regression on the L2-normalised rows of x [n, d <= 256] (fp32, on the GPU) against labels int64 [n] in [0, num_classes),
    2 <= num_classes <= 32 (gnnmp.h gmp_logreg_fit; csrc/logreg.hip): `iters` full-batch Adam updates (torch.optim.Adam's rule, lr, ridge
    l2 on the weights alone) of the mean cross-entropy, enqueued at once, two launches each, without a host round trip, an [n, C] array or
    a floating-point atomic: bitwise repeatable, and T iterations in one call equal T calls of one chained through `state`.  Starts from
    `state` (cloned, never mutated) or from logreg_init's zeros.  Returns LogRegFit(state, loss_history [iters], grad, logits): the last
    two are test hooks (None unless asked for) and change nothing else.  Raises when a label lies outside its range (the one read-back)."""
    fit, status = _logreg_enqueue(x, labels, num_classes, iters, lr, l2, state, return_grad, return_logits)
    bad = int(status.item())
    if bad:
        raise L.GnnmpError(f"logreg_fit: {bad} rows have a label outside [0, {num_classes})")
    return fit


def logreg_predict(x: Tensor, weight: Tensor, bias: Tensor, return_logits: bool = False):
    """pred [n] int64 = the class of the greatest logit <xn_i, W_c> + b_c of every row of x [n, d], rows normalised and logits computed
    exactly as logreg_fit does (gnnmp.h gmp_logreg_predict); ties to the lower class.  weight [C, d] and bias [C] fp32 on the GPU.
    return_logits adds the [n, C] logits as a second result."""
    _need(x, torch.float32, "x", 2); _need(weight, torch.float32, "weight", 2); _need(bias, torch.float32, "bias", 1)
    n, d = x.shape
    c = weight.size(0)
    if weight.size(1) != d or bias.numel() != c or weight.device != x.device or bias.device != x.device:
        raise L.GnnmpError(f"logreg_predict: x {tuple(x.shape)} on {x.device}, weight {tuple(weight.shape)} on {weight.device}, "
                           f"bias {tuple(bias.shape)} on {bias.device}")
    if not 2 <= c <= LOGREG_MAX_CLASSES or not 1 <= d <= LOGREG_MAX_DIM:
        raise L.GnnmpError(f"logreg_predict: num_classes={c} dim={d} (2 <= num_classes <= {LOGREG_MAX_CLASSES}, 1 <= dim <= {LOGREG_MAX_DIM})")
    dev, l = x.device, L.lib()
    pred = torch.zeros(n, dtype=torch.int64, device=dev)
    logits = torch.zeros(n, c, device=dev) if return_logits else None
    ws = _ws(l.gmp_logreg_workspace_bytes(n, c, d), dev)
    L.check(l.gmp_logreg_predict(_ptr(x), n, _ptr(weight), _ptr(bias), c, d, _ptr(pred), _ptr(logits), _ptr(ws), ws.numel(), _stream(x)),
            "gmp_logreg_predict")
    return (pred, logits) if return_logits else pred


REPR_MAX_DIM = 256              # gmp_repr_* (gnnmp.h)
REPR_MAX_ROWS = 2**20           # the rows gmp_repr_workspace_bytes sizes a workspace for


def _repr_args(who: str, z: Tensor, name: str, min_rows: int) -> Tuple[int, int]:
    _need(z, torch.float32, name, 2)
    n, d = z.shape
    if not min_rows <= n <= REPR_MAX_ROWS or not 1 <= d <= REPR_MAX_DIM:
        raise L.GnnmpError(f"{who}: {name} {tuple(z.shape)} ({min_rows} <= rows <= {REPR_MAX_ROWS}, 1 <= dim <= {REPR_MAX_DIM})")
    return n, d


def repr_pair_stats(z: Tensor, t: float = 2.0) -> Tensor:
    """The all-pairs sums of the rows of z [n, d] (fp32 contiguous, 2 <= n <= 2^20, 1 <= d <= 256) on the unit sphere, without the n x n
    similarity matrix (gnnmp.h gmp_repr_pair_stats; csrc/repr_stats.hip): an fp64 [2] tensor on the device, [0] = the sum over i < j of
    exp(-2 t (1 - s_ij)), [1] = the sum over i < j of s_ij, with s_ij the cosine similarity of rows i and j (a zero row scores 0).  t >= 0.
    No read-back; two calls on the same input give equal bits."""
    n, d = _repr_args("repr_pair_stats", z, "z", 2)
    if not float(t) >= 0.0:
        raise L.GnnmpError(f"repr_pair_stats: t={t} (must be >= 0)")
    dev, l = z.device, L.lib()
    out = torch.empty(2, dtype=torch.float64, device=dev)
    ws = _ws(l.gmp_repr_workspace_bytes(n, d), dev)
    L.check(l.gmp_repr_pair_stats(_ptr(z), n, d, float(t), _ptr(out), _ptr(ws), ws.numel(), _stream(z)), "gmp_repr_pair_stats")
    return out


def repr_alignment_sum(z1: Tensor, z2: Tensor, alpha: float = 2.0) -> Tensor:
    """An fp64 [1] tensor on the device: the sum over the rows i of max(0, 2 - 2 s_ii)^(alpha / 2), s_ii the cosine similarity of row i of
    z1 and row i of z2 (both [n, d] fp32 contiguous, 1 <= n <= 2^20, 1 <= d <= 256), i.e. of ||zn1_i - zn2_i||^alpha on the unit sphere
    (gnnmp.h gmp_repr_alignment).  alpha > 0.  No read-back."""
    n, d = _repr_args("repr_alignment_sum", z1, "z1", 1)
    _need(z2, torch.float32, "z2", 2)
    if tuple(z2.shape) != (n, d) or z2.device != z1.device:
        raise L.GnnmpError(f"repr_alignment_sum: z1 {tuple(z1.shape)} on {z1.device}, z2 {tuple(z2.shape)} on {z2.device}")
    if not float(alpha) > 0.0:
        raise L.GnnmpError(f"repr_alignment_sum: alpha={alpha} (must be positive)")
    dev, l = z1.device, L.lib()
    out = torch.empty(1, dtype=torch.float64, device=dev)
    ws = _ws(l.gmp_repr_workspace_bytes(n, d), dev)
    L.check(l.gmp_repr_alignment(_ptr(z1), _ptr(z2), n, d, float(alpha), _ptr(out), _ptr(ws), ws.numel(), _stream(z1)), "gmp_repr_alignment")
    return out


def repr_gram(z: Tensor) -> Tuple[Tensor, Tensor]:
    """(gram [d, d], colsum [d]), both fp64 on the device: Z^T Z and the sum of the rows of z [n, d] (fp32 contiguous, 1 <= n <= 2^20,
    1 <= d <= 256, rows as they are, not normalised), products and sums in fp64 (gnnmp.h gmp_repr_gram): every product of two fp32 values
    is exact in fp64, so the error is that of the fp64 sums alone.  gram is bitwise symmetric.  No read-back."""
    n, d = _repr_args("repr_gram", z, "z", 1)
    dev, l = z.device, L.lib()
    gram = torch.empty(d, d, dtype=torch.float64, device=dev)
    colsum = torch.empty(d, dtype=torch.float64, device=dev)
    ws = _ws(l.gmp_repr_workspace_bytes(n, d), dev)
    L.check(l.gmp_repr_gram(_ptr(z), n, d, _ptr(gram), _ptr(colsum), _ptr(ws), ws.numel(), _stream(z)), "gmp_repr_gram")
    return gram, colsum


CLS_MAX_ROWS, CLS_MAX_CLASSES = 262144, 32      # gmp_cls_counts: the pair count is n^2 compares (gnnmp.h)


def cls_counts_packed(targets: Tensor, predictions: Tensor, probabilities: Tensor) -> Tensor:
    """gmp_cls_counts into ONE int32 device buffer of 2 (C C + 4 C) + 1 words, so that a caller reads everything back with one copy: words
    [0, 2 C C) are confusion as int64, the next 8 C auc_counts as int64, the last word is status (cls_counts gives the three views)."""
    _need(targets, torch.int64, "targets", 1); _need(predictions, torch.int64, "predictions", 1)
    _need(probabilities, torch.float32, "probabilities", 2)
    n, c, dev, l = targets.numel(), probabilities.size(1), targets.device, L.lib()
    if predictions.numel() != n or probabilities.size(0) != n:
        raise L.GnnmpError(f"cls_counts: {n} targets, {predictions.numel()} predictions, probabilities {tuple(probabilities.shape)}")
    if predictions.device != dev or probabilities.device != dev:
        raise L.GnnmpError("cls_counts: the three inputs must be on one device")
    buf = torch.empty(2 * (c * c + 4 * c) + 1, dtype=torch.int32, device=dev)
    ws = _ws(l.gmp_cls_counts_workspace_bytes(n, c), dev)
    base = buf.data_ptr()
    L.check(l.gmp_cls_counts(_ptr(targets), _ptr(predictions), _ptr(probabilities), n, c, C.c_void_p(base), C.c_void_p(base + 8 * c * c),
                             C.c_void_p(base + 8 * (c * c + 4 * c)), _ptr(ws), ws.numel(), _stream(targets)), "gmp_cls_counts")
    return buf


def cls_counts(targets: Tensor, predictions: Tensor, probabilities: Tensor) -> Tuple[Tensor, Tensor, Tensor]:
    """The integer counts behind the classification metrics (gnnmp.h gmp_cls_counts), as device tensors: (confusion [C, C] int64 with
    [t, p] = rows of target t predicted p, auc_counts [C, 4] int64 = (n_pos, n_neg, n_greater, n_equal) per class, status [1] int32 =
    rows left out for a target / prediction outside [0, C) or a non-finite probability).  targets, predictions int64 [n],
    probabilities fp32 [n, C] contiguous; 1 <= n <= CLS_MAX_ROWS, 2 <= C <= CLS_MAX_CLASSES."""
    buf = cls_counts_packed(targets, predictions, probabilities)
    c = probabilities.size(1)
    k = c * c + 4 * c
    wide = buf[:2 * k].view(torch.int64)
    return wide[:c * c].view(c, c), wide[c * c:].view(c, 4), buf[2 * k:]


GRAPH_PROPS_SLOTS, GRAPH_PROPS_MAX_NODES = 16, 1024        # gmp_graph_props: counts per graph, largest graph the kernel takes (gnnmp.h)


def _max_graph_nodes(ptr: Tensor, G: int) -> int:
    """The largest ptr[g + 1] - ptr[g] of a batch of G graphs, read back from the device (one synchronisation); 0 without a graph."""
    return max(int((ptr[1:] - ptr[:-1]).max()), 0) if G else 0


def _batch_csr_args(who: str, ptr: Tensor, rowptr: Tensor, col: Tensor, labels: Optional[Tensor]) -> Tuple[int, int, torch.device]:
    """(G, N, device) of ptr int64 [G + 1], the batch's int32 CSR (rowptr [N + 1], col) and labels int64 [N] or None, all on ptr's device."""
    _need(ptr, torch.int64, "ptr", 1); _need(rowptr, torch.int32, "rowptr", 1); _need(col, torch.int32, "col", 1)
    G, N, dev = ptr.numel() - 1, rowptr.numel() - 1, ptr.device
    if G < 0 or N < 0:
        raise L.GnnmpError(f"{who}: ptr {tuple(ptr.shape)}, rowptr {tuple(rowptr.shape)} (G + 1 and N + 1 entries)")
    if rowptr.device != dev or col.device != dev:
        raise L.GnnmpError(f"{who}: ptr, rowptr and col must be on one device")
    if labels is not None:
        _need(labels, torch.int64, "labels", 1)
        if labels.numel() != N or labels.device != dev:
            raise L.GnnmpError(f"{who}: labels has {labels.numel()} entries on {labels.device} for {N} nodes on {dev}")
    return G, N, dev


def graph_properties(ptr: Tensor, eptr: Tensor, edge_index: Tensor, max_graph_nodes: Optional[int] = None) -> Tuple[Tensor, Tensor]:
    """The integer counts behind the 12 graph-property targets of a batch (gnnmp.h gmp_graph_props; the slot table is there): ptr int64
    [B + 1] node offsets, eptr int64 [B + 1] edge offsets, edge_index int64 [2, E] batch-global ids grouped by graph.  Returns (counts
    int64 [B, 16], clustering_sum float64 [B]) on the device; data.graph_properties.properties_from_counts turns them into the targets.
    Both start as zeros, so a graph the kernel refuses (status bit 0: more than GRAPH_PROPS_MAX_NODES nodes) reads as zeros with slot 12
    = 1.  max_graph_nodes: the largest ptr[g + 1] - ptr[g] when the caller knows it (None reads it back from ptr, one synchronisation)."""
    _need(ptr, torch.int64, "ptr", 1); _need(eptr, torch.int64, "eptr", 1); _need(edge_index, torch.int64, "edge_index", 2)
    B, dev = ptr.numel() - 1, ptr.device
    if B < 0 or eptr.numel() != B + 1 or edge_index.size(0) != 2:
        raise L.GnnmpError(f"graph_properties: ptr {tuple(ptr.shape)}, eptr {tuple(eptr.shape)}, edge_index {tuple(edge_index.shape)}")
    if eptr.device != dev or edge_index.device != dev:
        raise L.GnnmpError("graph_properties: the three inputs must be on one device")
    counts = torch.zeros(B, GRAPH_PROPS_SLOTS, dtype=torch.int64, device=dev)
    csum = torch.zeros(B, dtype=torch.float64, device=dev)
    if B == 0:
        return counts, csum
    if max_graph_nodes is None:
        max_graph_nodes = _max_graph_nodes(ptr, B)
    E = edge_index.size(1)
    L.check(L.lib().gmp_graph_props(_ptr(ptr), _ptr(eptr), _ptr(edge_index) if E else None, 0, E, B, int(max_graph_nodes), _ptr(counts),
                                    _ptr(csum), None, 0, _stream(ptr)), "gmp_graph_props")
    return counts, csum


WL_MAX_ITERS, WL_MAX_DIM, WL_MAX_GRAPH_NODES = 7, 256, 1024       # gmp_wl_refine / gmp_wl_gram (gnnmp.h)


class WLRefinement(NamedTuple):
    """wl_refine's outputs (gnnmp.h gmp_wl_refine)."""
    sorted: Tensor                 # int64 [(iters + 1) * N]: graph g's colours, ascending as unsigned words, at [(iters + 1) ptr[g], (iters + 1) ptr[g+1])
    hist: Tensor                   # int32 [G, dim]: the hashed feature map
    status: Tensor                 # int32 [G]: bit 0 = refused (too large), bits 8.. = skipped CSR entries
    colors: Optional[Tensor] = None   # int64 [iters + 1, N], only with return_colors


def wl_refine(ptr: Tensor, rowptr: Tensor, col: Tensor, labels: Optional[Tensor] = None, iters: int = 3, dim: int = 256,
              max_graph_nodes: Optional[int] = None, return_colors: bool = False, fill: int = 0) -> WLRefinement:
    """`iters` rounds of hashed Weisfeiler-Lehman colour refinement of a batch of graphs in one launch (gnnmp.h gmp_wl_refine holds the
    definition; csrc/wl.hip): ptr int64 [G + 1] node offsets, (rowptr, col) the int32 CSR of the batch's simple undirected graph
    (finetune.link_heuristics.simple_graph), labels int64 [N] or None (None: a node's degree inside its graph).  0 <= iters <= 7,
    1 <= dim <= 256.  Returns WLRefinement(sorted, hist, status[, colors]); the outputs start as `fill`, which is what a refused graph
    (status bit 0: more than min(max_graph_nodes, WL_MAX_GRAPH_NODES) nodes) keeps.  max_graph_nodes: the largest ptr[g + 1] - ptr[g]
    when the caller knows it (None reads it back from ptr, one synchronisation).  No other read-back: status stays on the device."""
    G, N, dev = _batch_csr_args("wl_refine", ptr, rowptr, col, labels)
    if not 0 <= int(iters) <= WL_MAX_ITERS or not 1 <= int(dim) <= WL_MAX_DIM:
        raise L.GnnmpError(f"wl_refine: iters={iters} dim={dim} (0 <= iters <= {WL_MAX_ITERS}, 1 <= dim <= {WL_MAX_DIM})")
    iters, dim = int(iters), int(dim)
    srt = torch.full(((iters + 1) * N,), fill, dtype=torch.int64, device=dev)
    hist = torch.full((G, dim), fill, dtype=torch.int32, device=dev)
    status = torch.zeros(G, dtype=torch.int32, device=dev)
    colors = torch.full((iters + 1, N), fill, dtype=torch.int64, device=dev) if return_colors else None
    if G:
        if max_graph_nodes is None:
            max_graph_nodes = _max_graph_nodes(ptr, G)
        L.check(L.lib().gmp_wl_refine(_ptr(ptr), G, _ptr(rowptr), _ptr(col), N, col.numel(), _ptr(labels), iters, dim, int(max_graph_nodes),
                                      _ptr(colors), _ptr(srt), _ptr(hist), _ptr(status), None, 0, _stream(ptr)), "gmp_wl_refine")
    return WLRefinement(srt, hist, status, colors)


def wl_gram(sorted_a: Tensor, ptr_a: Tensor, sorted_b: Tensor, ptr_b: Tensor, iters: int) -> Tensor:
    """K int64 [Ga, Gb], the Weisfeiler-Lehman subtree kernel between two batches refined by wl_refine with the same `iters` (gnnmp.h
    gmp_wl_gram): K[i, j] = the number of pairs of equal colours between graph i's segment of sorted_a and graph j's segment of
    sorted_b (the two may be the same tensors).  Exact integers."""
    _need(sorted_a, torch.int64, "sorted_a", 1); _need(ptr_a, torch.int64, "ptr_a", 1)
    _need(sorted_b, torch.int64, "sorted_b", 1); _need(ptr_b, torch.int64, "ptr_b", 1)
    dev = sorted_a.device
    if ptr_a.device != dev or sorted_b.device != dev or ptr_b.device != dev:
        raise L.GnnmpError("wl_gram: the four inputs must be on one device")
    if not 0 <= int(iters) <= WL_MAX_ITERS or ptr_a.numel() < 1 or ptr_b.numel() < 1:
        raise L.GnnmpError(f"wl_gram: iters={iters} (0 <= iters <= {WL_MAX_ITERS}), ptr_a {tuple(ptr_a.shape)}, ptr_b {tuple(ptr_b.shape)}")
    Ga, Gb = ptr_a.numel() - 1, ptr_b.numel() - 1
    K = torch.zeros(Ga, Gb, dtype=torch.int64, device=dev)
    L.check(L.lib().gmp_wl_gram(_ptr(sorted_a), _ptr(ptr_a), Ga, sorted_a.numel(), _ptr(sorted_b), _ptr(ptr_b), Gb, sorted_b.numel(),
                                int(iters), _ptr(K), _stream(sorted_a)), "gmp_wl_gram")
    return K


SP_MAX_DIST, SP_MAX_GRAPH_NODES, SP_MAX_DIM, SP_MAX_LABEL = 1023, 1024, 256, 2 ** 24     # gmp_sp_features / gmp_sp_gram (gnnmp.h)


class SPFeatureMap(NamedTuple):
    """sp_features' outputs (gnnmp.h gmp_sp_features)."""
    keys: Tensor                   # int64 [G, cap]: graph g's distinct keys (lo << 35 | hi << 11 | d), ascending, in [g, :nuniq[g]]
    counts: Tensor                 # int32 [G, cap]: the pairs per key
    nuniq: Tensor                  # int32 [G]: the distinct keys per graph (0 for a refused graph)
    hist: Tensor                   # int32 [G, dim]: the hashed feature map
    status: Tensor                 # int32 [G]: bit 0 = refused (too large), bit 1 = more than cap keys, bit 2 = a label outside [0, 2^24), bits 8.. = skipped CSR entries


def sp_max_unique(max_graph_nodes: int) -> int:
    """The largest row stride `cap` sp_features accepts for graphs of at most max_graph_nodes nodes (gnnmp.h gmp_sp_max_unique)."""
    return int(L.lib().gmp_sp_max_unique(int(max_graph_nodes)))


def sp_features(ptr: Tensor, rowptr: Tensor, col: Tensor, labels: Optional[Tensor] = None, max_dist: int = SP_MAX_DIST, dim: int = 256,
                max_graph_nodes: Optional[int] = None, cap: Optional[int] = None, fill: int = 0) -> SPFeatureMap:
    """The shortest-path feature map of a batch of graphs in one launch (gnnmp.h gmp_sp_features holds the definition; csrc/sp.hip): per
    graph, the sorted distinct keys (label, label, hop distance <= max_dist) of its node pairs with their counts, and the counts hashed
    into dim bins.  ptr int64 [G + 1] node offsets, (rowptr, col) the int32 CSR of the batch's simple undirected graph
    (finetune.link_heuristics.simple_graph), labels int64 [N] in [0, SP_MAX_LABEL) or None (None: a node's degree inside its graph).
    1 <= max_dist <= 1023, 1 <= dim <= 256, cap = the row stride of keys and counts, at most sp_max_unique(max_graph_nodes), which None
    takes.  Returns SPFeatureMap(keys, counts, nuniq, hist, status); keys, counts and hist start as `fill`, which is what a refused graph
    (status bits 0 - 2) and the tail of every row keep.  max_graph_nodes: the largest ptr[g + 1] - ptr[g] when the caller knows it (None
    reads it back from ptr, one synchronisation).  No other read-back: status stays on the device."""
    G, N, dev = _batch_csr_args("sp_features", ptr, rowptr, col, labels)
    if not 1 <= int(max_dist) <= SP_MAX_DIST or not 1 <= int(dim) <= SP_MAX_DIM:
        raise L.GnnmpError(f"sp_features: max_dist={max_dist} dim={dim} (1 <= max_dist <= {SP_MAX_DIST}, 1 <= dim <= {SP_MAX_DIM})")
    if max_graph_nodes is None:
        max_graph_nodes = _max_graph_nodes(ptr, G)
    limit = sp_max_unique(max_graph_nodes)
    cap = limit if cap is None else int(cap)
    if not 1 <= cap <= limit:
        raise L.GnnmpError(f"sp_features: cap={cap} (1 <= cap <= {limit} for graphs of up to {max_graph_nodes} nodes)")
    keys = torch.full((G, cap), fill, dtype=torch.int64, device=dev)
    counts = torch.full((G, cap), fill, dtype=torch.int32, device=dev)
    hist = torch.full((G, int(dim)), fill, dtype=torch.int32, device=dev)
    nuniq = torch.zeros(G, dtype=torch.int32, device=dev)
    status = torch.zeros(G, dtype=torch.int32, device=dev)
    if G:
        L.check(L.lib().gmp_sp_features(_ptr(ptr), G, _ptr(rowptr), _ptr(col), N, col.numel(), _ptr(labels), int(max_dist), int(dim),
                                        int(max_graph_nodes), cap, _ptr(keys), _ptr(counts), _ptr(nuniq), _ptr(hist), _ptr(status), None, 0,
                                        _stream(ptr)), "gmp_sp_features")
    return SPFeatureMap(keys, counts, nuniq, hist, status)


def sp_gram(keys_a: Tensor, counts_a: Tensor, nuniq_a: Tensor, keys_b: Tensor, counts_b: Tensor, nuniq_b: Tensor) -> Tensor:
    """K int64 [Ga, Gb], the shortest-path kernel between two batches of sp_features (gnnmp.h gmp_sp_gram): K[i, j] = the sum over the keys
    that graph i of a and graph j of b share of the product of their counts (the two may be the same tensors; their row strides may
    differ).  Exact integers."""
    for k, c, n, s in ((keys_a, counts_a, nuniq_a, "a"), (keys_b, counts_b, nuniq_b, "b")):
        _need(k, torch.int64, f"keys_{s}", 2); _need(c, torch.int32, f"counts_{s}", 2); _need(n, torch.int32, f"nuniq_{s}", 1)
        if k.shape != c.shape or n.numel() != k.size(0) or k.size(1) < 1:
            raise L.GnnmpError(f"sp_gram: keys_{s} {tuple(k.shape)}, counts_{s} {tuple(c.shape)}, nuniq_{s} {tuple(n.shape)} ([G, cap], [G, cap], [G])")
    dev = keys_a.device
    if any(t.device != dev for t in (counts_a, nuniq_a, keys_b, counts_b, nuniq_b)):
        raise L.GnnmpError("sp_gram: the six inputs must be on one device")
    Ga, Gb = keys_a.size(0), keys_b.size(0)
    K = torch.zeros(Ga, Gb, dtype=torch.int64, device=dev)
    L.check(L.lib().gmp_sp_gram(_ptr(keys_a), _ptr(counts_a), _ptr(nuniq_a), Ga, keys_a.size(1), _ptr(keys_b), _ptr(counts_b), _ptr(nuniq_b), Gb,
                                keys_b.size(1), _ptr(K), _stream(keys_a)), "gmp_sp_gram")
    return K


def _prop_args(who: str, rowptr: Tensor, col: Tensor, rows: int, what: str, left: Optional[Tensor], right: Optional[Tensor], others) -> int:
    """n of the int32 CSR that label_propagate / feature_propagate walk: rowptr [n + 1] for the `rows` rows of the matrix `what`, left /
    right fp32 [n] or None, and these and `others` on rowptr's device."""
    _need(rowptr, torch.int32, "rowptr", 1); _need(col, torch.int32, "col", 1)
    n = rowptr.numel() - 1
    if n < 0 or rows != n:
        raise L.GnnmpError(f"{who}: rowptr has {rowptr.numel()} entries for the {rows} rows of {what} (n + 1 entries)")
    for t, name in ((left, "left"), (right, "right")):
        if t is not None:
            _need(t, torch.float32, name, 1)
            if t.numel() != n:
                raise L.GnnmpError(f"{who}: {name} has {t.numel()} entries for {n} nodes")
    if any(t is not None and t.device != rowptr.device for t in (col, left, right) + tuple(others)):
        raise L.GnnmpError(f"{who}: every input must be on one device")
    return n


LABELPROP_MAX_CLASSES, LABELPROP_MAX_ROUNDS = 32, 10000            # gmp_label_propagate (gnnmp.h)


class LabelPropagation(NamedTuple):
    """label_propagate's outputs (gnnmp.h gmp_label_propagate)."""
    out: Tensor                    # fp32 [n, classes]: F after the last round
    pred: Tensor                   # int64 [n]: the argmax of each row of out, ties to the lower class
    status: Tensor                 # int32 [2]: CSR entries outside [0, n) (skipped), rows of out whose maximum is not > 0
    residual: Optional[Tensor] = None   # fp32 [rounds]: max |F(t+1) - F(t)| per round, only with return_residual


def label_propagate(rowptr: Tensor, col: Tensor, f0: Tensor, rounds: int, alpha: float, beta: float, left: Optional[Tensor] = None,
                    right: Optional[Tensor] = None, clamp: Optional[Tensor] = None, f_init: Optional[Tensor] = None,
                    return_residual: bool = False) -> LabelPropagation:
    """`rounds` rounds of F <- alpha * left[i] * (sum over the row's entries j, in order, of right[j] * F[j]) + beta * f0, rows with
    clamp[i] != 0 put back to f0, started from f_init (None: f0), one launch per round and no host synchronisation (gnnmp.h
    gmp_label_propagate holds the definition; csrc/label_prop.hip).  (rowptr, col) an int32 CSR over n nodes, f0 / f_init fp32
    [n, classes] with 1 <= classes <= 32, left / right fp32 [n] or None (ones), clamp uint8 [n] or None.  Every multiply and add is
    rounded on its own in a fixed order: the bits are reproducible, and `rounds` rounds equal `rounds` chained calls of one.  Returns
    LabelPropagation(out, pred, status[, residual]); status stays on the device."""
    _need(f0, torch.float32, "f0", 2)
    n, classes, dev = _prop_args("label_propagate", rowptr, col, f0.size(0), "f0", left, right, (f0, clamp, f_init)), f0.size(1), rowptr.device
    if not 1 <= classes <= LABELPROP_MAX_CLASSES or not 1 <= int(rounds) <= LABELPROP_MAX_ROUNDS:
        raise L.GnnmpError(f"label_propagate: classes={classes} rounds={rounds} (1 <= classes <= {LABELPROP_MAX_CLASSES}, "
                           f"1 <= rounds <= {LABELPROP_MAX_ROUNDS})")
    if clamp is not None:
        _need(clamp, torch.uint8, "clamp", 1)
        if clamp.numel() != n:
            raise L.GnnmpError(f"label_propagate: clamp has {clamp.numel()} entries for {n} nodes")
    if f_init is not None:
        _need(f_init, torch.float32, "f_init", 2)
        if f_init.shape != f0.shape:
            raise L.GnnmpError(f"label_propagate: f_init {tuple(f_init.shape)} against f0 {tuple(f0.shape)}")
    rounds, l = int(rounds), L.lib()
    out = torch.empty(n, classes, device=dev)
    pred = torch.empty(n, dtype=torch.int64, device=dev)
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    residual = torch.empty(rounds, device=dev) if return_residual else None
    ws = _ws(l.gmp_label_propagate_workspace_bytes(n, classes), dev)
    L.check(l.gmp_label_propagate(_ptr(rowptr), _ptr(col), n, col.numel(), _ptr(left), _ptr(right), _ptr(f0), _ptr(f_init), _ptr(clamp), classes,
                                  rounds, float(alpha), float(beta), _ptr(out), _ptr(pred), _ptr(residual), _ptr(status), _ptr(ws), ws.numel(),
                                  _stream(rowptr)), "gmp_label_propagate")
    return LabelPropagation(out, pred, status, residual)


FEATPROP_MAX_DIM = 16384                                           # gmp_feature_propagate (gnnmp.h)
FEATPROP_MAX_ROUNDS = 64


class FeaturePropagation(NamedTuple):
    """feature_propagate's outputs (gnnmp.h gmp_feature_propagate)."""
    out: Tensor                    # fp32 [n, d]: H after the last round
    status: Tensor                 # int32 [2]: CSR entries outside [0, n) (skipped), feature entries that break the CSR form (skipped)


def feature_propagate(rowptr: Tensor, col: Tensor, x, rounds: int, left: Optional[Tensor] = None, right: Optional[Tensor] = None,
                      out: Optional[Tensor] = None) -> FeaturePropagation:
    """`rounds` rounds of H <- left[i] * (sum over the row's entries j, in order, of right[j] * H[j]) from H = x, one launch per round and
    no host synchronisation (gnnmp.h gmp_feature_propagate holds the definition; csrc/feature_prop.hip).  (rowptr, col) an int32 CSR over
    n nodes; x a dense fp32 [n, d] tensor with contiguous rows (any leading dimension) or a graph.SparseFeatures, 1 <= d <= 16384,
    1 <= rounds <= 64; left / right fp32 [n] or None (ones); out (allocated when None) fp32 [n, d] with contiguous rows, not overlapping
    x -- its padding columns are left alone.  Every multiply and add is rounded on its own in a fixed order: the bits are reproducible,
    the CSR form gives the bits of the dense form on to_dense(), and `rounds` rounds equal `rounds` chained calls of one.  Returns
    FeaturePropagation(out, status); status stays on the device."""
    from .graph import SparseFeatures
    sparse = isinstance(x, SparseFeatures)
    if sparse:
        _sparse_ok(x)
    elif isinstance(x, Tensor):
        _need_rows(x, "x")
    else:
        raise L.GnnmpError(f"feature_propagate: x must be a dense fp32 tensor or SparseFeatures, got {type(x).__name__}")
    rows, d, dev = int(x.shape[0]), int(x.shape[1]), rowptr.device
    if not 1 <= d <= FEATPROP_MAX_DIM or not 1 <= int(rounds) <= FEATPROP_MAX_ROUNDS:
        raise L.GnnmpError(f"feature_propagate: d={d} rounds={rounds} (1 <= d <= {FEATPROP_MAX_DIM}, 1 <= rounds <= {FEATPROP_MAX_ROUNDS})")
    if out is None:
        out = torch.empty(rows, d, device=dev)
    else:
        _need_rows(out, "out")
        if tuple(out.shape) != (rows, d):
            raise L.GnnmpError(f"feature_propagate: out {tuple(out.shape)} against x {(rows, d)}")
    n = _prop_args("feature_propagate", rowptr, col, rows, "x", left, right, (out,) + ((x.rowptr, x.col, x.val) if sparse else (x,)))
    rounds, l = int(rounds), L.lib()
    status = torch.zeros(2, dtype=torch.int32, device=dev)
    ld = lambda t: t.stride(0) if t.size(0) > 1 else t.size(1)                     # noqa: E731
    ws = _ws(l.gmp_feature_propagate_workspace_bytes(n, d, rounds), dev)
    feat_args = (None, 0, _ptr(x.rowptr), _ptr(x.col), _ptr(x.val), x.val.numel()) if sparse else (_ptr(x), ld(x), None, None, None, 0)
    L.check(l.gmp_feature_propagate(_ptr(rowptr), _ptr(col), n, col.numel(), _ptr(left), _ptr(right), *feat_args, d, rounds, _ptr(out), ld(out),
                                    _ptr(status), _ptr(ws), ws.numel(), _stream(rowptr)), "gmp_feature_propagate")
    return FeaturePropagation(out, status)


GRAPH_FEAT_MAX_ROUNDS, GRAPH_FEAT_MAX_DIM, GRAPH_FEAT_MAX_GRAPH_NODES = 16, 256, 1024     # gmp_graph_feature_map (gnnmp.h)
GRAPH_FEAT_POOLS = ("sum", "mean", "max")


class GraphFeatureMap(NamedTuple):
    """graph_feature_map's outputs (gnnmp.h gmp_graph_feature_map)."""
    out: Tensor                    # fp32 [G, rounds + 1, 3, d]: per graph and level t the sum, mean and max pool of H(t) = S^t X
    status: Tensor                 # int32 [G]: bit 0 = refused (too large, all its outputs +0), bits 8.. = skipped CSR entries


def graph_feature_map(ptr: Tensor, rowptr: Tensor, col: Tensor, x: Tensor, rounds: int, left: Optional[Tensor] = None,
                      right: Optional[Tensor] = None, max_graph_nodes: Optional[int] = None) -> GraphFeatureMap:
    """The pooled-feature map of a batch of graphs in one launch (gnnmp.h gmp_graph_feature_map holds the definition; csrc/graph_feat.hip):
    per graph the sum, mean and max pool (GRAPH_FEAT_POOLS) over its nodes of H(t), t = 0 .. rounds, with H(0) = x and H(t + 1) =
    left[i] * (sum over the row's entries j inside the graph, in order, of right[j] * H(t)[j]) -- on a well-formed batch the bits of
    feature_propagate.  ptr int64 [G + 1] node offsets, (rowptr, col) ONE int32 CSR over the batch's N nodes, x fp32 [N, d] with contiguous
    rows (any leading dimension), 1 <= d <= 256, 0 <= rounds <= 16, left / right fp32 [N] or None (ones).  max_graph_nodes: the largest
    ptr[g + 1] - ptr[g] when the caller knows it (None reads it back from ptr, one synchronisation); a graph above it, or above 1024
    nodes, is refused with status bit 0 and zero outputs.  Returns GraphFeatureMap(out, status); no other read-back: status stays on the
    device."""
    _need(ptr, torch.int64, "ptr", 1)
    _need_rows(x, "x")
    G, d = ptr.numel() - 1, int(x.size(1))
    N = _prop_args("graph_feature_map", rowptr, col, int(x.size(0)), "x", left, right, (ptr, x))
    if G < 0:
        raise L.GnnmpError(f"graph_feature_map: ptr {tuple(ptr.shape)} (G + 1 entries)")
    if not 1 <= d <= GRAPH_FEAT_MAX_DIM or not 0 <= int(rounds) <= GRAPH_FEAT_MAX_ROUNDS:
        raise L.GnnmpError(f"graph_feature_map: d={d} rounds={rounds} (1 <= d <= {GRAPH_FEAT_MAX_DIM}, 0 <= rounds <= {GRAPH_FEAT_MAX_ROUNDS})")
    if max_graph_nodes is None:
        max_graph_nodes = _max_graph_nodes(ptr, G)
    if int(max_graph_nodes) < 0:
        raise L.GnnmpError(f"graph_feature_map: max_graph_nodes={max_graph_nodes} (>= 0)")
    rounds, dev = int(rounds), ptr.device
    out = torch.empty(G, rounds + 1, len(GRAPH_FEAT_POOLS), d, device=dev)
    status = torch.zeros(G, dtype=torch.int32, device=dev)
    if G:
        L.check(L.lib().gmp_graph_feature_map(_ptr(ptr), G, _ptr(rowptr), _ptr(col), N, col.numel(), _ptr(left), _ptr(right), _ptr(x),
                                              x.stride(0) if x.size(0) > 1 else d, d, rounds, int(max_graph_nodes), _ptr(out), _ptr(status),
                                              _stream(ptr)), "gmp_graph_feature_map")
    return GraphFeatureMap(out, status)


def gc_head_fwd(h: Tensor, ptr: Tensor, w0: Tensor, b0: Tensor, w3: Tensor, b3: Tensor, target: Tensor, g_scale: Tensor, p: float = 0.0,
                seed: int = 0, site: int = 0) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """The fused graph-classification head up to the loss (gnnmp.h gmp_gc_head_fwd): h [N, 256] (rows contiguous, any leading dimension),
    ptr int32 [B + 1], w0 [128, 256], b0 [128], w3 [C, 128], b3 [C], target int64 [B], g_scale fp32 [1].  Returns (pooled [B, 256],
    act [B, 128] = the pre-dropout ReLU output, logits [B, C], loss [1] = the sum over the batch, g_logits [B, C] scaled by g_scale)."""
    _need_rows(h, "h")
    _need(ptr, torch.int32, "ptr", 1); _need(target, torch.int64, "target", 1); _need(g_scale, torch.float32, "g_scale")
    for t, n in ((w0, "w0"), (b0, "b0"), (w3, "w3"), (b3, "b3")):
        _need(t, torch.float32, n)
    B, dev, l = ptr.numel() - 1, h.device, L.lib()
    if B < 1 or target.numel() != B:
        raise L.GnnmpError(f"gc_head_fwd: ptr has {ptr.numel()} entries for {target.numel()} targets")
    Cn, Hd = w3.size(0), w0.size(0)
    if w3.dim() != 2 or w3.size(1) != Hd or b0.numel() != Hd or b3.numel() != Cn or w0.size(1) != h.size(1):
        raise L.GnnmpError("gc_head_fwd: weight shapes")
    pooled, act, logits = torch.empty(B, h.size(1), device=dev), torch.empty(B, Hd, device=dev), torch.empty(B, Cn, device=dev)
    loss, g_logits = torch.empty(1, device=dev), torch.empty(B, Cn, device=dev)
    ws = _ws(l.gmp_gc_head_fwd_workspace_bytes(B), dev)
    ldh = h.stride(0) if h.size(0) > 1 else h.size(1)
    L.check(l.gmp_gc_head_fwd(_ptr(h), ldh, _ptr(ptr), h.size(0), B, h.size(1), Hd, Cn, _ptr(w0), _ptr(b0), _ptr(w3), _ptr(b3), _ptr(target),
                              _ptr(g_scale), _ptr(pooled), _ptr(act), _ptr(logits), _ptr(loss), _ptr(g_logits), float(p), seed & (2 ** 64 - 1),
                              site, _ptr(ws), ws.numel(), _stream(h)), "gmp_gc_head_fwd")
    return pooled, act, logits, loss, g_logits


def gc_head_bwd(ptr: Tensor, num_nodes: int, w0: Tensor, w3: Tensor, pooled: Tensor, act: Tensor, g_logits: Tensor, p: float = 0.0,
                seed: int = 0, site: int = 0) -> Tuple[Tensor, Tensor, Tensor, Tensor, Tensor]:
    """Backward of gc_head_fwd from its g_logits (gnnmp.h gmp_gc_head_bwd).  Returns (g_w0 [128, 256], g_b0 [128], g_w3 [C, 128], g_b3 [C],
    g_h [num_nodes, 256]: every row written, g_pooled[graph(i)] / max(count, 1))."""
    _need(ptr, torch.int32, "ptr", 1)
    for t, n in ((w0, "w0"), (w3, "w3"), (pooled, "pooled"), (act, "act"), (g_logits, "g_logits")):
        _need(t, torch.float32, n, 2)
    B, dev = ptr.numel() - 1, w0.device
    Cn, Hd, F = w3.size(0), w0.size(0), w0.size(1)
    if B < 1 or pooled.shape != (B, F) or act.shape != (B, Hd) or g_logits.shape != (B, Cn) or w3.size(1) != Hd:
        raise L.GnnmpError("gc_head_bwd: shapes")
    g_w0, g_b0, g_w3, g_b3 = torch.empty_like(w0), torch.empty(Hd, device=dev), torch.empty_like(w3), torch.empty(Cn, device=dev)
    g_h = torch.empty(num_nodes, F, device=dev)
    L.check(L.lib().gmp_gc_head_bwd(_ptr(ptr), num_nodes, B, F, Hd, Cn, _ptr(w0), _ptr(w3), _ptr(pooled), _ptr(act), _ptr(g_logits), float(p),
                                    seed & (2 ** 64 - 1), site, _ptr(g_w0), _ptr(g_b0), _ptr(g_w3), _ptr(g_b3), _ptr(g_h), F, _stream(w0)),
            "gmp_gc_head_bwd")
    return g_w0, g_b0, g_w3, g_b3, g_h
