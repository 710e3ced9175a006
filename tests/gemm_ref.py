"""Shared by test_gemm_ref_host.py, test_gemm_host.py and test_gpu_gemm_contract.py: the float64 definition of what gmp_gemm_f32,
gmp_gemm_f32_grouped and gmp_colsum (include/gnnmp.h, csrc/gemm_f32.hip, csrc/gemm_pipe.h) promise, operand views with the strides and base
residues the dispatch looks at, sentinel-backed outputs, and ctypes callers that take explicit leading dimensions, offsets and workspace
(ops.gemm needs a contiguous `out` and passes ldc = N).

The references are written with whole-matrix products and row masks, not per-group slices, so that test_gemm_ref_host.py can hold them against
a plain loop of torch.matmul.  The epilogue order is the kernels': v = alpha * product (+ bias); accumulate: v += C; relu: max(v, 0).

Exactness argument of the integer cases: operands in [-4, 4] and K <= 2048 keep every product and partial sum an integer below 2^15 * 2^4,
alpha in {1, 0.5, -2} and an integer bias / accumulator keep the epilogue within 24 bits -- fp32 must then give the fp64 value bit for bit
in ANY accumulation order.
"""
import ctypes as C

import torch

from gnn_pretraining_amd import _lib as L

NT, NN, TN = 0, 1, 2
OK, ERR_ARG, ERR_WORKSPACE = 0, -1, -3
LAYOUTS = ["packed", "padded", "odd", "shifted"]
LD_EXTRA = {"packed": 0, "padded": 4, "odd": 1, "shifted": 4}      # leading dimension = extent + this
SHIFT = {"packed": 0, "padded": 0, "odd": 0, "shifted": 1}         # floats the base sits past a 16-byte boundary
SENTINEL = -77777.0                  # exactly representable; no integer case produces it (every result is a multiple of 0.5 below 2^20)
POISON = 1.0e30                      # fills the columns between the extent and the leading dimension of an INPUT: a leak is not subtle


# ---- float64 references ---------------------------------------------------------------------------------------------------------
def _epilogue(v, bias, c0, alpha, accumulate, relu):
    v = alpha * v
    if bias is not None:
        v = v + bias.double()
    if accumulate:
        v = v + c0.double()
    return v.clamp_min(0) if relu else v


def ref_product(mode, A, B):
    A, B = A.double(), B.double()
    return A @ B.t() if mode == NT else A @ B if mode == NN else A.t() @ B


def ref_gemm(mode, A, B, bias=None, c0=None, alpha=1.0, accumulate=False, relu=False, product=None):
    """C [M, N] of gmp_gemm_f32; `product` = ref_product(mode, A, B) when the caller shares it between epilogues."""
    return _epilogue(ref_product(mode, A, B) if product is None else product, bias, c0, alpha, accumulate, relu)


def _row_masks(rows, total):
    idx = torch.arange(total)
    return [((idx >= rows[g]) & (idx < rows[g + 1])).double() for g in range(len(rows) - 1)]


def ref_grouped_rows(mode, A, weights, rows, biases=None, c0=None, alpha=1.0, accumulate=False, relu=False):
    """NT / NN grouped form: rows [rows[g], rows[g+1]) of A times weights[g] ([N, K] for NT, [K, N] for NN) (+ biases[g]) -> [rows[-1], N].
    Every group's product is taken over ALL rows and masked down to its own."""
    R = rows[-1]
    A = A[:R].double()
    out = None
    for g, m in enumerate(_row_masks(rows, R)):
        v = A @ weights[g].double().t() if mode == NT else A @ weights[g].double()
        v = alpha * v
        if biases is not None:
            v = v + biases[g].double()
        out = v * m[:, None] if out is None else out + v * m[:, None]
    if accumulate:
        out = out + c0[:R].double()
    return out.clamp_min(0) if relu else out


def ref_grouped_tn(A, B, rows, c0=None, alpha=1.0, accumulate=False, relu=False):
    """TN grouped form: per group alpha * A[r0:r1]^T B[r0:r1] (+ c0[g]) -> [groups, M_tn, N], and the rider colsum A[r0:r1] -> [groups, M_tn]
    (stored, never accumulated).  An empty group gives zeros, or c0[g] under accumulate."""
    A, B = A.double(), B.double()
    outs, sums = [], []
    for g, m in enumerate(_row_masks(rows, A.size(0))):
        Am = A * m[:, None]
        v = alpha * (Am.t() @ B)
        if accumulate:
            v = v + c0[g].double()
        outs.append(v.clamp_min(0) if relu else v)
        sums.append(Am.sum(0))
    return torch.stack(outs), torch.stack(sums)


def ref_colsum(A, c0=None, accumulate=False):
    s = A.double().sum(0)
    return s + c0.double() if accumulate else s


# ---- operand views -----------------------------------------------------------------------------------------------------------------
def _aligned_start(flat):
    """index of the first element of `flat` that sits on a 16-byte boundary"""
    assert flat.data_ptr() % 4 == 0
    return (-(flat.data_ptr() // 4)) % 4


def operand(values, layout, device="cpu", fill=POISON, ld_extra=None):
    """A [R, C] float32 view holding `values` with the leading dimension and base residue `layout` names; the gaps hold `fill`.
    ld_extra overrides the layout's leading dimension (extent + ld_extra), the base residue stays the layout's."""
    R, Cc = values.shape
    ld = Cc + (LD_EXTRA[layout] if ld_extra is None else ld_extra)
    flat = torch.full((R * ld + 8,), fill, dtype=torch.float32, device=device)
    v = flat.as_strided((R, Cc), (ld, 1), _aligned_start(flat) + SHIFT[layout])
    v.copy_(values)
    return v


def vector(values, layout, device="cpu", fill=POISON):
    """A 1-D float32 view of `values`: 16-byte aligned, or one float past a boundary for `shifted`."""
    flat = torch.full((values.numel() + 8,), fill, dtype=torch.float32, device=device)
    v = flat.as_strided((values.numel(),), (1,), _aligned_start(flat) + SHIFT[layout])
    v.copy_(values)
    return v


def flat_pack(pieces, offsets, device="cpu", fill=POISON):
    """One aligned flat float32 buffer with pieces[g] (1-D, or 2-D written packed) at offsets[g] floats; returns a view whose element 0 is
    16-byte aligned."""
    total = max(o + p.numel() for p, o in zip(pieces, offsets)) + 8
    flat = torch.full((total + 4,), fill, dtype=torch.float32)
    for p, o in zip(pieces, offsets):
        flat[o:o + p.numel()] = p.reshape(-1)
    dev = torch.empty(total + 4, dtype=torch.float32, device=device)
    s = _aligned_start(dev)
    view = dev[s:s + total]
    view.copy_(flat[:total])
    return view


class Out:
    """Sentinel-filled backing buffer with one or more [R, C] output windows (offset in floats from `ptr`, leading dimension ld) and guard
    space before and after.  stray() counts the elements outside every window that are no longer bitwise the sentinel."""

    def __init__(self, windows, span, guard, shift=0, device="cpu"):
        self.windows = list(windows)
        self.flat = torch.full((4 + guard + span + guard + 4,), SENTINEL, dtype=torch.float32, device=device)
        self.base = _aligned_start(self.flat) + guard + shift
        assert guard % 4 == 0

    @classmethod
    def single(cls, M, N, layout, device="cpu", guard_rows=4):
        ld = N + LD_EXTRA[layout]
        return cls([(0, M, N, ld)], max(M, 1) * ld, 4 * ((guard_rows * ld + 3) // 4), SHIFT[layout], device)

    @property
    def ptr(self):
        return self.flat.data_ptr() + 4 * self.base

    @property
    def ld(self):
        return self.windows[0][3]

    def win(self, i=0, flat=None):
        off, R, Cc, ld = self.windows[i]
        return (self.flat if flat is None else flat).as_strided((R, Cc), (ld, 1), self.base + off)

    def fill(self, values, i=0):
        self.win(i).copy_(values)
        return self

    def reset(self):
        self.flat.fill_(SENTINEL)
        return self

    def stray(self):
        m = self.flat.clone()
        for i in range(len(self.windows)):
            self.win(i, m).fill_(SENTINEL)
        bits = torch.tensor([SENTINEL], dtype=torch.float32).view(torch.int32).item()
        return int((m.view(torch.int32) != bits).sum().item())


# ---- ctypes callers (return the status code) -----------------------------------------------------------------------------------------
def _p(x):
    if x is None:
        return None
    return C.c_void_p(x if isinstance(x, int) else x.data_ptr())


def _ws(ws):
    """None, a uint8 tensor, or (address, bytes)"""
    if ws is None:
        return None, 0
    if isinstance(ws, tuple):
        return C.c_void_p(ws[0]), ws[1]
    return C.c_void_p(ws.data_ptr()), ws.numel()


def _stream():
    return torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else None


def _arr(ctype, xs):
    return None if xs is None else (ctype * len(xs))(*xs)


def gemm(mode, A, B, bias, Cp, M, N, K, lda, ldb, ldc, alpha=1.0, accumulate=0, relu=0, ws=None):
    wp, wb = _ws(ws)
    return L.lib().gmp_gemm_f32(mode, _p(A), _p(B), _p(bias), _p(Cp), M, N, K, lda, ldb, ldc, float(alpha), int(accumulate), int(relu), wp, wb, _stream())


def gemm_grouped(mode, A, B, bias, Cp, rows, b_off=None, bias_off=None, c_off=None, a_colsum=None, a_colsum_off=None, M_tn=0, N=0, K=0,
                 lda=0, ldb=0, ldc=0, alpha=1.0, accumulate=0, relu=0, ws=None, groups=None):
    wp, wb = _ws(ws)
    ng = (len(rows) - 1) if groups is None else groups
    return L.lib().gmp_gemm_f32_grouped(mode, _p(A), _p(B), _p(bias), _p(Cp), ng, _arr(C.c_int32, rows), _arr(C.c_int64, b_off),
                                        _arr(C.c_int64, bias_off), _arr(C.c_int64, c_off), _p(a_colsum), _arr(C.c_int64, a_colsum_off), M_tn, N, K,
                                        lda, ldb, ldc, float(alpha), int(accumulate), int(relu), wp, wb, _stream())


def colsum(A, out, M, N, lda, accumulate=0, ws=None):
    wp, wb = _ws(ws)
    return L.lib().gmp_colsum(_p(A), _p(out), M, N, lda, int(accumulate), wp, wb, _stream())


def gemm_workspace_bytes(mode, M, N, K):
    return L.lib().gmp_gemm_f32_workspace_bytes(mode, M, N, K)


def last_error():
    return L.lib().gmp_last_error_string()
