"""The full contract of the GEMM entry points -- gmp_gemm_f32, gmp_gemm_f32_grouped, gmp_colsum and the gate signal that rides on a GEMM
(include/gnnmp.h; csrc/gemm_f32.hip, csrc/gemm_pipe.h) -- against the float64 references of gemm_ref.py, called through ctypes with
explicit leading dimensions, base offsets and workspace: everything ops.gemm (contiguous out, ldc = N) never passes.

Data are small integers (operands, bias and accumulator in [-4, 4], alpha in {1, 0.5, -2}, K <= 2048): every product, partial sum and
epilogue value is exact in fp32, so each call must equal the float64 reference BIT FOR BIT (torch.equal) in any accumulation order, and an
asymmetric B exposes a permuted fragment.  One random-normal case per kernel family runs at the suite's existing bound, 2e-5 of the largest
reference magnitude (test_gpu_gemm_pipe.py).  No other tolerance.  Every output lives in a sentinel-filled buffer with guard rows: nothing
outside C[0:M, 0:N] may change.

Which path a case takes is read off the dispatch code (gmp::gemm_f32_epilogue, grouped_impl), never asserted:
  vecA / vecB (16-byte base, ld % 4 == 0) + M >= 1024, N >= 64, K >= 64, K % 32 == 0 (NN: N % 4 == 0)  -> pipelined kernel, else first kernel;
  first kernel: fast loader when vecA, vecB and (NT / NN) K % 32 == 0, (NN / TN) N % 4 == 0, (TN) M % 4 == 0, else the guarded loader;
  pipelined kernel: float4 epilogue when vecC (16-byte C, ldc % 4 == 0, bias and every offset 16-byte addressable), else the scalar one;
  a workspace turns few-tile / long-K problems into K-slices (split-K) of whichever kernel the problem takes;
  grouped TN with a workspace and a group of >= 256 rows is cut into row slices (pipelined kernel when M_tn % 4 == 0 and the operands are
  16-byte addressable, else first kernel) and reduced by the float4 reduce, or the scalar one when a c_off is not a multiple of 4.
"""
import ctypes as C
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_ref as R                                     # noqa: E402
from gnn_pretraining_amd import _lib as L, ops          # noqa: E402

DEV = torch.device("cuda:0")
NT, NN, TN = R.NT, R.NN, R.TN
MODE_NAME = {NT: "NT", NN: "NN", TN: "TN"}
REL_BOUND = 2e-5          # random-normal cases only: fp32 accumulation over K, of the largest reference magnitude (test_gpu_gemm_pipe.py)


def _ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).float()


def _same(got, ref):
    """bitwise agreement with the float64 reference (an fp32 value converts to float64 exactly)"""
    return torch.equal(got.cpu().double(), ref)


@pytest.fixture(autouse=True)
def _no_signal_left_pending():
    yield
    if L.lib().gmp_gate_open_pending():
        L.lib().gmp_gate_open_by_next_gemm(None, 0)


def _workspace(nbytes=8 << 20):
    return torch.empty(nbytes, dtype=torch.uint8, device=DEV)


# ---- a. single problems x layouts ------------------------------------------------------------------------------------------------------
# (M, N, K, workspace): first kernel; first kernel with K % 32 == 0 (fast loader where aligned); pipelined; pipelined with ragged M and N tiles;
# K-slices of the pipelined kernel (NT / NN; TN: split-K of the first kernel)
SHAPES = [(65, 130, 67, False), (130, 68, 64, False), (1025, 68, 96, False), (1283, 196, 96, False), (1100, 128, 1440, True)]
TN_SPLITK = (96, 68, 1030, True)          # output 96 x 68 over 1030 rows: split-K of the first kernel (partial last K-step, empty last slices)
SINGLE = [(m, s) for m in (NT, NN, TN) for s in SHAPES] + [(TN, TN_SPLITK)]
SINGLE_IDS = [f"{MODE_NAME[m]}-{s[0]}x{s[1]}x{s[2]}" for m, s in SINGLE]
EPILOGUES = [dict(bias=True, alpha=1.0, accumulate=0, relu=1), dict(bias=False, alpha=0.5, accumulate=1, relu=0),
             dict(bias=False, alpha=-2.0, accumulate=0, relu=1)]


@functools.lru_cache(maxsize=None)
def _single_data(mode, M, N, K, normal=False):
    g = torch.Generator().manual_seed(1000 * mode + M + N + K)
    draw = (lambda *s: torch.randn(*s, generator=g)) if normal else (lambda *s: _ints(g, *s))
    A = draw(K, M) if mode == TN else draw(M, K)
    B = draw(N, K) if mode == NT else draw(K, N)
    bias, c0 = draw(N), draw(M, N)
    return A, B, bias, c0, R.ref_product(mode, A, B)


def _run_single(mode, shape, la, lb, lc, bias_layout="packed", epilogues=EPILOGUES, normal=False):
    M, N, K, use_ws = shape
    A, B, bias, c0, prod = _single_data(mode, M, N, K, normal)
    Ad, Bd, bd = R.operand(A, la, DEV), R.operand(B, lb, DEV), R.vector(bias, bias_layout, DEV)
    out = R.Out.single(M, N, lc, DEV)
    ws = None
    if use_ws:
        need = R.gemm_workspace_bytes(mode, M, N, K)
        assert need > 0
        ws = _workspace(need)
    for e in epilogues:
        out.reset()
        if e["accumulate"]:
            out.fill(c0.to(DEV))
        rc = R.gemm(mode, Ad, Bd, bd if e["bias"] else None, out.ptr, M, N, K, Ad.stride(0), Bd.stride(0), out.ld, e["alpha"], e["accumulate"], e["relu"], ws)
        assert rc == R.OK, R.last_error()
        ref = R.ref_gemm(mode, A, B, bias if e["bias"] else None, c0, e["alpha"], e["accumulate"], e["relu"], product=prod)
        got = out.win().cpu().double()
        if normal:
            err = (got - ref).abs().max().item() / ref.abs().max().item()
            print(f"{MODE_NAME[mode]} {M}x{N}x{K} {e}: rel err {err:.3e}")
            assert err < REL_BOUND, e
        else:
            assert torch.equal(got, ref), e
        assert out.stray() == 0, f"{e}: wrote outside C[0:{M}, 0:{N}] (ldc {out.ld})"


@pytest.mark.parametrize("layout", R.LAYOUTS)
@pytest.mark.parametrize("mode,shape", SINGLE, ids=SINGLE_IDS)
def test_single_problem_in_every_layout(mode, shape, layout):
    """A, B and C together packed / padded (ld + 4) / odd (ld + 1) / shifted (base + one float, ld + 4): both kernels, both loaders, both
    epilogues of the pipelined kernel and both split-K forms, each with bias + ReLU, alpha 0.5 accumulated onto an integer C, alpha -2 + ReLU."""
    _run_single(mode, shape, layout, layout, layout)


@pytest.mark.parametrize("c_layout", ["odd", "shifted"])
@pytest.mark.parametrize("mode,shape", SINGLE, ids=SINGLE_IDS)
def test_single_problem_packed_operands_unaligned_output(mode, shape, c_layout):
    """packed A and B keep the kernel choice of the aligned problem; only C is not 16-byte addressable -- at M >= 1024 the scalar epilogue
    of the pipelined kernel"""
    _run_single(mode, shape, "packed", "packed", c_layout)


@pytest.mark.parametrize("mode,shape", [(NT, SHAPES[1]), (NT, SHAPES[3]), (NN, SHAPES[3]), (TN, TN_SPLITK)],
                         ids=["first-NT", "pipelined-NT", "pipelined-NN", "first-TN-splitk"])
def test_single_problem_random_normal(mode, shape):
    _run_single(mode, shape, "padded", "padded", "padded", normal=True)


# ---- d. a bias that is not 16-byte addressable (single form) -----------------------------------------------------------------------------
@pytest.mark.parametrize("c_layout", ["packed", "padded"])
def test_shifted_bias_at_pipelined_row_count(c_layout):
    """M = 1025 with aligned A, B, C: the pipelined kernel; the bias one float past a 16-byte boundary sends it to the scalar epilogue
    (gmp::gemm_f32_epilogue clears vecC), which reads the bias one float at a time"""
    _run_single(NT, SHAPES[2], "packed", "packed", c_layout, bias_layout="shifted", epilogues=EPILOGUES[:1])
    _run_single(NN, SHAPES[3], "packed", "packed", c_layout, bias_layout="shifted", epilogues=EPILOGUES[:1])


# ---- b. grouped NT / NN ---------------------------------------------------------------------------------------------------------------------
ROWS_SMALL = [0, 1, 1, 70, 200, 333]              # first kernel: a one-row group, an empty group, ragged tails
ROWS_PIPE = [0, 1100, 1100, 1101, 1400]           # max_rows >= 1024: pipelined kernel where aligned; groups far shorter than the grid's row extent
GROUPED = [(ROWS_SMALL, 64, 64), (ROWS_SMALL, 68, 96), (ROWS_SMALL, 7, 37), (ROWS_PIPE, 64, 64), (ROWS_PIPE, 68, 96)]
GROUPED_IDS = [f"{'small' if r is ROWS_SMALL else 'pipe'}-N{n}-K{k}" for r, n, k in GROUPED]
TAIL_ROWS = 3                                      # rows of A (and guard rows of C) beyond rows[-1]


def _ceil4(x):
    return (x + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def _grouped_data(mode, rows, N, K, normal=False):
    g = torch.Generator().manual_seed(7 * mode + rows[-1] + N + K)
    draw = (lambda *s: torch.randn(*s, generator=g)) if normal else (lambda *s: _ints(g, *s))
    ng = len(rows) - 1
    A = draw(rows[-1] + TAIL_ROWS, K)
    W = [draw(N, K) if mode == NT else draw(K, N) for _ in range(ng)]
    b = [draw(N) for _ in range(ng)]
    return A, W, b, draw(rows[-1], N)


def _run_grouped(mode, rows, N, K, b_shift=0, bias_shift=0, normal=False):
    A, W, b, c0 = _grouped_data(mode, tuple(rows), N, K, normal)
    ng = len(rows) - 1
    b_off = [g * (_ceil4(N * K) + 4) for g in range(ng)]
    bias_off = [g * (_ceil4(N) + 4) + bias_shift for g in range(ng)]
    b_off[2] += b_shift                            # one weight matrix off the 16-byte grid: no float4 loads of B for the whole call
    Wd, bd = R.flat_pack(W, b_off, DEV), R.flat_pack(b, bias_off, DEV)
    Ad = R.operand(A, "padded", DEV)
    out = R.Out.single(rows[-1], N, "padded", DEV, guard_rows=TAIL_ROWS + 1)
    ldb = K if mode == NT else N
    for e in EPILOGUES[:2]:
        out.reset()
        if e["accumulate"]:
            out.fill(c0.to(DEV))
        rc = R.gemm_grouped(mode, Ad, Wd, bd if e["bias"] else None, out.ptr, rows, b_off, bias_off if e["bias"] else None, None, None, None, 0, N, K,
                            Ad.stride(0), ldb, out.ld, e["alpha"], e["accumulate"], e["relu"])
        assert rc == R.OK, R.last_error()
        ref = R.ref_grouped_rows(mode, A, W, rows, b if e["bias"] else None, c0, e["alpha"], e["accumulate"], e["relu"])
        got = out.win().cpu().double()
        if normal:
            err = (got - ref).abs().max().item() / ref.abs().max().item()
            print(f"grouped {MODE_NAME[mode]} rows {rows[-1]} N {N} K {K} {e}: rel err {err:.3e}")
            assert err < REL_BOUND, e
        else:
            for g in range(ng):
                assert torch.equal(got[rows[g]:rows[g + 1]], ref[rows[g]:rows[g + 1]]), f"group {g}, {e}"
        assert out.stray() == 0, f"{e}: wrote outside the groups' rows (rows beyond rows[-1] included)"


@pytest.mark.parametrize("b_shift", [0, 1], ids=["aligned", "odd_b_off"])
@pytest.mark.parametrize("mode", [NT, NN], ids=["NT", "NN"])
@pytest.mark.parametrize("rows,N,K", GROUPED, ids=GROUPED_IDS)
def test_grouped_rows_own_weights_and_bias(rows, N, K, mode, b_shift):
    """every group's rows times its own weight matrix at b_off[g] (+ its bias at bias_off[g]); blocks past a short group return early, rows
    beyond rows[-1] keep the sentinel; with one odd b_off only the result is asserted, not the kernel chosen"""
    _run_grouped(mode, rows, N, K, b_shift=b_shift)


def test_grouped_bias_offset_of_4k_plus_1_at_pipelined_row_list():
    """aligned A, B and C at max_rows >= 1024 (the pipelined kernel) with every bias_off = 4 k + 1: grouped_impl clears vecC, the scalar
    epilogue reads the bias one float at a time"""
    _run_grouped(NT, ROWS_PIPE, 68, 96, bias_shift=1)
    _run_grouped(NT, ROWS_PIPE, 64, 64, bias_shift=1)


@pytest.mark.parametrize("rows", [ROWS_SMALL, ROWS_PIPE], ids=["first", "pipelined"])
def test_grouped_rows_random_normal(rows):
    _run_grouped(NT, rows, 68, 96, normal=True)


@pytest.mark.parametrize("rows,N", [([0, 70, 100, 170], 70), ([0, 1100, 1130, 2230], 1100)], ids=["first", "pipelined"])
def test_grouped_nt_xent_form_b_aliases_a(rows, N):
    """the grouped NT-Xent's similarity (ntxent.hip): B is A, b_off[g] = rows[g] * lda, N = the longest group -- per group the rows times the
    N rows that start at the group's first (the Gram matrix of a full group; a short group's trailing columns come from the rows that follow)"""
    g = torch.Generator().manual_seed(N)
    K = 64
    A = _ints(g, rows[-1] + TAIL_ROWS, K)
    Ad = R.operand(A, "padded", DEV)
    lda, ng = Ad.stride(0), len(rows) - 1
    assert all(rows[i] + N <= A.size(0) for i in range(ng))
    out = R.Out.single(rows[-1], N, "padded", DEV, guard_rows=TAIL_ROWS + 1)
    rc = R.gemm_grouped(NT, Ad, Ad, None, out.ptr, rows, [r * lda for r in rows[:-1]], None, None, None, None, 0, N, K, lda, lda, out.ld, alpha=0.5)
    assert rc == R.OK, R.last_error()
    ref = R.ref_grouped_rows(NT, A, [A[r:r + N] for r in rows[:-1]], rows, alpha=0.5)
    assert _same(out.win(), ref) and out.stray() == 0
    full = ref[rows[0]:rows[1], :rows[1] - rows[0]]
    assert torch.equal(full, full.t())             # (what "Gram" means here: the reference of a full group is symmetric)


# ---- c. grouped TN ---------------------------------------------------------------------------------------------------------------------------
TN_ROWS_LONG = [0, 400, 400, 401, 700]             # max_rows >= 256: row slices when a workspace is given; an empty and a one-row group
TN_ROWS_SHORT = [0, 100, 100, 101, 230]            # max_rows < 256: never sliced, with or without a workspace
# (name, M_tn, one c_off odd): 16-byte addressable throughout -> pipelined kernel + float4 reduce when sliced; M_tn % 4 != 0 (and with it an
# odd lda = M_tn + 4) -> first kernel, guarded loader, float4 reduce; an odd c_off -> first kernel, scalar reduce
TN_CASES = [("aligned", 64, False), ("m66", 66, False), ("odd_c_off", 64, True)]
TN_N = 68


@functools.lru_cache(maxsize=None)
def _tn_data(rows, M_tn, normal=False):
    g = torch.Generator().manual_seed(rows[-1] + M_tn)
    draw = (lambda *s: torch.randn(*s, generator=g)) if normal else (lambda *s: _ints(g, *s))
    ng = len(rows) - 1
    return draw(rows[-1] + 2, M_tn), draw(rows[-1] + 2, TN_N), draw(ng, M_tn, TN_N)


def _run_tn(rows, M_tn, odd_c, use_ws, normal=False):
    A, B, c0 = _tn_data(tuple(rows), M_tn, normal)
    N, ng = TN_N, len(rows) - 1
    Ad, Bd = R.operand(A, "padded", DEV), R.operand(B, "padded", DEV)          # lda = M_tn + 4, ldb = N + 4
    ldc = N + 4
    c_off = [g * (M_tn * ldc + 4) for g in range(ng)]
    if odd_c:
        c_off[1] += 1
    out = R.Out([(o, M_tn, N, ldc) for o in c_off], span=ng * (M_tn * ldc + 4) + 4, guard=4 * ldc, device=DEV)
    s_off = [g * (M_tn + 4) for g in range(ng)]
    sums = R.Out([(o, 1, M_tn, M_tn) for o in s_off], span=ng * (M_tn + 4), guard=M_tn + 6 - (M_tn + 6) % 4, device=DEV)
    sums_dense = R.Out([(g * M_tn, 1, M_tn, M_tn) for g in range(ng)], span=ng * M_tn, guard=M_tn + 6 - (M_tn + 6) % 4, device=DEV)
    ws = _workspace() if use_ws else None
    # (alpha, accumulate, relu, colsum buffer, explicit colsum offsets)
    for alpha, acc, relu, cs, cs_off in [(1.0, 0, 0, sums, s_off), (0.5, 1, 0, sums_dense, None), (-2.0, 0, 1, None, None), (0.5, 1, 1, sums, s_off)]:
        out.reset()
        if acc:
            for g in range(ng):
                out.fill(c0[g].to(DEV), g)
        if cs is not None:
            cs.reset()
        rc = R.gemm_grouped(TN, Ad, Bd, None, out.ptr, rows, None, None, c_off, None if cs is None else cs.ptr, cs_off, M_tn, N, 0,
                            Ad.stride(0), Bd.stride(0), ldc, alpha, acc, relu, ws)
        what = f"alpha {alpha} accumulate {acc} relu {relu} workspace {use_ws}"
        assert rc == R.OK, R.last_error()
        ref, ref_sums = R.ref_grouped_tn(A, B, rows, c0, alpha, acc, relu)
        for g in range(ng):
            got = out.win(g).cpu().double()
            if normal:
                scale = max(ref[g].abs().max().item(), 1e-30)
                if rows[g] == rows[g + 1]:
                    assert torch.equal(got, ref[g]), f"empty group {g}, {what}"
                else:
                    assert (got - ref[g]).abs().max().item() / scale < REL_BOUND, f"group {g}, {what}"
            else:
                assert torch.equal(got, ref[g]), f"group {g}, {what}"
            if rows[g] == rows[g + 1]:              # an empty group: zeros, or C unchanged under accumulate (ReLU applied)
                want = c0[g].double() if acc else torch.zeros(M_tn, N, dtype=torch.float64)
                assert torch.equal(got, want.clamp_min(0) if relu else want)
            if cs is not None and not normal:
                assert torch.equal(cs.win(g).cpu().double()[0], ref_sums[g]), f"column sums of group {g}, {what}"
        assert out.stray() == 0, f"{what}: wrote outside the groups' C windows (ldc {ldc})"
        if cs is not None:
            assert cs.stray() == 0, f"{what}: column sums outside their rows"


@pytest.mark.parametrize("use_ws", [True, False], ids=["workspace", "no_workspace"])
@pytest.mark.parametrize("rows", [TN_ROWS_LONG, TN_ROWS_SHORT], ids=["long", "short"])
@pytest.mark.parametrize("name,M_tn,odd_c", TN_CASES, ids=[c[0] for c in TN_CASES])
def test_grouped_tn_epilogue_offsets_and_leading_dimensions(name, M_tn, odd_c, rows, use_ws):
    """C_g = act(alpha G_g^T X_g (+ C_g)) with and without a workspace (the row-sliced reduce must honour accumulate and ReLU exactly as the
    unsliced kernels do), lda = M_tn + 4, ldb = ldc = N + 4, an empty and a one-row group, the column-sum rider with explicit offsets, with
    a_colsum_off = NULL (g * M_tn) and with a_colsum = NULL"""
    _run_tn(rows, M_tn, odd_c, use_ws)


@pytest.mark.parametrize("use_ws", [True, False], ids=["workspace", "no_workspace"])
def test_grouped_tn_random_normal(use_ws):
    _run_tn(TN_ROWS_LONG, 64, False, use_ws, normal=True)


# ---- e. the gate signal that rides on a GEMM ------------------------------------------------------------------------------------------------
def _lp_case():
    g = torch.Generator().manual_seed(11)
    K, Nn, F = 1024, 50, 256
    h, edges = _ints(g, Nn, F), torch.randint(0, Nn, (2, K), generator=g)
    w0, b0, gy1 = _ints(g, F, 3 * F), _ints(g, F), _ints(g, K, F)
    hs, hd = h[edges[0]].double(), h[edges[1]].double()
    feat = torch.cat([hs + hd, hs * hd, (hs - hd).abs()], 1)
    y1 = (feat @ w0.double().t() + b0.double()).clamp_min(0)
    dW0, db0 = gy1.double().t() @ feat, gy1.double().sum(0)
    gf = gy1.double() @ w0.double()
    gs, gp, ga = gf[:, :F], gf[:, F:2 * F], gf[:, 2 * F:]
    t = ga * torch.sign(hs - hd)
    dev = dict(h=h.to(DEV), edges=edges.to(DEV), w0=w0.to(DEV), b0=b0.to(DEV), gy1=gy1.to(DEV))
    return dev, dict(y1=y1, dW0=dW0, db0=db0, ghs=gs + gp * hd + t, ghd=gs + gp * hs - t)


def _launchers():
    """name -> callable that makes ONE call of the entry point and returns a function that checks its result (after a synchronise)"""
    def single(mode, shape):
        M, N, K, use_ws = shape
        A, B, bias, c0, prod = _single_data(mode, M, N, K)
        Ad, Bd = R.operand(A, "packed", DEV), R.operand(B, "packed", DEV)
        out = R.Out.single(M, N, "packed", DEV)
        ws = _workspace(R.gemm_workspace_bytes(mode, M, N, K)) if use_ws else None
        assert not use_ws or ws.numel() > 0

        def call():
            assert R.gemm(mode, Ad, Bd, None, out.reset().ptr, M, N, K, Ad.stride(0), Bd.stride(0), out.ld, ws=ws) == R.OK, R.last_error()
            return lambda: _same(out.win(), prod) and out.stray() == 0
        return call

    def grouped_rows(rows, N, K):
        A, W, b, c0 = _grouped_data(NT, tuple(rows), N, K)
        b_off = [g * N * K for g in range(len(W))]
        Ad, Wd = R.operand(A, "packed", DEV), R.flat_pack(W, b_off, DEV)
        out = R.Out.single(rows[-1], N, "packed", DEV)
        ref = R.ref_grouped_rows(NT, A, W, rows)

        def call():
            assert R.gemm_grouped(NT, Ad, Wd, None, out.reset().ptr, rows, b_off, None, None, None, None, 0, N, K, K, K, N) == R.OK, R.last_error()
            return lambda: _same(out.win(), ref) and out.stray() == 0
        return call

    def grouped_tn(use_ws):
        rows, M_tn, N = TN_ROWS_LONG, 64, TN_N
        A, B, c0 = _tn_data(tuple(rows), M_tn)
        Ad, Bd = R.operand(A, "packed", DEV), R.operand(B, "packed", DEV)
        c_off = [g * M_tn * N for g in range(len(rows) - 1)]
        out = R.Out([(o, M_tn, N, N) for o in c_off], span=len(c_off) * M_tn * N, guard=4 * N, device=DEV)
        ws = _workspace() if use_ws else None
        ref, _ = R.ref_grouped_tn(A, B, rows)

        def call():
            assert R.gemm_grouped(TN, Ad, Bd, None, out.reset().ptr, rows, None, None, c_off, None, None, M_tn, N, 0, M_tn, N, N, ws=ws) == R.OK, R.last_error()
            return lambda: all(_same(out.win(g), ref[g]) for g in range(len(c_off))) and out.stray() == 0
        return call

    lp, lp_ref = _lp_case()
    lp_ws = _workspace(16 << 20)

    def lp_fwd():
        y1 = ops.lp_feat_gemm_fwd(lp["h"], lp["edges"], lp["w0"], lp["b0"])
        return lambda: _same(y1, lp_ref["y1"])

    def lp_wgrad():
        dW0, db0 = ops.lp_feat_gemm_wgrad(lp["gy1"], lp["h"], lp["edges"], lp_ws)
        return lambda: _same(dW0, lp_ref["dW0"]) and _same(db0, lp_ref["db0"])

    def lp_fold():
        ghs, ghd = ops.lp_feat_gemm_bwd_fold(lp["gy1"], lp["w0"], lp["h"], lp["edges"])
        return lambda: _same(ghs, lp_ref["ghs"]) and _same(ghd, lp_ref["ghd"])

    return {
        "gemm_kernel": single(NT, SHAPES[0]),
        "gemm_kernel_splitk": single(TN, TN_SPLITK),
        "pipelined": single(NT, SHAPES[2]),
        "pipelined_k_slices": single(NT, SHAPES[4]),
        "grouped_nt_small": grouped_rows(ROWS_SMALL, 68, 96),
        "grouped_nt_pipelined": grouped_rows(ROWS_PIPE, 68, 96),
        "grouped_tn_workspace": grouped_tn(True),
        "grouped_tn_no_workspace": grouped_tn(False),
        "lp_feat_gemm_fwd": lp_fwd,
        "lp_feat_gemm_wgrad": lp_wgrad,
        "lp_feat_gemm_bwd_fold": lp_fold,
    }


LAUNCHER_NAMES = ["gemm_kernel", "gemm_kernel_splitk", "pipelined", "pipelined_k_slices", "grouped_nt_small", "grouped_nt_pipelined",
                  "grouped_tn_workspace", "grouped_tn_no_workspace", "lp_feat_gemm_fwd", "lp_feat_gemm_wgrad", "lp_feat_gemm_bwd_fold"]


@pytest.fixture(scope="module")
def launchers():
    return _launchers()


def _arm(flag, value):
    assert L.lib().gmp_gate_open_by_next_gemm(C.c_void_p(flag.data_ptr()), value) == R.OK
    assert L.lib().gmp_gate_open_pending() == 1


@pytest.mark.parametrize("name", LAUNCHER_NAMES)
def test_every_launcher_carries_the_gate_signal_once(launchers, name):
    """arm -> the call takes the signal (nothing pending right after it) -> after a synchronise the flag holds the value and the result is still
    bit for bit the reference; a second call of the same launcher leaves the (re-zeroed) flag alone.  No gate is waited on: flags are only read
    after a synchronise."""
    lib, call = L.lib(), launchers[name]
    flag = torch.zeros(4, dtype=torch.int32, device=DEV)
    value = 101 + LAUNCHER_NAMES.index(name)
    torch.cuda.synchronize()
    _arm(flag, value)
    check = call()
    assert lib.gmp_gate_open_pending() == 0
    torch.cuda.synchronize()
    assert flag.tolist() == [value, 0, 0, 0]
    assert check()
    flag.zero_()
    check = call()
    torch.cuda.synchronize()
    assert flag.tolist() == [0, 0, 0, 0] and lib.gmp_gate_open_pending() == 0
    assert check()


def test_a_call_that_launches_nothing_leaves_the_signal_pending(launchers):
    lib = L.lib()
    flag = torch.zeros(4, dtype=torch.int32, device=DEV)
    buf = torch.zeros(64, device=DEV)
    torch.cuda.synchronize()
    _arm(flag, 9)
    assert R.gemm(NT, buf, buf, None, buf, 0, 4, 4, 4, 4, 4) == R.OK                                     # M == 0
    assert lib.gmp_gate_open_pending() == 1
    assert R.gemm_grouped(NT, buf, buf, None, buf, [0, 0, 0], None, None, None, None, None, 0, 4, 4, 4, 4, 4) == R.OK      # every group empty
    assert lib.gmp_gate_open_pending() == 1
    assert R.gemm_grouped(TN, buf, buf, None, buf, [0, 3], None, None, None, None, None, 0, 4, 0, 4, 4, 4) == R.OK         # M_tn == 0
    assert lib.gmp_gate_open_pending() == 1
    assert lib.gmp_gate_open_by_next_gemm(None, 0) == R.OK                                                # cancel
    assert lib.gmp_gate_open_pending() == 0
    check = launchers["gemm_kernel"]()                                                                   # the cancelled signal rides on nothing
    torch.cuda.synchronize()
    assert flag.tolist() == [0, 0, 0, 0] and check()


# ---- f. gmp_colsum -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 63, 64, 130])
@pytest.mark.parametrize("M", [1, 255, 256, 257, 1030])
def test_colsum_strided_rows_and_accumulate(M, N):
    """lda = N + 3 with large values in the columns between N and lda (they must not leak in), stored and accumulated onto an integer vector;
    both sides of the 256-row partial block and of the 64-column block"""
    g = torch.Generator().manual_seed(M * 131 + N)
    A, c0 = _ints(g, M, N), _ints(g, N)
    Ad = R.operand(A, "packed", DEV, ld_extra=3)
    assert Ad.stride(0) == N + 3 or M == 1
    out = R.Out.single(1, N, "packed", DEV)
    ws = _workspace(max(L.lib().gmp_colsum_workspace_bytes(M, N), 16))
    for acc in (0, 1):
        out.reset()
        if acc:
            out.fill(c0.to(DEV)[None])
        assert R.colsum(Ad, out.ptr, M, N, N + 3, acc, ws) == R.OK, R.last_error()
        assert _same(out.win()[0], R.ref_colsum(A, c0, acc)), f"accumulate {acc}"
        assert out.stray() == 0
