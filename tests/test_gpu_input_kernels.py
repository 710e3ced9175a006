"""The three kernel families that turn a batch into the first activations, kernel by kernel against the plain references of
tests/input_ref.py (pinned on the CPU in test_input_ref_host.py): the COO -> CSR build (csrc/csr_build.hip), the stacked input encoders
(csrc/encoder.hip) and the sparse linear (csrc/sparse_linear.hip).

Every element of every output is compared.  Tolerances are those of test_gpu_kernel_edges.py, derived and not measured:
  * index arrays, "not written" regions (sentinel-filled), rows that are nothing but the bias, exact zeros: bit for bit;
  * sums: |got - want| <= (n_terms + 2) * 2^-24 * sum |terms| per element, n_terms counting every addend of that element (the bias
    included), sum |terms| from the reference run on absolute values.  Every product here sits inside an fma, so no extra = 4 case.

What each test closes (csrc file: gap):
  csr_build.hip     rows of exactly 0 / 1 / 32 / 33 / 64 / 65 / 300 entries in both orientations, perm and the order of col, on the small
                    path with the slot array in LDS and in global memory (either side of 2N + 1 + E = 39872) and on the large path;
                    N + 1 = 9 * 2048 and one more; a second chunk of scan_sums_kernel (N = 600,000); the grid stride of hist / fill
                    (E > 4096 * 256); E = 0 on the large path                          test_csr_build_special_rows_on_every_path
                    bad endpoints on both paths                                        test_csr_build_bad_endpoints_on_both_paths
                    one orientation, short workspace, N < 0                            test_csr_build_c_abi_*
                    a segment of 160,008 B of LDS, 300 tiny ones, the refusal          test_csr_build_segmented_*
  encoder.hip       every instantiation (DP 8 / 24 / 40 / 64) at its widest and at a narrower dpad, masks, bad src_row, partial tiles,
                    tile lists                                                         test_encoder_fwd
                    groups of several segments, empty and rowless groups, 4 / 17 / 33 tiles against the 16-way row split, the three
                    workspace forms                                                    test_encoder_bwd
                    argument checks of both entry points                               test_encoder_argument_checks
  sparse_linear.hip vec<1> and the second c0 pass, ldw / ldo / bias forms, rows and columns of 0 ... 200 entries, unsorted and
                    repeated columns, partial transpose tiles, status counted once     test_sparse_linear_*
                    the CSC build on both paths of the one-orientation gmp_csr_build   test_sparse_csc_build
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import input_ref as R                                                            # noqa: E402
from gnn_pretraining_amd import _lib as L, ops                                   # noqa: E402
from gnn_pretraining_amd.graph import SparseFeatures                             # noqa: E402
from test_gpu_kernel_edges import assert_bitwise, assert_within_sum_bound        # noqa: E402

DEV = "cuda:0"
ERR_ARG, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -3, -4                             # include/gnnmp.h
MAX_GROUPS = 24                                                                  # GMP_MAX_GROUPS of csrc/gnnmp_internal.h
SENT = -7


def P(t):
    return C.c_void_p(0 if t is None else t.data_ptr())


def ST():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def i32s(xs):
    return (C.c_int32 * len(xs))(*[int(v) for v in xs])


def i64s(xs):
    return (C.c_int64 * len(xs))(*[int(v) for v in xs])


def isent(n):
    return torch.full((n,), SENT, dtype=torch.int32, device=DEV)


def fsent(*shape):
    return torch.full(shape, float(SENT), dtype=torch.float32, device=DEV)


def untouched(t, what):
    assert_bitwise(t, torch.full_like(t, SENT), f"{what}: written")


# ================================================================================================ COO -> CSR
SMALL_MAX_N, LDS_INTS = 16384, 39872                                             # csrc/csr_build.hip: path switch, LDS budget of the small path
NEAR_2048 = lambda n: dict(rows=[2047, 5000, 0, 2048, 9000, 13000, n - 1])       # noqa: E731   degrees 33, 0, 1, 32, 64, 300, 65
CSR_CASES = {
    "small-300": (300, 3000, {}),
    "small-last-with-lds-slots": (16384, 7103, dict(big=200)),
    "small-first-with-global-slots": (16384, 7104, dict(big=200)),
    "small-global-slots-60000": (16384, 60000, {}),
    "large-16385": (16385, 50000, {}),
    "large-18431": (18431, 50000, NEAR_2048(18431)),                             # N + 1 = 9 * 2048
    "large-18432": (18432, 50000, NEAR_2048(18432)),
    "large-600000": (600000, 50000, dict(rows=[0, 100000, 524287, 524288, 550000, 300000, 599999])),    # scan block 256 starts at row 524288
    "large-grid-stride": (20000, 1100000, {}),                                   # E > 4096 * 256
}
NAMES = ("rowptr", "col", "perm")


@functools.lru_cache(maxsize=None)
def graph(name):
    n, e, kw = CSR_CASES[name]
    ei, degs = R.special_graph(n, e, **kw)
    return n, ei, degs, {by: R.ref_csr(ei, n, by) for by in ("dst", "src")}


@pytest.mark.parametrize("name", list(CSR_CASES))
def test_csr_build_special_rows_on_every_path(name):
    n, ei, degs, want = graph(name)
    e = ei.size(1)
    assert (n <= SMALL_MAX_N) == name.startswith("small")
    if name == "small-last-with-lds-slots":
        assert 2 * n + 1 + e == LDS_INTS                                         # the last size whose slot array still fits in LDS
    if name == "small-first-with-global-slots":
        assert 2 * n + 1 + e == LDS_INTS + 1                                     # the first size that keeps it in global memory
    if name == "large-grid-stride":
        assert e > 4096 * 256
    csr = ops.csr_build(ei.to(DEV), n)
    torch.cuda.synchronize()
    assert int(csr.status) == 0
    for by, got in (("dst", (csr.rowptr, csr.col, csr.perm)), ("src", (csr.rowptr_t, csr.col_t, csr.perm_t))):
        rp = want[by][0]
        assert all(int(rp[h + 1] - rp[h]) == d for h, d in degs.items()), "the special rows lost their degrees"
        for a, b, nm in zip(got, want[by], NAMES):
            assert_bitwise(a, b, f"{name} by {by}: {nm}")


def test_csr_build_large_path_without_edges():
    n = 20000
    csr = ops.csr_build(torch.zeros(2, 0, dtype=torch.int64, device=DEV), n)
    torch.cuda.synchronize()
    assert int(csr.status) == 0
    assert_bitwise(csr.rowptr, torch.zeros(n + 1, dtype=torch.int32), "rowptr")
    assert_bitwise(csr.rowptr_t, torch.zeros(n + 1, dtype=torch.int32), "rowptr_t")


def csr_call(ei, n, both=True, short=0, spare=0):
    """gmp_csr_build into sentinel-filled arrays; returns (rc, [rowptr, col, perm, rowptr_t, col_t, perm_t], status).  The three
    transposed arrays are allocated (and must stay sentinel-filled) even when NULL is passed for them."""
    lib, e = L.lib(), ei.size(1)
    bufs = [isent(m + spare) for m in (n + 1, e, e, n + 1, e, e)]
    status = isent(1)
    need = lib.gmp_csr_build_workspace_bytes(n, e)
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    args = bufs if both else bufs[:3] + [None] * 3
    rc = lib.gmp_csr_build(P(ei), n, e, *[P(t) for t in args], P(status), P(ws), need - short, ST())
    torch.cuda.synchronize()
    return rc, bufs, status


@pytest.mark.parametrize("name", ["small-300", "large-16385"])
def test_csr_build_bad_endpoints_on_both_paths(name):
    n, ei, _, _ = graph(name)
    bad = R.with_bad_endpoints(ei, n)
    rc, bufs, status = csr_call(bad.to(DEV), n)
    assert rc == 0 and int(status) == 12                                         # four of the twelve have two bad endpoints: counted once
    for by, got in (("dst", bufs[:3]), ("src", bufs[3:])):
        rp, col, perm, dropped = R.ref_csr(bad, n, by)
        kept = col.numel()
        assert dropped == 12 and kept == ei.size(1) - 12 == int(rp[-1])
        assert_bitwise(got[0], rp, f"{name} by {by}: rowptr")
        assert_bitwise(got[1][:kept], col, f"{name} by {by}: col")
        assert_bitwise(got[2][:kept], perm, f"{name} by {by}: perm")
        untouched(got[1][kept:], f"{name} by {by}: col past rowptr[N]")
        untouched(got[2][kept:], f"{name} by {by}: perm past rowptr[N]")


@pytest.mark.parametrize("name", ["small-300", "large-16385"])
def test_csr_build_c_abi_one_orientation_short_workspace_and_bad_size(name):
    n, ei, _, want = graph(name)
    e = ei.size(1)
    rc, bufs, status = csr_call(ei.to(DEV), n, both=False, spare=64)
    assert rc == 0 and int(status) == 0
    for got, w, nm, m in zip(bufs[:3], want["dst"], NAMES, (n + 1, e, e)):
        assert_bitwise(got[:m], w, f"{name} one orientation: {nm}")
        untouched(got[m:], f"{name} one orientation: past the end of {nm}")
    for got, nm in zip(bufs[3:], NAMES):
        untouched(got, f"{name} one orientation: spare {nm}_t")
    rc, bufs, status = csr_call(ei.to(DEV), n, short=1)
    assert rc == ERR_WORKSPACE, (rc, L.lib().gmp_last_error_string())
    for got in bufs + [status]:
        untouched(got, f"{name} short workspace")
    dummy = isent(4)
    rc = L.lib().gmp_csr_build(P(ei.to(DEV)), -1, e, *[P(dummy)] * 6, P(dummy), P(dummy), 1 << 30, ST())
    assert rc == ERR_ARG, (rc, L.lib().gmp_last_error_string())
    torch.cuda.synchronize()
    untouched(dummy, "N = -1")


def seg_call(ei, n, seg_row, seg_edge, max_rows, max_edges):
    lib, e = L.lib(), ei.size(1)
    bufs = [isent(n + 1), isent(e), isent(e), isent(n + 1), isent(e), isent(e)]
    status = isent(1)
    sr, se = torch.tensor(seg_row, dtype=torch.int32, device=DEV), torch.tensor(seg_edge, dtype=torch.int32, device=DEV)
    rc = lib.gmp_csr_build_segmented(P(ei), n, e, P(sr), P(se), len(seg_row) - 1, max_rows, max_edges, *[P(t) for t in bufs], P(status), ST())
    torch.cuda.synchronize()
    return rc, bufs, status


def test_csr_build_segmented_large_segment_tiny_segments_and_refusal():
    ei, n, seg_row, seg_edge = R.segmented_batch()
    assert (2 * 8000 + 24000 + 2) * 4 == 160008 and n <= SMALL_MAX_N
    dev = ei.to(DEV)
    whole = ops.csr_build(dev, n)
    rc, bufs, status = seg_call(dev, n, seg_row, seg_edge, 8000, 24000)
    assert rc == 0 and int(status) == 0 and int(whole.status) == 0
    names = NAMES + tuple(nm + "_t" for nm in NAMES)
    refs = R.ref_csr(ei, n, "dst")[:3] + R.ref_csr(ei, n, "src")[:3]
    for got, w, ref, nm in zip(bufs, (whole.rowptr, whole.col, whole.perm, whole.rowptr_t, whole.col_t, whole.perm_t), refs, names):
        assert_bitwise(got, w, f"segmented vs whole-batch build: {nm}")
        assert_bitwise(got, ref, f"segmented vs reference: {nm}")
    rc, bufs, status = seg_call(dev, n, seg_row, seg_edge, 8192, 24576)          # 2 * 8192 + 24576 + 2 ints: more than one workgroup's LDS
    assert rc == ERR_UNSUPPORTED, (rc, L.lib().gmp_last_error_string())
    for got in bufs + [status]:
        untouched(got, "refused segmented build")
    s = next(s for s in range(3, len(seg_row) - 1) if seg_edge[s + 1] > seg_edge[s])
    leaving = ei.clone()
    leaving[0, seg_edge[s]] = 0                                                  # a valid row of the graph, in another segment
    rc, bufs, status = seg_call(leaving.to(DEV), n, seg_row, seg_edge, 8000, 24000)
    assert rc == 0 and int(status) == 1


# ================================================================================================ stacked encoders
DPADS = sorted(R.ENC_LAYOUTS)
MASKS = [None, "random", "all"]
DP_OF = lambda dpad: 8 if dpad <= 8 else 24 if dpad <= 24 else 40 if dpad <= 40 else 64          # noqa: E731


class EncDev:
    def __init__(self, c):
        self.c = c
        self.x, self.src, self.ptr, self.dom, self.params = (t.to(DEV) for t in (c.x_all, c.src_row, c.seg_ptr, c.seg_dom, c.params))
        self.mask = None if c.colmask is None else torch.from_numpy(c.colmask.view(np.int64)).to(DEV)
        self.S = c.seg_dom.numel()

    def fwd(self, tiles, z, num_tiles=None, dpad=None, domains=None, d_in=None):
        c = self.c
        t = tiles.to(DEV).contiguous()
        rc = L.lib().gmp_encoder_fwd(P(self.x), c.R, c.N, self.S, P(self.src), P(self.ptr), P(self.dom), P(self.mask), P(t),
                                     t.size(0) if num_tiles is None else num_tiles, P(self.params), len(c.d_in) if domains is None else domains,
                                     i64s(c.w_off + [0] * 8), i64s(c.b_off + [0] * 8), i32s((c.d_in if d_in is None else d_in) + [1] * 8),
                                     c.dpad if dpad is None else dpad, P(z), ST())
        torch.cuda.synchronize()
        return rc

    def bwd(self, gz, gseg, off_w, off_b, out, ws, ws_bytes, dpad=None, domains=None, d_in=None, groups=None):
        c = self.c
        rc = L.lib().gmp_encoder_bwd(P(self.x), c.R, c.N, self.S, P(self.src), P(self.ptr), P(self.dom), P(self.mask), P(gz),
                                     len(c.d_in) if domains is None else domains, i32s((c.d_in if d_in is None else d_in) + [1] * 8),
                                     c.dpad if dpad is None else dpad, len(gseg) - 1 if groups is None else groups, i32s(gseg),
                                     i64s(off_w), i64s(off_b), P(out), P(ws), ws_bytes, ST())
        torch.cuda.synchronize()
        return rc


@pytest.mark.parametrize("masks", MASKS, ids=["nomask", "random", "allmasked"])
@pytest.mark.parametrize("dpad", DPADS)
def test_encoder_fwd(dpad, masks):
    c = R.EncCase(dpad, R.FWD_SIZES, masks)
    d, N, S = EncDev(c), c.N, len(R.FWD_SIZES)
    tiles = c.tiles()
    assert tiles.size(0) == sum((n + 31) // 32 for n in R.FWD_SIZES)
    z, z2 = fsent(N, R.H), fsent(N, R.H)
    assert d.fwd(tiles, z) == 0 and d.fwd(tiles, z2) == 0
    what = f"encoder fwd dpad {dpad} masks {masks}"
    assert_within_sum_bound(z, c.ref_fwd(), c.ref_fwd(absolute=True), (c.din_row + 1).double().unsqueeze(1), what)
    assert_bitwise(z, z2, f"{what}: two runs")
    dom_row = c.seg_dom.long().repeat_interleave(c.seg_ptr[1:].long() - c.seg_ptr[:-1].long())
    bias = c.params[torch.tensor(c.b_off)[dom_row].unsqueeze(1) + torch.arange(R.H)]
    rows = torch.tensor(c.bad_rows + c.full_rows) if masks != "all" else torch.arange(N)
    assert_bitwise(z.cpu()[rows], bias[rows], f"{what}: rows that are nothing but the bias")
    # every second tile: the rows of the others keep the sentinel
    half = fsent(N, R.H)
    assert d.fwd(tiles[::2], half) == 0
    covered = torch.zeros(N, dtype=torch.bool)
    for s, r0 in tiles[::2].tolist():
        covered[r0:min(r0 + 32, int(c.seg_ptr[s + 1]))] = True
    assert 0 < int(covered.sum()) < N
    assert_bitwise(half.cpu()[covered], z.cpu()[covered], f"{what}: every second tile")
    untouched(half.cpu()[~covered], f"{what}: rows of the tiles left out")
    # tiles outside the batch and an empty tile list write nothing
    none = fsent(N, R.H)
    assert d.fwd(torch.tensor([[-1, 0], [S, 0], [0, -1], [0, N]], dtype=torch.int32), none) == 0
    assert d.fwd(tiles, none, num_tiles=0) == 0
    untouched(none, f"{what}: bad tiles / no tiles")


def bwd_slots(c, gseg):
    """Odd offsets of dW [256, d_in] and db [256] per group in one flat gradient buffer, with gaps; (off_w, off_b, d_in per group, size)."""
    off_w, off_b, din, cur = [], [], [], 5
    for g in range(len(gseg) - 1):
        k = c.d_in[int(c.seg_dom[min(gseg[g], c.seg_dom.numel() - 1)])]
        din.append(k)
        off_w.append(cur); cur += 256 * k + 2
        off_b.append(cur); cur += 256 + 4
    return off_w, off_b, din, cur + 3


@pytest.mark.parametrize("masks", MASKS, ids=["nomask", "random", "allmasked"])
@pytest.mark.parametrize("dpad", DPADS)
def test_encoder_bwd(dpad, masks):
    c = R.bwd_case(dpad, masks)
    d, gseg, G = EncDev(c), R.BWD_GSEG, len(R.BWD_GSEG) - 1
    gz = torch.randn(c.N, R.H, generator=torch.Generator().manual_seed(dpad))
    gz_dev = gz.to(DEV)
    off_w, off_b, din, total = bwd_slots(c, gseg)
    need = G * 16 * R.H * (DP_OF(dpad) + 1) * 4
    want, terms = c.ref_bwd(gz, gseg), c.ref_bwd(gz, gseg, absolute=True)
    assert want[1] is None and want[2][2] == 0 and [w[2] for w in want if w is not None] == [100, 0, 513, 1005, 33]
    outs = {}
    for form in ("workspace", "null", "short"):
        ws = torch.full((need,), 255, dtype=torch.uint8, device=DEV)            # NaN patterns: a partial read before it is written shows
        args = {"workspace": (ws, need), "null": (None, 0), "short": (ws, need - 1)}[form]
        out, out2 = fsent(total), fsent(total)
        assert d.bwd(gz_dev, gseg, off_w, off_b, out, *args) == 0 and d.bwd(gz_dev, gseg, off_w, off_b, out2, *args) == 0
        what = f"encoder bwd dpad {dpad} masks {masks} {form}"
        assert_bitwise(out, out2, f"{what}: two runs")
        if form == "short":
            assert bool((ws == 255).all()), f"{what}: a workspace one byte short was used"
        outs[form] = out = out.cpu()
        written = torch.zeros(total, dtype=torch.bool)
        for g in range(G):
            if want[g] is None:
                continue                                                       # the empty group: its slots keep the sentinel (checked below)
            dW, db = out[off_w[g]:off_w[g] + 256 * din[g]].view(256, din[g]), out[off_b[g]:off_b[g] + 256]
            written[off_w[g]:off_w[g] + 256 * din[g]] = True
            written[off_b[g]:off_b[g] + 256] = True
            rows = want[g][2]
            if rows == 0:
                assert_bitwise(dW, torch.zeros(256, din[g]), f"{what}: dW of the rowless group")
                assert_bitwise(db, torch.zeros(256), f"{what}: db of the rowless group")
                continue
            assert_within_sum_bound(dW, want[g][0], terms[g][0], rows, f"{what}: dW of group {g} ({rows} rows)")
            assert_within_sum_bound(db, want[g][1], terms[g][1], rows, f"{what}: db of group {g} ({rows} rows)")
        untouched(out[~written], f"{what}: outside the slots of the groups with segments")
        if masks == "random":                                                   # column 0 masked in every row of the last group
            assert bool((out[off_w[G - 1]:off_w[G - 1] + 256 * din[G - 1]].view(256, -1)[:, 0] == 0).all())
            assert bool((out[off_b[G - 1]:off_b[G - 1] + 256] != 0).all())
    assert_bitwise(outs["short"], outs["null"], "a workspace one byte short behaves as none")
    out = fsent(total)
    assert d.bwd(gz_dev, gseg, off_w, off_b, out, None, 0, groups=0) == 0
    untouched(out, "groups = 0")


def test_encoder_argument_checks():
    c = R.EncCase(8, R.FWD_SIZES, None)
    d, S = EncDev(c), len(R.FWD_SIZES)
    tiles, z = c.tiles(), fsent(c.N, R.H)
    bad_d_in = lambda v: [c.d_in[0], c.d_in[1], v] + c.d_in[3:]                  # noqa: E731
    for kw in (dict(dpad=0), dict(dpad=65), dict(domains=0), dict(domains=9), dict(d_in=bad_d_in(0)), dict(d_in=bad_d_in(9))):
        assert d.fwd(tiles, z, **kw) == ERR_ARG, (kw, L.lib().gmp_last_error_string())
    untouched(z, "refused encoder fwd")
    gseg = [0, 1, 2, 3]                                                          # one segment, hence one domain, per group
    off_w, off_b, _, total = bwd_slots(c, gseg)
    gz, out = torch.zeros(c.N, R.H, device=DEV), fsent(total)
    ws = torch.empty(MAX_GROUPS * 16 * R.H * 9 * 4, dtype=torch.uint8, device=DEV)
    call = lambda seg=gseg, **kw: d.bwd(gz, seg, off_w + [5] * 32, off_b + [5] * 32, out, ws, ws.numel(), **kw)          # noqa: E731
    for kw in (dict(dpad=0), dict(dpad=65), dict(domains=0), dict(domains=9), dict(d_in=bad_d_in(0)), dict(d_in=bad_d_in(9))):
        assert call(**kw) == ERR_ARG, (kw, L.lib().gmp_last_error_string())
    assert call(seg=[0] * (MAX_GROUPS + 2), groups=MAX_GROUPS + 1) == ERR_ARG
    for seg in ([-1, 1, 2, 3], [0, 1, 2, S + 1], [0, 2, 1, 3], [S + 1, S + 1, S + 1, S + 1], [1, 0, 2, 3], [0, 1, 3, 2]):
        assert call(seg=seg) == ERR_ARG, (seg, L.lib().gmp_last_error_string())
    untouched(out, "refused encoder bwd")
    assert call() == 0                                                            # the same call with good arguments goes through


# ================================================================================================ sparse linear
HS = [64, 128, 192, 256, 320, 512, 1024]
BAD_IDS, INT32_MAX = (3, 100, 400), 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def matrix():
    return R.sparse_matrix()


def sp_wide(rowptr, col, val, N, K, W, ldw, bias, H, ldo, status):
    """gmp_sparse_linear_fwd into a sentinel-filled [N, ldo] buffer (ops.sparse_linear_fwd only writes packed outputs)."""
    lib = L.lib()
    out = fsent(N, ldo)
    ws = torch.empty(max(lib.gmp_sparse_linear_workspace_bytes(K, H), 16), dtype=torch.uint8, device=DEV)
    rc = lib.gmp_sparse_linear_fwd(P(rowptr), P(col), P(val), N, K, P(W), ldw, P(bias), P(out), H, ldo, P(status), P(ws), ws.numel(), ST())
    assert rc == 0, lib.gmp_last_error_string()
    return out


def check_sparse_fwd(rowptr, col, val, N, K, H, ldws, what, seed):
    gen = torch.Generator().manual_seed(seed)
    sp = SparseFeatures(rowptr, col, val, (N, K)).to(DEV)
    empty = torch.nonzero(rowptr[1:] == rowptr[:-1]).flatten()
    assert empty.numel() > 0
    for ldw in ldws:
        slot, b = torch.randn(H, ldw, generator=gen), torch.randn(H, generator=gen)
        W = slot.to(DEV)[:, :K]
        for bias in (b, None):
            tag = f"{what} H {H} ldw {ldw} {'bias' if bias is not None else 'no bias'}"
            bd = None if bias is None else bias.to(DEV)
            status = torch.zeros(1, dtype=torch.int32, device=DEV)
            y = ops.sparse_linear_fwd(sp, W, bd, out=fsent(N, H), status=status)
            y2 = ops.sparse_linear_fwd(sp, W, bd, out=fsent(N, H), status=status)
            wide = sp_wide(sp.rowptr, sp.col, sp.val, N, K, W, ldw, bd, H, H + 4, status)
            torch.cuda.synchronize()
            want, nnz_row = R.ref_sparse_fwd(rowptr, col, val, K, slot, bias)
            terms, _ = R.ref_sparse_fwd(rowptr, col, val, K, slot, bias, absolute=True)
            assert_within_sum_bound(y, want, terms, (nnz_row + 1).double().unsqueeze(1), tag)
            assert_bitwise(y.cpu()[empty], (torch.zeros(H) if bias is None else bias).expand(empty.numel(), H).contiguous(), f"{tag}: empty rows")
            assert_bitwise(y, y2, f"{tag}: two runs")
            assert_bitwise(wide[:, :H].contiguous(), y, f"{tag}: ldo = H + 4")
            untouched(wide[:, H:].contiguous(), f"{tag}: columns [H, ldo)")
            assert int(status) == 0


@pytest.mark.parametrize("H", HS)
def test_sparse_linear_fwd_every_width_stride_and_row_length(H):
    rowptr, col, val = matrix()
    check_sparse_fwd(rowptr, col, val, R.SP_N, R.SP_K, H, (R.SP_K, R.SP_K + 1, R.SP_K + 8), "sparse fwd", H)


@pytest.mark.parametrize("K", [1, 7, 63, 64, 65])
def test_sparse_linear_fwd_narrow_inputs(K):
    rowptr, col, val = R.random_csr(20, K, min(K, 10) + 3, K)
    check_sparse_fwd(rowptr, col, val, 20, K, 64, (K, K + 3), f"sparse fwd K {K}", K)


@pytest.mark.parametrize("H", [64, 128, 512])                                    # one pass; two passes of vec<1>; two passes of vec<4>
def test_sparse_linear_fwd_counts_each_bad_column_once(H):
    rowptr, col, val = matrix()
    N, K = R.SP_N, R.SP_K
    bad = col.clone()
    bad[BAD_IDS[0]], bad[BAD_IDS[1]], bad[BAD_IDS[2]] = -1, K, INT32_MAX
    gen = torch.Generator().manual_seed(H)
    W, b = torch.randn(H, K, generator=gen), torch.randn(H, generator=gen)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    y = ops.sparse_linear_fwd(SparseFeatures(rowptr, bad, val, (N, K)).to(DEV), W.to(DEV), b.to(DEV), out=fsent(N, H), status=status)
    torch.cuda.synchronize()
    assert int(status) == 3
    want, nnz_row = R.ref_sparse_fwd(rowptr, bad, val, K, W, b)
    assert int(nnz_row.sum()) == col.numel() - 3
    assert_within_sum_bound(y, want, R.ref_sparse_fwd(rowptr, bad, val, K, W, b, absolute=True)[0], (nnz_row + 1).double().unsqueeze(1),
                            f"sparse fwd H {H} with three bad columns")


@pytest.mark.parametrize("H", HS)
def test_sparse_linear_wgrad_every_width_stride_and_column_length(H):
    rowptr, col, val = matrix()
    N, K = R.SP_N, R.SP_K
    colptr, row, val_t, _ = R.ref_csc(rowptr, col, val, K)
    G = torch.randn(N, H, generator=torch.Generator().manual_seed(H))
    want, nnz_col = R.ref_sparse_wgrad(rowptr, col, val, K, G)
    terms, _ = R.ref_sparse_wgrad(rowptr, col, val, K, G, absolute=True)
    csc, g = tuple(t.to(DEV) for t in (colptr, row, val_t)), G.to(DEV)
    for ldw in (K, K + 1, K + 3, K + 8):
        tag = f"sparse wgrad H {H} ldw {ldw}"
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        dW = ops.sparse_linear_wgrad(csc, N, g, out=fsent(H, ldw), status=status)
        dW2 = ops.sparse_linear_wgrad(csc, N, g, out=fsent(H, ldw), status=status)
        torch.cuda.synchronize()
        assert_within_sum_bound(dW[:, :K], want, terms, nnz_col.double().unsqueeze(0), tag)
        assert_bitwise(dW[:, R.SP_COLS[0]].contiguous(), torch.zeros(H), f"{tag}: the column without entries")
        assert_bitwise(dW[:, K:].contiguous(), torch.zeros(H, ldw - K), f"{tag}: columns [K, ldw)")
        assert_bitwise(dW, dW2, f"{tag}: two runs")
        assert int(status) == 0
    if H in (64, 128, 512):                                                       # CSC rows outside [0, N): skipped, each counted once
        bad = row.clone()
        bad[BAD_IDS[0]], bad[BAD_IDS[1]], bad[BAD_IDS[2]] = -1, N, INT32_MAX
        status = torch.zeros(1, dtype=torch.int32, device=DEV)
        dW = ops.sparse_linear_wgrad((csc[0], bad.to(DEV), csc[2]), N, g, out=fsent(H, K), status=status)
        torch.cuda.synchronize()
        assert int(status) == 3
        wt, n = R.ref_sparse_fwd(colptr, bad, val_t, N, G.T.contiguous(), None)              # the CSC is the CSR of X^T: dW^T = X^T G
        ta, _ = R.ref_sparse_fwd(colptr, bad, val_t, N, G.T.contiguous(), None, absolute=True)
        assert_within_sum_bound(dW, wt.T.contiguous(), ta.T.contiguous(), n.double().unsqueeze(0), f"sparse wgrad H {H} with three bad rows")


def test_sparse_csc_build():
    rowptr, col, val = matrix()
    gen = torch.Generator().manual_seed(9)
    wide_ptr = torch.tensor([0, 0, 10, 20, 35, 40], dtype=torch.int32)
    wide_col = torch.randint(0, 20000, (40,), generator=gen, dtype=torch.int32)
    wide_col[0], wide_col[39], wide_col[7] = 19999, 0, wide_col[30]              # the last column, the first, one column twice
    bad = col.clone()
    bad[BAD_IDS[0]], bad[BAD_IDS[1]], bad[BAD_IDS[2]] = -1, R.SP_K, INT32_MAX
    cases = [("matrix", rowptr, col, val, R.SP_N, R.SP_K, 0),
             ("large path", wide_ptr, wide_col, torch.randn(40, generator=gen), 5, 20000, 0),     # max(N, K) > 16384 rows in gmp_csr_build
             ("nnz = 0", torch.zeros(6, dtype=torch.int32), torch.zeros(0, dtype=torch.int32), torch.zeros(0), 5, 7, 0),
             ("bad columns", rowptr, bad, val, R.SP_N, R.SP_K, 3)]
    for name, rp, cl, vl, N, K, dropped in cases:
        colptr, row, val_t, status = ops.sparse_csc_build(SparseFeatures(rp, cl, vl, (N, K)).to(DEV))
        torch.cuda.synchronize()
        wp, wr, wv, wd = R.ref_csc(rp, cl, vl, K)
        kept = wr.numel()
        assert wd == dropped == int(status) and int(colptr[K]) == kept == cl.numel() - dropped, name
        assert_bitwise(colptr, wp, f"csc {name}: colptr")
        assert_bitwise(row[:kept], wr, f"csc {name}: row")
        assert_bitwise(val_t[:kept], wv, f"csc {name}: val_t")
