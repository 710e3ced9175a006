"""Segment sums, row movers, pooling, the link-prediction edge features and the head dropout, kernel by kernel through the C ABI,
against plain float64 torch on the CPU (the kernel's float32 inputs cast to double).  The loss kernels: test_gpu_kernel_edges_losses.py.

Every element of every output is compared.  Tolerances are derived, not measured:
  * pure movers (row_gather without seg_ptr, max-pool forward, fwd_rows against the whole, dropout mask positions, zero rows,
    "not written" sentinels): bit for bit;
  * sums: per output element |got - want| <= (n_terms + 2) * 2^-24 * sum |terms| -- the running-sum bound of fp32, valid for any
    order of summation.  n_terms counts every addend of that element (self term, a mean's scale, an addend, a pre-filled output);
    `rowdot`, whose terms are themselves rounded products, gets n_terms + 4.  The sum of |terms| comes from the reference run on
    absolute values.
Gradient references are autograd through the float64 forward (the per-row <g, x> of the eps gradient: eps as one leaf per row).
The references themselves are pinned on the CPU against the oracle's / torch's own fp32 functions (test_reference_*).

What each test closes (csrc file: gap):
  aggregate.hip   rows_per_wave > 1, F != 256 at N >= 65536, rows of > 64 neighbours in every instantiation, gmp_gin_aggregate_bwd_ex x 4
                                               test_aggregate_chunked_rows_and_hub_rows
                  gmp_gin_aggregate_fwd_rows   test_aggregate_fwd_rows_equals_the_whole_bitwise
                  gmp_group_sum_1d             test_group_sum_1d
                  gmp_segment_sum              test_segment_sum (scalar widths, idx, mean, accumulate, empty segments, > 8192 segments)
  pool_gather.hip gmp_segment_max_fwd/bwd      test_segment_max_sizes_signs_and_empty_segments, test_segment_max_beyond_the_grid_clamp
                  gmp_row_gather               test_row_gather (scalar widths, bad indices, seg_ptr with empty source segments)
                  gmp_lp_edge_features_*       test_lp_edge_features_bad_endpoints_read_as_zero_rows
  elementwise.hip gmp_dropout_fwd, gmp_relu_dropout_bwd   test_dropout_*
"""
import functools

import pytest
import torch

from gnn_pretraining_amd import ops
from oracle import graph_ops as OG

DEV = "cuda:0"
gpu = pytest.mark.gpu
U = 2.0 ** -24                       # unit roundoff of float32
SENTINEL = -7.0


def assert_within_sum_bound(got, want, terms_abs, n_terms, what, extra=2):
    """|got - want| <= (n_terms + extra) * 2^-24 * sum|terms| for every element; prints the worst ratio before it asserts."""
    got = got.detach().cpu().double()
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} vs {tuple(want.shape)}"
    if got.numel() == 0:
        return
    bound = (torch.as_tensor(n_terms, dtype=torch.float64) + extra) * U * terms_abs
    err = (got - want).abs()
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite output"
    ratio = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err > 0, torch.inf, 0.0).double())
    worst = ratio.max().item()
    print(f"[sum bound] {what}: worst err/bound {worst:.3f}, max abs err {err.max().item():.3e}")
    assert worst <= 1.0, f"{what}: {int((ratio > 1).sum())} elements beyond the bound, worst err/bound {worst:.3f} at {int(ratio.argmax())}"


def assert_bitwise(got, want, what):
    got, want = got.detach(), want.detach()
    if got.device != want.device:
        got, want = got.cpu(), want.cpu()
    assert got.shape == want.shape and got.dtype == want.dtype, f"{what}: {got.shape} {got.dtype} vs {want.shape} {want.dtype}"
    same = (got.view(torch.int32) == want.view(torch.int32)) if got.dtype == torch.float32 else (got == want)
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ"


# ------------------------------------------------------------------------------------------------ float64 references (CPU)
def ref_aggregate(x, ei, eps):
    """GIN aggregation: out[i] = (1 + eps) x[i] + sum over edges j -> i of x[j].  eps: a scalar or one value per row ([N, 1])."""
    adj = torch.sparse_coo_tensor(torch.stack([ei[1], ei[0]]), torch.ones(ei.size(1), dtype=torch.float64), (x.size(0), x.size(0)))
    return torch.sparse.mm(adj, x) + (1.0 + eps) * x


def ref_segment_sum(src, ptr, idx, mean):
    """out[s] = sum of src[idx[k]] (or src[k]) over k in [ptr[s], ptr[s+1]), divided by max(count, 1) under `mean`."""
    cnt = (ptr[1:] - ptr[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(cnt.numel()), cnt)
    rows = torch.arange(int(ptr[0]), int(ptr[-1])) if idx is None else idx[int(ptr[0]):int(ptr[-1])].long()
    out = torch.zeros(cnt.numel(), src.size(1), dtype=torch.float64).index_add_(0, seg, src[rows])
    return out / cnt.clamp(min=1).double().unsqueeze(1) if mean else out


def ref_max_pool(x, ptr):
    """PyG's global_max_pool on the CPU: zeros.scatter_reduce('amax', include_self=False); an empty segment stays 0.  Autograd through
    it splits the gradient evenly between tied maxima and counts the zero-initialised output as one more tie when the maximum is 0."""
    cnt = (ptr[1:] - ptr[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(cnt.numel()), cnt)
    rows = x[int(ptr[0]):int(ptr[-1])]
    return x.new_zeros(cnt.numel(), x.size(1)).scatter_reduce(0, seg.view(-1, 1).expand_as(rows), rows, reduce="amax", include_self=False)


def ref_lp_features(h, edges):
    """[hs + hd | hs * hd | |hs - hd|] with an endpoint outside [0, N) read as a zero row; returns (feat, hs, hd) with hs / hd leaves."""
    n = h.size(0)
    hz = torch.cat([h, torch.zeros(1, h.size(1), dtype=h.dtype)])
    pick = lambda e: hz[torch.where((e >= 0) & (e < n), e, torch.full_like(e, n))].clone().requires_grad_()
    hs, hd = pick(edges[0]), pick(edges[1])
    return torch.cat([hs + hd, hs * hd, (hs - hd).abs()], dim=1), hs, hd


def ptr_of(sizes):
    p = torch.zeros(len(sizes) + 1, dtype=torch.int32)
    p[1:] = torch.tensor(sizes, dtype=torch.int32).cumsum(0)
    return p


# ------------------------------------------------------------------------------------------------ the references against fp32 torch (CPU)
def test_reference_aggregate_matches_the_oracle():
    gen = torch.Generator().manual_seed(1)
    n, F = 500, 12
    x, ei, eps = torch.randn(n, F, generator=gen), torch.randint(0, n, (2, 3000), generator=gen), torch.tensor([0.37])
    g = torch.randn(n, F, generator=gen)
    xr, er = x.clone().requires_grad_(), eps.clone().requires_grad_()
    want = OG.gin_aggregate(xr, ei, er)
    want.backward(g)
    x64, e64 = x.double().requires_grad_(), torch.full((n, 1), 0.37, dtype=torch.float64).fill_(float(eps)).requires_grad_()
    got = ref_aggregate(x64, ei, e64)
    got.backward(g.double())
    assert (got.detach() - want.detach().double()).abs().max() <= 1e-5 * want.abs().max()
    assert (x64.grad - xr.grad.double()).abs().max() <= 1e-5 * xr.grad.abs().max()
    assert abs(e64.grad.sum().item() - er.grad.item()) <= 1e-5 * (g * x).abs().sum().item()


def test_reference_segment_sum_matches_the_oracle_mean_pool():
    gen = torch.Generator().manual_seed(2)
    sizes = [0, 3, 1, 0, 40, 7, 0]
    ptr = ptr_of(sizes)
    n = int(ptr[-1])
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    x = torch.randn(n, 7, generator=gen)
    want = OG.global_mean_pool(x, batch, size=len(sizes))
    assert (ref_segment_sum(x.double(), ptr, None, True) - want.double()).abs().max() <= 1e-6 * want.abs().max()
    perm = torch.randperm(n, generator=gen)
    inv = torch.empty(n, dtype=torch.long)
    inv[perm] = torch.arange(n)
    assert (ref_segment_sum(x[perm].double(), ptr, inv.int(), True) - want.double()).abs().max() <= 1e-6 * want.abs().max()
    s = torch.zeros(len(sizes), 7).index_add_(0, batch, x)
    assert (ref_segment_sum(x.double(), ptr, None, False) - s.double()).abs().max() <= 1e-6 * s.abs().max()


def test_reference_max_pool_matches_the_oracle_and_its_tie_rule():
    gen = torch.Generator().manual_seed(3)
    sizes = [5, 1, 17, 4]
    ptr = ptr_of(sizes)
    batch = torch.repeat_interleave(torch.arange(len(sizes)), torch.tensor(sizes))
    x = torch.relu(torch.randn(int(ptr[-1]), 8, generator=gen))
    x[:, 0] = 0.0                                              # a column where every row ties at 0
    x[5:6] = -x[5:6].abs() - 1.0                               # a one-row, all-negative segment
    g = torch.randn(len(sizes), 8, generator=gen)
    xr = x.clone().requires_grad_()
    want = OG.global_max_pool(xr, batch)
    want.backward(g)
    x64 = x.double().requires_grad_()
    got = ref_max_pool(x64, ptr)
    got.backward(g.double())
    assert torch.equal(got.detach().float(), want.detach())
    assert (x64.grad - xr.grad.double()).abs().max() <= 1e-6 * xr.grad.abs().max()
    # the two documented rules, stated outright: maximum 0 -> g / (n + 1) (the zero-initialised output ties); maximum < 0 -> g / n
    assert torch.allclose(x64.grad[:5, 0], (g[0, 0] / 6).double().expand(5)) and torch.equal(x64.grad[5], g[1].double())


# ------------------------------------------------------------------------------------------------ aggregation: chunked rows, hub rows
HUB_DEGREES = (65, 128, 129, 1000)


@functools.lru_cache(maxsize=2)
def hub_graph(n):
    """A random graph of ~3 edges per row, both directions of a handful of hub rows of degree 65, 128, 129 and 1000 (first row, last row,
    two in between: hubs of the forward AND of the transposed CSR), and isolated rows (second row, last-but-one, a few random)."""
    gen = torch.Generator().manual_seed(n)
    ei = torch.randint(0, n, (2, 3 * n), generator=gen)
    hubs = [0, n // 3, (2 * n) // 3 + 1, n - 1]
    isolated = torch.tensor([1, n - 2] + torch.randint(2, n - 2, (6,), generator=gen).tolist())
    isolated = isolated[~torch.isin(isolated, torch.tensor(hubs))]
    special = torch.cat([torch.tensor(hubs), isolated])
    ei = ei[:, ~(torch.isin(ei[0], special) | torch.isin(ei[1], special))]          # the random part touches neither hubs nor isolated rows
    plain = torch.arange(n)[~torch.isin(torch.arange(n), special)]
    extra = []
    for h, deg in zip(hubs, HUB_DEGREES):
        leaves = plain[torch.randint(0, plain.numel(), (deg,), generator=gen)]
        extra += [torch.stack([leaves, torch.full_like(leaves, h)]), torch.stack([torch.full_like(leaves, h), leaves])]
    ei = torch.cat([ei] + extra, dim=1)
    ei = ei[:, torch.randperm(ei.size(1), generator=gen)].contiguous()
    indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
    assert all(int(indeg[h]) == d == int(outdeg[h]) for h, d in zip(hubs, HUB_DEGREES)) and int(indeg[1]) == 0 == int(outdeg[n - 2])
    return ei, indeg.double(), outdeg.double(), hubs


AGG_CASES = [(8192, 256), (8193, 256), (8200, 256), (20011, 256), (65535, 256), (70001, 128), (70001, 512),
             (9001, 4), (9001, 64), (9001, 260), (9001, 1024)]


@gpu
@pytest.mark.parametrize("n,F", AGG_CASES)
def test_aggregate_chunked_rows_and_hub_rows(n, F):
    """seg_sum_kernel where a wave walks a chunk of rows (N > 8192: rows_per_wave 2 ... 9, partial last chunk, waves without rows), at every
    float4-per-lane count, on rows of 0 ... 1000+ neighbours: forward, backward with / without the eps gradient, and the four forms of
    gmp_gin_aggregate_bwd_ex, rowdot row by row."""
    ei, indeg, outdeg, _ = hub_graph(n)
    gen = torch.Generator().manual_seed(n + F)
    x, g, add = (torch.randn(n, F, generator=gen) for _ in range(3))
    eps = 0.37
    epsf = torch.tensor([eps])
    e64 = float(epsf.double())
    # float64: forward, then autograd with eps as one leaf per row (its gradient is rowdot, summed: g_eps)
    x64, g64, a64 = x.double().requires_grad_(), g.double(), add.double()
    epsv = torch.full((n, 1), e64, dtype=torch.float64).requires_grad_()
    out64 = ref_aggregate(x64, ei, epsv)
    gx64, rowdot64 = torch.autograd.grad((out64 * g64).sum(), [x64, epsv], retain_graph=True)
    gxa64, = torch.autograd.grad((out64 * g64).sum() + (x64 * a64).sum(), [x64])
    rowdot64 = rowdot64.view(-1)
    fwd_abs = ref_aggregate(x.double().abs(), ei, e64)
    bwd_abs = ref_aggregate(g64.abs(), ei.flip(0), e64)
    dot_abs = (g64 * x.double()).abs().sum(1)
    nf, nb = (indeg + 1).unsqueeze(1), (outdeg + 1).unsqueeze(1)

    csr = ops.csr_build(ei.to(DEV), n)
    xd, gd, ad, ed = x.to(DEV), g.to(DEV), add.to(DEV), epsf.to(DEV)
    assert_within_sum_bound(ops.gin_aggregate_fwd(xd, csr.rowptr, csr.col, ed), out64.detach(), fwd_abs, nf, "gin_aggregate_fwd")
    gx, ge = ops.gin_aggregate_bwd(gd, csr.rowptr_t, csr.col_t, ed, None)
    assert ge is None
    assert_within_sum_bound(gx, gx64, bwd_abs, nb, "gin_aggregate_bwd g_x (no eps gradient)")
    gx, ge = ops.gin_aggregate_bwd(gd, csr.rowptr_t, csr.col_t, ed, xd)
    assert_within_sum_bound(gx, gx64, bwd_abs, nb, "gin_aggregate_bwd g_x")
    assert_within_sum_bound(ge, rowdot64.sum().view(1), dot_abs.sum().view(1), n * F, "gin_aggregate_bwd g_eps", extra=4)
    for with_x in (False, True):
        for with_add in (False, True):
            gx, rd = ops.gin_aggregate_bwd_ex(gd, csr.rowptr_t, csr.col_t, ed, xd if with_x else None, ad if with_add else None)
            what = f"gin_aggregate_bwd_ex(rowdot={with_x}, addend={with_add})"
            if with_add:
                assert_within_sum_bound(gx, gxa64, bwd_abs + a64.abs(), nb + 1, what + " g_x")
            else:
                assert_within_sum_bound(gx, gx64, bwd_abs, nb, what + " g_x")
            assert (rd is not None) == with_x
            if with_x:
                assert_within_sum_bound(rd, rowdot64, dot_abs, F, what + " rowdot", extra=4)


@gpu
@pytest.mark.parametrize("F", [64, 256, 1024])
def test_aggregate_fwd_rows_equals_the_whole_bitwise(F):
    """gmp_gin_aggregate_fwd_rows offsets rowptr, self and out by row0 while col keeps the global numbering: two halves written into one
    buffer are gin_aggregate_fwd of the whole, bit for bit (a row's sum keeps its order), rows outside a range keep the sentinel."""
    n = 20011
    ei, _, _, hubs = hub_graph(n)
    gen = torch.Generator().manual_seed(F)
    x = torch.randn(n, F, generator=gen).to(DEV)
    eps = torch.tensor([0.37], device=DEV)
    csr = ops.csr_build(ei.to(DEV), n)
    whole = ops.gin_aggregate_fwd(x, csr.rowptr, csr.col, eps)
    hub = hubs[1]
    nbrs = csr.col[int(csr.rowptr[hub]):int(csr.rowptr[hub + 1])].sort().values
    inside = int(nbrs[nbrs.numel() // 2])                      # a split between the rows the hub row reads
    assert int(nbrs[0]) < inside <= int(nbrs[-1])
    for r in (0, 1, hub, hub + 1, inside, 8192, n - 1, n):     # r = 0 / n: an empty range; r = 1 / n - 1: a one-row range
        out = torch.full_like(x, SENTINEL)
        ops.gin_aggregate_fwd_rows(x, csr.rowptr, csr.col, eps, out, 0, r)
        assert_bitwise(out[:r], whole[:r], f"rows [0, {r})")
        assert_bitwise(out[r:], torch.full_like(out[r:], SENTINEL), f"rows [{r}, n) untouched")
        ops.gin_aggregate_fwd_rows(x, csr.rowptr, csr.col, eps, out, r, n)
        assert_bitwise(out, whole, f"halves split at {r}")
    for r0, r1 in ((hub, hub + 1), (5, 5), (max(inside - 9000, 0), inside + 3)):
        out = torch.full_like(x, SENTINEL)
        ops.gin_aggregate_fwd_rows(x, csr.rowptr, csr.col, eps, out, r0, r1)
        want = torch.full_like(x, SENTINEL)
        want[r0:r1] = whole[r0:r1]
        assert_bitwise(out, want, f"rows [{r0}, {r1}) alone")


@gpu
def test_group_sum_1d():
    """empty groups, one group of many thousand rows, values before the first / behind the last group, scattered output slots"""
    gen = torch.Generator().manual_seed(4)
    rows = [3, 3, 10, 10, 10, 300, 301, 20301, 20301, 20560, 20560]      # 10 groups: empty ones first, in the middle (twice), last
    v = torch.randn(20600, generator=gen)
    sizes = [b - a for a, b in zip(rows[:-1], rows[1:])]
    want = torch.stack([v[a:b].double().sum() for a, b in zip(rows[:-1], rows[1:])])
    tabs = torch.stack([v[a:b].double().abs().sum() for a, b in zip(rows[:-1], rows[1:])])
    got = ops.group_sum_1d(v.to(DEV), rows)
    assert_within_sum_bound(got, want, tabs, torch.tensor(sizes), "group_sum_1d")
    empty = torch.tensor(sizes) == 0
    assert int(empty.sum()) == 5
    assert_bitwise(got.cpu()[empty], torch.zeros(5), "empty groups")
    off = [17, 2, 9, 0, 5, 11, 4, 21, 13, 8]
    out = torch.full((23,), SENTINEL, device=DEV)
    assert ops.group_sum_1d(v.to(DEV), rows, out=out, out_off=off) is out
    full = torch.full((23,), SENTINEL, dtype=torch.float64)
    full[off] = want
    fabs = torch.zeros(23, dtype=torch.float64)
    fabs[off] = tabs
    nt = torch.zeros(23)
    nt[off] = torch.tensor(sizes, dtype=torch.float32)
    assert_within_sum_bound(out, full, fabs, nt, "group_sum_1d scattered (unnamed slots keep the sentinel)")
    one = ops.group_sum_1d(v.to(DEV), [0, 20600])
    assert_within_sum_bound(one, v.double().sum().view(1), v.double().abs().sum().view(1), 20600, "group_sum_1d, one group")


# ------------------------------------------------------------------------------------------------ segment_sum / row_gather
SEG_SIZES = [0, 0, 1, 4, 63, 64, 65, 0, 200, 3, 0, 0, 17, 130, 0]         # empty segments at the start, in the middle, at the end
WIDTHS = [1, 7, 12, 30, 4, 256, 1024]                                    # 1 ... 30: the one-thread-per-element kernels


@gpu
@pytest.mark.parametrize("F", WIDTHS)
@pytest.mark.parametrize("with_idx", [False, True])
@pytest.mark.parametrize("layout", ["few", "many"])
def test_segment_sum(F, with_idx, layout):
    """gmp_segment_sum: sum / mean, fresh output / accumulate into a pre-filled one, with and without idx, at every kernel form; `many`:
    9,001 segments of 0 ... 5 rows, so a wave of the vector kernel walks two segments."""
    gen = torch.Generator().manual_seed(F * 4 + with_idx)
    sizes = SEG_SIZES if layout == "few" else [0, 0] + torch.randint(0, 6, (8997,), generator=gen).tolist() + [0, 0]
    ptr = ptr_of(sizes)
    slots = int(ptr[-1])
    nsrc = slots + 11 if with_idx else slots
    src = torch.randn(nsrc, F, generator=gen)
    idx = torch.randint(0, nsrc, (slots,), generator=gen).int() if with_idx else None
    pre = torch.randn(len(sizes), F, generator=gen)
    cnt = torch.tensor(sizes, dtype=torch.float64).unsqueeze(1)
    srcd, ptrd, idxd = src.to(DEV), ptr.to(DEV), None if idx is None else idx.to(DEV)
    for mean in (False, True):
        want = ref_segment_sum(src.double(), ptr, idx, mean)
        tabs = ref_segment_sum(src.double().abs(), ptr, idx, mean)
        got = ops.segment_sum(srcd, ptrd, idxd, mean=mean)
        assert_within_sum_bound(got, want, tabs, cnt + mean, f"segment_sum(mean={mean})")
        assert_bitwise(got.cpu()[cnt.view(-1) == 0], torch.zeros(int((cnt == 0).sum()), F), "empty segments are 0")
        out = pre.to(DEV)
        assert ops.segment_sum(srcd, ptrd, idxd, mean=mean, out=out, accumulate=True) is out
        assert_within_sum_bound(out, want + pre.double(), tabs + pre.double().abs(), cnt + mean + 1, f"segment_sum(mean={mean}, accumulate)")
        out = torch.full((len(sizes), F), SENTINEL, device=DEV)
        ops.segment_sum(srcd, ptrd, idxd, mean=mean, out=out, accumulate=False)
        assert_bitwise(out, got, "accumulate=0 overwrites a pre-filled output")


@gpu
@pytest.mark.parametrize("F", WIDTHS)
def test_row_gather(F):
    """gmp_row_gather: a pure mover without seg_ptr (bit for bit), indices outside [0, nsrc) -- negative, nsrc, far beyond int32 -- give
    exact zero rows; with seg_ptr every row is divided by max(count, 1) of its source segment (empty source segments: undivided).  M is
    past one sweep of the grid for the narrow widths (32,768 rows of the wave-per-row kernel, 1,048,576 elements of the scalar one)."""
    gen = torch.Generator().manual_seed(F)
    sizes = SEG_SIZES
    ptr = ptr_of(sizes)
    nsrc = len(sizes)
    M = 40000 if F <= 30 else 3000
    src = torch.randn(nsrc, F, generator=gen)
    idx = torch.randint(0, nsrc, (M,), generator=gen)
    bad = torch.tensor([-1, -5, nsrc, nsrc + 3, 2 ** 40, -2 ** 40, 2 ** 31, -2 ** 31 - 1])
    where = torch.randperm(M, generator=gen)[:bad.numel() * 3]
    idx[where] = bad.repeat(3)
    idx[0], idx[M - 1] = -1, nsrc
    ok = (idx >= 0) & (idx < nsrc)
    safe = torch.where(ok, idx, torch.zeros_like(idx))
    want = torch.where(ok.unsqueeze(1), src[safe], torch.zeros(1, F))
    got = ops.row_gather(src.to(DEV), idx.to(DEV)).cpu()
    assert_bitwise(got, want, "row_gather")
    assert_bitwise(got[~ok], torch.zeros(int((~ok).sum()), F), "zero rows for bad indices")
    cnt = torch.tensor(sizes, dtype=torch.float64).clamp(min=1)
    want64 = want.double() / cnt[safe].unsqueeze(1)
    got = ops.row_gather(src.to(DEV), idx.to(DEV), ptr.to(DEV)).cpu()
    assert_within_sum_bound(got, want64, want64.abs(), 2, "row_gather with seg_ptr")          # one term and its scale
    assert_bitwise(got[~ok], torch.zeros(int((~ok).sum()), F), "zero rows for bad indices (seg_ptr)")
    one = cnt[safe] == 1                                                                      # segments of 0 or 1 rows: undivided
    assert_bitwise(got[one], want[one], "rows of source segments with count <= 1")


@gpu
@pytest.mark.parametrize("F", [7, 256])
def test_mean_pool_backward_is_row_gather_with_seg_ptr(F):
    """the use the seg_ptr form exists for: the gradient of global_mean_pool, from autograd through the float64 mean pool"""
    gen = torch.Generator().manual_seed(F + 1)
    ptr = ptr_of(SEG_SIZES)
    n = int(ptr[-1])
    batch = torch.repeat_interleave(torch.arange(len(SEG_SIZES)), torch.tensor(SEG_SIZES))
    x, g = torch.randn(n, F, generator=gen), torch.randn(len(SEG_SIZES), F, generator=gen)
    x64 = x.double().requires_grad_()
    ref_segment_sum(x64, ptr, None, True).backward(g.double())
    got = ops.row_gather(g.to(DEV), batch.to(DEV), ptr.to(DEV))
    assert_within_sum_bound(got, x64.grad, x64.grad.abs(), 2, "mean pool backward")


# ------------------------------------------------------------------------------------------------ max pooling
MAX_SIZES = [0, 1, 4, 15, 16, 17, 200, 0, 33, 5, 16, 0]       # 16 rows = one pass of the 4 x 4-wave unroll; 15 / 17 / 33: its tails


def max_pool_input(gen, sizes, F, extra_rows=0):
    """Values on a grid of 1/4 (ties everywhere); segment k is all-negative when k % 3 == 0, post-ReLU (tied zeros, whole zero columns)
    when k % 3 == 1, mixed signs otherwise."""
    ptr = ptr_of(sizes)
    n = int(ptr[-1])
    x = (torch.randn(n + extra_rows, F, generator=gen) * 4).round() / 4 + 0.0     # + 0.0: no -0.0 (which zero a max of +-0 returns is undefined)
    for k, (a, b) in enumerate(zip(ptr[:-1].tolist(), ptr[1:].tolist())):
        if k % 3 == 0:
            x[a:b] = -x[a:b].abs() - 0.25
        elif k % 3 == 1:
            x[a:b] = torch.relu(x[a:b])
            x[a:b, :3] = 0.0
    return x, ptr


@gpu
@pytest.mark.parametrize("F", [4, 256, 260, 512])
def test_segment_max_sizes_signs_and_empty_segments(F):
    """gmp_segment_max_fwd bit for bit and gmp_segment_max_bwd against autograd through the float64 pool: segments of exactly 1, 4, 15, 16, 17,
    33 and 200 rows, empty ones (output 0, nothing written), all-negative ones (the zero-initialised output is NOT a tie there), tied
    maxima; accumulate; rows behind the last segment keep their sentinel."""
    gen = torch.Generator().manual_seed(F)
    x, ptr = max_pool_input(gen, MAX_SIZES, F, extra_rows=3)
    n, B = int(ptr[-1]), len(MAX_SIZES)
    g = torch.randn(B, F, generator=gen)
    x64 = x.double().requires_grad_()
    want = ref_max_pool(x64, ptr)
    want.backward(g.double())
    gx64 = x64.grad
    assert bool((want.detach()[[3, 6]] < 0).all()) and bool((gx64[n:] == 0).all())
    xd, ptrd, gd = x.to(DEV), ptr.to(DEV), g.to(DEV)
    out = ops.segment_max_fwd(xd, ptrd)
    assert_bitwise(out, want.detach().float(), "segment_max_fwd")
    assert_bitwise(out.cpu()[torch.tensor(MAX_SIZES) == 0], torch.zeros(3, F), "empty segments are 0")
    buf = torch.full_like(xd, SENTINEL)
    assert ops.segment_max_bwd(gd, xd, out, ptrd, g_x=buf) is buf
    assert_within_sum_bound(buf[:n], gx64[:n], gx64[:n].abs(), 1, "segment_max_bwd")          # one division
    assert_bitwise(buf[n:], torch.full((3, F), SENTINEL), "rows of no segment are not written")
    assert_bitwise(ops.segment_max_bwd(gd, xd, out, ptrd)[:n], buf[:n], "segment_max_bwd into a fresh buffer")
    pre = torch.randn(n + 3, F, generator=gen)
    buf = pre.to(DEV)
    ops.segment_max_bwd(gd, xd, out, ptrd, g_x=buf, accumulate=True)
    assert_within_sum_bound(buf[:n], gx64[:n] + pre[:n].double(), gx64[:n].abs() + pre[:n].double().abs(), 2, "segment_max_bwd accumulate")
    assert_bitwise(buf[n:], pre[n:], "accumulate: rows of no segment are not written")


@gpu
def test_segment_max_beyond_the_grid_clamp():
    """B = 70,000 segments (the launch stops at 65,536 workgroups, which then stride) of 0 ... 2 rows"""
    gen = torch.Generator().manual_seed(70000)
    sizes = torch.randint(0, 3, (70000,), generator=gen).tolist()
    x, ptr = max_pool_input(gen, sizes, 4)
    g = torch.randn(len(sizes), 4, generator=gen)
    x64 = x.double().requires_grad_()
    want = ref_max_pool(x64, ptr)
    want.backward(g.double())
    out = ops.segment_max_fwd(x.to(DEV), ptr.to(DEV))
    assert_bitwise(out, want.detach().float(), "segment_max_fwd, 70,000 segments")
    gx = ops.segment_max_bwd(g.to(DEV), x.to(DEV), out, ptr.to(DEV), g_x=torch.full_like(x, SENTINEL, device=DEV))
    assert_within_sum_bound(gx, x64.grad, x64.grad.abs(), 1, "segment_max_bwd, 70,000 segments")


# ------------------------------------------------------------------------------------------------ link-prediction edge features
@gpu
@pytest.mark.parametrize("F", [4, 256, 260])
def test_lp_edge_features_bad_endpoints_read_as_zero_rows(F):
    """An endpoint outside [0, N) reads as a zero row (include/gnnmp.h), each endpoint on its own, as in the fused scorer: a pair with one
    bad endpoint is [h | 0 | |h|] of the good one.  Forward and per-pair gradients against autograd through the float64 features."""
    gen = torch.Generator().manual_seed(F)
    n, K = 300, 33000                                          # K past one sweep of the grid (32,768 pairs)
    h = torch.relu(torch.randn(n, F, generator=gen))
    edges = torch.randint(0, n, (2, K), generator=gen)
    bad = torch.tensor([-1, n, n + 7, 2 ** 40, -2 ** 40, 2 ** 31])
    edges[0, 10:16], edges[1, 20:26] = bad, bad                # one bad endpoint
    edges[:, 30:36] = torch.stack([bad, bad.flip(0)])          # both bad
    edges[:, 40:43] = 5                                        # self pairs: |hs - hd| at its kink
    g = torch.randn(K, 3 * F, generator=gen)
    feat64, hs, hd = ref_lp_features(h.double(), edges)
    feat64.backward(g.double())
    fabs = torch.cat([hs.abs() + hd.abs(), (hs * hd).abs(), hs.abs() + hd.abs()], dim=1).detach()
    feat = ops.lp_edge_features_fwd(h.to(DEV), edges.to(DEV))
    assert_within_sum_bound(feat, feat64.detach(), fabs, 2, "lp_edge_features_fwd")
    assert_bitwise(feat[30:36], torch.zeros(6, 3 * F), "both endpoints bad: a zero row")
    assert_bitwise(feat[10:16], torch.cat([h[edges[1, 10:16]], torch.zeros(6, F), h[edges[1, 10:16]]], 1), "source bad: [hd | 0 | hd]")
    assert_bitwise(feat[20:26], torch.cat([h[edges[0, 20:26]], torch.zeros(6, F), h[edges[0, 20:26]]], 1), "target bad: [hs | 0 | hs]")
    ghs, ghd = ops.lp_edge_features_bwd(g.to(DEV), h.to(DEV), edges.to(DEV))
    gs, gp, ga = g.double().split(F, dim=1)
    for got, want, other in ((ghs, hs.grad, hd), (ghd, hd.grad, hs)):
        assert_within_sum_bound(got, want, gs.abs() + (gp * other.detach()).abs() + ga.abs(), 3, "lp_edge_features_bwd", extra=4)
    assert_bitwise(ghs[30:36], g[30:36, :F], "both endpoints bad: g_hs is the gradient of the sum alone")
    assert_bitwise(ghd[30:36], g[30:36, :F], "both endpoints bad: g_hd is the gradient of the sum alone")


# ------------------------------------------------------------------------------------------------ dropout
DROP_SEED, DROP_SITE = 20240607, 103


@gpu
def test_dropout_mask_fraction_scale_and_prefix():
    """gmp_dropout_fwd: kept values are x * (1 / (1 - p)), one fp32 multiplication; the mask is keyed by element index, so a shorter
    tensor draws a prefix of a longer one's; over n = 2^20 elements at p = 0.2 the dropped fraction of a fair mask is within
    6 sigma = 6 sqrt(p (1 - p) / n) = 0.0024 of p; p = 0 is the identity."""
    gen = torch.Generator().manual_seed(6)
    n, p = 2 ** 20, 0.2
    x = torch.randn(n, generator=gen)
    x[x == 0] = 1.0
    ones = ops.dropout_fwd(torch.ones(n, device=DEV), p, DROP_SEED, DROP_SITE).cpu()
    inv = torch.tensor(1.0) / (torch.tensor(1.0) - torch.tensor(p, dtype=torch.float32))
    keep = ones != 0
    assert_bitwise(ones, torch.where(keep, inv, torch.tensor(0.0)), "dropout(ones) is 0 or 1 / (1 - p)")
    frac = 1.0 - keep.double().mean().item()
    print(f"[dropout] dropped fraction {frac:.5f} of {n}")
    assert abs(frac - p) <= 6 * (p * (1 - p) / n) ** 0.5, f"dropped fraction {frac}"
    y = ops.dropout_fwd(x.to(DEV), p, DROP_SEED, DROP_SITE)
    assert_bitwise(y, x * ones, "kept values are x * (1 / (1 - p)), dropped ones x * 0")
    for m in (4, 1028, 2 ** 20 - 4096):
        assert_bitwise(ops.dropout_fwd(torch.ones(m, device=DEV), p, DROP_SEED, DROP_SITE), ones[:m], f"the mask of {m} elements is a prefix")
    other = ops.dropout_fwd(torch.ones(n, device=DEV), p, DROP_SEED, DROP_SITE + 1).cpu()
    assert 0.25 < ((other != 0) != keep).double().mean().item() < 0.39          # another site: an independent mask (2 p (1 - p) = 0.32)
    assert_bitwise(ops.dropout_fwd(x.to(DEV), 0.0, DROP_SEED, DROP_SITE), x, "p = 0")


@gpu
@pytest.mark.parametrize("n", [2 ** 20, 2 ** 20 - 4096, 8])
@pytest.mark.parametrize("p", [0.2, 0.0])
def test_relu_dropout_bwd_applies_the_forward_mask_and_an_exact_gate(n, p):
    """gmp_relu_dropout_bwd: out = g * mask * (act > 0) with the mask of gmp_dropout_fwd element for element (same seed and site; two sizes
    sharing a prefix) and the gate exact at act == 0, -0.0 and the smallest normal numbers."""
    gen = torch.Generator().manual_seed(n)
    g = torch.randn(n, generator=gen)
    g[g == 0] = 1.0
    act = torch.relu(torch.randn(n, generator=gen))            # about half exact zeros
    act[:8] = torch.tensor([0.0, -0.0, 1.1754944e-38, -1.1754944e-38, 1e-30, -1e-30, 3.0, -3.0])
    mask = ops.dropout_fwd(torch.ones(n, device=DEV), p, DROP_SEED, DROP_SITE).cpu()
    got = ops.relu_dropout_bwd(g.to(DEV), act.to(DEV), p, DROP_SEED, DROP_SITE)
    assert_bitwise(got, torch.where(act > 0, g * mask, torch.tensor(0.0)), "relu_dropout_bwd")
    assert bool((got.cpu()[act > 0] != 0).eq(mask[act > 0] != 0).all()), "the backward's mask is the forward's"
