"""The references of tests/input_ref.py pinned on the CPU: ref_csr against oracle.graph_ops.coo_to_csr, the encoder and sparse-linear
references against fp32 torch (torch.nn.functional.linear and autograd through it, a dense matmul), and the properties the GPU tests
rely on in the shared inputs (exact degrees, exact sizes on either side of a kernel switch, exact row and column lengths)."""
import numpy as np
import torch
import torch.nn.functional as F

import input_ref as R
from oracle import graph_ops as OG


def close(got, want, tol=1e-5):
    want = want.double()
    assert got.shape == want.shape
    assert (got - want).abs().max().item() <= tol * max(want.abs().max().item(), 1e-30)


def test_ref_csr_equals_the_oracle_on_clean_input():
    for n, e, seed in ((1, 0, 0), (5, 40, 1), (300, 3000, 2), (2000, 500, 3)):
        ei = torch.randint(0, n, (2, e), generator=torch.Generator().manual_seed(seed))
        for by in ("dst", "src"):
            got, want = R.ref_csr(ei, n, by), OG.coo_to_csr(ei, n, by)
            assert got[3] == 0
            for a, b in zip(got[:3], want):
                assert a.dtype == b.dtype == torch.int32 and torch.equal(a, b)
    ei, degs = R.special_graph(300, 3000)
    for by in ("dst", "src"):
        rp, col, perm, dropped = R.ref_csr(ei, 300, by)
        want = OG.coo_to_csr(ei, 300, by)
        assert dropped == 0 and all(torch.equal(a, b) for a, b in zip((rp, col, perm), want))
        assert all(int(rp[h + 1] - rp[h]) == d for h, d in degs.items())


def test_ref_csr_drops_bad_endpoints_and_keeps_original_edge_ids():
    n = 300
    ei, _ = R.special_graph(n, 3000)
    bad = R.with_bad_endpoints(ei, n)
    is_bad = ((bad < 0) | (bad >= n)).any(0)
    assert int(is_bad.sum()) == 12 and int(((bad < 0) | (bad >= n)).all(0).sum()) == 4           # four edges with two bad endpoints
    assert {-1, n, 2 ** 31, 2 ** 40, -2 ** 40} == set(bad[(bad < 0) | (bad >= n)].tolist())
    keep = torch.nonzero(~is_bad).flatten()
    for by in ("dst", "src"):
        rp, col, perm, dropped = R.ref_csr(bad, n, by)
        wrp, wcol, wperm = OG.coo_to_csr(bad[:, keep], n, by)                 # the oracle on the survivors, edge ids mapped back
        assert dropped == 12 and int(rp[-1]) == 3000 - 12 == col.numel() == perm.numel()
        assert torch.equal(rp, wrp) and torch.equal(col, wcol) and torch.equal(perm.long(), keep[wperm.long()])


def test_special_graphs_have_the_sizes_the_kernel_switches_need():
    LDS_INTS = 39872                                                          # csr_build.hip: (160 KiB - 4 KiB - 256 B) / 4
    for e, side in ((7103, True), (7104, False)):
        ei, degs = R.special_graph(16384, e, big=200)
        assert ei.size(1) == e and (2 * 16384 + 1 + e <= LDS_INTS) == side and sorted(degs.values()) == [0, 1, 32, 33, 64, 65, 200]
    ei, degs = R.special_graph(18431, 50000, rows=[2047, 5000, 0, 2048, 9000, 13000, 18430])
    assert degs[2047] == 33 and degs[2048] == 32 and degs[18430] == 65 and degs[0] == 1
    ei, n, seg_row, seg_edge = R.segmented_batch()
    assert len(seg_row) == len(seg_edge) == 305 and seg_row[-1] == n and seg_edge[-1] == ei.size(1)
    assert max(b - a for a, b in zip(seg_row[:-1], seg_row[1:])) == 8000 and max(b - a for a, b in zip(seg_edge[:-1], seg_edge[1:])) == 24000
    seg_of_row = torch.repeat_interleave(torch.arange(304), torch.tensor(seg_row[1:]) - torch.tensor(seg_row[:-1]))
    seg_of_edge = torch.repeat_interleave(torch.arange(304), torch.tensor(seg_edge[1:]) - torch.tensor(seg_edge[:-1]))
    assert torch.equal(seg_of_row[ei[0]], seg_of_edge) and torch.equal(seg_of_row[ei[1]], seg_of_edge)      # block diagonal


def test_ref_encoder_matches_fp32_linear_and_autograd():
    for dpad in (8, 40, 64):
        c = R.EncCase(dpad, R.FWD_SIZES, "random")
        assert sorted(set(c.seg_dom.tolist())) == [0] + list(range(2, len(c.d_in))) and c.seg_dom.tolist() != sorted(c.seg_dom.tolist())
        assert all(o % 2 == 1 for o in c.w_off) and c.full_rows
        xm = R.encoder_rows(c.x_all, c.src_row, c.colmask, dpad)
        assert all(bool((xm[r] == 0).all()) for r in c.bad_rows)
        r = 2                                                                # r % 5 == 2: bit d_in - 1 alone
        k = int(c.din_row[r])
        assert xm[r, k - 1] == 0 and (k == 1 or bool((xm[r, :k - 1] == c.x_all[c.src_row[r], :k - 1].double()).all()))
        r = 3                                                                # only bits >= d_in: the row is untouched below d_in
        k = int(c.din_row[r])
        assert bool((xm[r, :k] == c.x_all[c.src_row[r], :k].double()).all())
        z = c.ref_fwd()
        gz = torch.randn(c.N, R.H, generator=torch.Generator().manual_seed(dpad))
        for s, d in enumerate(c.seg_dom.tolist()):
            r0, r1, k = int(c.seg_ptr[s]), int(c.seg_ptr[s + 1]), c.d_in[d]
            if r1 == r0:
                continue
            W = c.params[c.w_off[d]:c.w_off[d] + R.H * k].view(R.H, k).clone().requires_grad_()
            b = c.params[c.b_off[d]:c.b_off[d] + R.H].clone().requires_grad_()
            want = F.linear(xm[r0:r1, :k].float(), W, b)
            close(z[r0:r1], want.detach())
            want.backward(gz[r0:r1])
            dW, db, rows = c.ref_bwd(gz, [s, s + 1])[0]
            assert rows == r1 - r0
            close(dW, W.grad); close(db, b.grad)
        for r in c.bad_rows + c.full_rows:                                   # nothing but the bias
            d = int(c.seg_dom[int(torch.searchsorted(c.seg_ptr, torch.tensor(r, dtype=torch.int32), right=True)) - 1])
            assert torch.equal(z[r], c.params[c.b_off[d]:c.b_off[d] + R.H].double())
    c = R.bwd_case(40, "random")
    assert R.BWD_GSEG[1] == R.BWD_GSEG[2] and c.ref_bwd(torch.zeros(c.N, R.H), R.BWD_GSEG)[1] is None
    tiles = lambda g: sum((n + 31) // 32 for n in R.BWD_SIZES[R.BWD_GSEG[g]:R.BWD_GSEG[g + 1]])          # noqa: E731
    assert [tiles(g) for g in range(6)] == [4, 0, 0, 17, 33, 2]
    for g in range(6):
        assert len({int(c.seg_dom[s]) for s in range(R.BWD_GSEG[g], R.BWD_GSEG[g + 1])}) <= 1
    dW, db, rows = c.ref_bwd(torch.ones(c.N, R.H), R.BWD_GSEG)[5]
    assert rows == 33 and bool((dW[:, 0] == 0).all()) and bool((db == 33).all())          # a masked column adds nothing, the row counts


def test_ref_sparse_matches_a_dense_fp32_matmul():
    rowptr, col, val = R.sparse_matrix()
    N, K = R.SP_N, R.SP_K
    L = (rowptr[1:] - rowptr[:-1]).tolist()
    assert L[:10] == R.SP_ROW_LENGTHS and len(L) == N
    assert any(col[rowptr[r]:rowptr[r + 1]].tolist() != sorted(col[rowptr[r]:rowptr[r + 1]].tolist()) for r in range(N))
    gen = torch.Generator().manual_seed(4)
    rows = torch.repeat_interleave(torch.arange(N), torch.tensor(L))
    dense = torch.zeros(N, K).index_put_((rows, col.long()), val, accumulate=True)        # the repeated column of row 9 sums
    W, b, G = torch.randn(128, K + 3, generator=gen), torch.randn(128, generator=gen), torch.randn(N, 128, generator=gen)
    y, nnz_row = R.ref_sparse_fwd(rowptr, col, val, K, W, b)
    close(y, dense @ W[:, :K].T + b)
    assert nnz_row.tolist() == L
    close(R.ref_sparse_fwd(rowptr, col, val, K, W, None)[0], dense @ W[:, :K].T)
    dW, nnz_col = R.ref_sparse_wgrad(rowptr, col, val, K, G)
    close(dW, G.T @ dense)
    assert all(int(nnz_col[c]) == n for n, c in R.SP_COLS.items())
    ya, _ = R.ref_sparse_fwd(rowptr, col, val, K, W, b, absolute=True)
    assert bool((ya >= y.abs() - 1e-12).all())
    # entries with a column outside [0, K) are dropped
    bad = col.clone()
    ids = [3, 100, 400]
    bad[ids[0]], bad[ids[1]], bad[ids[2]] = -1, K, 2 ** 31 - 1
    d2 = dense.clone()
    for i in ids:
        d2[rows[i], col[i]] -= val[i]
    y2, n2 = R.ref_sparse_fwd(rowptr, bad, val, K, W, b)
    close(y2, d2 @ W[:, :K].T + b)
    assert int(n2.sum()) == col.numel() - 3
    close(R.ref_sparse_wgrad(rowptr, bad, val, K, G)[0], G.T @ d2)
    # the CSC form: the package's own host stable sort on clean input; kept count and order with bad columns
    from gnn_pretraining_amd.graph import SparseFeatures
    want = SparseFeatures(rowptr, col, val, (N, K)).csc()
    colptr, row, val_t, dropped = R.ref_csc(rowptr, col, val, K)
    assert dropped == 0 and torch.equal(colptr, want[0]) and torch.equal(row, want[1]) and torch.equal(val_t, want[2])
    colptr, row, val_t, dropped = R.ref_csc(rowptr, bad, val, K)
    assert dropped == 3 and int(colptr[-1]) == col.numel() - 3 == row.numel()
    for k in range(K):
        seg = row[int(colptr[k]):int(colptr[k + 1])]
        assert seg.tolist() == sorted(seg.tolist())
