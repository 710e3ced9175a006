"""tests/gemm_ref.py held to its own promises on the CPU: the masked-product grouped references equal a plain loop of per-group
torch.matmul in float64, the layout builder returns the strides and pointer residues its names say, and the sentinel check sees one
planted stray write wherever it lands."""
import pytest
import torch

import gemm_ref as R


def _ints(g, *shape):
    return torch.randint(-4, 5, shape, generator=g).float()


@pytest.mark.parametrize("mode", [R.NT, R.NN])
@pytest.mark.parametrize("rows", [[0, 1, 1, 70, 200, 333], [0, 40, 40, 41]])
def test_grouped_row_reference_is_a_loop_of_matmuls(mode, rows):
    g = torch.Generator().manual_seed(len(rows))
    N, K, ng = 7, 37, len(rows) - 1
    A = _ints(g, rows[-1] + 3, K)
    W = [_ints(g, N, K) if mode == R.NT else _ints(g, K, N) for _ in range(ng)]
    b = [_ints(g, N) for _ in range(ng)]
    c0 = _ints(g, rows[-1], N)
    got = R.ref_grouped_rows(mode, A, W, rows, b, c0, alpha=0.5, accumulate=True, relu=True)
    assert got.dtype == torch.float64 and tuple(got.shape) == (rows[-1], N)
    for i in range(ng):
        a, e = rows[i], rows[i + 1]
        w = W[i].double().t() if mode == R.NT else W[i].double()
        want = (0.5 * torch.matmul(A[a:e].double(), w) + b[i].double() + c0[a:e].double()).clamp_min(0)
        assert torch.equal(got[a:e], want), f"group {i}"
    plain, last = R.ref_grouped_rows(mode, A, W, rows), ng - 1          # no epilogue: the bare product
    w = W[last].double().t() if mode == R.NT else W[last].double()
    assert torch.equal(plain[rows[last]:], torch.matmul(A[rows[last]:rows[-1]].double(), w))


@pytest.mark.parametrize("rows", [[0, 100, 100, 101, 230], [0, 5]])
def test_grouped_tn_reference_is_a_loop_of_matmuls(rows):
    g = torch.Generator().manual_seed(rows[-1])
    ng, M, N = len(rows) - 1, 6, 9
    A, B, c0 = _ints(g, rows[-1] + 2, M), _ints(g, rows[-1] + 2, N), _ints(g, ng, M, N)
    out, sums = R.ref_grouped_tn(A, B, rows, c0, alpha=0.5, accumulate=True)
    plain, _ = R.ref_grouped_tn(A, B, rows)
    for i in range(ng):
        a, e = rows[i], rows[i + 1]
        prod = torch.matmul(A[a:e].double().t(), B[a:e].double())
        assert torch.equal(plain[i], prod) and torch.equal(out[i], 0.5 * prod + c0[i].double())
        assert torch.equal(sums[i], A[a:e].double().sum(0))
        if a == e:
            assert torch.equal(out[i], c0[i].double()) and not plain[i].any()


def test_single_reference_modes_and_epilogue_order():
    g = torch.Generator().manual_seed(0)
    A, Bt, Bn, At, b, c0 = _ints(g, 5, 8), _ints(g, 3, 8), _ints(g, 8, 3), _ints(g, 8, 5), _ints(g, 3), _ints(g, 5, 3)
    assert torch.equal(R.ref_gemm(R.NT, A, Bt), A.double() @ Bt.double().t())
    assert torch.equal(R.ref_gemm(R.NN, A, Bn), A.double() @ Bn.double())
    assert torch.equal(R.ref_gemm(R.TN, At, Bn), At.double().t() @ Bn.double())
    want = (-2.0 * (A.double() @ Bn.double()) + b.double() + c0.double()).clamp_min(0)
    assert torch.equal(R.ref_gemm(R.NN, A, Bn, b, c0, alpha=-2.0, accumulate=True, relu=True), want)
    assert torch.equal(R.ref_colsum(A, b.new_ones(8), accumulate=True), A.double().sum(0) + 1)


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_layouts_have_the_strides_and_residues_their_names_promise(layout):
    vals = torch.arange(5 * 8, dtype=torch.float32).reshape(5, 8)
    v = R.operand(vals, layout)
    want_ld = {"packed": 8, "padded": 12, "odd": 9, "shifted": 12}[layout]
    want_res = 4 if layout == "shifted" else 0
    assert v.stride() == (want_ld, 1) and v.data_ptr() % 16 == want_res
    assert torch.equal(v, vals)
    b = R.vector(vals[0], layout)
    assert b.data_ptr() % 16 == want_res and torch.equal(b, vals[0])
    o = R.Out.single(5, 8, layout)
    assert o.ld == want_ld and o.ptr % 16 == want_res and o.ptr == o.win().data_ptr() and o.win().stride() == (want_ld, 1)
    assert o.stray() == 0
    if want_ld > 8:          # the gap of an input holds the poison, never data
        gap = v.as_strided((4, want_ld - 8), (want_ld, 1), v.storage_offset() + 8)
        assert (gap == R.POISON).all()


def test_flat_pack_is_aligned_and_places_pieces_at_their_offsets():
    a, b = torch.arange(6, dtype=torch.float32).reshape(2, 3), torch.arange(4, dtype=torch.float32) + 10
    f = R.flat_pack([a, b], [5, 16])
    assert f.data_ptr() % 16 == 0
    assert torch.equal(f[5:11], a.reshape(-1)) and torch.equal(f[16:20], b) and f[4] == R.POISON and f[11] == R.POISON


@pytest.mark.parametrize("layout", R.LAYOUTS)
def test_sentinel_check_catches_one_planted_stray_write(layout):
    o = R.Out.single(6, 5, layout, guard_rows=2)
    o.win().copy_(torch.ones(6, 5))              # writes inside the window are not strays
    assert o.stray() == 0
    first_inside, ld = o.base, o.ld
    spots = [first_inside - 1, first_inside + 6 * ld, 0, o.flat.numel() - 1]       # just before, the row after the last, both ends of the buffer
    if ld > 5:
        spots.append(first_inside + 5)                                              # the gap between two rows
        spots.append(first_inside + 5 * ld + 5)                                     # right behind the last element
    for s in spots:
        keep = o.flat[s].item()
        o.flat[s] = 3.0
        assert o.stray() == 1, f"stray write at {s - first_inside} from the window not seen"
        o.flat[s] = keep
        assert o.stray() == 0
    o.flat[first_inside - 1] = -R.SENTINEL       # a different bit pattern of the same magnitude counts
    assert o.stray() == 1


def test_sentinel_check_with_several_windows():
    o = R.Out([(0, 2, 3, 4), (9, 2, 3, 4)], span=20, guard=8)      # c_off = 9: an odd offset
    o.win(1).fill_(2.0)
    assert o.stray() == 0 and o.win(1).data_ptr() == o.ptr + 36
    o.flat[o.base + 8] = 0.0                     # between the two windows
    assert o.stray() == 1
