"""The pooled-feature map on the GPU (csrc/graph_feat.hip: ops.graph_feature_map, finetune/graph_baselines.py, --feat-baseline) against the
CPU definition of tests/graph_feat_ref.py.  The definition fixes every rounding and every order, so the kernel's output is compared BIT
FOR BIT.  Columns never interact and fewer rounds are a prefix of more, so the reference is computed once per batch -- 256 columns, 16
rounds -- and every width and depth is a slice of it; test_graph_feat_host.py holds the reference to a second route."""
import ctypes as C
import functools
import json
import sys

import numpy as np
import pytest
import torch

import graph_feat_ref as R
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd._lib import GnnmpError
from gnn_pretraining_amd.finetune import graph_baselines as GB, node_baselines as NB
from gnn_pretraining_amd.graph import Batch, Data

pytestmark = pytest.mark.gpu
DEV = "cuda"
GMP_ERR_ARG = -1
CS = 16                                                             # the kernel's strip: widths 15, 16 and 17 stand on its two sides
WIDTHS = (1, 4, 5, CS - 1, CS, CS + 1, 21, 37, 256)
ROUNDS = (0, 1, 3, 16)
SIZES = {"small": R.SMALL_SIZES, "large": R.LARGE_SIZES}


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def _bits(t):
    """The fp32 words of a tensor or an array, so that -0 differs from +0."""
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    assert a.dtype == np.float32
    return np.ascontiguousarray(a).view(np.uint32)


@functools.lru_cache(maxsize=None)
def _batch(kind):
    return R.make_batch(SIZES[kind], {"small": 1, "large": 2}[kind])


@functools.lru_cache(maxsize=None)
def _x(kind):
    return R.features(int(_batch(kind).ptr[-1]), R.MAX_DIM, 7)


@functools.lru_cache(maxsize=None)
def _ref(kind):
    """All 256 columns and 16 rounds by the definition, once; callers slice and must not write."""
    b = _batch(kind)
    return R.feature_map(b.ptr, b.rowptr, b.col, _x(kind), R.MAX_ROUNDS, b.scale, b.scale)


@functools.lru_cache(maxsize=None)
def _dev(kind):
    b = _batch(kind)
    return (_t(b.ptr, torch.int64), _t(b.rowptr, torch.int32), _t(b.col, torch.int32), _t(b.scale, torch.float32), _t(_x(kind), torch.float32))


def _gpu(batch, x, rounds, scaled=True, max_graph_nodes=None):
    s = _t(batch.scale, torch.float32) if scaled else None
    return ops.graph_feature_map(_t(batch.ptr, torch.int64), _t(batch.rowptr, torch.int32), _t(batch.col, torch.int32), _t(x, torch.float32),
                                 rounds, left=s, right=s, max_graph_nodes=max_graph_nodes)


def _assert_same(got, want_out, want_status):
    assert got.out.dtype == torch.float32 and got.status.dtype == torch.int32 and got.out.is_contiguous()
    assert tuple(got.out.shape) == want_out.shape
    assert np.array_equal(got.status.cpu().numpy(), want_status)
    assert np.array_equal(_bits(got.out), _bits(want_out))


# ---------------------------------------------------------------------------- 1. bit for bit against the definition
@pytest.mark.parametrize("d", WIDTHS)
@pytest.mark.parametrize("kind", ["small", "large"])
def test_every_width_and_depth_equals_the_reference_bit_for_bit(kind, d):
    ptr, rowptr, col, scale, x = _dev(kind)
    want = _ref(kind)
    assert not want.status.any() and np.isfinite(want.out).all()
    xd = x[:, :d].contiguous()
    for rounds in ROUNDS:
        got = ops.graph_feature_map(ptr, rowptr, col, xd, rounds, left=scale, right=scale)
        _assert_same(got, np.ascontiguousarray(want.out[:, :rounds + 1, :, :d]), want.status)
    assert not got.out[0].any()                                                    # the empty graph: +0 everywhere
    assert np.array_equal(_bits(got.out[1, 0, 0]), _bits(xd[0])) and np.array_equal(_bits(got.out[1, 0, 2]), _bits(xd[0]))      # one node


# ---------------------------------------------------------------------------- 2. H(t) is gmp_feature_propagate's
def test_max_slice_is_the_amax_of_feature_propagate_at_every_level():
    ptr, rowptr, col, scale, x = _dev("large")
    xd = x[:, :21].contiguous()
    rounds = 3
    got = ops.graph_feature_map(ptr, rowptr, col, xd, rounds, left=scale, right=scale)
    sizes = R.LARGE_SIZES
    bounds = _batch("large").ptr.tolist()
    for t in range(rounds + 1):
        H = xd if t == 0 else ops.feature_propagate(rowptr, col, xd, t, left=scale, right=scale).out
        for g, n in enumerate(sizes):
            if n:
                assert torch.equal(got.out[g, t, 2], torch.amax(H[bounds[g]:bounds[g + 1]], dim=0)), (t, g)


def test_small_integers_pool_exactly():
    """Features in {-2 .. 2} and no scales: every H(t) is an integer below 2 * 20^2 = 800 in size and every sum of up to 1,024 of them
    stays below 2^24, so fp32 is exact and all three pools equal int64 arithmetic."""
    b = _batch("large")
    N, rounds = int(b.ptr[-1]), 2
    xi = np.random.default_rng(5).integers(-2, 3, size=(N, 5)).astype(np.int64)
    got = _gpu(b, xi.astype(np.float32), rounds, scaled=False).out.cpu().numpy()
    steps, skipped = R.window_steps(b.ptr, b.rowptr, b.col)
    assert not skipped.any()
    H = xi
    for t in range(rounds + 1):
        assert np.abs(H).max() < 2 ** 24 // 1024
        for g, n in enumerate(R.LARGE_SIZES):
            rows = H[b.ptr[g]:b.ptr[g + 1]]
            s = rows.sum(axis=0).astype(np.float32) if n else np.zeros(5, np.float32)
            want = np.stack([s, s / np.float32(max(n, 1)), rows.max(axis=0).astype(np.float32) if n else np.zeros(5, np.float32)])
            assert np.array_equal(_bits(got[g, t]), _bits(want)), (t, g)
        nxt = np.zeros_like(H)
        for rows_p, j in steps:
            nxt[rows_p] += H[j]
        H = nxt


# ---------------------------------------------------------------------------- 3. entries that leave their graph
def test_strays_are_skipped_counted_once_and_leave_the_neighbours_alone():
    b, g, other = _batch("small"), 5, 4                                            # the 64-node graph, towards the 63-node one and outside
    x = _x("small")[:, :21]                                                        # two strips: only the first one counts
    bad, count = R.with_strays(b, g, other)
    clean = _gpu(b, x, 3)
    for rounds in (3, 16, 0):
        want = R.feature_map(bad.ptr, bad.rowptr, bad.col, x, rounds, b.scale, b.scale)
        assert want.status[g] == (count << 8 if rounds else 0) and np.count_nonzero(want.status) == (1 if rounds else 0)
        got = _gpu(bad, x, rounds)
        _assert_same(got, want.out, want.status)
    got = _gpu(bad, x, 3)
    keep = [k for k in range(len(R.SMALL_SIZES)) if k != g]
    assert torch.equal(got.out[keep], clean.out[keep]) and not torch.equal(got.out[g, 1:], clean.out[g, 1:])
    assert torch.equal(got.out[g, 0], clean.out[g, 0])                             # the level that reads no entry


def _graph_batch(ptr, edge_index, x):
    ptr = np.asarray(ptr, np.int64)
    vec = np.repeat(np.arange(ptr.size - 1), np.diff(ptr))
    return Batch(torch.as_tensor(x), torch.as_tensor(np.asarray(edge_index, np.int64)), torch.from_numpy(vec), torch.from_numpy(ptr), ptr.tolist(),
                 [0] * ptr.size, torch.zeros(ptr.size - 1, dtype=torch.int64)).to(DEV)


def test_an_edge_between_two_graphs_is_refused_loudly_by_pooled_features():
    ptr = [0, 4, 9]
    ring = lambda lo, hi: [(v, v + 1 if v + 1 < hi else lo) for v in range(lo, hi)]          # noqa: E731
    edges = np.array(ring(0, 4) + ring(4, 9)).T
    x = np.random.default_rng(0).standard_normal((9, 3)).astype(np.float32)
    ok = GB.pooled_features(_graph_batch(ptr, edges, x), 2)
    assert tuple(ok.shape) == (2, 3 * 3 * 3)
    with pytest.raises(GnnmpError, match="1 adjacency entries of graph 0 point outside the graph and were skipped"):
        GB.pooled_features(_graph_batch(ptr, np.concatenate([edges, [[1], [6]]], axis=1), x), 2)


# ---------------------------------------------------------------------------- 4. the two instances
@pytest.mark.parametrize("bound", [256, 64])
def test_a_smaller_bound_selects_the_small_instance_and_refuses_the_rest(bound):
    ptr, rowptr, col, scale, x = _dev("large")
    sizes = np.array(R.LARGE_SIZES)
    full = _ref("large")
    refused = sizes > bound
    assert refused.any() and not refused.all()
    want = np.ascontiguousarray(full.out[:, :4, :, :37]).copy()
    want[refused] = 0.0
    got = ops.graph_feature_map(ptr, rowptr, col, x[:, :37].contiguous(), 3, left=scale, right=scale, max_graph_nodes=bound)
    _assert_same(got, want, refused.astype(np.int32))                              # bit 0 and +0 rows; the graphs that fit keep their bits
    b = _batch("large")
    ref = R.feature_map(b.ptr, b.rowptr, b.col, _x("large")[:, :37], 3, b.scale, b.scale, max_graph_nodes=bound)
    assert np.array_equal(_bits(ref.out), _bits(want)) and np.array_equal(ref.status, refused.astype(np.int32))


def test_a_graph_of_1025_nodes_is_refused_loudly():
    n = ops.GRAPH_FEAT_MAX_GRAPH_NODES + 1
    sizes = (6, n, 2)
    b = R.make_batch(sizes, 9)
    x = R.features(int(b.ptr[-1]), 4, 9)
    got, want = _gpu(b, x, 2), R.feature_map(b.ptr, b.rowptr, b.col, x, 2, b.scale, b.scale, max_graph_nodes=n)
    assert want.status.tolist() == [0, 1, 0] and not want.out[1].any() and want.out[0].any() and want.out[2].any()
    _assert_same(got, want.out, want.status)
    ring = np.stack([np.arange(n), (np.arange(n) + 1) % n]) + 6
    edges = np.concatenate([np.array([[0, 1, 2], [1, 2, 0]]), ring, np.array([[6 + n], [7 + n]])], axis=1)
    with pytest.raises(GnnmpError, match=r"graph 1 has 1025 nodes"):
        GB.pooled_features(_graph_batch(b.ptr, edges, x), 2)


# ---------------------------------------------------------------------------- 5. signed zeros and subnormals
def test_signed_zeros_and_subnormals_are_kept():
    ptr = np.array([0, 2, 5, 8], np.int64)
    rowptr = np.arange(9, dtype=np.int32)                                          # one self-loop per node
    col = np.arange(8, dtype=np.int32)
    tiny = np.float32(1e-40)
    x = np.array([[-0.0, 0.0], [0.0, -0.0], [-0.0, -0.0], [-0.0, -0.0], [-0.0, -0.0],
                  [tiny, 3 * tiny], [2 * tiny, -tiny], [-tiny / 4, 2e-38]], np.float32)
    half = np.full(8, 0.5, np.float32)
    b = R.Batch(ptr, rowptr, col, half)
    for rounds, scaled in ((0, False), (2, False), (2, True)):
        want = R.feature_map(ptr, rowptr, col, x, rounds, half if scaled else None, half if scaled else None)
        got = _gpu(b, x, rounds, scaled=scaled)
        _assert_same(got, want.out, want.status)
    out = _bits(_gpu(b, x, 0, scaled=False).out)
    assert out[0].tolist() == [[[0, 0], [0, 0], [0, 0]]]                           # max(-0, +0) = +0; +0 + -0 = +0
    assert out[1, 0, 0].tolist() == [0, 0] and out[1, 0, 1].tolist() == [0, 0]     # all -0: the accumulator starts at +0
    assert out[1, 0, 2].tolist() == [0x80000000, 0x80000000]                       # ... and the largest of them is -0
    sub = _gpu(b, x, 2, scaled=True).out[2].cpu().numpy()
    assert (np.abs(sub[:, :, 0]) < 1.17549435e-38).all() and (sub[:, 0, 0] != 0).all() and (sub[:, 1, 0] != 0).all()      # subnormal sums and means


# ---------------------------------------------------------------------------- 6. calling conventions
def test_strided_x_no_scales_zero_rounds_and_repeatability():
    ptr, rowptr, col, scale, x = _dev("small")
    b, want = _batch("small"), _ref("small")
    view = x[:, 3:3 + 21]                                                          # ldx = 256 > d, base not on 16 bytes
    assert view.stride(0) == 256 and not view.is_contiguous()
    got = ops.graph_feature_map(ptr, rowptr, col, view, 3, left=scale, right=scale)
    _assert_same(got, np.ascontiguousarray(want.out[:, :4, :, 3:24]), want.status)
    again = ops.graph_feature_map(ptr, rowptr, col, view, 3, left=scale, right=scale)
    assert torch.equal(got.out, again.out) and torch.equal(got.status, again.status)
    plain = R.feature_map(b.ptr, b.rowptr, b.col, _x("small")[:, :5], 3)
    _assert_same(ops.graph_feature_map(ptr, rowptr, col, x[:, :5].contiguous(), 3), plain.out, plain.status)
    zero = ops.graph_feature_map(ptr, rowptr, col, view, 0)                        # no round: the pools of x itself, no entry read
    _assert_same(zero, np.ascontiguousarray(want.out[:, :1, :, 3:24]), want.status)
    one_sided = R.feature_map(b.ptr, b.rowptr, b.col, _x("small")[:, :5], 2, left=b.scale)
    _assert_same(ops.graph_feature_map(ptr, rowptr, col, x[:, :5].contiguous(), 2, left=scale), one_sided.out, one_sided.status)


def test_two_streams_do_not_disturb_each_other():
    a, b = _dev("large"), _dev("small")
    xa, xb = a[4][:, :37].contiguous(), b[4][:, :17].contiguous()
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        o1 = ops.graph_feature_map(a[0], a[1], a[2], xa, 16, left=a[3], right=a[3])
    with torch.cuda.stream(s2):
        o2 = ops.graph_feature_map(b[0], b[1], b[2], xb, 3, left=b[3], right=b[3])
    torch.cuda.synchronize()
    w1, w2 = _ref("large"), _ref("small")
    _assert_same(o1, np.ascontiguousarray(w1.out[:, :, :, :37]), w1.status)
    _assert_same(o2, np.ascontiguousarray(w2.out[:, :4, :, :17]), w2.status)


# ---------------------------------------------------------------------------- 7. argument errors and empty inputs
def test_argument_errors_launch_nothing():
    ptr, rowptr, col, scale, x = _dev("small")
    xd = x[:, :21].contiguous()
    G, N, nnz, d, rounds = ptr.numel() - 1, rowptr.numel() - 1, col.numel(), 21, 3
    out = torch.full((G, rounds + 1, 3, d), 7.0, device=DEV)
    st = torch.full((G,), 7, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())                    # noqa: E731

    def call(ptr_=ptr, G_=G, rp_=rowptr, col_=col, N_=N, nnz_=nnz, x_=xd, ldx=d, d_=d, rounds_=rounds, mgn=1024, out_=out, st_=st):
        return L.lib().gmp_graph_feature_map(p(ptr_), G_, p(rp_), p(col_), N_, nnz_, p(scale), p(scale), p(x_), ldx, d_, rounds_, mgn, p(out_),
                                             p(st_), None)

    for rc in (call(d_=0), call(d_=257, ldx=257), call(rounds_=-1), call(rounds_=17), call(G_=-1), call(N_=-1), call(N_=2 ** 31), call(nnz_=-1),
               call(nnz_=2 ** 31), call(mgn=-1), call(ptr_=None), call(rp_=None), call(col_=None), call(x_=None), call(out_=None),
               call(st_=None), call(ldx=d - 1), call(out_=xd)):
        assert rc == GMP_ERR_ARG
    assert b"overlaps" in L.lib().gmp_last_error_string()
    assert call(G_=0) == 0                                                         # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((st == 7).all())
    assert call() == 0                                                             # and the same call, unbroken, writes every word
    torch.cuda.synchronize()
    want = _ref("small")
    assert np.array_equal(_bits(out), _bits(np.ascontiguousarray(want.out[:, :4, :, :21]))) and not st.any()
    out.fill_(7.0); st.fill_(7)
    assert call(mgn=64) == 0                                                       # a refused graph's words are written too: +0 and bit 0
    torch.cuda.synchronize()
    big = torch.from_numpy(np.array(R.SMALL_SIZES) > 64).to(DEV)
    assert not out[big].any() and bool((st[big] == 1).all()) and not st[~big].any()
    assert np.array_equal(_bits(out[~big]), _bits(np.ascontiguousarray(want.out[:, :4, :, :21])[~big.cpu().numpy()]))
    with pytest.raises(GnnmpError, match="rounds"):
        ops.graph_feature_map(ptr, rowptr, col, xd, 17)
    with pytest.raises(GnnmpError, match="d="):
        ops.graph_feature_map(ptr, rowptr, col, torch.zeros(N, 257, device=DEV), 1)
    with pytest.raises(GnnmpError, match="rowptr has"):
        ops.graph_feature_map(ptr, rowptr, col, xd[:-1], 1)
    with pytest.raises(GnnmpError, match="left has"):
        ops.graph_feature_map(ptr, rowptr, col, xd, 1, left=scale[:-1].contiguous())
    with pytest.raises(GnnmpError, match="no CPU fallback"):
        ops.graph_feature_map(ptr, rowptr, col, xd.cpu(), 1)
    none = ops.graph_feature_map(torch.zeros(1, dtype=torch.int64, device=DEV), rowptr, col, xd, 2)
    assert tuple(none.out.shape) == (0, 3, 3, 21) and tuple(none.status.shape) == (0,)
    hollow = ops.graph_feature_map(torch.zeros(3, dtype=torch.int64, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV),
                                   torch.zeros(0, dtype=torch.int32, device=DEV), torch.zeros(0, 4, device=DEV), 2)      # two empty graphs, no node
    assert tuple(hollow.out.shape) == (2, 3, 3, 4) and not hollow.out.any() and not hollow.status.any()


# ---------------------------------------------------------------------------- 8. the baseline on the separable fixture
def _fixture_datasets():
    from gnn_pretraining_amd.data.pretrain_data_loaders import GraphDataset
    from gnn_pretraining_amd.data.store import GraphStore
    data = [Data(torch.from_numpy(x), torch.from_numpy(np.ascontiguousarray(e.T)), torch.tensor([int(c)])) for _, e, x, c in R.fixture_graphs()]
    store = GraphStore.from_data_list(data)
    return GraphDataset(store, np.arange(R.N_TRAIN)), GraphDataset(store, np.arange(R.N_TRAIN, R.N_TRAIN + R.N_EVAL))


def test_feature_baseline_on_the_separable_fixture():
    """The four accuracies are the float64 reference's -- 0.5, 0.5 without the graph, 1.0, 1.0 with two rounds -- and every sgcpool logit
    lies within half of the reference's own smallest top-2 margin (10.35 / 2, see test_graph_feat_host.py) of the float64 logit."""
    train_ds, eval_ds = _fixture_datasets()
    raw, sgc = R.reference_baseline("rawpool"), R.reference_baseline("sgcpool")
    scores = GB.feature_baseline(train_ds, eval_ds, R.FIXTURE_CLASSES, R.FIXTURE_ROUNDS, k=R.FIXTURE_K, device=DEV)
    print("feature_baseline", scores)
    assert set(scores) == {"rawpool_knn_accuracy", "rawpool_logreg_accuracy", "sgcpool_knn_accuracy", "sgcpool_logreg_accuracy"}
    assert (scores["rawpool_knn_accuracy"], scores["rawpool_logreg_accuracy"]) == (raw.knn_accuracy, raw.logreg_accuracy) == (0.5, 0.5)
    assert (scores["sgcpool_knn_accuracy"], scores["sgcpool_logreg_accuracy"]) == (sgc.knn_accuracy, sgc.logreg_accuracy) == (1.0, 1.0)
    # by hand, from the same pieces
    graphs = R.fixture_graphs()
    tb, eb = train_ds.collate(torch.arange(R.N_TRAIN)).to(DEV), eval_ds.collate(torch.arange(R.N_EVAL)).to(DEV)
    pt, pe = GB.pooled_features(tb, R.FIXTURE_ROUNDS), GB.pooled_features(eb, R.FIXTURE_ROUNDS)
    assert np.array_equal(_bits(pt), _bits(R.pooled(graphs[:R.N_TRAIN], R.FIXTURE_ROUNDS)))
    assert np.array_equal(_bits(pe), _bits(R.pooled(graphs[R.N_TRAIN:], R.FIXTURE_ROUNDS)))
    zt, ze = GB.standardise(pt, pe)
    assert zt.is_cuda and np.abs(zt.cpu().numpy() - sgc.z_train).max() <= 1e-6 and np.abs(ze.cpu().numpy() - sgc.z_eval).max() <= 1e-6
    y_train = tb.y.to(torch.int64).contiguous()
    W, bias, _ = NB.softmax_fit(zt.contiguous(), y_train, R.FIXTURE_CLASSES)
    logits = ops.gemm(ops.NT, ze.contiguous(), W, bias=bias).cpu().numpy().astype(np.float64)
    gap = float(np.abs(logits - sgc.logits).max())
    print("largest |logit - float64 logit|", gap, "bound", sgc.margin / 2)
    assert gap <= sgc.margin / 2


# ---------------------------------------------------------------------------- 9. the command-line path
def _run_cli(root, monkeypatch, name, extra):
    from gnn_pretraining_amd import operators as O
    from gnn_pretraining_amd.finetune import finetune as FT
    monkeypatch.setattr(FT, "OUTPUT_DIR", root / name)
    monkeypatch.setattr(O.DROPOUT, "count", 0)                                    # the module path's dropout counter is process-wide
    log = root / f"{name}.jsonl"
    monkeypatch.setattr(sys, "argv", ["finetune", "--domain_name", "PTC_MR", "--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1",
                                      "--seed", "5", "--epochs", "1", "--data-root", str(root / "data"), "--data-scale", "0.1",
                                      "--log", str(log)] + extra)
    FT.main()
    rec = [json.loads(line) for line in log.read_text().splitlines()]
    state = torch.load(next((root / name).glob("model_*.pt")), map_location="cpu", weights_only=True)["model_state_dict"]
    return rec, state


@pytest.mark.parametrize("engine", [[], ["--gc-engine"]], ids=["module", "gc-engine"])
def test_cli_feat_baseline_logs_the_four_keys_and_leaves_training_alone(tmp_path, monkeypatch, engine):
    """python -m gnn_pretraining_amd.finetune.finetune ... --feat-baseline 2, in process: one epoch on the synthetic PTC_MR stand-in.  The
    test record carries exactly the four new keys, equal to feature_baseline called directly on the same splits; no other record carries
    them; every other key but the timing ones, and the checkpoint, are bit for bit those of the same run without the flag."""
    from gnn_pretraining_amd.constants import NUM_CLASSES
    from gnn_pretraining_amd.data.finetune_data_loaders import create_finetune_data_loader
    keys = ["test/rawpool_knn_accuracy", "test/rawpool_logreg_accuracy", "test/sgcpool_knn_accuracy", "test/sgcpool_logreg_accuracy"]
    rec1, state1 = _run_cli(tmp_path, monkeypatch, "with", engine + ["--feat-baseline", "2"])
    rec0, state0 = _run_cli(tmp_path, monkeypatch, "without", engine)
    test1 = [r for r in rec1 if keys[0] in r]
    test0 = [r for r in rec0 if "test/accuracy" in r][0]
    assert len(test1) == 1 and "test/accuracy" in test1[0]
    assert set(test1[0]) - set(test0) == set(keys) and set(test0) <= set(test1[0])
    assert not any("pool_" in k for r in rec1 if r is not test1[0] for k in r) and not any("pool_" in k for r in rec0 for k in r)
    sets = {sp: create_finetune_data_loader("PTC_MR", sp, 32, torch.Generator(), tmp_path / "data").dataset for sp in ("train", "test")}
    direct = GB.feature_baseline(sets["train"], sets["test"], NUM_CLASSES["PTC_MR"], 2, device=DEV)
    assert all(test1[0][f"test/{k}"] == v for k, v in direct.items()) and len(direct) == 4
    assert all(0.0 <= v <= 1.0 for v in direct.values())
    assert state1.keys() == state0.keys() and all(torch.equal(state1[k], state0[k]) for k in state1)
    for k, v in test0.items():
        assert "time" in k or test1[0][k] == v or (v != v and test1[0][k] != test1[0][k]), k
