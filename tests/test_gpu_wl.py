"""The Weisfeiler-Lehman subtree baseline on the GPU (csrc/wl.hip: ops.wl_refine / ops.wl_gram, finetune/graph_baselines.py, --wl-baseline)
against the CPU definition of tests/wl_ref.py.  Everything the kernels compute is integer arithmetic, so everything is compared for
EQUALITY.  test_wl_host.py shows that on these very graph sets the hashed definition is classical Weisfeiler-Lehman."""
import ctypes as C
import functools
import json
import sys

import numpy as np
import pytest
import torch

import wl_ref as R
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd._lib import GnnmpError
from gnn_pretraining_amd.finetune import graph_baselines as GB
from gnn_pretraining_amd.graph import Batch, Data

pytestmark = pytest.mark.gpu
DEV = "cuda"
GMP_ERR_ARG = -1
FILL = -7


def _t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def _u64(t):
    return t.cpu().numpy().view(np.uint64)


@functools.lru_cache(maxsize=None)
def _batch(kind="labels"):
    graphs = R.fixed_graphs()
    if kind == "wide":
        graphs = R.with_wide_labels(graphs)
    if kind == "permuted":
        graphs = R.permuted(graphs, 3)
    return R.make_batch(graphs)


@functools.lru_cache(maxsize=None)
def _ref(kind, iters, dim, use_labels=True, max_graph_nodes=R.MAX_GRAPH_NODES, fill=0):
    return R.refine(_batch(kind), iters, dim, use_labels, max_graph_nodes, fill)


def _gpu_refine(batch, iters, dim, use_labels=True, **kw):
    return ops.wl_refine(_t(batch.ptr, torch.int64), _t(batch.rowptr, torch.int32), _t(batch.col, torch.int32),
                         _t(batch.labels, torch.int64) if use_labels else None, iters, dim, return_colors=True, **kw)


def _assert_refined(got, want):
    assert got.sorted.dtype == torch.int64 and got.hist.dtype == torch.int32 and got.status.dtype == torch.int32
    assert np.array_equal(got.status.cpu().numpy(), want.status)
    assert np.array_equal(_u64(got.colors), want.colors)
    assert np.array_equal(_u64(got.sorted), want.sorted)
    assert np.array_equal(got.hist.cpu().numpy(), want.hist)


def _graph_batch(b, x=None, extra_edges=None):
    """wl_ref's batch as the package's collated Batch on the device (x: one-hot of the labels unless given)."""
    N = b.rowptr.size - 1
    ei = R.edge_index_of(b)
    if extra_edges is not None:
        ei = np.concatenate([ei, np.asarray(extra_edges, dtype=np.int64).reshape(2, -1)], axis=1)
    if x is None:
        x = torch.nn.functional.one_hot(torch.from_numpy(b.labels), int(b.labels.max(initial=0)) + 1).float()
    vec = np.repeat(np.arange(b.ptr.size - 1), np.diff(b.ptr))
    return Batch(x, torch.from_numpy(ei), torch.from_numpy(vec), torch.from_numpy(b.ptr), b.ptr.tolist(), [0] * b.ptr.size,
                 torch.zeros(b.ptr.size - 1, dtype=torch.int64)).to(DEV)


# ---------------------------------------------------------------------------- 1. colours, sorted lists, histograms, status
@pytest.mark.parametrize("iters", [0, 1, 3, 7])
@pytest.mark.parametrize("kind,use_labels", [("labels", True), ("labels", False), ("wide", True)])
def test_refinement_equals_the_reference_bit_for_bit(kind, use_labels, iters):
    for dim in (1, 100, 256):
        _assert_refined(_gpu_refine(_batch(kind), iters, dim, use_labels), _ref(kind, iters, dim, use_labels))


# ---------------------------------------------------------------------------- 2. the other instance, refused graphs keep the fill
@pytest.mark.parametrize("cap", [256, 64])
def test_a_smaller_bound_selects_the_small_instance_and_refuses_the_rest(cap):
    b = _batch()
    sizes = np.diff(b.ptr)
    want = _ref("labels", 3, 100, True, cap, FILL)
    got = _gpu_refine(b, 3, 100, max_graph_nodes=cap, fill=FILL)
    _assert_refined(got, want)
    assert np.array_equal((want.status & 1) == 1, sizes > cap) and want.status[R.INDEX["cycle1024"]] == 1
    if cap == 256:
        assert want.status[R.INDEX["random257"]] == 1 and want.status[R.INDEX["random256"]] == 0
    full, srt = _ref("labels", 3, 100), _u64(got.sorted)
    for g in range(sizes.size):                                                   # the graphs that fit: the bits of the unbounded call
        seg = slice(4 * b.ptr[g], 4 * b.ptr[g + 1])
        if sizes[g] <= cap:
            assert np.array_equal(srt[seg], full.sorted[seg]) and np.array_equal(got.hist[g].cpu().numpy(), full.hist[g])
        else:
            assert np.all(srt[seg].view(np.int64) == FILL) and bool((got.hist[g] == FILL).all())


# ---------------------------------------------------------------------------- 3. a graph above the limit
def test_a_graph_of_1025_nodes_is_refused_loudly():
    n = ops.WL_MAX_GRAPH_NODES + 1
    graphs = [(6, R._cycle(6), np.zeros(6, dtype=np.int64)), (n, R._cycle(n), np.zeros(n, dtype=np.int64)), (2, [(0, 1)], np.zeros(2, dtype=np.int64))]
    b = R.make_batch(graphs)
    got, want = _gpu_refine(b, 2, 16, fill=FILL), R.refine(b, 2, 16, fill=FILL)
    assert want.status.tolist() == [0, 1, 0]
    _assert_refined(got, want)
    with pytest.raises(GnnmpError, match=r"graph 1 has 1025 nodes"):
        GB.wl_features(_graph_batch(b), 2)


# ---------------------------------------------------------------------------- 4. entries that leave their graph
def test_entries_pointing_into_a_neighbouring_graph_are_skipped_and_counted():
    b = _batch()
    g, other = R.INDEX["path64"], R.INDEX["star65"]
    col = b.col.copy()
    v = int(b.ptr[g]) + 10                                                        # an inner node of the path: both its entries now point at the star
    assert b.rowptr[v + 1] - b.rowptr[v] == 2
    col[b.rowptr[v]:b.rowptr[v + 1]] = [b.ptr[other], b.ptr[other] + 7]
    bad = b._replace(col=col)
    want = R.refine(bad, 3, 256)
    assert want.status[g] == 2 << 8 and np.count_nonzero(want.status) == 1
    got = _gpu_refine(bad, 3, 256)
    _assert_refined(got, want)
    clean, srt = _ref("labels", 3, 256), _u64(got.sorted)
    for k in range(b.ptr.size - 1):                                               # every other graph: as without the damage
        seg = slice(4 * b.ptr[k], 4 * b.ptr[k + 1])
        assert np.array_equal(srt[seg], clean.sorted[seg]) == (k != g)
    with pytest.raises(GnnmpError, match="skipped"):                              # an edge between two graphs of a batch
        GB.wl_features(_graph_batch(b, extra_edges=[[int(b.ptr[g])], [int(b.ptr[other])]]), 3)


# ---------------------------------------------------------------------------- 5. the Gram
@pytest.mark.parametrize("iters", [0, 3, 7])
def test_gram_rectangular_and_against_itself(iters):
    graphs = R.fixed_graphs()
    pick = [R.INDEX[k] for k in ("empty", "c6", "c3c3", "k40", "cycle1024", "star65")] + [len(graphs) - 1]
    a, b = R.make_batch([graphs[i] for i in pick]), R.make_batch(graphs[:31])
    ra, rb = R.refine(a, iters, 8), R.refine(b, iters, 8)
    ga, gb = _gpu_refine(a, iters, 8), _gpu_refine(b, iters, 8)
    pa, pb = _t(a.ptr, torch.int64), _t(b.ptr, torch.int64)
    K = ops.wl_gram(ga.sorted, pa, gb.sorted, pb, iters)
    assert K.dtype == torch.int64 and tuple(K.shape) == (7, 31)
    want = R.gram(ra.sorted, a.ptr, rb.sorted, b.ptr, iters)
    assert np.array_equal(K.cpu().numpy(), want)
    assert np.array_equal(ops.wl_gram(gb.sorted, pb, ga.sorted, pa, iters).cpu().numpy(), want.T)
    assert not K[0].any() and K[3, R.INDEX["k40"]] == 40 * 40 * (iters + 1)       # the empty graph; one long run against one long run
    S = ops.wl_gram(gb.sorted, pb, gb.sorted, pb, iters).cpu().numpy()
    assert np.array_equal(S, R.gram(rb.sorted, b.ptr, rb.sorted, b.ptr, iters)) and np.array_equal(S, S.T)
    for g in range(31):
        _, counts = np.unique(R.segment(rb.sorted, b.ptr, g, iters), return_counts=True)
        assert S[g, g] == int(np.sum(counts.astype(np.int64) ** 2))
    c = R.INDEX["cycle1024"]
    assert S[c, c] == 1024 * 1024 * (iters + 1) and not S[R.INDEX["empty"]].any()


# ---------------------------------------------------------------------------- 6. node numbering does not matter on the device
def test_node_permutations_change_nothing_on_the_device():
    a, b = _batch(), _batch("permuted")
    for use_labels in (True, False):
        ga, gb = _gpu_refine(a, 3, 100, use_labels), _gpu_refine(b, 3, 100, use_labels)
        assert torch.equal(ga.sorted, gb.sorted) and torch.equal(ga.hist, gb.hist)
        pa, pb = _t(a.ptr, torch.int64), _t(b.ptr, torch.int64)
        assert torch.equal(ops.wl_gram(ga.sorted, pa, ga.sorted, pa, 3), ops.wl_gram(gb.sorted, pb, ga.sorted, pa, 3))
    assert not torch.equal(ga.colors, gb.colors)


# ---------------------------------------------------------------------------- 7. no global state
def test_two_streams_do_not_disturb_each_other():
    a, b = _batch(), _batch("wide")
    args_a = (_t(a.ptr, torch.int64), _t(a.rowptr, torch.int32), _t(a.col, torch.int32), _t(a.labels, torch.int64))
    args_b = (_t(b.ptr, torch.int64), _t(b.rowptr, torch.int32), _t(b.col, torch.int32), _t(b.labels, torch.int64))
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        o1 = ops.wl_refine(*args_a, 7, 256, max_graph_nodes=1024, return_colors=True)
        k1 = ops.wl_gram(o1.sorted, args_a[0], o1.sorted, args_a[0], 7)
    with torch.cuda.stream(s2):
        o2 = ops.wl_refine(*args_b, 3, 100, max_graph_nodes=1024, return_colors=True)
        k2 = ops.wl_gram(o2.sorted, args_b[0], o2.sorted, args_b[0], 3)
    torch.cuda.synchronize()
    _assert_refined(o1, _ref("labels", 7, 256))
    _assert_refined(o2, _ref("wide", 3, 100))
    w1, w2 = _ref("labels", 7, 256), _ref("wide", 3, 100)
    assert np.array_equal(k1.cpu().numpy(), R.gram(w1.sorted, a.ptr, w1.sorted, a.ptr, 7))
    assert np.array_equal(k2.cpu().numpy(), R.gram(w2.sorted, b.ptr, w2.sorted, b.ptr, 3))


# ---------------------------------------------------------------------------- argument errors and empty inputs
def test_argument_errors_and_empty_inputs():
    b = _batch()
    ptr, rp, cl, lab = _t(b.ptr, torch.int64), _t(b.rowptr, torch.int32), _t(b.col, torch.int32), _t(b.labels, torch.int64)
    G, N, nnz = ptr.numel() - 1, rp.numel() - 1, cl.numel()
    srt, hist, st = torch.zeros(4 * N, dtype=torch.int64, device=DEV), torch.zeros(G, 256, dtype=torch.int32, device=DEV), torch.zeros(G, dtype=torch.int32, device=DEV)
    K = torch.zeros(G, G, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())                   # noqa: E731

    def refine(ptr_=ptr, G_=G, rp_=rp, N_=N, nnz_=nnz, iters=3, dim=256, mgn=1024, srt_=srt, hist_=hist, st_=st):
        return L.lib().gmp_wl_refine(p(ptr_), G_, p(rp_), p(cl), N_, nnz_, p(lab), iters, dim, mgn, None, p(srt_), p(hist_), p(st_), None, 0, None)

    def gram(sa=srt, pa=ptr, Ga=G, la=4 * N, Gb=G, lb=4 * N, iters=3, K_=K):
        return L.lib().gmp_wl_gram(p(sa), p(pa), Ga, la, p(srt), p(ptr), Gb, lb, iters, p(K_), None)

    for rc in (refine(iters=-1), refine(iters=8), refine(dim=0), refine(dim=257), refine(ptr_=None), refine(rp_=None), refine(srt_=None),
               refine(hist_=None), refine(st_=None), refine(G_=-1), refine(N_=-1), refine(N_=2 ** 31), refine(nnz_=-1), refine(mgn=-1),
               gram(iters=-1), gram(iters=8), gram(sa=None), gram(pa=None), gram(K_=None), gram(Ga=-1), gram(la=-1), gram(Ga=2 ** 31)):
        assert rc == GMP_ERR_ARG
    assert refine(G_=0) == 0 and gram(Ga=0) == 0 and gram(Gb=0) == 0              # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert not srt.any() and not hist.any() and not K.any()
    with pytest.raises(GnnmpError, match="iters"):
        ops.wl_refine(ptr, rp, cl, lab, iters=8)
    with pytest.raises(GnnmpError, match="dim"):
        ops.wl_refine(ptr, rp, cl, lab, dim=257)
    with pytest.raises(GnnmpError, match="labels has"):
        ops.wl_refine(ptr, rp, cl, lab[:-1].contiguous())
    with pytest.raises(GnnmpError):
        ops.wl_refine(ptr.cpu(), rp, cl, lab)
    with pytest.raises(GnnmpError):
        ops.wl_gram(srt.cpu(), ptr, srt, ptr, 3)
    one = torch.zeros(1, dtype=torch.int64, device=DEV)
    empty = ops.wl_refine(one, torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV))
    assert empty.sorted.shape == (0,) and empty.hist.shape == (0, 256) and empty.status.shape == (0,)
    assert ops.wl_gram(empty.sorted, one, srt, ptr, 3).shape == (0, G)


# ---------------------------------------------------------------------------- 8. the baseline on a separable set
def _baseline_datasets():
    from gnn_pretraining_amd.data.pretrain_data_loaders import GraphDataset
    from gnn_pretraining_amd.data.store import GraphStore
    graphs, y = R.baseline_graphs()
    data = []
    for (n, edges, _), cls in zip(graphs, y):
        e = torch.as_tensor(np.asarray(edges, dtype=np.int64).T.copy())
        data.append(Data(torch.full((n, 3), 0.5), e, torch.tensor([int(cls)])))       # no one-hot rows: the refinement starts from degrees
    store = GraphStore.from_data_list(data)
    nt = R.BASELINE_TRAIN
    return GraphDataset(store, np.arange(nt)), GraphDataset(store, np.arange(nt, len(graphs))), graphs, y


def test_wl_baseline_on_a_separable_set():
    train_ds, eval_ds, graphs, y = _baseline_datasets()
    nt, h, k = R.BASELINE_TRAIN, R.BASELINE_ITERS, R.BASELINE_K
    scores = GB.wl_baseline(train_ds, eval_ds, 2, h, k=k, device=DEV)
    assert set(scores) == {"knn_accuracy", "logreg_accuracy"}
    # by hand, from the same pieces
    tb, eb = train_ds.collate(torch.arange(nt)).to(DEV), eval_ds.collate(torch.arange(len(eval_ds))).to(DEV)
    ft, fe = GB.wl_features(tb, h), GB.wl_features(eb, h)
    rtb, reb = R.make_batch(graphs[:nt]), R.make_batch(graphs[nt:])
    rt, re_ = R.refine(rtb, h, 256, False), R.refine(reb, h, 256, False)
    assert np.array_equal(_u64(ft.sorted), rt.sorted) and np.array_equal(fe.hist.cpu().numpy(), re_.hist)
    K_et, K_ee, K_tt = GB.wl_kernel(fe, ft), GB.wl_kernel(fe, fe).diagonal(), GB.wl_kernel(ft, ft).diagonal()
    want_et = R.gram(re_.sorted, reb.ptr, rt.sorted, rtb.ptr, h)
    assert np.array_equal(K_et.cpu().numpy(), want_et)
    sim = R.normalised_similarity(want_et, np.diag(R.gram(re_.sorted, reb.ptr, re_.sorted, reb.ptr, h)), np.diag(R.gram(rt.sorted, rtb.ptr, rt.sorted, rtb.ptr, h)))
    idx, val = GB.wl_neighbours(GB.normalised_similarity(K_et, K_ee, K_tt), k)
    assert tuple(idx.shape) == (R.BASELINE_EVAL, k) and np.array_equal(idx.cpu().numpy(), R.top_k(sim, k))
    y_train, y_eval = torch.from_numpy(y[:nt]).to(DEV), torch.from_numpy(y[nt:]).to(DEV)
    _, knn_pred = ops.knn_vote(idx, val.float().contiguous(), y_train, 2)
    fit = ops.logreg_fit(ft.hist.float().contiguous(), y_train, 2)
    lr_pred = ops.logreg_predict(fe.hist.float().contiguous(), fit.state.weight, fit.state.bias)
    assert scores["knn_accuracy"] == float((knn_pred == y_eval).float().mean())
    assert scores["logreg_accuracy"] == float((lr_pred == y_eval).float().mean())
    print("wl_baseline", scores)
    assert scores["knn_accuracy"] > 0.5 and scores["logreg_accuracy"] > 0.5


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
def test_cli_wl_baseline_logs_the_two_keys_and_leaves_training_alone(tmp_path, monkeypatch, engine):
    """python -m gnn_pretraining_amd.finetune.finetune ... --wl-baseline 3, in process: one epoch on the synthetic PTC_MR stand-in.  The test
    record carries the two keys, equal to wl_baseline called directly on the same splits; every other key but the timing ones, and the
    checkpoint, are bit for bit those of the same run without the flag."""
    from gnn_pretraining_amd.constants import NUM_CLASSES
    from gnn_pretraining_amd.data.finetune_data_loaders import create_finetune_data_loader
    keys = ["test/wl_knn_accuracy", "test/wl_logreg_accuracy"]
    rec1, state1 = _run_cli(tmp_path, monkeypatch, "with", engine + ["--wl-baseline", "3"])
    rec0, state0 = _run_cli(tmp_path, monkeypatch, "without", engine)
    test1 = [r for r in rec1 if keys[0] in r]
    assert len(test1) == 1 and "test/accuracy" in test1[0] and all(k in test1[0] for k in keys)
    assert not any("wl_" in k for r in rec1 if r is not test1[0] for k in r) and not any("wl_" in k for r in rec0 for k in r)
    sets = {sp: create_finetune_data_loader("PTC_MR", sp, 32, torch.Generator(), tmp_path / "data").dataset for sp in ("train", "test")}
    direct = GB.wl_baseline(sets["train"], sets["test"], NUM_CLASSES["PTC_MR"], 3, device=DEV)
    assert test1[0][keys[0]] == direct["knn_accuracy"] and test1[0][keys[1]] == direct["logreg_accuracy"]
    assert state1.keys() == state0.keys() and all(torch.equal(state1[k], state0[k]) for k in state1)
    timing = ("test/training_time", "test/time_per_epoch")
    for k, v in [r for r in rec0 if "test/accuracy" in r][0].items():
        assert k in timing or "time" in k or test1[0][k] == v or (v != v and test1[0][k] != test1[0][k]), k
