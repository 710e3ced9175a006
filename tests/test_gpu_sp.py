"""The shortest-path kernel baseline on the GPU (csrc/sp.hip: ops.sp_features / ops.sp_gram, finetune/graph_baselines.py, --sp-baseline)
against the CPU definition of tests/sp_ref.py.  Everything the kernels compute is integer arithmetic, so everything is compared for
EQUALITY.  The reference's distance matrices are computed once per batch and shared; test_sp_host.py holds them to a second route."""
import ctypes as C
import functools
import json
import sys

import numpy as np
import pytest
import torch

import sp_ref as R
import wl_ref
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


@functools.lru_cache(maxsize=None)
def _batch(kind="labels"):
    graphs = R.fixed_graphs()
    if kind == "wide":
        graphs = R.with_wide_labels(graphs)
    if kind == "permuted":
        graphs = R.permuted(graphs, 3)
    return R.make_batch(graphs)


@functools.lru_cache(maxsize=None)
def _dist(kind="labels"):
    return R.batch_distances(_batch("permuted" if kind == "permuted" else "labels"))       # (labels do not move a distance)


@functools.lru_cache(maxsize=None)
def _ref(kind, max_dist, dim, use_labels=True, max_graph_nodes=R.MAX_GRAPH_NODES, cap=None, fill=FILL):
    return R.features(_batch(kind), max_dist, dim, use_labels, max_graph_nodes, cap, fill, dist=_dist(kind))


def _gpu(batch, max_dist, dim, use_labels=True, max_graph_nodes=None, cap=None, fill=FILL):
    return ops.sp_features(_t(batch.ptr, torch.int64), _t(batch.rowptr, torch.int32), _t(batch.col, torch.int32),
                           _t(batch.labels, torch.int64) if use_labels else None, max_dist, dim, max_graph_nodes, cap, fill=fill)


def _assert_features(got, want):
    assert got.keys.dtype == torch.int64 and all(t.dtype == torch.int32 for t in (got.counts, got.nuniq, got.hist, got.status))
    assert np.array_equal(got.status.cpu().numpy(), want.status)
    assert np.array_equal(got.nuniq.cpu().numpy(), want.nuniq)
    assert np.array_equal(got.keys.cpu().numpy(), want.keys)                       # the untouched tails and rows hold the fill in both
    assert np.array_equal(got.counts.cpu().numpy(), want.counts)
    assert np.array_equal(got.hist.cpu().numpy(), want.hist)


def _gram(a, b):
    return ops.sp_gram(a.keys, a.counts, a.nuniq, b.keys, b.counts, b.nuniq)


def _graph_batch(b, x=None, extra_edges=None):
    """wl_ref's batch as the package's collated Batch on the device (x: one-hot of the labels unless given)."""
    ei = wl_ref.edge_index_of(b)
    if extra_edges is not None:
        ei = np.concatenate([ei, np.asarray(extra_edges, dtype=np.int64).reshape(2, -1)], axis=1)
    if x is None:
        x = torch.nn.functional.one_hot(torch.from_numpy(b.labels), int(b.labels.max(initial=0)) + 1).float()
    vec = np.repeat(np.arange(b.ptr.size - 1), np.diff(b.ptr))
    return Batch(x, torch.from_numpy(ei), torch.from_numpy(vec), torch.from_numpy(b.ptr), b.ptr.tolist(), [0] * b.ptr.size,
                 torch.zeros(b.ptr.size - 1, dtype=torch.int64)).to(DEV)


# ---------------------------------------------------------------------------- 1. keys, counts, histograms, status
@pytest.mark.parametrize("max_dist", [1, 2, 5, 1023])
@pytest.mark.parametrize("use_labels", [True, False], ids=["labels", "degrees"])
def test_features_equal_the_reference_bit_for_bit(use_labels, max_dist):
    for dim in (1, 100, 256):
        want = _ref("labels", max_dist, dim, use_labels)
        assert not want.status.any()
        _assert_features(_gpu(_batch(), max_dist, dim, use_labels), want)
    c = R.INDEX["cycle1024"]
    assert want.nuniq[c] == min(max_dist, 512) and want.counts[c, :want.nuniq[c]].sum() == (523776 if max_dist == 1023 else 1024 * max_dist)


# ---------------------------------------------------------------------------- 2. the other instance, refused graphs keep the fill
@pytest.mark.parametrize("bound", [256, 64])
def test_a_smaller_bound_selects_the_small_instance_and_refuses_the_rest(bound):
    b = _batch()
    sizes = np.diff(b.ptr)
    want = _ref("labels", 1023, 100, True, bound)
    got = _gpu(b, 1023, 100, max_graph_nodes=bound)
    assert got.keys.shape == (sizes.size, 4096)
    _assert_features(got, want)
    assert np.array_equal((want.status & 1) == 1, sizes > bound) and want.status[R.INDEX["cycle1024"]] == 1
    if bound == 256:
        assert want.status[R.INDEX["random257"]] == 1 and want.status[R.INDEX["random256"]] == 0
    full = _ref("labels", 1023, 100)
    for g in range(sizes.size):                                                    # the graphs that fit: the bits of the unbounded call
        if sizes[g] <= bound:
            m = full.nuniq[g]
            assert want.nuniq[g] == m and np.array_equal(want.keys[g, :m], full.keys[g, :m]) and np.array_equal(want.hist[g], full.hist[g])
        else:
            assert want.nuniq[g] == 0 and np.all(want.keys[g] == FILL) and np.all(want.counts[g] == FILL) and np.all(want.hist[g] == FILL)


# ---------------------------------------------------------------------------- 3. a graph above the limit, labels out of range
def test_a_graph_of_1025_nodes_is_refused_loudly():
    n = ops.SP_MAX_GRAPH_NODES + 1
    z = lambda k: np.zeros(k, dtype=np.int64)                                      # noqa: E731
    b = R.make_batch([(6, wl_ref._cycle(6), z(6)), (n, wl_ref._cycle(n), z(n)), (2, [(0, 1)], z(2))])
    got, want = _gpu(b, 4, 16), R.features(b, 4, 16, max_graph_nodes=n, fill=FILL)
    assert want.status.tolist() == [0, 1, 0] and want.nuniq.tolist() == [3, 0, 1]
    _assert_features(got, want)
    with pytest.raises(GnnmpError, match=r"graph 1 has 1025 nodes"):
        GB.sp_features(_graph_batch(b), 4)


def test_labels_outside_24_bits_set_bit_2():
    b = _batch("wide")
    want = _ref("wide", 5, 100)
    assert np.array_equal(want.status == 4, np.diff(b.ptr) > 0) and not want.nuniq.any()
    _assert_features(_gpu(b, 5, 100), want)
    top = b._replace(labels=np.where(np.arange(b.labels.size) == int(b.ptr[R.INDEX["k40"]]) + 3, R.MAX_LABEL, 0).astype(np.int64))
    want = R.features(top, 5, 100, fill=FILL, dist=_dist())
    assert np.flatnonzero(want.status).tolist() == [R.INDEX["k40"]] and want.status[R.INDEX["k40"]] == 4
    _assert_features(_gpu(top, 5, 100), want)
    edge = b._replace(labels=np.full(b.labels.size, R.MAX_LABEL - 1, dtype=np.int64))          # the largest legal label
    want = R.features(edge, 5, 100, fill=FILL, dist=_dist())
    assert not want.status.any()
    _assert_features(_gpu(edge, 5, 100), want)
    with pytest.raises(GnnmpError, match="label outside"):
        GB.sp_features(_graph_batch(_batch()), 5, labels=_t(top.labels, torch.int64))


# ---------------------------------------------------------------------------- 4. entries that leave their graph
def test_entries_pointing_into_a_neighbouring_graph_are_skipped_and_counted():
    b = _batch()
    g, other = R.INDEX["path64"], R.INDEX["star65"]
    col = b.col.copy()
    v = int(b.ptr[g]) + 10                                                         # an inner node of the path: both its entries now point at the star
    assert b.rowptr[v + 1] - b.rowptr[v] == 2
    col[b.rowptr[v]:b.rowptr[v + 1]] = [b.ptr[other], b.ptr[other] + 7]
    bad = b._replace(col=col)
    dist = list(_dist())
    dist[g] = None                                                                 # (only this graph's distances may have moved)
    for use_labels in (True, False):
        want = R.features(bad, 1023, 256, use_labels, fill=FILL, dist=dist)
        assert want.status[g] == 2 << 8 and np.count_nonzero(want.status) == 1
        got = _gpu(bad, 1023, 256, use_labels)
        _assert_features(got, want)
        clean = _ref("labels", 1023, 256, use_labels)
        for k in range(b.ptr.size - 1):                                            # every other graph: as without the damage; the path itself stays
            assert np.array_equal(want.keys[k], clean.keys[k]) == (k != g or use_labels)       # connected through its neighbours' entries and loses a degree
    with pytest.raises(GnnmpError, match="skipped"):                               # an edge between two graphs of a batch
        GB.sp_features(_graph_batch(b, extra_edges=[[int(b.ptr[g])], [int(b.ptr[other])]]), 3)


# ---------------------------------------------------------------------------- 5. more distinct keys than the row stride
@pytest.mark.parametrize("bound", [None, 300], ids=["small instance", "beside the large instance"])
def test_key_overflow_sets_bit_1_at_the_first_graph_that_does_not_fit(bound):
    cap = ops.sp_max_unique(bound or 0)
    assert cap == R.max_unique(bound or 0)
    n = max(k for k in range(2, 257) if k * (k - 1) // 2 <= cap)                   # 91 at 4096 keys, 45 at 1024
    b = R.make_batch([R.distinct_label_path(n), R.distinct_label_path(n + 1), R.distinct_label_path(5)])
    mgn = bound or n + 1
    want = R.features(b, 1023, 64, max_graph_nodes=mgn, fill=FILL)
    assert want.status.tolist() == [0, 2, 0] and want.nuniq.tolist() == [n * (n - 1) // 2, 0, 10]
    got = _gpu(b, 1023, 64, max_graph_nodes=mgn)
    assert got.keys.shape == (3, cap)
    _assert_features(got, want)
    d = n // 2 - 5                                                                 # without the long distances the larger path fits too
    short = R.features(b, d, 64, max_graph_nodes=mgn, fill=FILL)
    assert short.status.tolist() == [0, 0, 0] and short.nuniq[1] == sum(n + 1 - k for k in range(1, d + 1)) <= cap
    _assert_features(_gpu(b, d, 64, max_graph_nodes=mgn), short)
    small = R.features(b, 1023, 64, max_graph_nodes=mgn, cap=16, fill=FILL)        # an explicit smaller stride
    assert small.status.tolist() == [2, 2, 0]
    got = _gpu(b, 1023, 64, max_graph_nodes=mgn, cap=16)
    assert got.keys.shape == (3, 16)
    _assert_features(got, small)
    with pytest.raises(GnnmpError, match="cap"):
        _gpu(b, 1023, 64, max_graph_nodes=mgn, cap=cap + 1)
    if bound is None:                                                              # (the baseline sizes the stride from the batch's own largest graph)
        with pytest.raises(GnnmpError, match="graph 1 has more than 4096 distinct"):
            GB.sp_features(_graph_batch(b, x=torch.zeros(int(b.ptr[-1]), 2)), 1023, labels=_t(b.labels, torch.int64))


# ---------------------------------------------------------------------------- 6. the Gram
@pytest.mark.parametrize("max_dist", [1, 5, 1023])
def test_gram_rectangular_and_against_itself(max_dist):
    graphs = R.fixed_graphs()
    pick = [R.INDEX[k] for k in ("empty", "c6", "c3c3", "k40", "cycle1024", "star65")] + [len(graphs) - 1]
    a = R.make_batch([graphs[i] for i in pick])
    dist = _dist()
    ra, rb = R.features(a, max_dist, 8, dist=[dist[i] for i in pick]), _ref("labels", max_dist, 8, fill=0)
    ga, gb = _gpu(a, max_dist, 8, cap=600, fill=0), _gpu(_batch(), max_dist, 8, fill=0)         # two different row strides
    K = _gram(ga, gb)
    assert K.dtype == torch.int64 and tuple(K.shape) == (7, len(graphs))
    want = R.gram(ra, rb)
    assert np.array_equal(K.cpu().numpy(), want)
    assert np.array_equal(_gram(gb, ga).cpu().numpy(), want.T)
    assert not K[0].any() and K[3, R.INDEX["k40"]] == 780 * 780                    # the empty graph; one key against the same key
    S = _gram(gb, gb).cpu().numpy()
    assert np.array_equal(S, R.gram(rb, rb)) and np.array_equal(S, S.T)
    feat = GB.SPFeatures(gb.keys, gb.counts, gb.nuniq, gb.hist, max_dist)
    assert np.array_equal(np.diag(S), GB.sp_self_similarity(feat).cpu().numpy()) and np.array_equal(np.diag(S), R.self_similarity(rb))
    if max_dist == 1023:
        c = R.INDEX["cycle1024"]
        assert S[c, c] == 511 * 1024 * 1024 + 512 * 512 and S[R.INDEX["c6"], R.INDEX["c3c3"]] == 36
    filled = _gpu(_batch(), max_dist, 8)                                           # the fill behind nuniq is never read
    assert np.array_equal(_gram(filled, filled).cpu().numpy(), S)


# ---------------------------------------------------------------------------- 7. against gmp_graph_props
def test_largest_distance_is_the_diameter_and_every_pair_is_counted():
    b = _batch()
    got = _gpu(b, 1023, 256)
    ei = _t(wl_ref.edge_index_of(b), torch.int64)
    eptr = _t(b.rowptr.astype(np.int64)[b.ptr], torch.int64)
    props, _ = ops.graph_properties(_t(b.ptr, torch.int64), eptr, ei, max_graph_nodes=1024)
    props, keys, counts, nuniq = props.cpu().numpy(), got.keys.cpu().numpy(), got.counts.cpu().numpy(), got.nuniq.cpu().numpy()
    connected = [g for g in range(nuniq.size) if props[g, 7] == 1 and props[g, 0] >= 2]
    assert {R.INDEX[k] for k in ("edge", "star65", "path64", "c6", "k40", "cycle1024")} <= set(connected)
    for g in connected:
        n, m = int(props[g, 0]), int(nuniq[g])
        assert int((keys[g, :m] & 2047).max()) == props[g, 8], g                   # slot 8: the diameter
        assert int(counts[g, :m].sum()) == n * (n - 1) // 2, g
    assert props[R.INDEX["cycle1024"], 8] == 512 and props[R.INDEX["path64"], 8] == 63


# ---------------------------------------------------------------------------- 8. node numbering does not matter on the device
def test_node_permutations_change_nothing_on_the_device():
    a, b = _batch(), _batch("permuted")
    assert not np.array_equal(a.col, b.col)
    for use_labels in (True, False):
        ga, gb = _gpu(a, 1023, 100, use_labels), _gpu(b, 1023, 100, use_labels)
        assert all(torch.equal(x, y) for x, y in zip(ga, gb))
        assert torch.equal(_gram(ga, ga), _gram(gb, ga))


# ---------------------------------------------------------------------------- 9. no global state
def test_two_streams_do_not_disturb_each_other():
    a, b = _batch(), _batch("permuted")
    args_a = (_t(a.ptr, torch.int64), _t(a.rowptr, torch.int32), _t(a.col, torch.int32), _t(a.labels, torch.int64))
    args_b = (_t(b.ptr, torch.int64), _t(b.rowptr, torch.int32), _t(b.col, torch.int32), None)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        o1 = ops.sp_features(*args_a, 1023, 256, 1024, fill=FILL)
        k1 = _gram(o1, o1)
    with torch.cuda.stream(s2):
        o2 = ops.sp_features(*args_b, 5, 100, 1024, cap=64, fill=FILL)
        k2 = _gram(o2, o2)
    torch.cuda.synchronize()
    w1, w2 = _ref("labels", 1023, 256), _ref("permuted", 5, 100, False, cap=64)
    _assert_features(o1, w1)
    _assert_features(o2, w2)
    assert np.array_equal(k1.cpu().numpy(), R.gram(w1, w1)) and np.array_equal(k2.cpu().numpy(), R.gram(w2, w2))


# ---------------------------------------------------------------------------- argument errors and empty inputs
def test_argument_errors_and_empty_inputs():
    b = _batch()
    ptr, rp, cl, lab = _t(b.ptr, torch.int64), _t(b.rowptr, torch.int32), _t(b.col, torch.int32), _t(b.labels, torch.int64)
    G, N, nnz, cap = ptr.numel() - 1, rp.numel() - 1, cl.numel(), 1024
    keys, cnt = torch.zeros(G, cap, dtype=torch.int64, device=DEV), torch.zeros(G, cap, dtype=torch.int32, device=DEV)
    nu, hist, st = (torch.zeros(G, dtype=torch.int32, device=DEV), torch.zeros(G, 256, dtype=torch.int32, device=DEV),
                    torch.zeros(G, dtype=torch.int32, device=DEV))
    K = torch.zeros(G, G, dtype=torch.int64, device=DEV)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())                    # noqa: E731

    def feat(ptr_=ptr, G_=G, rp_=rp, N_=N, nnz_=nnz, md=5, dim=256, mgn=1024, cap_=cap, keys_=keys, cnt_=cnt, nu_=nu, hist_=hist, st_=st):
        return L.lib().gmp_sp_features(p(ptr_), G_, p(rp_), p(cl), N_, nnz_, p(lab), md, dim, mgn, cap_, p(keys_), p(cnt_), p(nu_), p(hist_),
                                       p(st_), None, 0, None)

    def gram(ka=keys, ca=cnt, na=nu, Ga=G, cap_a=cap, Gb=G, cap_b=cap, K_=K):
        return L.lib().gmp_sp_gram(p(ka), p(ca), p(na), Ga, cap_a, p(keys), p(cnt), p(nu), Gb, cap_b, p(K_), None)

    for rc in (feat(md=0), feat(md=1024), feat(dim=0), feat(dim=257), feat(cap_=0), feat(cap_=1025), feat(mgn=256, cap_=4097), feat(ptr_=None),
               feat(rp_=None), feat(keys_=None), feat(cnt_=None), feat(nu_=None), feat(hist_=None), feat(st_=None), feat(G_=-1), feat(N_=-1),
               feat(N_=2 ** 31), feat(nnz_=-1), feat(nnz_=2 ** 31), feat(mgn=-1),
               gram(ka=None), gram(ca=None), gram(na=None), gram(K_=None), gram(Ga=-1), gram(Gb=-1), gram(cap_a=0), gram(cap_b=4097),
               gram(Ga=2 ** 31), gram(Ga=2 ** 17, Gb=2 ** 17)):
        assert rc == GMP_ERR_ARG
    assert feat(G_=0) == 0 and gram(Ga=0) == 0 and gram(Gb=0) == 0                 # nothing to do, nothing launched
    torch.cuda.synchronize()
    assert not keys.any() and not cnt.any() and not nu.any() and not hist.any() and not st.any() and not K.any()
    with pytest.raises(GnnmpError, match="max_dist"):
        ops.sp_features(ptr, rp, cl, lab, 1024)
    with pytest.raises(GnnmpError, match="dim"):
        ops.sp_features(ptr, rp, cl, lab, 5, 257)
    with pytest.raises(GnnmpError, match="labels has"):
        ops.sp_features(ptr, rp, cl, lab[:-1].contiguous(), 5)
    with pytest.raises(GnnmpError):
        ops.sp_features(ptr.cpu(), rp, cl, lab, 5)
    with pytest.raises(GnnmpError):
        ops.sp_gram(keys.cpu(), cnt, nu, keys, cnt, nu)
    one = torch.zeros(1, dtype=torch.int64, device=DEV)
    empty = ops.sp_features(one, torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(0, dtype=torch.int32, device=DEV), None, 5)
    assert empty.keys.shape == (0, 4096) and empty.hist.shape == (0, 256) and empty.status.shape == (0,)
    assert ops.sp_gram(empty.keys, empty.counts, empty.nuniq, keys, cnt, nu).shape == (0, G)


# ---------------------------------------------------------------------------- 10. the baseline on a separable set
def _baseline_datasets():
    from gnn_pretraining_amd.data.pretrain_data_loaders import GraphDataset
    from gnn_pretraining_amd.data.store import GraphStore
    graphs, y = R.baseline_graphs()
    data = []
    for (n, edges, _), cls in zip(graphs, y):
        e = torch.as_tensor(np.asarray(edges, dtype=np.int64).T.copy())
        data.append(Data(torch.full((n, 3), 0.5), e, torch.tensor([int(cls)])))        # no one-hot rows: the labels are the degrees
    store = GraphStore.from_data_list(data)
    nt = wl_ref.BASELINE_TRAIN
    return GraphDataset(store, np.arange(nt)), GraphDataset(store, np.arange(nt, len(graphs))), graphs, y


def test_sp_baseline_on_a_separable_set():
    train_ds, eval_ds, graphs, y = _baseline_datasets()
    nt, k, md = wl_ref.BASELINE_TRAIN, wl_ref.BASELINE_K, 1023
    scores = GB.sp_baseline(train_ds, eval_ds, 2, md, k=k, device=DEV)
    assert set(scores) == {"knn_accuracy", "logreg_accuracy"}
    # by hand, from the same pieces
    tb, eb = train_ds.collate(torch.arange(nt)).to(DEV), eval_ds.collate(torch.arange(len(eval_ds))).to(DEV)
    ft, fe = GB.sp_features(tb, md), GB.sp_features(eb, md)
    cap, big = ft.keys.size(1), [max(n for n, _, _ in part) for part in (graphs[:nt], graphs[nt:])]
    assert [cap, fe.keys.size(1)] == [n * (n - 1) // 2 for n in big]               # the stride: the node pairs of the split's largest graph
    rt, re_ = R.features(R.make_batch(graphs[:nt]), md, 256, False, cap=cap), R.features(R.make_batch(graphs[nt:]), md, 256, False, cap=fe.keys.size(1))
    assert np.array_equal(ft.keys.cpu().numpy(), rt.keys) and np.array_equal(ft.counts.cpu().numpy(), rt.counts)
    assert np.array_equal(ft.nuniq.cpu().numpy(), rt.nuniq) and np.array_equal(fe.hist.cpu().numpy(), re_.hist)
    K_et, K_ee, K_tt = GB.sp_kernel(fe, ft), GB.sp_kernel(fe, fe).diagonal(), GB.sp_kernel(ft, ft).diagonal()
    want_et = R.gram(re_, rt)
    assert np.array_equal(K_et.cpu().numpy(), want_et)
    assert torch.equal(K_ee, GB.sp_self_similarity(fe)) and torch.equal(K_tt, GB.sp_self_similarity(ft))
    sim = R.normalised_similarity(want_et, R.self_similarity(re_), R.self_similarity(rt))
    idx, val = GB.wl_neighbours(GB.normalised_similarity(K_et, K_ee, K_tt), k)
    assert tuple(idx.shape) == (wl_ref.BASELINE_EVAL, k) and np.array_equal(idx.cpu().numpy(), R.top_k(sim, k))
    y_train, y_eval = torch.from_numpy(y[:nt]).to(DEV), torch.from_numpy(y[nt:]).to(DEV)
    _, knn_pred = ops.knn_vote(idx, val.float().contiguous(), y_train, 2)
    fit = ops.logreg_fit(ft.hist.float().contiguous(), y_train, 2)
    lr_pred = ops.logreg_predict(fe.hist.float().contiguous(), fit.state.weight, fit.state.bias)
    assert scores["knn_accuracy"] == float((knn_pred == y_eval).float().mean())
    assert scores["logreg_accuracy"] == float((lr_pred == y_eval).float().mean())
    print("sp_baseline", scores)
    assert scores["knn_accuracy"] == 1.0


# ---------------------------------------------------------------------------- 11. the command-line path
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
def test_cli_sp_baseline_logs_the_two_keys_and_leaves_training_alone(tmp_path, monkeypatch, engine):
    """python -m gnn_pretraining_amd.finetune.finetune ... --sp-baseline 8, in process: one epoch on the synthetic PTC_MR stand-in.  The test
    record carries the two keys, equal to sp_baseline called directly on the same splits; every other key but the timing ones, and the
    checkpoint, are bit for bit those of the same run without the flag.  Beside --wl-baseline 3 both pairs of keys are there, each as in
    the run where its flag stood alone."""
    from gnn_pretraining_amd.constants import NUM_CLASSES
    from gnn_pretraining_amd.data.finetune_data_loaders import create_finetune_data_loader
    sp_keys, wl_keys = ["test/sp_knn_accuracy", "test/sp_logreg_accuracy"], ["test/wl_knn_accuracy", "test/wl_logreg_accuracy"]
    rec1, state1 = _run_cli(tmp_path, monkeypatch, "with", engine + ["--sp-baseline", "8"])
    rec0, state0 = _run_cli(tmp_path, monkeypatch, "without", engine)
    test1 = [r for r in rec1 if sp_keys[0] in r]
    assert len(test1) == 1 and "test/accuracy" in test1[0] and all(k in test1[0] for k in sp_keys)
    assert not any("sp_" in k for r in rec1 if r is not test1[0] for k in r) and not any("sp_" in k for r in rec0 for k in r)
    assert not any("wl_" in k for r in rec1 for k in r)
    sets = {sp: create_finetune_data_loader("PTC_MR", sp, 32, torch.Generator(), tmp_path / "data").dataset for sp in ("train", "test")}
    direct = GB.sp_baseline(sets["train"], sets["test"], NUM_CLASSES["PTC_MR"], 8, device=DEV)
    assert test1[0][sp_keys[0]] == direct["knn_accuracy"] and test1[0][sp_keys[1]] == direct["logreg_accuracy"]
    assert state1.keys() == state0.keys() and all(torch.equal(state1[k], state0[k]) for k in state1)
    timing = ("test/training_time", "test/time_per_epoch")
    test0 = [r for r in rec0 if "test/accuracy" in r][0]
    for k, v in test0.items():
        assert k in timing or "time" in k or test1[0][k] == v or (v != v and test1[0][k] != test1[0][k]), k
    # both baselines in one run
    rec2, state2 = _run_cli(tmp_path, monkeypatch, "both", engine + ["--sp-baseline", "8", "--wl-baseline", "3"])
    rec3, _ = _run_cli(tmp_path, monkeypatch, "wl", engine + ["--wl-baseline", "3"])
    test2, test3 = [r for r in rec2 if "test/accuracy" in r][0], [r for r in rec3 if "test/accuracy" in r][0]
    assert all(test2[k] == test1[0][k] for k in sp_keys) and all(test2[k] == test3[k] for k in wl_keys)
    assert not any("sp_" in k for k in test3)
    assert all(torch.equal(state2[k], state0[k]) for k in state0)
    for k, v in test0.items():
        assert k in timing or "time" in k or test2[k] == v or (v != v and test2[k] != test2[k]), k
