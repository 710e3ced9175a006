"""The walk-based link baselines on the GPU (csrc/lp_walk.hip: ops.lp_walk_score / lp_walk_rank, finetune/link_walks.py, --lp-walks)
against the CPU reference of tests/lp_walk_ref.py.  Scores are float32 folds in a fixed order (or integers, for hops) and counts are
integers, so everything is compared for EQUALITY."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lp_heur_ref as R
import lp_walk_ref as W
from link_rank_util import HUB, N_BIG, big as _big, filter_csr as _filter_csr, run_cli as _run_cli, t as _t
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd._lib import GnnmpError
from gnn_pretraining_amd.finetune import link_heuristics as LH, link_walks as LW
from gnn_pretraining_amd.finetune.metrics import ranking_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
GMP_ERR_ARG = -1
ROUNDS = {"katz": 4, "ppr": 10, "hops": 4}


def _gpu_rank(rowptr, col, src, dst, rounds, damping=1.0, w=None, mode="sum", filt_rows=None):
    n = len(rowptr) - 1
    fr, fc = _filter_csr(filt_rows, n) if filt_rows is not None else (None, None)
    out = ops.lp_walk_rank(_t(rowptr, torch.int32), _t(col, torch.int32), _t(src, torch.int64), _t(dst, torch.int64), rounds, float(damping),
                           None if w is None else _t(w, torch.float32), mode, fr, fc)
    return tuple(t.cpu().numpy() for t in out)


def _gpu_score(rowptr, col, src, dst, rounds, damping=1.0, w=None, mode="sum"):
    return ops.lp_walk_score(_t(rowptr, torch.int32), _t(col, torch.int32), _t(src, torch.int64), _t(dst, torch.int64), rounds, float(damping),
                             None if w is None else _t(w, torch.float32), mode).cpu().numpy()


def _assert_ranks(got, want):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    assert np.array_equal(got[0], want[0]), (got[0], want[0])
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1], want[1], got[2], want[2])


# ---------------------------------------------------------------------------- 1. the three kinds on a seeded random graph
@functools.lru_cache(maxsize=None)
def _big_ref(kind, filtered):
    edges, rowptr, col, src, dst, known = _big()
    w, a, mode = W.params(rowptr, kind)
    return W.ranks(rowptr, col, src, dst, ROUNDS[kind], a, w, mode, R.filter_rows(known, N_BIG) if filtered else None)


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("kind", W.KINDS)
def test_three_kinds_against_the_reference_on_a_random_graph(kind, filtered):
    edges, rowptr, col, src, dst, known = _big()
    want = _big_ref(kind, filtered)
    if not filtered and kind == "katz":                                          # the reference is not vacuous
        assert (want[1] > 0).sum() > 20 and (want[2] > 0).sum() > 20 and (want[0] > 0).sum() > 20
    graph, pairs = _t(edges, torch.int64), _t(np.stack([src, dst]), torch.int64)
    ranks = LW.walk_ranks(graph, N_BIG, pairs, kind, ROUNDS[kind], filter_edges=_t(known, torch.int64) if filtered else None)
    _assert_ranks((ranks.logit.cpu().numpy(), ranks.n_greater.cpu().numpy(), ranks.n_equal.cpu().numpy()), want)
    assert np.array_equal(ranks.rank.cpu().numpy().astype(np.float64), R.rank_of(want[1], want[2]))
    scores = LW.walk_scores(graph, N_BIG, pairs, kind, ROUNDS[kind]).cpu().numpy()
    assert scores.tobytes() == ranks.logit.cpu().numpy().tobytes()               # the pair scorer IS score_true
    assert LH.simple_graph(graph, N_BIG)[0] is LH.simple_graph(graph, N_BIG)[0]  # link_heuristics' graph, cached per tensor


# ---------------------------------------------------------------------------- 2. sizes, across the two storage paths
def _sizes():
    """The last size leaves LDS; 4,096 | 4,097 is where the LDS path changes its block size and accumulators per thread."""
    lds = L.lib().gmp_lp_walk_lds_nodes()
    return [2, 3, 65, 257, 4096, 4097, lds - 1, lds, lds + 1]


@pytest.mark.parametrize("which", range(9))
def test_sizes_across_both_storage_paths(which):
    n = _sizes()[which]
    assert (L.lib().gmp_lp_walk_workspace_bytes(16, n) > 0) == (which == 8)      # only the last size leaves LDS
    rng = np.random.RandomState(300 + which)
    edges = rng.randint(0, n, size=(2, 3 * n))
    rowptr, col = R.simple_csr(edges, n)
    src, dst = rng.randint(0, n, size=16), rng.randint(0, n, size=16)
    for i in range(2, 9):                                                        # some destinations at distance two
        if rowptr[src[i] + 1] > rowptr[src[i]]:
            z = col[rowptr[src[i]]]
            dst[i] = col[rowptr[z + 1] - 1]
    dst[0] = n - 1                                                              # a true destination and a filter entry at the last node
    dst[1] = n - 1; src[1] = col[rowptr[n - 1]] if rowptr[n] > rowptr[n - 1] else 0
    filt = R.filter_rows(np.concatenate([rng.randint(0, n, size=(2, n)), [[src[2], src[3]], [n - 1, n - 1]]], axis=1), n)
    for kind in W.KINDS:
        w, a, mode = W.params(rowptr, kind)
        want = W.ranks(rowptr, col, src, dst, 3, a, w, mode, filt)
        _assert_ranks(_gpu_rank(rowptr, col, src, dst, 3, a, w, mode, filt), want)
        assert np.array_equal(_gpu_score(rowptr, col, src, dst, 3, a, w, mode), want[0])


def test_more_queries_than_blocks_on_both_storage_paths():
    """A block takes several queries once there are more than the grid holds: 1,024 resident blocks on the workspace path (1,100 queries
    from 8 sources), 65,536 blocks on the LDS path (65,543 explicit pairs on a 5-node path, where runs of equal sources also form)."""
    n = L.lib().gmp_lp_walk_lds_nodes() + 1
    assert L.lib().gmp_lp_walk_resident_blocks() < 1100
    rng = np.random.RandomState(77)
    rowptr, col = R.simple_csr(rng.randint(0, n, size=(2, 2 * n)), n)
    pool = rng.randint(0, n, size=8)
    src = pool[rng.randint(0, 8, size=1100)]
    dst = rng.randint(0, n, size=1100)
    near = np.nonzero(np.diff(rowptr)[src] > 0)[0][:550]                         # half the destinations next to their source: a score above 0
    dst[near] = col[rowptr[src[near]]]
    w, a, mode = W.params(rowptr, "ppr")
    want = W.ranks(rowptr, col, src, dst, 2, a, w, mode)
    assert (want[0] > 0).sum() > 100
    _assert_ranks(_gpu_rank(rowptr, col, src, dst, 2, a, w, mode), want)
    assert np.array_equal(_gpu_score(rowptr, col, src, dst, 2, a, w, mode), want[0])
    rowptr, col = R.simple_csr([[0, 1, 2, 3], [1, 2, 3, 4]], 5)
    src, dst = rng.randint(-1, 6, size=65543), rng.randint(-1, 6, size=65543)          # (with endpoints outside the graph)
    for mode in ("sum", "hops"):
        assert np.array_equal(_gpu_score(rowptr, col, src, dst, 3, 0.5, None, mode), W.pair_scores(rowptr, col, src, dst, 3, 0.5, None, mode))


# ---------------------------------------------------------------------------- 3. the add order
def test_rows_fold_in_ascending_z():
    """0, 1 and 5 are each joined to 2 < 3 < 4, w = [1, .5, 2^24, 1, 1, .5, .5], damping 1, two rounds from 0: y_1 = e_2 + e_3 + e_4 and
    y_2[1] = ((0 + 2^24) + 1) + 1 = 2^24 in float32 (each + 1 is a tie that rounds to even); any other order gives 2^24 + 2."""
    n = 7
    rowptr, col = R.simple_csr([[0, 0, 0, 1, 1, 1, 5, 5, 5], [2, 3, 4, 2, 3, 4, 2, 3, 4]], n)
    w = np.asarray([1.0, 0.5, 2.0 ** 24, 1.0, 1.0, 0.5, 0.5], dtype=np.float32)
    acc = _gpu_score(rowptr, col, np.zeros(n, dtype=np.int64), np.arange(n), 2, 1.0, w)
    assert acc.tolist() == [16777216.0, 16777216.0, 1.0, 1.0, 1.0, 16777216.0, 0.0]
    assert np.array_equal(acc, W.walk_acc(rowptr, col, [0], 2, 1.0, w)[0])
    st, ng, ne = _gpu_rank(rowptr, col, [0], [1], 2, 1.0, w)
    # candidate 5 has the true pair's bits: equal, not greater
    assert (st.tolist(), ng.tolist(), ne.tolist()) == ([16777216.0], [0], [1])
    want = W.ranks(rowptr, col, [0], [1], 2, 1.0, w)
    assert (want[0].tolist(), want[1].tolist(), want[2].tolist()) == ([16777216.0], [0], [1])


# ---------------------------------------------------------------------------- 4. subnormals
def test_subnormals_are_kept_and_hops_do_not_read_them():
    """A path 0 - 1 - ... - 6 plus the isolated node 7, damping 2^-26, five rounds from 0: acc[5] = 2^-130, a float32 subnormal."""
    rowptr, col = R.simple_csr([list(range(6)), list(range(1, 7))], 8)
    a = 2.0 ** -26
    acc = _gpu_score(rowptr, col, np.zeros(8, dtype=np.int64), np.arange(8), 5, a)
    assert acc[5] == np.float32(2.0 ** -130) and acc[5] != 0.0                   # kept, not flushed
    assert acc.tobytes() == W.walk_acc(rowptr, col, [0], 5, a)[0].tobytes()
    assert acc[6] == 0.0 and acc[7] == 0.0
    got = _gpu_rank(rowptr, col, [0, 0, 0], [5, 6, 7], 5, a)
    _assert_ranks(got, W.ranks(rowptr, col, [0, 0, 0], [5, 6, 7], 5, a))
    assert got[1].tolist() == [4, 5, 5] and got[2].tolist() == [0, 1, 1]         # 5 is above 6 and 7, which tie at 0
    hops = _gpu_score(rowptr, col, np.zeros(8, dtype=np.int64), np.arange(8), 5, mode="hops")
    assert hops.tolist() == [0.0, -1.0, -2.0, -3.0, -4.0, -5.0, -6.0, -6.0]


# ---------------------------------------------------------------------------- 7. the two modes agree on what is reached
def test_walk_sum_is_positive_exactly_within_reach():
    """With damping 1/2 and four rounds nothing underflows: acc[c] > 0 exactly where dist(s, c) <= 4 (c != s: an isolated source does
    not return to itself)."""
    edges, rowptr, col, _, _, _ = _big()
    sources = np.asarray([HUB, 690, 695, 17, 333, 689])
    cand = np.arange(N_BIG)
    s, c = np.repeat(sources, N_BIG), np.tile(cand, len(sources))
    acc = _gpu_score(rowptr, col, s, c, 4, 0.5).reshape(len(sources), N_BIG)
    hops = _gpu_score(rowptr, col, s, c, 4, mode="hops").reshape(len(sources), N_BIG)
    other = cand[None, :] != sources[:, None]
    assert np.array_equal((acc > 0) & other, (hops >= -4.0) & other)
    assert 0 < int(((hops == -5.0) & other).sum()) and 0 < int(((hops >= -4.0) & other).sum())
    assert bool((hops[np.arange(len(sources)), sources] == 0.0).all()) and bool((hops[2][cand != 695] == -5.0).all())
    for i, src in enumerate(sources.tolist()):
        assert np.array_equal(-hops[i], W.cut_dist(W.hop_dist(rowptr, col, src), 4).astype(np.float32))


# ---------------------------------------------------------------------------- 9. what is accepted and what is refused
def _raw(fn, *args):
    return getattr(L.lib(), fn)(*args)


def test_argument_errors_and_empty_inputs():
    edges, rowptr, col, src, dst, _ = _big()
    rp, cl, s, d = _t(rowptr, torch.int32), _t(col, torch.int32), _t(src, torch.int64), _t(dst, torch.int64)
    w = torch.ones(N_BIG, device=DEV)
    out, ng, ne = torch.empty(97, device=DEV), torch.empty(97, dtype=torch.int32, device=DEV), torch.empty(97, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())                   # noqa: E731
    nnz = cl.numel()

    def score(n=N_BIG, nnz_=nnz, P=97, weight=None, damping=0.5, rounds=3, mode=0, rowptr_=rp, col_=cl, src_=s, out_=out, ws=None, wsb=0):
        return _raw("gmp_lp_walk_score", p(rowptr_), p(col_), n, nnz_, p(src_), p(d), P, p(weight), damping, rounds, mode, p(out_), p(ws), wsb, None)

    def rank(n=N_BIG, nnz_=nnz, Q=97, weight=None, damping=0.5, rounds=3, mode=0, rowptr_=rp, col_=cl, dst_=d, ng_=ng, frow=None, fcol=None,
             fnnz=0, ws=None, wsb=0):
        return _raw("gmp_lp_walk_rank", p(rowptr_), p(col_), n, nnz_, p(s), p(dst_), Q, p(weight), damping, rounds, mode, p(frow), p(fcol), fnnz,
                    p(out), p(ng_), p(ne), p(ws), wsb, None)

    for call in (score, rank):
        for kw in (dict(rounds=0), dict(rounds=65), dict(rounds=-3), dict(damping=float("nan")), dict(damping=0.0), dict(damping=-0.5),
                   dict(damping=1.5), dict(damping=float("inf")), dict(weight=w, mode=1), dict(mode=2), dict(mode=-1), dict(n=2 ** 31), dict(n=-1),
                   dict(nnz_=2 ** 31), dict(nnz_=-1), dict(rowptr_=None), dict(col_=None)):
            assert call(**kw) == GMP_ERR_ARG, (call.__name__, kw)
    for rc in (score(P=-1), score(src_=None), score(out_=None), rank(Q=-1), rank(dst_=None), rank(ng_=None), rank(fnnz=-1),
               rank(frow=rp, fcol=None, fnnz=3), rank(frow=None, fcol=cl, fnnz=3)):
        assert rc == GMP_ERR_ARG
    # beyond the LDS limit the vectors need the workspace: an edgeless graph of lds_nodes + 1 nodes
    big = L.lib().gmp_lp_walk_lds_nodes() + 1
    rp_big = torch.zeros(big + 1, dtype=torch.int32, device=DEV)
    need = L.lib().gmp_lp_walk_workspace_bytes(97, big)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    for call in (score, rank):
        assert call(n=big, nnz_=0, rowptr_=rp_big, col_=None) == GMP_ERR_ARG                         # none
        assert call(n=big, nnz_=0, rowptr_=rp_big, col_=None, ws=ws, wsb=need - 1) == GMP_ERR_ARG    # too small
        assert call(n=big, nnz_=0, rowptr_=rp_big, col_=None, ws=ws, wsb=need) == 0
    torch.cuda.synchronize()
    assert out.tolist() == [0.0] * 97 and ng.tolist() == [0] * 97 and bool((ne >= big - 2).all())   # nobody is reached: every candidate ties
    assert score(P=0) == 0 and rank(Q=0) == 0                                    # nothing to do, nothing launched
    assert score(damping=float("nan"), mode=1) == 0 and rank(damping=-1.0, mode=1) == 0             # hops do not read the damping
    assert score(damping=1.0) == 0 and rank(rounds=64, damping=2.0 ** -20) == 0
    torch.cuda.synchronize()
    with pytest.raises(GnnmpError, match="mode"):
        ops.lp_walk_score(rp, cl, s, d, 3, mode="katz")
    with pytest.raises(GnnmpError, match="rounds"):
        ops.lp_walk_rank(rp, cl, s, d, 65)
    with pytest.raises(GnnmpError, match="damping"):
        ops.lp_walk_score(rp, cl, s, d, 3, damping=0.0)
    with pytest.raises(GnnmpError, match="damping"):
        ops.lp_walk_rank(rp, cl, s, d, 3, damping=float("nan"))
    with pytest.raises(GnnmpError, match="hops take no weight"):
        ops.lp_walk_rank(rp, cl, s, d, 3, weight=w, mode="hops")
    with pytest.raises(GnnmpError, match="weight has"):
        ops.lp_walk_score(rp, cl, s, d, 3, weight=w[:-1].contiguous())
    with pytest.raises(GnnmpError, match="differ in length"):
        ops.lp_walk_rank(rp, cl, s, d[:-1].contiguous(), 3)
    with pytest.raises(GnnmpError, match="go together"):
        ops.lp_walk_rank(rp, cl, s, d, 3, filter_rowptr=rp)
    with pytest.raises(GnnmpError):
        ops.lp_walk_score(rp.cpu(), cl, s, d, 3)
    with pytest.raises(ValueError):
        LW.walk_ranks(_t(edges, torch.int64), N_BIG, _t(np.stack([src, dst]), torch.int64), "cn", 3)
    empty = torch.empty(0, dtype=torch.int64, device=DEV)
    assert ops.lp_walk_score(rp, cl, empty, empty, 3).shape == (0,)
    st, g, e = ops.lp_walk_rank(rp, cl, empty, empty, 3)
    assert st.shape == g.shape == e.shape == (0,) and g.dtype == torch.int32
    # a pair outside the graph scores 0 / -(R + 1)
    assert _gpu_score(rowptr, col, [-1, 3, N_BIG], [3, N_BIG + 5, -7], 3, 0.5).tolist() == [0.0, 0.0, 0.0]
    assert _gpu_score(rowptr, col, [-1, 3, N_BIG], [3, N_BIG + 5, -7], 3, mode="hops").tolist() == [-4.0, -4.0, -4.0]
    st, g, e = _gpu_rank(rowptr, col, [N_BIG + 1], [3], 3, mode="hops")         # as a query: every candidate but the destination ties
    assert (st.tolist(), g.tolist(), e.tolist()) == ([-4.0], [0], [N_BIG - 1])


# ---------------------------------------------------------------------------- 10. the command-line path
METRICS = ("mrr", "hits@1", "hits@10", "hits@50")
WALK_KEYS = [f"test/{kind}_{m}" for kind in W.KINDS for m in METRICS]


def test_cli_lp_walks_logs_the_twelve_keys_and_leaves_training_alone(tmp_path, monkeypatch):
    """python -m gnn_pretraining_amd.finetune.finetune ... --lp-walks 4 (no engine), in process: one epoch on the synthetic Cora_LP
    stand-in.  The test record carries the 12 keys, each the ranking_metrics of the reference's ranks on the dataset's own edges; with
    --lp-engine the same values, and the checkpoint and every other test key are those of the same run without the flag."""
    from gnn_pretraining_amd.data.finetune_data_loaders import create_finetune_data_loader
    rec, _ = _run_cli(tmp_path, monkeypatch, "with", ["--lp-walks", "4"])
    test = [r for r in rec if WALK_KEYS[0] in r]
    assert len(test) == 1 and "test/auc" in test[0] and all(k in test[0] for k in WALK_KEYS)
    assert not any(k.split("/")[-1].split("_")[0] in W.KINDS + R.KINDS for r in rec if r is not test[0] for k in r)
    assert not any(k.split("/")[-1].split("_")[0] in R.KINDS for k in test[0])   # no --lp-heuristics: none of its keys
    sets = {sp: create_finetune_data_loader("Cora_LP", sp, 32, torch.Generator(), tmp_path / "data").dataset for sp in ("train", "val", "test")}
    n = sets["train"].data.num_nodes
    train, pos = sets["train"].train_edges.numpy(), sets["test"].pos_edges.numpy()
    known = np.concatenate([train, sets["val"].pos_edges.numpy(), pos], axis=1)
    rowptr, col = R.simple_csr(train, n)                                         # the message-passing graph: the train split alone
    filt = R.filter_rows(np.concatenate([known, known[::-1]], axis=1), n)
    for kind in W.KINDS:
        w, a, mode = W.params(rowptr, kind)
        _, ng, ne = W.ranks(rowptr, col, pos[0], pos[1], 4, a, w, mode, filt)
        for m, v in ranking_metrics(R.rank_of(ng, ne)).items():
            assert test[0][f"test/{kind}_{m}"] == v, (kind, m)
    assert set(ranking_metrics(R.rank_of(ng, ne))) == set(METRICS)
    # on the engine, whose dropout stream is its own: the same 12 values -- they do not depend on the model -- and the checkpoint of the
    # run without the flag, bit for bit
    rec1, state1 = _run_cli(tmp_path, monkeypatch, "engine_with", ["--lp-engine", "--lp-walks", "4"])
    rec0, state0 = _run_cli(tmp_path, monkeypatch, "engine_without", ["--lp-engine"])
    test1 = [r for r in rec1 if WALK_KEYS[0] in r]
    assert len(test1) == 1 and all(test1[0][k] == test[0][k] for k in WALK_KEYS)
    assert not any(k in r for r in rec0 for k in WALK_KEYS)
    assert state1.keys() == state0.keys() and all(torch.equal(state1[k], state0[k]) for k in state1)
    test0 = [r for r in rec0 if "test/auc" in r][0]
    assert set(test1[0]) == set(test0) | set(WALK_KEYS)
    for k, v in test0.items():
        assert k == "test/training_time" or test1[0][k] == v or (v != v and test1[0][k] != test1[0][k]), k


def test_cli_lp_walks_next_to_lp_heuristics_logs_all_28_keys(tmp_path, monkeypatch):
    both, _ = _run_cli(tmp_path, monkeypatch, "both", ["--lp-heuristics", "--lp-walks", "4"])
    heur, _ = _run_cli(tmp_path, monkeypatch, "heur", ["--lp-heuristics"])
    heur_keys = [f"test/{kind}_{m}" for kind in R.KINDS for m in METRICS]
    test = [r for r in both if WALK_KEYS[0] in r]
    assert len(test) == 1 and all(k in test[0] for k in WALK_KEYS + heur_keys) and len(set(WALK_KEYS + heur_keys)) == 28
    alone = [r for r in heur if heur_keys[0] in r][0]
    assert all(test[0][k] == alone[k] for k in heur_keys)                        # the 16 keys of --lp-heuristics are unchanged
    assert not any(k in alone for k in WALK_KEYS)
