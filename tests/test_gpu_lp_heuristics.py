"""The structural link baselines on the GPU (csrc/lp_heuristics.hip: ops.lp_cn_score / lp_cn_rank / graph_simple_check,
finetune/link_heuristics.py, --lp-heuristics) against the CPU reference of tests/lp_heur_ref.py.  Scores are float32 sums in a fixed
order and counts are integers, so everything is compared for EQUALITY; only Jaccard's float quotient, which no comparison reads, gets
one float32 ulp around the float64 quotient (IEEE division is within half an ulp; the margin allows one that is not correctly rounded)."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import lp_heur_ref as R
from link_rank_util import N_BIG, big as _big, filter_csr as _filter_csr, run_cli as _run_cli, t as _t
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd._lib import GnnmpError
from gnn_pretraining_amd.finetune import link_heuristics as LH
from gnn_pretraining_amd.finetune.metrics import ranking_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
GMP_ERR_ARG = -1


def _mode(kind):
    return "jaccard" if kind == "jaccard" else "sum"


def _gpu_rank(rowptr, col, src, dst, w=None, mode="sum", filt_rows=None):
    n = len(rowptr) - 1
    fr, fc = _filter_csr(filt_rows, n) if filt_rows is not None else (None, None)
    out = ops.lp_cn_rank(_t(rowptr, torch.int32), _t(col, torch.int32), _t(src, torch.int64), _t(dst, torch.int64),
                         None if w is None else _t(w, torch.float32), mode, fr, fc)
    return tuple(t.cpu().numpy() for t in out)


def _gpu_score(rowptr, col, src, dst, w=None, mode="sum"):
    return ops.lp_cn_score(_t(rowptr, torch.int32), _t(col, torch.int32), _t(src, torch.int64), _t(dst, torch.int64),
                           None if w is None else _t(w, torch.float32), mode).cpu().numpy()


def _assert_scores(got, want, mode):
    assert got.dtype == np.float32
    if mode == "jaccard":
        assert bool(np.all(np.abs(got.astype(np.float64) - want) <= np.spacing(want.astype(np.float32)).astype(np.float64))), (got, want)
    else:
        assert np.array_equal(got.astype(np.float64), want), (got, want)


def _assert_ranks(got, want, mode):
    _assert_scores(got[0], want[0], mode)
    assert got[1].dtype == np.int32 and got[2].dtype == np.int32
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1], want[1], got[2], want[2])


# ---------------------------------------------------------------------------- 1. the four kinds on a seeded random graph
@functools.lru_cache(maxsize=None)
def _big_ref(kind, filtered):
    edges, rowptr, col, src, dst, known = _big()
    return R.ranks(rowptr, col, src, dst, R.weights(rowptr, kind), _mode(kind), R.filter_rows(known, N_BIG) if filtered else None)


@pytest.mark.parametrize("filtered", [False, True])
@pytest.mark.parametrize("kind", R.KINDS)
def test_four_kinds_against_the_reference_on_a_random_graph(kind, filtered):
    edges, rowptr, col, src, dst, known = _big()
    want = _big_ref(kind, filtered)
    if not filtered:                                                             # the reference is not vacuous
        assert (want[1] > 0).sum() > 20 and (want[2] > 0).sum() > 20 and (want[0] > 0).sum() > 20
    graph, pairs = _t(edges, torch.int64), _t(np.stack([src, dst]), torch.int64)
    rp, cl = LH.simple_graph(graph, N_BIG)
    assert np.array_equal(rp.cpu().numpy(), rowptr) and np.array_equal(cl.cpu().numpy(), col) and rp.dtype == torch.int32
    ranks = LH.heuristic_ranks(graph, N_BIG, pairs, kind, filter_edges=_t(known, torch.int64) if filtered else None)
    _assert_ranks((ranks.logit.cpu().numpy(), ranks.n_greater.cpu().numpy(), ranks.n_equal.cpu().numpy()), want, _mode(kind))
    assert np.array_equal(ranks.rank.cpu().numpy().astype(np.float64), R.rank_of(want[1], want[2]))
    scores = LH.heuristic_scores(graph, N_BIG, pairs, kind).cpu().numpy()
    assert np.array_equal(scores, ranks.logit.cpu().numpy())                     # the pair scorer IS score_true
    assert LH.simple_graph(graph, N_BIG)[0] is rp                                # cached per tensor


# ---------------------------------------------------------------------------- 2. tile boundaries
def _tile_sizes():
    tc = L.lib().gmp_lp_cn_tile_nodes()
    return [2, 3, 65, tc - 1, tc, tc + 1, 2 * tc + 3]


@pytest.mark.parametrize("which", range(7))
def test_tile_boundaries(which):
    n = _tile_sizes()[which]
    rng = np.random.RandomState(100 + which)
    edges = rng.randint(0, n, size=(2, 3 * n))
    rowptr, col = R.simple_csr(edges, n)
    src, dst = rng.randint(0, n, size=50), rng.randint(0, n, size=50)
    for i in range(2, 26):                                                       # half the destinations at distance two: a score above 0
        if rowptr[src[i] + 1] > rowptr[src[i]]:
            z = col[rowptr[src[i]]]
            dst[i] = col[rowptr[z + 1] - 1]
    dst[0] = n - 1                                                              # a true destination and a filter entry in the last (partial) tile
    dst[1] = n - 1; src[1] = col[rowptr[n - 1]] if rowptr[n] > rowptr[n - 1] else 0
    filt = R.filter_rows(np.concatenate([rng.randint(0, n, size=(2, n)), [[src[0], src[1]], [max(n - 2, 0), max(n - 2, 0)]]], axis=1), n)
    for kind in ("cn", "aa", "jaccard"):
        w = R.weights(rowptr, kind)
        want = R.ranks(rowptr, col, src, dst, w, _mode(kind), filt)
        _assert_ranks(_gpu_rank(rowptr, col, src, dst, w, _mode(kind), filt), want, _mode(kind))


# ---------------------------------------------------------------------------- 3. the add order
def test_sums_add_in_ascending_z():
    """0, 1 and 5 share the neighbours 2 < 3 < 4 with weights 2^24, 1, 1: ((0 + 2^24) + 1) + 1 is 2^24 in float32 (each + 1 is a tie that
    rounds to even), any other order gives 2^24 + 2."""
    n = 7
    rowptr, col = R.simple_csr([[0, 0, 0, 1, 1, 1, 5, 5, 5], [2, 3, 4, 2, 3, 4, 2, 3, 4]], n)
    w = np.asarray([0.5, 0.5, 2.0 ** 24, 1.0, 1.0, 0.5, 0.5], dtype=np.float32)
    assert _gpu_score(rowptr, col, [0, 1, 5], [1, 0, 0], w).tolist() == [16777216.0] * 3
    st, ng, ne = _gpu_rank(rowptr, col, [0, 0], [1, 6], w)
    assert st.tolist() == [16777216.0, 0.0]
    # candidate 5 of the first query has the true pair's bits: equal, not greater; against (0, 6) candidates 1 and 5 are above, 2, 3, 4 tie
    assert (ng.tolist(), ne.tolist()) == ([0, 2], [1, 3])
    want = R.ranks(rowptr, col, [0, 0], [1, 6], w)
    assert (want[0].tolist(), want[1].tolist(), want[2].tolist()) == ([16777216.0, 0.0], [0, 2], [1, 3])


# ---------------------------------------------------------------------------- 6. Jaccard is compared in integers
def test_jaccard_equal_quotients_from_different_counts_tie():
    """J(0, 3) = 1 / 2 and J(0, 4) = 2 / 4."""
    rowptr, col = R.simple_csr([[0, 0, 3, 4, 4, 4, 4], [1, 2, 1, 1, 2, 5, 6]], 8)
    st, ng, ne = _gpu_rank(rowptr, col, [0], [3], None, "jaccard")
    assert (st.tolist(), ng.tolist(), ne.tolist()) == ([0.5], [0], [1])
    want = R.ranks(rowptr, col, [0], [3], None, "jaccard")
    assert (want[1].tolist(), want[2].tolist()) == ([0], [1])


@functools.lru_cache(maxsize=None)
def _close_quotients():
    """Node 0 has the 16,384 neighbours 10 .. 16,393.  Node 1 takes the first 8,192 of them and one more node: J(0, 1) = 8192 / 16385.
    Node 2 takes the first 8,193 and three more: J(0, 2) = 8193 / 16387.  8193 * 16385 - 8192 * 16387 = 1: node 2 is ahead, by 3.7e-9, an
    eighth of the float32 spacing at 0.5 -- the two quotients are one float32."""
    a = np.arange(10, 10 + 16384)
    e = [np.stack([np.zeros_like(a), a]), np.stack([np.ones(8192, dtype=np.int64), a[:8192]]), np.asarray([[1], [3]]),
         np.stack([np.full(8193, 2), a[:8193]]), np.asarray([[2, 2, 2], [4, 5, 6]])]
    n = 10 + 16384
    rowptr, col = R.simple_csr(np.concatenate(e, axis=1), n)
    return rowptr, col, n


def test_jaccard_quotients_closer_than_float32_are_still_ordered():
    rowptr, col, n = _close_quotients()
    assert np.float32(8192 / 16385) == np.float32(8193 / 16387) and 8193 * 16385 > 8192 * 16387
    src, dst = [0, 0], [1, 2]
    want = R.ranks(rowptr, col, src, dst, None, "jaccard")
    assert want[1].tolist() == [1, 0] and want[2].tolist() == [0, 0]             # 2 is above 1; nothing is above or level with 2
    got = _gpu_rank(rowptr, col, src, dst, None, "jaccard")
    _assert_ranks(got, want, "jaccard")


# ---------------------------------------------------------------------------- 8. what is accepted and what is refused
def test_simple_graph_cleans_a_messy_edge_list():
    messy = torch.tensor([[3, 3, 1, 2, 2, 0, 4, 3], [1, 1, 3, 2, 0, 2, 0, 3]], device=DEV)        # doubled, both ways, loops, one way only
    rowptr, col = LH.simple_graph(messy, 6)
    assert rowptr.tolist() == [0, 2, 3, 4, 5, 6, 6] and col.tolist() == [2, 4, 3, 0, 1, 0]
    assert ops.graph_simple_check(rowptr, col).item() == 0
    with pytest.raises(GnnmpError, match="outside"):
        LH.simple_graph(torch.tensor([[0], [6]], device=DEV), 6)
    with pytest.raises(GnnmpError):
        LH.simple_graph(torch.tensor([[0], [1]], device=DEV, dtype=torch.int32), 6)
    with pytest.raises(ValueError):
        LH.heuristic_scores(messy, 6, messy, "katz")


def _violations(rowptr, col):
    return int(ops.graph_simple_check(_t(rowptr, torch.int32), _t(col, torch.int32)).item())


def test_graph_simple_check_counts_planted_violations():
    """Dirty graphs go to the checker only."""
    edges, rowptr, col, _, _, _ = _big()
    assert _violations(rowptr, col) == 0
    v = 5
    b, e = int(rowptr[v]), int(rowptr[v + 1])
    assert e - b >= 2
    bump = np.concatenate([rowptr[:v + 1], rowptr[v + 1:] + 1])
    at = b + int(np.searchsorted(col[b:e], v))
    assert _violations(bump, np.insert(col, at, v)) == 1                          # a self-loop, in order
    assert _violations(bump, np.insert(col, b, col[b])) == 1                      # a duplicate
    swapped = col.copy()
    swapped[[b, b + 1]] = swapped[[b + 1, b]]
    assert _violations(rowptr, swapped) >= 1                                      # an unsorted pair (and the mirrors a search now misses)
    drop = np.concatenate([rowptr[:v + 1], rowptr[v + 1:] - 1])
    assert _violations(drop, np.delete(col, b)) == 1                              # (col[b], v) is left without (v, col[b])
    beyond = col.copy()
    beyond[e - 1] = N_BIG
    assert _violations(rowptr, beyond) == 2                                       # out of range, and the neighbour it replaced lost its mirror
    assert _violations(np.concatenate([rowptr[:-1], rowptr[-1:] + 1]), np.append(col, 0)) == 1    # the isolated last node points at 0, one way


def _raw(fn, *args):
    return getattr(L.lib(), fn)(*args)


def test_argument_errors_and_empty_inputs():
    edges, rowptr, col, src, dst, _ = _big()
    rp, cl, s, d = _t(rowptr, torch.int32), _t(col, torch.int32), _t(src, torch.int64), _t(dst, torch.int64)
    w = torch.ones(N_BIG, device=DEV)
    out, ng, ne = torch.empty(97, device=DEV), torch.empty(97, dtype=torch.int32, device=DEV), torch.empty(97, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())                   # noqa: E731
    nnz, tc = cl.numel(), L.lib().gmp_lp_cn_tile_nodes()

    def score(n=N_BIG, P=97, weight=None, mode=0, rowptr_=rp, src_=s, out_=out):
        return _raw("gmp_lp_cn_score", p(rowptr_), p(cl), n, nnz, p(src_), p(d), P, p(weight), mode, p(out_), None)

    def rank(n=N_BIG, Q=97, weight=None, mode=0, dst_=d, ng_=ng, frow=None, fcol=None, fnnz=0):
        return _raw("gmp_lp_cn_rank", p(rp), p(cl), n, nnz, p(s), p(dst_), Q, p(weight), mode, p(frow), p(fcol), fnnz, p(out), p(ng_), p(ne),
                    None, 0, None)

    for rc in (score(mode=2), score(mode=-1), score(weight=w, mode=1), score(n=2 ** 31), score(n=-1), score(P=-1), score(rowptr_=None),
               score(src_=None), score(out_=None),
               rank(mode=2), rank(weight=w, mode=1), rank(n=2 ** 31), rank(Q=-1), rank(dst_=None), rank(ng_=None),
               rank(n=tc, Q=2 ** 31), rank(frow=rp, fcol=None, fnnz=3),
               _raw("gmp_graph_simple_check", p(rp), p(cl), N_BIG, nnz, None, None),
               _raw("gmp_graph_simple_check", None, p(cl), N_BIG, nnz, p(ng), None)):
        assert rc == GMP_ERR_ARG
    assert score(P=0) == 0 and rank(Q=0) == 0                                    # nothing to do, nothing launched
    torch.cuda.synchronize()
    with pytest.raises(GnnmpError, match="mode"):
        ops.lp_cn_score(rp, cl, s, d, mode="katz")
    with pytest.raises(GnnmpError, match="Jaccard"):
        ops.lp_cn_rank(rp, cl, s, d, weight=w, mode="jaccard")
    with pytest.raises(GnnmpError, match="weight has"):
        ops.lp_cn_score(rp, cl, s, d, weight=w[:-1].contiguous())
    with pytest.raises(GnnmpError, match="differ in length"):
        ops.lp_cn_rank(rp, cl, s, d[:-1].contiguous())
    with pytest.raises(GnnmpError, match="go together"):
        ops.lp_cn_rank(rp, cl, s, d, filter_rowptr=rp)
    with pytest.raises(GnnmpError):
        ops.lp_cn_score(rp.cpu(), cl, s, d)
    empty = torch.empty(0, dtype=torch.int64, device=DEV)
    assert ops.lp_cn_score(rp, cl, empty, empty).shape == (0,)
    st, g, e = ops.lp_cn_rank(rp, cl, empty, empty)
    assert st.shape == g.shape == e.shape == (0,) and g.dtype == torch.int32
    # a pair outside the graph scores 0 (and, as a query, has no neighbours: every candidate ties at 0)
    assert _gpu_score(rowptr, col, [-1, 3, N_BIG], [3, N_BIG + 5, -7]).tolist() == [0.0, 0.0, 0.0]


# ---------------------------------------------------------------------------- 9. the command-line path
def test_cli_lp_heuristics_logs_the_sixteen_keys_and_leaves_training_alone(tmp_path, monkeypatch):
    """python -m gnn_pretraining_amd.finetune.finetune ... --lp-heuristics (no engine), in process: one epoch on the synthetic Cora_LP
    stand-in.  The test record carries the 16 baseline keys, each the ranking_metrics of the reference's ranks on the dataset's own
    edges; with --lp-engine the same values, and the checkpoint is bitwise the one of the same run without the flag."""
    from gnn_pretraining_amd.data.finetune_data_loaders import create_finetune_data_loader
    rec, _ = _run_cli(tmp_path, monkeypatch, "with", ["--lp-heuristics"])
    keys = [f"test/{kind}_{m}" for kind in LH.KINDS for m in ("mrr", "hits@1", "hits@10", "hits@50")]
    test = [r for r in rec if keys[0] in r]
    assert len(test) == 1 and "test/auc" in test[0] and all(k in test[0] for k in keys)
    assert not any(k.split("/")[-1].split("_")[0] in LH.KINDS for r in rec if r is not test[0] for k in r)
    sets = {sp: create_finetune_data_loader("Cora_LP", sp, 32, torch.Generator(), tmp_path / "data").dataset for sp in ("train", "val", "test")}
    n = sets["train"].data.num_nodes
    train, pos = sets["train"].train_edges.numpy(), sets["test"].pos_edges.numpy()
    known = np.concatenate([train, sets["val"].pos_edges.numpy(), pos], axis=1)
    rowptr, col = R.simple_csr(train, n)                                         # the message-passing graph: the train split alone
    filt = R.filter_rows(np.concatenate([known, known[::-1]], axis=1), n)
    for kind in LH.KINDS:
        _, ng, ne = R.ranks(rowptr, col, pos[0], pos[1], R.weights(rowptr, kind), _mode(kind), filt)
        for m, v in ranking_metrics(R.rank_of(ng, ne)).items():
            assert test[0][f"test/{kind}_{m}"] == v, (kind, m)
    # on the engine, whose dropout stream is its own (two module-path runs in one process share a global counter and differ anyway):
    # the same 16 values -- they do not depend on the model -- and the checkpoint of the run without the flag, bit for bit
    rec1, state1 = _run_cli(tmp_path, monkeypatch, "engine_with", ["--lp-engine", "--lp-heuristics"])
    rec0, state0 = _run_cli(tmp_path, monkeypatch, "engine_without", ["--lp-engine"])
    test1 = [r for r in rec1 if keys[0] in r]
    assert len(test1) == 1 and all(test1[0][k] == test[0][k] for k in keys)
    assert not any(k in r for r in rec0 for k in keys)
    assert state1.keys() == state0.keys() and all(torch.equal(state1[k], state0[k]) for k in state1)
    for k, v in [r for r in rec0 if "test/auc" in r][0].items():
        assert k == "test/training_time" or test1[0][k] == v or (v != v and test1[0][k] != test1[0][k]), k
