"""The four all-candidate link rankers (ops.lp_rank, lp_cn_rank, lp_walk_rank, emb_link_rank) under ONE statement of their protocol:
link_rank_ref.candidates says who is a candidate, and each family's own explicit pair scorer says what a score is.  Counts are integers
and a ranker promises its pair scorer's bits, so everything is compared for equality.  Below that, the cases every family has to pass,
once, over the kinds of all three: the filter row's edge cases, counts against explicit pair scores, repeatability."""
import functools

import numpy as np
import pytest
import torch

import link_rank_ref as P
import lp_heur_ref as HR
import lp_walk_ref as WR
from link_rank_util import HUB, N_BIG, big, filter_csr as _filter_csr, t as _t
from gnn_pretraining_amd import ops

pytestmark = pytest.mark.gpu
DEV = "cuda"
N, ROUNDS = 70, 3                       # three 32-candidate tiles of lp_rank and emb_link_rank, the last one partial


# a repeated source, src == dst, a destination outside [0, N); row 3 of the filter unsorted, with a duplicate and entries >= N, row 40 total
SRC, DST = [3, 3, 17, 40, 12, 25], [50, 8, 17, 11, N + 5, 69]
ROWS = {3: [50, 7, 20, 7, N, 2 ** 31 - 1, N + 30, 64, 31, 32], 40: np.random.RandomState(3).permutation(N).tolist(), 41: [1, 2, 3]}


@functools.lru_cache(maxsize=None)
def _families():
    """{name: (rank(src, dst, filter_rowptr, filter_col), score(src, dst))}, each family's two entry points over one set of inputs."""
    rng = np.random.RandomState(70)
    rowptr, col = (_t(a, torch.int32) for a in HR.simple_csr(rng.randint(0, N, size=(2, 4 * N)), N))
    gen = torch.Generator().manual_seed(70)
    h, h5 = torch.randn(N, 256, generator=gen).to(DEV), torch.randn(N, 5, generator=gen).to(DEV)
    w = tuple((torch.randn(*shape, generator=gen) * 0.05).to(DEV) for shape in ((256, 768), (256,), (256,), (1,)))
    out = {"lp_rank": (lambda s, d, fr, fc: ops.lp_rank(h, s, d, *w, fr, fc), lambda s, d: ops.lp_score_fwd(h, s, d, *w, 0.0, 0, 0)[1])}
    for mode in ("sum", "jaccard"):
        out[f"lp_cn_rank/{mode}"] = (lambda s, d, fr, fc, m=mode: ops.lp_cn_rank(rowptr, col, s, d, None, m, fr, fc),
                                     lambda s, d, m=mode: ops.lp_cn_score(rowptr, col, s, d, None, m))
    for mode in ("sum", "hops"):
        out[f"lp_walk_rank/{mode}"] = (lambda s, d, fr, fc, m=mode: ops.lp_walk_rank(rowptr, col, s, d, ROUNDS, 0.5, None, m, fr, fc),
                                       lambda s, d, m=mode: ops.lp_walk_score(rowptr, col, s, d, ROUNDS, 0.5, None, m))
    for mode in ("cos", "dot"):
        out[f"emb_link_rank/{mode}"] = (lambda s, d, fr, fc, m=mode: ops.emb_link_rank(h5, s, d, m, fr, fc),
                                        lambda s, d, m=mode: ops.emb_link_score(h5, s, d, m))
    return out


@pytest.mark.parametrize("family", ["lp_rank", "lp_cn_rank/sum", "lp_cn_rank/jaccard", "lp_walk_rank/sum", "lp_walk_rank/hops",
                                    "emb_link_rank/cos", "emb_link_rank/dot"])
def test_four_rankers_one_protocol(family):
    """n_greater / n_equal of every ranker equal counting, over link_rank_ref's candidate set, the family's own explicit score of the
    source against all 70 destinations; score_true has the bits of the explicit score of the true pair.  (Jaccard's ranker compares
    cn / union exactly in integers while its scorer returns the float32 quotient: with unions below 2 * 70 two different quotients
    differ by more than 1 / 140^2 = 5e-5 relative, far above float32's 6e-8, and equal ones round alike, so the two orders agree here.)"""
    rank, score = _families()[family]
    src, dst = _t(SRC, torch.int64), _t(DST, torch.int64)
    got = tuple(t.cpu().numpy() for t in rank(src, dst, *_filter_csr(ROWS, N)))
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    true = score(src, dst).cpu().numpy()
    every = score(src.repeat_interleave(N), torch.arange(N, device=DEV).repeat(len(SRC))).cpu().numpy().reshape(len(SRC), N)
    want = P.ranks(N, SRC, DST, lambda q, s: every[q], lambda q, s, d, row: true[q], ROWS)
    assert got[0].tobytes() == true.tobytes()
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1], want[1], got[2], want[2])
    assert got[1][3] == 0 and got[2][3] == 0                                       # row 40 filters every candidate
    assert int(want[1].sum() + want[2].sum()) > 0                                  # the comparison is not vacuous
    for q, (s, d) in enumerate(zip(SRC, DST)):                                     # the candidate set, restated
        assert want[1][q] + want[2][q] <= N - len({c for c in [s, d] + ROWS.get(s, []) if 0 <= c < N})


# ---------------------------------------------------------------------------- the cases every family passes, on the 700-node graph
WALK_ROUNDS = {"katz": 4, "ppr": 10, "hops": 4}
EMB_DIM = 24


@functools.lru_cache(maxsize=None)
def _family(kind):
    """(rank(src, dst, rows=None) -> three numpy arrays, score(src, dst) -> numpy, ref(src, dst, rows=None) -> the CPU reference's three,
    exact) of a kind of link_heuristics, link_walks or link_probe on big()'s graph.  rows = {source: destinations}, written into the filter
    CSR verbatim.  The embedding family's reference replays the counting on the kernel's own score matrix; exact is False for Jaccard,
    whose float quotient, which no comparison reads, gets one float32 ulp around the float64 quotient."""
    _, rowptr, col, _, _, _ = big()
    rp, cl = _t(rowptr, torch.int32), _t(col, torch.int32)
    pair = lambda src, dst: (_t(src, torch.int64), _t(dst, torch.int64))                                     # noqa: E731
    csr = lambda rows: (None, None) if rows is None else _filter_csr(rows, N_BIG)                           # noqa: E731
    host = lambda out: tuple(o.cpu().numpy() for o in out)                                                   # noqa: E731
    if kind in HR.KINDS:
        w, mode = HR.weights(rowptr, kind), "jaccard" if kind == "jaccard" else "sum"
        wt = None if w is None else _t(w, torch.float32)
        return (lambda src, dst, rows=None: host(ops.lp_cn_rank(rp, cl, *pair(src, dst), wt, mode, *csr(rows))),
                lambda src, dst: ops.lp_cn_score(rp, cl, *pair(src, dst), wt, mode).cpu().numpy(),
                lambda src, dst, rows=None: HR.ranks(rowptr, col, src, dst, w, mode, rows), mode != "jaccard")
    if kind in WR.KINDS:
        (w, a, mode), rounds = WR.params(rowptr, kind), WALK_ROUNDS[kind]
        wt = None if w is None else _t(w, torch.float32)
        return (lambda src, dst, rows=None: host(ops.lp_walk_rank(rp, cl, *pair(src, dst), rounds, float(a), wt, mode, *csr(rows))),
                lambda src, dst: ops.lp_walk_score(rp, cl, *pair(src, dst), rounds, float(a), wt, mode).cpu().numpy(),
                lambda src, dst, rows=None: WR.ranks(rowptr, col, src, dst, rounds, a, w, mode, rows), True)
    h = torch.randn(N_BIG, EMB_DIM, generator=torch.Generator().manual_seed(24)).to(DEV)

    def replay(src, dst, rows=None):
        mat = ops.emb_link_rank(h, *pair(src, dst), kind, *csr(rows), return_matrix=True)[3].cpu().numpy()
        return P.ranks(N_BIG, src, dst, lambda q, s: mat[q], lambda q, s, d, row: row[d] if 0 <= d < N_BIG else np.float32(0), rows)

    return (lambda src, dst, rows=None: host(ops.emb_link_rank(h, *pair(src, dst), kind, *csr(rows))),
            lambda src, dst: ops.emb_link_score(h, *pair(src, dst), kind).cpu().numpy(), replay, True)


def _assert_ranks(got, want, exact):
    assert got[0].dtype == np.float32 and got[1].dtype == np.int32 and got[2].dtype == np.int32
    score, ref = got[0].astype(np.float64), np.asarray(want[0], dtype=np.float64)
    if exact:
        assert np.array_equal(score, ref), (score, ref)
    else:
        assert bool(np.all(np.abs(score - ref) <= np.spacing(ref.astype(np.float32)).astype(np.float64))), (score, ref)
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (got[1], want[1], got[2], want[2])


@pytest.mark.parametrize("kind", ["cn", "ra", "jaccard", "katz", "ppr", "hops", "cos", "dot"])
def test_filter_rows_unsorted_duplicated_out_of_range_empty_and_total(kind):
    rank, _, ref, exact = _family(kind)
    rng = np.random.RandomState(5)
    src, dst = np.asarray([HUB, 17, 23, 40]), np.asarray([33, 90, 91, 92])
    everyone = rng.permutation(N_BIG).tolist()
    rows = {HUB: [650, 3, 3, 650, -5, N_BIG, N_BIG + 100, HUB, 33, 12, 2 ** 31 - 1, 3] + rng.randint(0, N_BIG, size=40).tolist(),
            17: [],                                                              # an empty row
            23: everyone + everyone[:7],                                         # every candidate filtered: 0 and 0
            41: [1, 2, 3]}                                                       # another source's row is not read
    got = rank(src, dst, rows)
    _assert_ranks(got, ref(src, dst, rows), exact)
    assert got[1][2] == 0 and got[2][2] == 0
    plain = rank(src[[1, 3]], dst[[1, 3]])
    assert np.array_equal(plain[1], got[1][[1, 3]]) and np.array_equal(plain[2], got[2][[1, 3]])


@pytest.mark.parametrize("kind", ["cn", "aa", "ra", "katz", "ppr", "hops", "cos", "dot"])
def test_rank_counts_equal_counting_over_explicit_pairs(kind):
    rank, score, _, _ = _family(kind)
    _, _, _, src, dst, _ = big()
    qs = [0, 10, 13, 15, 20, 40, 70, 91]
    st, ng, ne = rank(src[qs], dst[qs])
    cand = np.arange(N_BIG)
    every = score(np.repeat(src[qs], N_BIG), np.tile(cand, len(qs))).reshape(len(qs), N_BIG)
    for i, q in enumerate(qs):
        valid = (cand != src[q]) & (cand != dst[q])
        assert every[i, dst[q]].tobytes() == st[i].tobytes()
        assert int(((every[i] > st[i]) & valid).sum()) == ng[i] and int(((every[i] == st[i]) & valid).sum()) == ne[i]
    # a pair on its own has the bits it has among all candidates of its source
    assert score(src[qs], dst[qs]).tobytes() == st.tobytes()


@pytest.mark.parametrize("kind", ["aa", "jaccard", "ppr", "hops", "cos", "dot"])
def test_two_calls_and_split_calls_are_bitwise_equal(kind):
    rank = _family(kind)[0]
    _, _, _, src, dst, known = big()
    filt = P.filter_rows(known, N_BIG)
    one, two = (rank(src, dst, filt) for _ in range(2))
    head, tail = (rank(src[sl], dst[sl], filt) for sl in (slice(0, 48), slice(48, None)))
    for a, b, h, t in zip(one, two, head, tail):
        assert a.tobytes() == b.tobytes() and a.tobytes() == np.concatenate([h, t]).tobytes()
