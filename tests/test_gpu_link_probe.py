"""The embedding link probe on the GPU (csrc/emb_link.hip, ops.emb_link_score / emb_link_rank, finetune/link_probe.py, --link-probe)
against tests/link_probe_ref.py: (1) bit-exact on exact arithmetic at every tile width and chunk boundary, (2) the four places a pair's
score appears and gmp_knn_topk's matrix pinned to one another on random rows, (3) float64 with a derived bound and no query left out,
(4) the edges of the contract, (5) planted structure, (6) --link-probe end to end."""
import ctypes as C
import json
import math

import numpy as np
import pytest
import torch

import link_probe_ref as R
from link_rank_util import t as _t
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd.finetune import link_probe as LPR
from gnn_pretraining_amd.finetune.metrics import ranking_metrics

pytestmark = pytest.mark.gpu
DEV = "cuda"
GMP_ERR_ARG, GMP_ERR_WORKSPACE = -1, -3


def _bits(t):
    return t.contiguous().view(torch.int32)


def _exact_rows(n, d, seed):
    """four_ones rows, and from d = 16 on sixteen_signs rows for the second half: norms exactly 2 and 4, every product and sum exact"""
    x = R.four_ones(n, d, seed)
    if d >= 16:
        x[n // 2:] = R.sixteen_signs(n - n // 2, d, seed + 1)
    return x


def _queries(rng, Q, N):
    """random pairs; the first third repeats one source"""
    src, dst = rng.integers(0, N, size=Q), rng.integers(0, N, size=Q)
    src[:Q // 3] = src[0]
    return src.astype(np.int64), dst.astype(np.int64)


def _filter(rng, src, dst, N):
    """[2, E] known pairs on the queries' sources: random destinations some of them outside [0, N), duplicates, (s, s) and (s, dst)"""
    E = 4 * N + 8
    fs, fc = rng.choice(src, size=E), rng.integers(-2, N + 3, size=E)
    k = min(8, src.size)
    fs = np.concatenate([fs, fs[:16], src[:k], src[:k]])
    fc = np.concatenate([fc, fc[:16], src[:k], dst[:k]])
    return np.stack([fs, fc]).astype(np.int64)


def _csr(filt, N):
    """the filter as the kernel takes it: int32 rowptr / col, rows in the order the entries came (unsorted), out-of-range columns kept"""
    s, c = filt
    keep = (s >= 0) & (s < N)
    s, c = s[keep], c[keep]
    order = np.argsort(s, kind="stable")
    rowptr = np.zeros(N + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(np.bincount(s, minlength=N))
    return _t(rowptr, torch.int32), _t(c[order], torch.int32)


def _rank(h, src, dst, mode, filt=None, matrix=False):
    N = h.shape[0]
    rowptr, col = _csr(filt, N) if filt is not None else (None, None)
    out = ops.emb_link_rank(_t(h, torch.float32), _t(src, torch.int64), _t(dst, torch.int64), mode, rowptr, col, return_matrix=matrix)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out]


# ---------------------------------------------------------------------------- 1. exact arithmetic
SHAPES = [(1, 1, 8), (5, 3, 6), (33, 31, 16), (129, 33, 24), (129, 1025, 32), (301, 2500, 40), (301, 2500, 100), (301, 2500, 160), (301, 2500, 256)]


@pytest.mark.parametrize("Q,N,d", SHAPES)
def test_bit_exact_on_exact_arithmetic(Q, N, d):
    rng = np.random.default_rng(1000 * d + N)
    h = _exact_rows(N, d, seed=d + N)
    src, dst = _queries(rng, Q, N)
    filt = _filter(rng, src, dst, N)
    for mode in R.KINDS:
        S = R.scores(h, mode)
        for f in (filt, None):
            want = R.ranks(S, src, dst, f)
            got = _rank(h, src, dst, mode, f)
            assert np.array_equal(got[0].astype(np.float64), want[0]), (mode, f is None)
            assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]), (mode, f is None)
        score = ops.emb_link_score(_t(h, torch.float32), _t(src, torch.int64), _t(dst, torch.int64), mode).cpu().numpy()
        assert np.array_equal(score.astype(np.float64), R.pair_scores(h, src, dst, mode)), mode
        if N >= 31:
            assert int(want[2].max()) > 0                                    # ties are there to be counted


# ---------------------------------------------------------------------------- 2. one chain, four places, and the k-NN scan's
@pytest.mark.parametrize("positive", [False, True])
@pytest.mark.parametrize("Q,N,d", [(300, 1000, 256), (257, 2500, 40), (500, 140, 256)])
def test_cross_pins_on_random_rows(Q, N, d, positive):
    gen = torch.Generator().manual_seed(7 * N + d + positive)
    h = torch.randn(N, d, generator=gen)
    h = (h.abs() if positive else h).numpy()
    rng = np.random.default_rng(N + d)
    src, dst = _queries(rng, Q, N)
    filt = _filter(rng, src, dst, N)
    hd, sd, dd = _t(h, torch.float32), _t(src, torch.int64), _t(dst, torch.int64)
    for mode in R.KINDS:
        st, ng, ne, mat = _rank(h, src, dst, mode, filt, matrix=True)
        assert np.array_equal(st.view(np.int32), mat[np.arange(Q), dst].view(np.int32)), mode
        score = ops.emb_link_score(hd, sd, dd, mode)
        assert torch.equal(_bits(score).cpu(), torch.from_numpy(st.view(np.int32))), mode
        want = R.ranks(None, src, dst, filt, similarity=mat)
        assert np.array_equal(ng, want[1]) and np.array_equal(ne, want[2]), mode
        again = _rank(h, src, dst, mode, filt, matrix=True)                   # the same bits from a second call
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip((st, ng, ne, mat), again)), mode
        plain = _rank(h, src, dst, mode, filt)                                # the matrix hook changes no other bit
        assert all(np.array_equal(a.view(np.int32), b.view(np.int32)) for a, b in zip((st, ng, ne), plain)), mode
        if mode == "cos":
            _, _, knn = ops.knn_topk(hd[sd].contiguous(), hd, 1, return_matrix=True)
            assert torch.equal(_bits(knn).cpu(), torch.from_numpy(mat.view(np.int32)))


# ---------------------------------------------------------------------------- 3. float64, bounded
def _candidates(src, dst, N, filt):
    cand = np.ones((src.size, N), dtype=bool)
    q = np.arange(src.size)
    cand[q, src] = False
    cand[q, dst] = False
    rows = {}
    for s, c in filt.T.tolist():
        if 0 <= c < N:
            rows.setdefault(s, []).append(c)
    for i, s in enumerate(src.tolist()):
        cand[i, np.array(rows.get(s, []), dtype=np.int64)] = False
    return cand


@pytest.mark.parametrize("mode", R.KINDS)
@pytest.mark.parametrize("Q,N,d", [(300, 1000, 256), (257, 2500, 40)])
def test_against_float64_with_a_bound(Q, N, d, mode):
    """cos: |matrix - fp64| < 1e-5, the project's figure for this chain at d <= 256 (test_gpu_knn.py).  dot: elementwise
    (d + 2) 2^-24 sum_k |a_k| |b_k| -- the textbook bound d u sum |a_k b_k| of a length-d fp32 dot product with u = 2^-24, plus two
    roundings for the MFMA's internal pair sum; derived, not measured.  With tol that bound (per query its maximum) a candidate more than
    2 tol above the true score in fp64 must be counted greater, and nothing below t - 2 tol may be counted at all."""
    gen = torch.Generator().manual_seed(N + d)
    h = torch.randn(N, d, generator=gen).numpy()
    rng = np.random.default_rng(N * d)
    src, dst = _queries(rng, Q, N)
    filt = _filter(rng, src, dst, N)
    st, ng, ne, mat = _rank(h, src, dst, mode, filt, matrix=True)
    S64 = R.scores(h, mode)[src]
    err = np.abs(mat.astype(np.float64) - S64)
    if mode == "cos":
        print(f"cos {Q}x{N}x{d}: max |matrix - fp64| = {err.max():.3e} (bound 1e-5)")
        assert float(err.max()) < 1e-5
        tol = np.full(Q, 1e-5)
    else:
        a = np.abs(h.astype(np.float64))
        bound = (d + 2) * 2.0 ** -24 * (a[src] @ a.T)
        print(f"dot {Q}x{N}x{d}: max |matrix - fp64| = {err.max():.3e}, max error / bound = {(err / bound).max():.3f}")
        assert bool((err <= bound).all())
        tol = bound.max(axis=1)
    cand = _candidates(src, dst, N, filt)
    t64 = S64[np.arange(Q), dst]
    lo = ((S64 > (t64 + 2 * tol)[:, None]) & cand).sum(axis=1)
    hi = ((S64 >= (t64 - 2 * tol)[:, None]) & cand).sum(axis=1)
    assert bool((lo <= ng).all()) and bool((ng + ne <= hi).all())


# ---------------------------------------------------------------------------- 4. the edges of the contract
def test_zero_rows_and_endpoints_outside_the_graph():
    N, d = 40, 16
    h = _exact_rows(N, d, seed=3)
    h[5] = 0.0
    src = np.array([5, 7, 5, -1, N, 3, 3, 2 ** 40, -1], dtype=np.int64)
    dst = np.array([7, 5, 5, 2, 2, -5, N + 7, 3, N], dtype=np.int64)
    filt = np.array([[5, 3, 3], [9, 11, 11]], dtype=np.int64)
    for mode in R.KINDS:
        S = R.scores(h, mode)
        want = R.ranks(S, src, dst, filt)
        st, ng, ne = _rank(h, src, dst, mode, filt)
        assert np.array_equal(st.astype(np.float64), want[0]) and np.array_equal(ng, want[1]) and np.array_equal(ne, want[2]), mode
        assert st[:3].tolist() == [0.0] * 3 and not np.signbit(st).any()                 # +0.0 for the zero row and for every outside endpoint
        assert st[3:].tolist() == [0.0] * 6
        score = ops.emb_link_score(_t(h, torch.float32), _t(src, torch.int64), _t(dst, torch.int64), mode).cpu().numpy()
        assert np.array_equal(score.view(np.int32), st.view(np.int32))
    assert ne[3] == N - 1 and ng[3] == 0                                                 # a source outside: every candidate but dst ties at 0


def test_one_node_no_queries_and_a_filter_that_covers_everything():
    one = torch.full((1, 8), 3.0, device=DEV)
    z = torch.zeros(1, dtype=torch.int64, device=DEV)
    for mode, want in (("cos", 1.0), ("dot", 72.0)):
        st, ng, ne = ops.emb_link_rank(one, z, z, mode)
        assert (st.tolist(), ng.tolist(), ne.tolist()) == ([pytest.approx(want, abs=1e-6)], [0], [0])
    h = _t(_exact_rows(50, 16, seed=1), torch.float32)
    empty = torch.empty(0, dtype=torch.int64, device=DEV)
    st, ng, ne, mat = ops.emb_link_rank(h, empty, empty, return_matrix=True)
    assert st.shape == ng.shape == ne.shape == (0,) and mat.shape == (0, 50) and ng.dtype == ne.dtype == torch.int32
    assert ops.emb_link_score(h, empty, empty, "dot").shape == (0,)
    src, dst = torch.tensor([4, 9], device=DEV), torch.tensor([6, 9], device=DEV)
    everything = torch.stack([torch.tensor([4] * 50 + [9] * 50), torch.arange(50).repeat(2)]).to(DEV)
    st, ng, ne = ops.emb_link_rank(h, src, dst, "dot", filter_edges=everything)
    assert ng.tolist() == [0, 0] and ne.tolist() == [0, 0]
    with pytest.raises(L.GnnmpError, match="not both"):
        ops.emb_link_rank(h, src, dst, filter_edges=everything, filter_rowptr=torch.zeros(51, dtype=torch.int32, device=DEV))
    free = ops.emb_link_rank(h, src, dst, "dot")
    assert free[1].tolist() != [0, 0] or free[2].tolist() != [0, 0]
    lr = LPR.embedding_ranks(h, torch.stack([src, dst]), "dot", filter_edges=everything)
    assert lr.rank.tolist() == [1.0, 1.0] and torch.equal(_bits(lr.logit), _bits(st))


def test_argument_errors_leave_the_outputs_untouched():
    N, d, Q = 60, 24, 10
    h = _t(_exact_rows(N, d, seed=2), torch.float32)
    rng = np.random.default_rng(5)
    src, dst = (_t(a, torch.int64) for a in _queries(rng, Q, N))
    rowptr, col = torch.zeros(N + 1, dtype=torch.int32, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
    lib = L.lib()
    need = lib.gmp_emb_link_workspace_bytes(N, Q, d)
    ws = torch.empty(need + 256, dtype=torch.uint8, device=DEV)
    st = torch.full((Q,), -7.5, device=DEV)
    ng, ne = torch.full((Q,), -9, dtype=torch.int32, device=DEV), torch.full((Q,), -9, dtype=torch.int32, device=DEV)
    p = lambda t: C.c_void_p(0 if t is None else t.data_ptr())                   # noqa: E731

    def rank(n=N, dim=d, mode=0, q=Q, h_=h, src_=src, frow=None, fcol=None, fnnz=0, st_=st, wsb=need + 256, ws_=ws):
        return lib.gmp_emb_link_rank(p(h_), n, dim, mode, p(src_), p(dst), q, p(frow), p(fcol), fnnz, p(st_), p(ng), p(ne), None, p(ws_), wsb, None)

    def score(n=N, dim=d, mode=0, q=Q, h_=h, src_=src, st_=st, wsb=need + 256, ws_=ws):
        return lib.gmp_emb_link_score(p(h_), n, dim, mode, p(src_), p(dst), q, p(st_), p(ws_), wsb, None)

    for call in (rank, score):
        for kw in (dict(dim=257), dict(dim=0), dict(mode=2), dict(mode=-1), dict(n=2 ** 31), dict(n=-1), dict(q=-1), dict(h_=None), dict(src_=None),
                   dict(st_=None)):
            assert call(**kw) == GMP_ERR_ARG, (call.__name__, kw)
        assert call(wsb=need - 1) == GMP_ERR_WORKSPACE and call(ws_=None) == GMP_ERR_WORKSPACE
    assert rank(frow=rowptr, fcol=None, fnnz=3) == GMP_ERR_ARG and rank(frow=None, fcol=col, fnnz=3) == GMP_ERR_ARG
    assert rank(frow=rowptr, fcol=col, fnnz=-1) == GMP_ERR_ARG
    torch.cuda.synchronize()
    assert st.tolist() == [-7.5] * Q and ng.tolist() == [-9] * Q and ne.tolist() == [-9] * Q
    assert rank(q=0) == 0 and score(q=0) == 0 and rank(q=0, h_=None, src_=None, st_=None, ws_=None, wsb=0) == 0
    torch.cuda.synchronize()
    assert st.tolist() == [-7.5] * Q and ng.tolist() == [-9] * Q                  # nothing to do, nothing launched
    # filter_nnz == 0 with both arrays given, and with one of them: no filter
    want = [o.clone() for o in ops.emb_link_rank(h, src, dst)]
    for kw in (dict(frow=rowptr, fcol=col), dict(frow=rowptr), dict(fcol=col)):
        assert rank(**kw) == 0
        torch.cuda.synchronize()
        assert torch.equal(_bits(st), _bits(want[0])) and torch.equal(ng, want[1]) and torch.equal(ne, want[2])
    with pytest.raises(L.GnnmpError, match="dim=257"):
        ops.emb_link_rank(torch.zeros(4, 257, device=DEV), src, dst)
    with pytest.raises(L.GnnmpError, match="differ in length"):
        ops.emb_link_score(h, src, dst[:-1].contiguous())
    with pytest.raises(L.GnnmpError, match="go together"):
        ops.emb_link_rank(h, src, dst, filter_rowptr=rowptr)


# ---------------------------------------------------------------------------- 5. planted structure
def _planted(scale_row=None):
    """64 nodes in 32 pairs: partners share a direction (all entries positive) up to 1 % noise; unrelated nodes overlap by about 2 / pi"""
    gen = torch.Generator().manual_seed(11)
    u = torch.randn(32, 64, generator=gen).abs()
    u = u / u.norm(dim=1, keepdim=True)
    emb = u.repeat_interleave(2, dim=0) + 0.01 * torch.randn(64, 64, generator=gen) / 8
    if scale_row is not None:
        emb[scale_row] *= 10
    edges = torch.stack([torch.arange(0, 64, 2), torch.arange(1, 64, 2)])
    neg = torch.stack([torch.arange(0, 64, 2), (torch.arange(1, 64, 2) + 2) % 64])        # a node with somebody else's partner
    pairs = torch.cat([edges, neg], dim=1)
    labels = torch.cat([torch.ones(32), torch.zeros(32)])
    return emb.to(DEV), edges.to(DEV), pairs.to(DEV), labels.to(DEV)


def test_planted_pairs_are_found_and_a_long_row_moves_dot_but_not_cos():
    emb, edges, pairs, labels = _planted()
    out = LPR.link_probe(emb, edges, None, pairs, labels)
    assert set(out) == {f"embed_{k}_{m}" for k in R.KINDS for m in ("mrr", "hits@1", "hits@10", "hits@50", "auc")}
    assert out["embed_cos_mrr"] == 1.0 and out["embed_cos_auc"] == 1.0 and out["embed_cos_hits@1"] == 1.0
    emb, edges, pairs, labels = _planted(scale_row=7)
    others = torch.tensor([s for s in range(64) if s != 7], device=DEV)
    to7 = torch.stack([others, torch.full_like(others, 7)])
    assert bool((LPR.embedding_scores(emb, to7, "dot") > 0).all())                        # every source overlaps with node 7
    dot, cos = LPR.embedding_ranks(emb, to7, "dot"), LPR.embedding_ranks(emb, to7, "cos")
    assert dot.rank.tolist() == [1.0] * 63                                                # ten times as long: first for everybody
    not_partner = others != 6
    assert bool((cos.n_greater[not_partner] >= 1).all()) and cos.rank[others == 6].tolist() == [1.0]      # the direction did not move
    out = LPR.link_probe(emb, edges, None, pairs, labels)
    assert out["embed_cos_mrr"] == 1.0 and out["embed_cos_auc"] == 1.0
    assert out["embed_dot_mrr"] < 0.6 and out["embed_dot_hits@1"] == 1 / 32       # node 7 stands before every partner but its own: (6, 7) alone stays first


# ---------------------------------------------------------------------------- 6. --link-probe end to end
EMBED_KEYS = [f"test/embed_{k}_{m}" for k in R.KINDS for m in ("mrr", "hits@1", "hits@10", "hits@50", "auc")]


def _finetune(tmp_path, monkeypatch, name, **flags):
    from gnn_pretraining_amd.finetune import finetune as FT
    monkeypatch.setattr(FT, "OUTPUT_DIR", tmp_path / name)
    cfg = FT.FinetuneConfig("Cora_LP", "full_finetune", "b1", 5, lp_engine=True, **flags)
    log = tmp_path / f"{name}.jsonl"
    test = FT.finetune(cfg, epochs=1, device=DEV, data_root=str(tmp_path / "data"), data_scale=0.1, log_path=str(log))
    rec = [json.loads(line) for line in log.read_text().splitlines()]
    state = torch.load(next((tmp_path / name).glob("model_*.pt")), map_location=DEV, weights_only=True)["model_state_dict"]
    return cfg, test, rec, state


def test_finetune_with_the_link_probe_logs_its_keys_and_leaves_training_alone(tmp_path, monkeypatch):
    from gnn_pretraining_amd.data.finetune_data_loaders import create_finetune_data_loader
    from gnn_pretraining_amd.finetune.engine import LinkPredictionEngine
    from gnn_pretraining_amd.models.finetune_model import create_finetune_model
    cfg, test1, rec1, state1 = _finetune(tmp_path, monkeypatch, "with", link_probe=True)
    _, test0, rec0, state0 = _finetune(tmp_path, monkeypatch, "without")
    assert set(test1) == set(test0) | set(EMBED_KEYS) and not any(k.startswith("test/embed_") for k in test0)
    for k, v in test0.items():                                                   # training and evaluation as without the flag, bit for bit
        assert k == "test/training_time" or test1[k] == v or (v != v and test1[k] != test1[k]), k
    assert state1.keys() == state0.keys() and all(torch.equal(state1[k], state0[k]) for k in state1)
    assert all(math.isfinite(test1[k]) and 0.0 <= test1[k] <= 1.0 for k in EMBED_KEYS)
    val_keys = {f"val/embed_{k}_{m}" for k in R.KINDS for m in ("mrr", "auc")}
    assert rec1[0]["step"] == 0 and set(rec1[0]) == val_keys | {"step"} and "val/embed_cos_mrr" in rec1[0]       # before any training
    val = [r for r in rec1 if "val/auc" in r]
    assert len(val) == 1 and val_keys <= set(val[0]) and not any(k.startswith("val/embed_") and k not in val_keys for k in val[0])
    assert not any(k.startswith(("val/embed_", "test/embed_")) for r in rec0 for k in r)
    # by hand: the returned state on a fresh engine, the test split's positives, the three splits' positives as the filter
    sets = {sp: create_finetune_data_loader("Cora_LP", sp, cfg.batch_size, torch.Generator(), tmp_path / "data").dataset for sp in ("train", "val", "test")}
    model = create_finetune_model(torch.device(DEV), cfg)
    model.load_state_dict(state1)
    eng = LinkPredictionEngine(model, sets["train"].data.x, sets["train"].train_edges.to(DEV).contiguous(), torch.device(DEV), seed=cfg.seed,
                               max_pairs=2 * cfg.batch_size)
    known = torch.cat([sets["train"].train_edges, sets["val"].pos_edges, sets["test"].pos_edges], dim=1).to(DEV)
    known = torch.cat([known, known.flip(0)], dim=1).contiguous()
    with torch.no_grad():
        emb = eng.embed()
        for kind in R.KINDS:
            ranks = LPR.embedding_ranks(emb, sets["test"].pos_edges.to(DEV).contiguous(), kind, filter_edges=known).rank
            for m, v in ranking_metrics(ranks).items():
                assert test1[f"test/embed_{kind}_{m}"] == v, (kind, m)
            auc = LPR.pair_auc(LPR.embedding_scores(emb, sets["test"].edges.to(DEV).contiguous(), kind), sets["test"].labels.to(DEV))
            assert test1[f"test/embed_{kind}_auc"] == auc
