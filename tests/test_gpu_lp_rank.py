"""All-candidate link ranking (csrc/lp_rank.hip: gmp_lp_rank / gmp_lp_topk; LinkPredictionEngine.rank / top_k; --lp-ranking).

The yardstick is code that is not under test: gmp_lp_score_fwd with p = 0 over the explicit pair list of every (source, candidate),
masked with torch integer ops, compared and sorted (stable, descending) with torch.  The ranking kernels promise that scorer's logits
bit for bit, so every comparison here is exact: integer counts equal, indices equal, logits equal as bit patterns.  One test restates
the scorer in float64 torch so that the yardstick is not the library alone."""
import functools
import json
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from gnn_pretraining_amd import operators as OP, ops, synthetic as S                # noqa: E402
from gnn_pretraining_amd.models import FinetuneGNN                                  # noqa: E402

DEV = torch.device("cuda:0")
NINF = float("-inf")


def _bits(t):
    return t.contiguous().view(torch.int32)


@functools.lru_cache(maxsize=None)
def _weights():
    torch.manual_seed(20)
    mlp = FinetuneGNN(torch.device("cpu"), "Cora_LP", "full_finetune").classification_head.predictor.mlp
    return tuple(t.detach().clone().to(DEV).contiguous() for t in (mlp[0].weight, mlp[0].bias, mlp[3].weight, mlp[3].bias))


@functools.lru_cache(maxsize=None)
def _embeddings(N, tie=False):
    h = torch.randn(N, 256, generator=torch.Generator().manual_seed(1000 + N))
    if tie:
        h[9] = h[5]                                            # two candidates with the same row: the same logit from every source
    return h.to(DEV).contiguous()


@functools.lru_cache(maxsize=None)
def _dense(N, tie=False):
    """The scorer's logit of every pair (s, c), s and c in [0, N]: index N stands for an index outside [0, N) (a zero row).  CPU."""
    s, c = torch.meshgrid(torch.arange(N + 1), torch.arange(N + 1), indexing="ij")
    _, logit = ops.lp_score_fwd(_embeddings(N, tie), s.reshape(-1).to(DEV), c.reshape(-1).to(DEV), *_weights(), 0.0, 0, 0)
    return logit.view(N + 1, N + 1).cpu()


def _row(idx, N):
    return torch.where((idx >= 0) & (idx < N), idx, torch.full_like(idx, N))


def _skip(N, src, filt, dst=None):
    """[Q, N] bool: the candidates a query leaves out (torch integer ops)."""
    ar = torch.arange(N)
    skip = ar[None, :] == src[:, None]
    if dst is not None:
        skip |= ar[None, :] == dst[:, None]
    if filt is not None and filt.numel():
        ok = (filt[0] >= 0) & (filt[0] < N) & (filt[1] >= 0) & (filt[1] < N)
        adj = torch.zeros(N + 1, N, dtype=torch.bool)
        adj[filt[0][ok], filt[1][ok]] = True
        skip |= adj[_row(src, N)]
    return skip


def _want_rank(M, N, src, dst, filt):
    lt = M[_row(src, N), _row(dst, N)]
    cand, keep = M[_row(src, N)][:, :N], ~_skip(N, src, filt, dst)
    return lt, ((cand > lt[:, None]) & keep).sum(1).to(torch.int32), ((cand == lt[:, None]) & keep).sum(1).to(torch.int32)


def _want_topk(M, N, src, k, filt):
    cand = M[_row(src, N)][:, :N].clone()
    skip = _skip(N, src, filt)
    cand[skip] = NINF
    val, idx = torch.sort(cand, dim=1, descending=True, stable=True)
    idx[torch.arange(N)[None, :] >= (~skip).sum(1)[:, None]] = -1
    if N < k:
        val = torch.cat([val, torch.full((len(src), k - N), NINF)], dim=1)
        idx = torch.cat([idx, torch.full((len(src), k - N), -1, dtype=torch.int64)], dim=1)
    return idx[:, :k], val[:, :k]


def _rank(N, src, dst, filt, tie=False):
    logit, ng, ne = OP.lp_rank(_embeddings(N, tie), torch.stack([src, dst]).to(DEV), *_weights(), filter_edges=None if filt is None else filt.to(DEV))
    return logit.cpu(), ng.cpu(), ne.cpu()


def _topk(N, src, k, filt, tie=False):
    idx, logit = OP.lp_topk(_embeddings(N, tie), src.to(DEV), k, *_weights(), filter_edges=None if filt is None else filt.to(DEV))
    return idx.cpu(), logit.cpu()


def _check_rank(N, src, dst, filt, tie=False):
    got, want = _rank(N, src, dst, filt, tie), _want_rank(_dense(N, tie), N, src, dst, filt)
    assert torch.equal(_bits(got[0]), _bits(want[0])), "logit_true"
    assert torch.equal(got[1], want[1]), ("n_greater", got[1], want[1])
    assert torch.equal(got[2], want[2]), ("n_equal", got[2], want[2])
    return got


def _check_topk(N, src, k, filt, tie=False):
    got, want = _topk(N, src, k, filt, tie), _want_topk(_dense(N, tie), N, src, k, filt)
    assert torch.equal(got[0], want[0]), ("top-k indices", got[0], want[0])
    assert torch.equal(_bits(got[1]), _bits(want[1])), "top-k logits"
    return got


@pytest.mark.parametrize("Q", [1, 33])
@pytest.mark.parametrize("N", [1, 2, 31, 32, 33, 70, 257])
def test_rank_and_topk_equal_the_scorer_yardstick(N, Q):
    """Tile edges (N = 31, 32, 33, 70: the last candidate tile partly filled), several tiles and several top-k parts (257), more than
    one query tile (Q = 33), with and without a random filter (unsorted rows with repeats, as randint draws them); k = 1, 5, 64 -- 64
    is more than the candidates for N <= 64 (padding), and for N = 1 there is no candidate at all: rank 1, top-k all padding."""
    gen = torch.Generator().manual_seed(7 * N + Q)
    src, dst = torch.randint(0, N, (Q,), generator=gen), torch.randint(0, N, (Q,), generator=gen)
    filt = torch.randint(0, N, (2, 3 * N), generator=gen)
    for f in (None, filt):
        _, ng, ne = _check_rank(N, src, dst, f)
        if N == 1:
            assert int(ng.sum()) == 0 and int(ne.sum()) == 0                           # rank = 1 + 0 + 0 / 2
        for k in (1, 5, 64):
            idx, logit = _check_topk(N, src, k, f)
            if N == 1:
                assert bool((idx == -1).all()) and bool((logit == NINF).all())
            if k >= N:
                assert bool((idx[:, N - 1:] == -1).all())                               # at most N - 1 candidates: the rest is padding


def test_filter_and_query_edge_cases():
    N = 70
    M = _dense(N)
    s = 40
    t = lambda *v: torch.tensor(v, dtype=torch.int64)
    base = torch.stack([t(3, 3, 3, 12, 12, 60), t(50, 7, 20, 69, 0, 33)])              # row 3: 50, 7, 20 -- unsorted as stored
    # src == dst
    _, ng, ne = _check_rank(N, t(s), t(s), base)
    assert int(ng) + int(ne) <= N - 1
    # a filter row that contains the query's dst: dst is left out once
    f = torch.cat([base, torch.stack([t(s, s), t(11, 25)])], dim=1)
    a = _check_rank(N, t(s), t(11), f)
    b = _check_rank(N, t(s), t(11), torch.cat([base, torch.stack([t(s), t(25)])], dim=1))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    # a filter row that contains the source itself
    a = _check_rank(N, t(s), t(11), torch.cat([base, torch.stack([t(s, s), t(s, 25)])], dim=1))
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    _check_topk(N, t(s), 64, torch.cat([base, torch.stack([t(s, s), t(s, 25)])], dim=1))
    # duplicates in a filter row do not double-count
    dup = torch.cat([base, torch.stack([t(s, s, s, s), t(25, 25, 25, 25)])], dim=1)
    a = _check_rank(N, t(s), t(11), dup)
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
    ia, la = _check_topk(N, t(s), 64, dup)
    ib, lb = _check_topk(N, t(s), 64, torch.cat([base, torch.stack([t(s), t(25)])], dim=1))
    assert torch.equal(ia, ib) and torch.equal(_bits(la), _bits(lb))
    # an unsorted filter row (3: 50, 7, 20) against the same row sorted
    srt = torch.stack([t(3, 3, 3, 12, 12, 60), t(7, 20, 50, 0, 69, 33)])
    a, b2 = _check_rank(N, t(3, 3), t(50, 8), base), _check_rank(N, t(3, 3), t(50, 8), srt)
    assert torch.equal(a[1], b2[1]) and torch.equal(a[2], b2[2])
    assert torch.equal(_check_topk(N, t(3), 64, base)[0], _check_topk(N, t(3), 64, srt)[0])
    # an empty filter and no filter give the same result
    empty = torch.empty(2, 0, dtype=torch.int64)
    a, b2 = _check_rank(N, t(s, 3), t(11, 50), empty), _check_rank(N, t(s, 3), t(11, 50), None)
    assert all(torch.equal(x, y) for x, y in zip(a[1:], b2[1:])) and torch.equal(_bits(a[0]), _bits(b2[0]))
    assert torch.equal(_check_topk(N, t(s, 3), 5, empty)[0], _check_topk(N, t(s, 3), 5, None)[0])
    # an isolated source (no filter row) next to one with a row: only src and dst are left out
    _, ng, ne = _check_rank(N, t(41, 3), t(2, 50), base)
    row = M[41, :N]
    keep = (torch.arange(N) != 41) & (torch.arange(N) != 2)
    assert int(ng[0]) == int(((row > M[41, 2]) & keep).sum()) and int(ne[0]) == int(((row == M[41, 2]) & keep).sum())
    # a duplicated query gives duplicated output
    lg, ng, ne = _check_rank(N, t(3, s, 3), t(50, 11, 50), base)
    assert _bits(lg)[0] == _bits(lg)[2] and ng[0] == ng[2] and ne[0] == ne[2]
    idx, logit = _check_topk(N, t(3, s, 3), 5, base)
    assert torch.equal(idx[0], idx[2]) and torch.equal(_bits(logit[0]), _bits(logit[2]))
    # src / dst outside [0, N) read as a zero row (the scorer's convention); such a source has no filter row
    _check_rank(N, t(N, 5, -1), t(4, N + 3, 6), base)
    _check_topk(N, t(N, -1), 5, base)


def test_a_forced_tie_shows_in_n_equal_and_topk_order():
    """Rows 5 and 9 of h are the same vector, so candidates 5 and 9 share their logit from every source: the true edge (s, 5) has
    n_equal >= 1 (candidate 9), and the top-k list of s holds 5 directly in front of 9 (N = 33, k = 32: every candidate is listed)."""
    N = 33
    M = _dense(N, tie=True)
    src = torch.tensor([0, 20, 32])
    assert torch.equal(_bits(M[src, 5]), _bits(M[src, 9]))
    _, ng, ne = _check_rank(N, src, torch.full((3,), 5), None, tie=True)
    assert bool((ne >= 1).all())
    _, ng9, ne9 = _check_rank(N, src, torch.full((3,), 9), None, tie=True)
    assert torch.equal(ng, ng9) and torch.equal(ne, ne9)
    idx, _ = _check_topk(N, src, 32, None, tie=True)
    for q in range(3):
        pos5 = int((idx[q] == 5).nonzero())
        assert int(idx[q, pos5 + 1]) == 9


def test_ranks_against_a_float64_restatement_of_the_scorer():
    """N = 257, Q = 33, seed 31.  The scorer restated in float64 torch on the CPU gives every (query, candidate) logit; cells whose
    float64 logit lies within 1e-4 (the project's fp32-against-oracle bar) of the query's true logit cannot be decided in fp32 and
    are left out, at most 1 % of all cells.  Measured on the CPU for this seed, fp32 torch scorer against the float64 one: 3 of the
    8,481 cells (0.035 %) are left out, 31 of the 33 queries have none, every other fp32 comparison agrees with float64, and the
    largest fp32 logit error is 4.3e-7.  Per query the kernel's n_greater must then
    lie between the float64 count over the decided cells and that count plus the query's undecided cells, and n_equal cannot exceed
    the undecided cells."""
    N, Q = 257, 33
    gen = torch.Generator().manual_seed(31)
    src, dst = torch.randint(0, N, (Q,), generator=gen), torch.randint(0, N, (Q,), generator=gen)
    filt = torch.randint(0, N, (2, 2 * N), generator=gen)
    w0, b0, w3, b3 = (t.cpu().double() for t in _weights())
    h = _embeddings(N).cpu().double()

    def score64(s, d):
        hs, hd = h[s], h[d]
        feat = torch.cat([hs + hd, hs * hd, (hs - hd).abs()], dim=-1)
        return torch.relu(feat @ w0.t() + b0) @ w3.reshape(-1) + b3

    lt = score64(src, dst)
    cand = score64(src[:, None].expand(Q, N), torch.arange(N)[None, :].expand(Q, N))
    keep = ~_skip(N, src, filt, dst)
    near = ((cand - lt[:, None]).abs() <= 1e-4) & keep
    share = float(near.sum()) / (Q * N)
    print(f"fp64 cross-check: {int(near.sum())} of {Q * N} cells within 1e-4 of the true logit ({100 * share:.3f} %)")
    assert share <= 0.01
    lo = ((cand > lt[:, None]) & keep & ~near).sum(1)
    logit, ng, ne = _rank(N, src, dst, filt)
    assert float((logit.double() - lt).abs().max()) <= 1e-4
    assert bool((ng >= lo).all()) and bool((ng <= lo + near.sum(1)).all()), (ng, lo, near.sum(1))
    assert bool((ne <= near.sum(1)).all())
    assert int((near.sum(1) == 0).sum()) > 0                  # some queries are decided exactly: there n_greater == the float64 count


# --------------------------------------------------------------------------- the engine
def _lp_setup(seed):
    from gnn_pretraining_amd.data.data_setup import create_link_prediction_splits
    from gnn_pretraining_amd.finetune.engine import LinkPredictionEngine
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    c = S.cora_like(gen)
    train_pos = create_link_prediction_splits(c)["train_pos"].contiguous()
    hm = FinetuneGNN(DEV, "Cora_LP", "full_finetune")
    hm.train()
    eng = LinkPredictionEngine(hm, c.x, train_pos, DEV, seed=seed)
    eng.lr.mul_(30)
    return gen, c, train_pos, hm, eng


def _rand_pairs(gen, n, k):
    return torch.stack([torch.randint(0, n, (k,), generator=gen), torch.randint(0, n, (k,), generator=gen)])


def test_engine_rank_and_top_k_agree_with_predict():
    gen, c, train_pos, hm, eng = _lp_setup(201)
    N = c.num_nodes
    eng.mining_forward()
    eng.step(train_pos[:, :256].to(DEV), _rand_pairs(gen, N, 256).to(DEV))            # a trained state, model.training still on
    edges = train_pos[:, 300:303].contiguous().to(DEV)
    known = train_pos.to(DEV)
    r = eng.rank(edges, filter_edges=known)                                            # embeddings=None: embeds itself
    assert r.rank.dtype == torch.float32 and r.n_greater.dtype == torch.int32
    assert torch.equal(_bits(ops.sigmoid_fwd(r.logit)), _bits(eng.predict(edges)))
    assert torch.equal(r.rank, 1.0 + r.n_greater.float() + 0.5 * r.n_equal.float())
    # the same counts from predict() over the explicit pair list of every (source, candidate)
    ar = torch.arange(N, device=DEV)
    adj = torch.zeros(N, N, dtype=torch.bool, device=DEV)
    adj[known[0], known[1]] = True
    for q in range(edges.size(1)):
        s, d = int(edges[0, q]), int(edges[1, q])
        eng.predict(torch.stack([torch.full((N,), s, device=DEV), ar]))
        cand = eng.logit[:N].clone()
        keep = (ar != s) & (ar != d) & ~adj[s]
        assert _bits(cand[d:d + 1]).item() == _bits(r.logit[q:q + 1]).item()
        assert int(r.n_greater[q]) == int(((cand > cand[d]) & keep).sum()) and int(r.n_equal[q]) == int(((cand == cand[d]) & keep).sum())
    sources = edges[0].contiguous()
    idx, prob = eng.top_k(sources, 10, filter_edges=known)
    assert idx.shape == (3, 10) and bool((idx >= 0).all()) and not bool(adj[sources[:, None], idx].any()) and not bool((idx == sources[:, None]).any())
    want = eng.predict(torch.stack([sources[:, None].expand(3, 10).reshape(-1), idx.reshape(-1)]))
    assert torch.equal(_bits(prob.reshape(-1)), _bits(want))
    assert bool((prob[:, :-1] >= prob[:, 1:]).all())
    # one embedding shared by several calls, as in an evaluation pass
    emb = eng.embed()
    r2 = eng.rank(edges, filter_edges=known, embeddings=emb)
    idx2, _ = eng.top_k(sources, 10, filter_edges=known, embeddings=emb)
    assert torch.equal(r2.n_greater, r.n_greater) and torch.equal(r2.n_equal, r.n_equal) and torch.equal(idx2, idx)


def test_engine_rank_and_top_k_refuse_overwritten_embeddings():
    gen, c, train_pos, hm, eng = _lp_setup(203)
    edges = train_pos[:, :4].contiguous().to(DEV)
    emb = eng.embed()
    eng.rank(edges, embeddings=emb)
    eng.mining_forward()                                       # a forward overwrites the buffer embed() returned
    with pytest.raises(ValueError, match="overwritten"):
        eng.rank(edges, embeddings=emb)
    with pytest.raises(ValueError, match="overwritten"):
        eng.top_k(edges[0].contiguous(), 3, embeddings=emb)
    with pytest.raises(ValueError, match="embed"):
        eng.rank(edges, embeddings=eng.embed().clone())
    eng.rank(edges)
    eng.top_k(edges[0].contiguous(), 3)


def test_steps_after_rank_and_top_k_are_bitwise_the_steps_without_them():
    snaps = []
    for with_ranking in (True, False):
        gen, c, train_pos, hm, eng = _lp_setup(205)
        known = train_pos.to(DEV)
        for s in range(2):
            neg = _rand_pairs(gen, c.num_nodes, 256).to(DEV)
            eng.mining_forward()
            eng.step(train_pos[:, 256 * s:256 * (s + 1)].to(DEV), neg)
            if with_ranking and s == 0:
                eng.rank(train_pos[:, 600:616].contiguous().to(DEV), filter_edges=known)
                eng.top_k(train_pos[0, 600:616].contiguous().to(DEV), 7, filter_edges=known)
        eng.flush_counters()
        torch.cuda.synchronize()
        state = {k: v.clone() for k, v in hm.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}
        snaps.append((eng.flat.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), state))
    a, b = snaps
    for x, y, name in zip(a[:3], b[:3], ("flat", "exp_avg", "exp_avg_sq")):
        assert torch.equal(_bits(x), _bits(y)), name
    assert a[3].keys() == b[3].keys() and len(a[3]) > 0
    for n in a[3]:
        assert torch.equal(a[3][n], b[3][n]), n


def test_cli_lp_ranking_logs_mrr_and_hits(tmp_path, monkeypatch):
    """python -m gnn_pretraining_amd.finetune.finetune ... --lp-engine --engine-eval --lp-ranking (what run_finetune.py starts per job), in
    process: one epoch on the synthetic Cora_LP stand-in; the test record carries the ranking metrics."""
    from gnn_pretraining_amd.finetune import finetune as FT
    monkeypatch.setattr(FT, "OUTPUT_DIR", tmp_path / "finetune")
    log = tmp_path / "log.jsonl"
    monkeypatch.setattr(sys, "argv", ["finetune", "--domain_name", "Cora_LP", "--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1",
                                      "--seed", "5", "--epochs", "1", "--data-root", str(tmp_path / "data"), "--data-scale", "0.1",
                                      "--log", str(log), "--lp-engine", "--engine-eval", "--lp-ranking"])
    FT.main()
    rec = [json.loads(line) for line in log.read_text().splitlines()]
    test = [r for r in rec if "test/mrr" in r]
    assert len(test) == 1 and "test/auc" in test[0]
    mrr, h10 = test[0]["test/mrr"], test[0]["test/hits@10"]
    assert mrr == mrr and 0.0 < mrr <= 1.0 and 0.0 <= h10 <= 1.0
    assert test[0]["test/hits@1"] <= h10 <= test[0]["test/hits@50"]
