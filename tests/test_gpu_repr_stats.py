"""The label-free embedding statistics on the GPU (csrc/repr_stats.hip through ops.repr_* and gnn_pretraining_amd/repr_stats.py) against
the fp64 definitions of tests/repr_ref.py, and the two flags that log them (--repr-stats of pre-training and of fine-tuning), which must
leave training bit for bit as it is.

Bounds.  A single similarity is one fp32 MFMA chain over unit rows, held to 1e-5 as tests/test_gpu_knn.py (b) holds it; mean_cosine is a
mean of such values.  uniformity = log of a mean of exp(2 t (s - 1)): an error ds in s moves the log by at most 2 t ds, and the fp32
exp and the fp32 sum of a lane's 16 values add a relative error of a few 1e-7, bounded here by 2e-6.  The Gram matrix is a sum of
exact products in fp64: RankMe through it differs from the SVD route by the conditioning of the eigenvalue route alone (a singular
value near zero comes out of eigvalsh as sqrt of about 1e-16 of the largest eigenvalue), which tests/test_repr_host.py holds to the same
1e-6 relative on numpy's own fp64 Gram matrix of such inputs.  Measured on the MI355X: at most 2.6e-7 (the rank-8 set), 9e-8 on the
100 x 256 set, below 1e-9 on the others."""
import functools
import json
import math
import random

import numpy as np
import pytest
import torch

import repr_ref as R
from gnn_pretraining_amd import _lib as L, ops, repr_stats as RS
from gnn_pretraining_amd.finetune import finetune as FT
from gnn_pretraining_amd.pretrain import pretrain as PT

pytestmark = pytest.mark.gpu
DEV = "cuda"
COS_TOL = 1e-5


def gpu(z):
    return torch.from_numpy(np.ascontiguousarray(z, dtype=np.float32)).to(DEV)


# ---------------------------------------------------------------------------- (a) pair coverage, exact
@functools.lru_cache(maxsize=None)
def four_ones_case(n, d):
    z = R.four_ones(n, d, seed=1000 * d + n)
    return z, R.pair_stats(z, 0.0)[1]


@pytest.mark.parametrize("d", [8, 32, 40, 100, 160, 256])
@pytest.mark.parametrize("n", [2, 3, 31, 32, 33, 127, 128, 129, 257, 1000, 2500])
def test_every_pair_is_counted_once(n, d):
    """four ones per row: every s_ij is a multiple of 0.25 and every partial sum is exact, so a skipped or doubled tile, a wrong
    diagonal mask or a padding column shows in the last bit"""
    z, want_cos = four_ones_case(n, d)
    got = ops.repr_pair_stats(gpu(z), 0.0).tolist()
    assert got[1] == want_cos, (got[1], want_cos)
    assert got[0] == n * (n - 1) / 2                                         # t = 0: every pair contributes exp(0) = 1


# ---------------------------------------------------------------------------- (b), (d) random and structured embeddings
@functools.lru_cache(maxsize=None)
def embedding(name):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "randn_1000x256":
        z = rng.standard_normal((1000, 256))
    elif name == "randn_257x40":
        z = rng.standard_normal((257, 40))
    elif name == "abs_500x256":
        z = np.abs(rng.standard_normal((500, 256)))
    elif name == "collapsed_600x64":
        z = rng.standard_normal((1, 64)) + 1e-3 * rng.standard_normal((600, 64))
    elif name == "rank8_700x128":
        z = rng.standard_normal((700, 8)) @ rng.standard_normal((8, 128))
    elif name == "wide_100x256":
        z = rng.standard_normal((100, 256))
    else:
        raise KeyError(name)
    return z.astype(np.float32)


EMBEDDINGS = ["randn_1000x256", "randn_257x40", "abs_500x256", "collapsed_600x64", "rank8_700x128"]


@functools.lru_cache(maxsize=None)
def uniformity_ref(name, t):
    return R.uniformity(embedding(name), t)


@functools.lru_cache(maxsize=None)
def rankme_ref(name, center):
    return R.rankme(embedding(name), center=center)


@pytest.mark.parametrize("t", [2.0, 8.0])
@pytest.mark.parametrize("name", EMBEDDINGS)
def test_uniformity_and_mean_cosine(name, t):
    want = uniformity_ref(name, t)
    got = RS.uniformity(gpu(embedding(name)), t)
    print(name, t, "mean_cosine", got["mean_cosine"], want["mean_cosine"], "uniformity", got["uniformity"], want["uniformity"])
    assert abs(got["mean_cosine"] - want["mean_cosine"]) <= COS_TOL
    assert abs(got["uniformity"] - want["uniformity"]) <= 2 * t * COS_TOL + 2e-6


@pytest.mark.parametrize("center", [False, True])
@pytest.mark.parametrize("name", EMBEDDINGS + ["wide_100x256"])
def test_rankme(name, center):
    want = rankme_ref(name, center)
    got = RS.rankme(gpu(embedding(name)), center=center)
    print(name, center, "rankme", got, want)
    assert abs(got - want) <= 1e-6 * want


def test_embedding_stats_merges_the_two():
    z = gpu(embedding("randn_257x40"))
    s = RS.embedding_stats(z, t=2.0)
    assert sorted(s) == ["mean_cosine", "rankme", "uniformity"]
    assert s["rankme"] == RS.rankme(z) and {k: s[k] for k in ("uniformity", "mean_cosine")} == RS.uniformity(z, 2.0)


# ---------------------------------------------------------------------------- (c) Gram, exact
@pytest.mark.parametrize("n,d", [(1, 1), (3, 5), (64, 16), (65, 17), (1000, 40), (5000, 100), (2500, 256)])
def test_gram_of_integer_rows_is_exact(n, d):
    """every element of an fp64 MFMA tile in its place: an integer Gram matrix is exact whatever the order of the sums"""
    z = R.integer_rows(n, d, seed=n + d)
    want_g, want_c = R.gram(z)
    gram, colsum = ops.repr_gram(gpu(z))
    assert gram.dtype == torch.float64 and tuple(gram.shape) == (d, d) and tuple(colsum.shape) == (d,)
    g, c = gram.cpu().numpy(), colsum.cpu().numpy()
    assert np.array_equal(g, want_g.astype(np.float64)), np.argwhere(g != want_g)[:8]
    assert np.array_equal(c, want_c.astype(np.float64))
    assert torch.equal(gram, gram.t())


def test_gram_of_random_rows_is_bitwise_symmetric_and_close():
    z = embedding("randn_1000x256")
    gram, colsum = ops.repr_gram(gpu(z))
    assert torch.equal(gram, gram.t())
    want_g, want_c = R.gram(z)
    assert np.abs(gram.cpu().numpy() - want_g).max() <= 1e-12 * np.abs(want_g).max()
    assert np.abs(colsum.cpu().numpy() - want_c).max() <= 1e-12 * np.abs(z).sum(axis=0).max()


# ---------------------------------------------------------------------------- (e) alignment
@pytest.mark.parametrize("n,d", [(1, 8), (5, 40), (257, 100), (1025, 256), (4999, 32)])
def test_alignment_of_four_ones_pairs_is_exact(n, d):
    a, b = R.four_ones(n, d, seed=n), R.four_ones(n, d, seed=n + 1)
    assert ops.repr_alignment_sum(gpu(a), gpu(b), 2.0).item() == R.alignment_sum(a, b, 2.0)     # every term a multiple of 0.5


@pytest.mark.parametrize("alpha", [1.0, 2.0])
def test_alignment_of_random_pairs(alpha):
    rng = np.random.default_rng(5)
    a = rng.standard_normal((1500, 200)).astype(np.float32)
    b = (a + 0.5 * rng.standard_normal(a.shape)).astype(np.float32)
    got, want = RS.alignment(gpu(a), gpu(b), alpha), R.alignment_sum(a, b, alpha) / len(a)
    print("alignment", alpha, got, want)
    assert abs(got - want) <= 1e-5
    z = gpu(a)
    assert 0.0 <= RS.alignment(z, z) <= 1e-6


# ---------------------------------------------------------------------------- (f) contract
def test_zero_rows_score_zero_and_give_no_nan():
    z = embedding("randn_257x40").copy()
    z[[0, 17, 256]] = 0.0
    got, want = RS.uniformity(gpu(z), 2.0), R.uniformity(z, 2.0)
    assert abs(got["mean_cosine"] - want["mean_cosine"]) <= COS_TOL and abs(got["uniformity"] - want["uniformity"]) <= 4 * COS_TOL + 2e-6
    e, c = ops.repr_pair_stats(torch.zeros(130, 24, device=DEV), 1.0).tolist()
    assert c == 0.0 and abs(e / (130 * 129 / 2) - math.exp(-2.0)) <= 2e-6 * math.exp(-2.0)
    assert RS.alignment(torch.zeros(9, 24, device=DEV), torch.ones(9, 24, device=DEV)) == 2.0       # s_ii = 0
    gram, colsum = ops.repr_gram(torch.zeros(9, 24, device=DEV))
    assert not gram.any() and not colsum.any() and math.isfinite(RS.rankme(torch.zeros(9, 24, device=DEV)))


def test_two_rows_and_one_column():
    z = np.array([[1.0, 2.0, 2.0], [2.0, -1.0, 0.5]], dtype=np.float32)
    got, want = ops.repr_pair_stats(gpu(z), 2.0).tolist(), R.pair_stats(z, 2.0)
    assert abs(got[1] - want[1]) <= COS_TOL and abs(got[0] - want[0]) <= (4 * COS_TOL + 2e-6) * want[0]
    z = np.array([[2.0], [-3.0], [0.5], [0.0], [-1.0]], dtype=np.float32)                     # d = 1: every similarity is 1, -1 or 0
    got, want = ops.repr_pair_stats(gpu(z), 0.5).tolist(), R.pair_stats(z, 0.5)
    assert got[1] == want[1] == -2.0 and abs(got[0] - want[0]) <= 2e-6 * want[0]
    gram, colsum = ops.repr_gram(gpu(z))
    assert gram.tolist() == [[14.25]] and colsum.tolist() == [-1.5]


def test_calls_are_reproducible_bit_for_bit():
    z, other = gpu(embedding("randn_1000x256")), gpu(embedding("randn_257x40"))
    first = (ops.repr_pair_stats(z, 2.0), *ops.repr_gram(z), ops.repr_alignment_sum(z, z.flip(0).contiguous(), 1.0))
    again = (ops.repr_pair_stats(z, 2.0), *ops.repr_gram(z), ops.repr_alignment_sum(z, z.flip(0).contiguous(), 1.0))
    ops.repr_pair_stats(other, 8.0), ops.repr_gram(other), ops.repr_alignment_sum(other, other, 2.0)     # another shape in between
    third = (ops.repr_pair_stats(z, 2.0), *ops.repr_gram(z), ops.repr_alignment_sum(z, z.flip(0).contiguous(), 1.0))
    for a, b, c in zip(first, again, third):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_bad_arguments_are_refused():
    z = torch.randn(10, 8, device=DEV)
    for bad in (z.cpu(), z.t(), z.double(), torch.randn(10, 257, device=DEV), z[:, ::2], z[0]):
        for call in (lambda x: ops.repr_pair_stats(x), lambda x: ops.repr_gram(x), lambda x: ops.repr_alignment_sum(x, x)):
            with pytest.raises(L.GnnmpError):
                call(bad)
    with pytest.raises(L.GnnmpError):
        ops.repr_pair_stats(z[:1].contiguous())                             # one row has no pair
    assert ops.repr_gram(z[:1].contiguous())[0].shape == (8, 8)              # ... but a Gram matrix
    for t in (-1.0, float("nan")):
        with pytest.raises(L.GnnmpError):
            ops.repr_pair_stats(z, t)
    for alpha in (0.0, -2.0):
        with pytest.raises(L.GnnmpError):
            ops.repr_alignment_sum(z, z, alpha)
    with pytest.raises(L.GnnmpError):
        ops.repr_alignment_sum(z, z[:5].contiguous())
    with pytest.raises(L.GnnmpError):
        ops.repr_alignment_sum(z, z.cpu())


# ---------------------------------------------------------------------------- (g) fine-tuning
FT_KEYS = ("val/repr_uniformity", "val/repr_mean_cosine", "val/repr_rankme")
FT_EPOCHS = 2


@pytest.fixture(scope="module")
def ft_run(tmp_path_factory):
    root, cache = tmp_path_factory.mktemp("repr_ft"), {}

    def make(domain, kw, flag):
        if (domain, flag) in cache:
            return cache[domain, flag]
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(FT, "OUTPUT_DIR", root / "finetune")
            log = root / f"{domain}_{int(flag)}.jsonl"
            cfg = FT.FinetuneConfig(domain, "full_finetune", "b1", 1, repr_stats=flag, **kw)
            test = FT.finetune(cfg, epochs=FT_EPOCHS, data_root=str(root / "data"), data_scale=0.1, log_path=str(log))
            state = torch.load(FT.OUTPUT_DIR / f"model_{cfg.exp_name}_{cfg.seed}.pt", map_location="cpu", weights_only=True)["model_state_dict"]
        cache[domain, flag] = (test, state, [json.loads(line) for line in open(log)])
        return cache[domain, flag]

    return make


@pytest.mark.parametrize("domain,kw,val_key", [("Cora_NC", {}, "val/accuracy"), ("Cora_LP", {"lp_engine": True}, "val/auc")], ids=["Cora_NC", "Cora_LP"])
def test_finetune_logs_the_statistics_and_trains_bit_for_bit_as_without_them(domain, kw, val_key, ft_run):
    test_on, state_on, rec_on = ft_run(domain, kw, True)
    test_off, state_off, rec_off = ft_run(domain, kw, False)
    first = [r for r in rec_on if r["step"] == 0]
    assert len(first) == 1 and rec_on[0] is first[0] and sorted(first[0]) == sorted(FT_KEYS + ("step",))
    per_epoch = [r for r in rec_on if val_key in r]
    assert len(per_epoch) == FT_EPOCHS
    for r in first + per_epoch:
        assert all(math.isfinite(r[k]) for k in FT_KEYS)
        assert r["val/repr_uniformity"] <= 1e-6 and -1.0 <= r["val/repr_mean_cosine"] <= 1.0 + 1e-6 and 1.0 - 1e-6 <= r["val/repr_rankme"] <= 256.0
    assert not any(k.startswith("val/repr_") for r in rec_off for k in r)
    for k in test_off:
        if k not in ("test/training_time",):
            assert test_on[k] == test_off[k] or (test_on[k] != test_on[k] and test_off[k] != test_off[k]), k
    assert math.isfinite(test_on["test/loss"])
    assert state_on.keys() == state_off.keys() and all(torch.equal(state_on[n], state_off[n]) for n in state_on)


# ---------------------------------------------------------------------------- (h) pre-training
PT_NAMES = ("uniformity", "mean_cosine", "rankme")


@pytest.fixture(scope="module")
def pt_run(tmp_path_factory):
    root, cache = tmp_path_factory.mktemp("repr_pt"), {}

    def make(level):
        if level in cache:
            return cache[level]
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(PT, "OUTPUT_DIR", root / "pretrain" / level)
            log = root / f"{level}.jsonl"
            # the reference rule of gradient surgery shuffles the tasks with Python's unseeded global `random`, as the reference does:
            # two runs are comparable only from the same state of it
            random.seed(20260)
            path = PT.pretrain(PT.PretrainConfig("s4", 7), epochs=1, steps_per_epoch=3, log_path=str(log), data_root=str(root / "data"),
                               data_scale=0.03, repr_stats=level)
            ckpt = torch.load(path, map_location="cpu", weights_only=True)
        cache[level] = (ckpt, [json.loads(line) for line in open(log)])
        return cache[level]

    return make


def _same(a, b):
    if isinstance(a, torch.Tensor):
        return isinstance(b, torch.Tensor) and torch.equal(a, b)
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(_same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(_same(x, y) for x, y in zip(a, b))
    return a == b


def _check_pretrain_records(records, domains):
    keys = [f"val/repr/{d}/{k}" for d in domains for k in PT_NAMES + ("alignment",)] + [f"val/repr/{k}" for k in PT_NAMES]
    first = [r for r in records if r["step"] == 0]
    assert len(first) == 1 and records[0] is first[0] and sorted(first[0]) == sorted(keys + ["step"])
    after = [r for r in records if "val/loss/total" in r]
    assert len(after) == 1 and after[0]["step"] == 3
    for r in first + after:
        assert all(math.isfinite(r[k]) for k in keys)
        for k in PT_NAMES:
            assert abs(r[f"val/repr/{k}"] - sum(r[f"val/repr/{d}/{k}"] for d in domains) / len(domains)) <= 1e-12 * max(1.0, abs(r[f"val/repr/{k}"]))
        assert all(0.0 <= r[f"val/repr/{d}/alignment"] <= 4.0 and 1.0 - 1e-6 <= r[f"val/repr/{d}/rankme"] <= 256.0 for d in domains)


def test_pretrain_logs_the_statistics_and_leaves_the_checkpoint_bit_for_bit(pt_run):
    domains = PT.PRETRAIN_DOMAINS["s4"]
    ckpt_on, rec_on = pt_run("graph")
    ckpt_off, rec_off = pt_run("off")
    _check_pretrain_records(rec_on, domains)
    assert not any(k.startswith("val/repr") for r in rec_off for k in r)
    assert not any(k.startswith("val/repr") for k in ckpt_on["val_metrics"]) and ckpt_on["val_metrics"].keys() == ckpt_off["val_metrics"].keys()
    assert _same(ckpt_on["model_state_dict"], ckpt_off["model_state_dict"])
    assert _same(ckpt_on["rng_state"], ckpt_off["rng_state"])
    assert _same(ckpt_on["val_metrics"], ckpt_off["val_metrics"])


def test_pretrain_node_level_logs_the_same_keys(pt_run):
    _check_pretrain_records(pt_run("node")[1], PT.PRETRAIN_DOMAINS["s4"])
