"""Host-side contract of the label-free embedding statistics (csrc/repr_stats.hip, gnn_pretraining_amd/repr_stats.py): the fp64
reference of tests/repr_ref.py pinned on cases worked out by hand, the Gram route to RankMe against the SVD route, declaration /
binding / export of the four C-ABI entry points, the workspace, every bad call refused before anything is launched, and the two
command-line flags with the configurations fine-tuning refuses.  Runs without a GPU."""
import ctypes
import math

import numpy as np
import pytest

import repr_ref as R
from gnn_pretraining_amd import _lib as L, ops, repr_stats as RS
from gnn_pretraining_amd.finetune import finetune as FT
from gnn_pretraining_amd.pretrain import pretrain as PT

ERR_ARG, ERR_WORKSPACE = -1, -3
BASE = ["--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1", "--seed", "1"]


# ---------------------------------------------------------------------------- the reference, by hand
def test_reference_two_orthogonal_rows():
    z = np.array([[3.0, 0.0], [0.0, 0.5]], dtype=np.float32)
    e, c = R.pair_stats(z, t=2.0)
    assert c == 0.0 and abs(e - math.exp(-4.0)) < 1e-15                     # ||zn_0 - zn_1||^2 = 2: exp(-2 t)
    u = R.uniformity(z, t=2.0)
    assert abs(u["uniformity"] + 4.0) < 1e-12 and u["mean_cosine"] == 0.0
    assert R.alignment_sum(z[:1], z[1:], alpha=2.0) == 2.0 and abs(R.alignment_sum(z[:1], z[1:], alpha=1.0) - math.sqrt(2.0)) < 1e-15
    p = (3 / 3.5, 0.5 / 3.5)                                                # the singular values are 3 and 0.5
    assert abs(R.rankme(z) - math.exp(-sum(x * math.log(x) for x in p))) < 1e-5


def test_reference_identical_rows_collapse():
    z = np.tile(np.array([[1.0, 2.0, -2.0, 0.0]], dtype=np.float32), (7, 1))
    u = R.uniformity(z, t=2.0)
    assert abs(u["uniformity"]) < 1e-12 and abs(u["mean_cosine"] - 1.0) < 1e-12
    assert abs(R.rankme(z) - 1.0) < 1e-4                                     # one direction: (1 + eps) and three times eps
    assert R.alignment_sum(z, z) < 1e-12
    zero = np.zeros((3, 4), dtype=np.float32)                               # zero rows stay zero: every similarity is 0
    e, c = R.pair_stats(zero, t=1.0)
    assert abs(e - 3 * math.exp(-2.0)) < 1e-15 and c == 0.0


def test_reference_orthonormal_set_has_full_rank():
    q, _ = np.linalg.qr(np.random.default_rng(0).standard_normal((32, 6)))
    assert abs(R.rankme(q) - 6.0) < 1e-4
    assert abs(R.rankme(np.eye(5, dtype=np.float32)) - 5.0) < 1e-4
    assert abs(R.rankme(np.eye(5, 9, dtype=np.float32)) - 5.0) < 1e-3        # n < d: four singular values are the padding


def test_reference_pair_sum_identity():
    """2 sum_{i<j} s_ij = ||sum_i zn_i||^2 - sum_i ||zn_i||^2"""
    rng = np.random.default_rng(1)
    for z in (rng.standard_normal((50, 9)).astype(np.float32), R.four_ones(40, 16, 2), np.vstack([np.zeros((2, 5)), rng.standard_normal((9, 5))])):
        zn = R.normalize(z)
        want = ((zn.sum(axis=0) ** 2).sum() - (zn * zn).sum()) / 2
        assert abs(R.pair_stats(z, 0.5)[1] - want) < 1e-10
        assert R.pair_stats(z, 0.0)[0] == len(z) * (len(z) - 1) / 2


@pytest.mark.parametrize("center", [False, True])
def test_gram_route_matches_svd_route(center):
    rng = np.random.default_rng(2)
    base = rng.standard_normal((1, 64))
    cases = [rng.standard_normal((300, 64)), np.abs(rng.standard_normal((200, 32))), base + 1e-3 * rng.standard_normal((150, 64)),
             rng.standard_normal((120, 8)) @ rng.standard_normal((8, 48)), rng.standard_normal((20, 64))]
    for z in cases:
        z = z.astype(np.float32)
        g, c = R.gram(z)
        assert abs(RS.rankme_from_gram(g, c, z.shape[0], center=center) - R.rankme(z, center=center)) <= 1e-6 * R.rankme(z, center=center)
    z = R.integer_rows(50, 7, 3)
    g, c = R.gram(z)
    assert g.dtype == np.int64 and np.array_equal(g, g.T) and np.array_equal(c, z.sum(axis=0).astype(np.int64))


# ---------------------------------------------------------------------------- the C ABI
def test_symbols_are_declared_bound_and_exported():
    assert ops.REPR_MAX_DIM == 256 and ops.REPR_MAX_ROWS == 2 ** 20
    for fn in ("repr_pair_stats", "repr_alignment_sum", "repr_gram"):
        assert callable(getattr(ops, fn))


def test_workspace_holds_no_matrix():
    ws = L.lib().gmp_repr_workspace_bytes
    assert 0 < ws(65535, 256) < 1 << 30                                      # the n x n matrix: 17 GB
    assert ws(65535, 256) <= 4 * 65535 * 256 + 64 * 8 * 256 * 256 + (1 << 20)
    assert 0 < ws(1, 1) <= ws(2, 1) and 0 < ws(1 << 20, 256)
    for n, d in [(2708, 256), (19717, 256), (65535, 256), (5000, 100)]:
        assert 0 < ws(n, d) <= ws(2 * n, d) <= 2 * ws(n, d)
    for bad in [(0, 8), (-1, 8), (5, 0), (5, 257), ((1 << 20) + 1, 8)]:
        assert ws(*bad) == 0


def pair_call(z=0x1000, n=9, d=8, t=2.0, out=0x2000, ws=0x3000, ws_bytes=1 << 24):
    """the pointers are never dereferenced by the host and nothing is launched on a refused call"""
    vp = ctypes.c_void_p
    return L.lib().gmp_repr_pair_stats(vp(z), n, d, t, vp(out), vp(ws), ws_bytes, None)


def align_call(z1=0x1000, z2=0x1800, n=9, d=8, alpha=2.0, out=0x2000, ws=0x3000, ws_bytes=1 << 24):
    vp = ctypes.c_void_p
    return L.lib().gmp_repr_alignment(vp(z1), vp(z2), n, d, alpha, vp(out), vp(ws), ws_bytes, None)


def gram_call(z=0x1000, n=9, d=8, gram=0x2000, colsum=0x2800, ws=0x3000, ws_bytes=1 << 24):
    vp = ctypes.c_void_p
    return L.lib().gmp_repr_gram(vp(z), n, d, vp(gram), vp(colsum), vp(ws), ws_bytes, None)


@pytest.mark.parametrize("call,kw", [(pair_call, dict(n=1)), (pair_call, dict(n=0)), (pair_call, dict(n=(1 << 20) + 1)), (pair_call, dict(d=0)),
                                     (pair_call, dict(d=257)), (pair_call, dict(t=-1.0)), (pair_call, dict(t=float("nan"))), (pair_call, dict(z=0)),
                                     (pair_call, dict(out=0)), (align_call, dict(n=0)), (align_call, dict(d=257)), (align_call, dict(alpha=0.0)),
                                     (align_call, dict(alpha=-2.0)), (align_call, dict(z2=0)), (align_call, dict(out=0)), (gram_call, dict(n=0)),
                                     (gram_call, dict(n=(1 << 24) + 1)), (gram_call, dict(d=0)), (gram_call, dict(d=257)), (gram_call, dict(z=0)),
                                     (gram_call, dict(gram=0)), (gram_call, dict(colsum=0))])
def test_bad_sizes_and_null_pointers_are_refused(call, kw):
    assert call(**kw) == ERR_ARG
    assert b"repr_" in L.lib().gmp_last_error_string()


@pytest.mark.parametrize("call", [pair_call, align_call, gram_call])
def test_a_short_workspace_is_refused(call):
    need = L.lib().gmp_repr_workspace_bytes(9, 8)
    assert call(ws_bytes=need - 1) == ERR_WORKSPACE and call(ws=0) == ERR_WORKSPACE


# ---------------------------------------------------------------------------- the flags
def test_pretrain_flag_is_off_by_default_and_takes_the_two_levels():
    base = ["--exp_name", "s4", "--seed", "1"]
    assert PT.parse_args(base).repr_stats == "off"
    for level in ("graph", "node", "off"):
        assert PT.parse_args(base + ["--repr-stats", level]).repr_stats == level
    with pytest.raises(SystemExit):
        PT.parse_args(base + ["--repr-stats", "edge"])
    with pytest.raises(ValueError, match="repr_stats"):
        PT.pretrain(PT.PretrainConfig("s4", 7), epochs=1, repr_stats="edge")


def test_finetune_flag_is_off_by_default_and_is_no_probe():
    a = FT.build_parser().parse_args(["--domain_name", "Cora_NC"] + BASE)
    assert a.repr_stats is False and FT.config_from_args(a).repr_stats is False
    assert FT.FinetuneConfig("Cora_NC", "full_finetune", "b1", 1).repr_stats is False
    a = FT.build_parser().parse_args(["--domain_name", "Cora_NC", "--repr-stats"] + BASE)
    assert FT.config_from_args(a).repr_stats is True
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--lp-engine", "--repr-stats"] + BASE)      # no class labels needed
    assert FT.config_from_args(a).repr_stats is True
    assert FT.FinetuneConfig("ENZYMES", "full_finetune", "b1", 1, gc_engine=True, repr_stats=True, knn_probe=5).repr_stats is True
    assert len(FT.PROBES) == 3 and all(p.field != "repr_stats" for p in FT.PROBES)


def test_finetune_refuses_the_flag_without_an_engine(monkeypatch):
    with pytest.raises(ValueError, match="repr_stats needs an active fine-tune engine.*--lp-engine"):
        FT.FinetuneConfig("Cora_LP", "full_finetune", "b1", 1, repr_stats=True)
    with pytest.raises(ValueError, match="repr_stats needs an active fine-tune engine.*--gc-engine"):
        FT.FinetuneConfig("ENZYMES", "full_finetune", "b1", 1, repr_stats=True)
    monkeypatch.setenv("GMP_FINETUNE_ENGINE", "0")
    with pytest.raises(ValueError, match="GMP_FINETUNE_ENGINE=0"):
        FT.FinetuneConfig("Cora_NC", "full_finetune", "b1", 1, repr_stats=True)
    assert FT.FinetuneConfig("Cora_NC", "full_finetune", "b1", 1).repr_stats is False         # off: nothing to refuse
