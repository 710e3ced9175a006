"""Host-side checks of the shortest-path kernel baseline (csrc/sp.hip, finetune/graph_baselines.py, --sp-baseline): that the two routes of
tests/sp_ref.py to the distances agree on every graph the GPU tests use, the reference's own invariances, what the kernel sees that
Weisfeiler-Lehman cannot, the flag and the config, and the new symbols.  The kernels themselves are compared against sp_ref bit for bit in
test_gpu_sp.py."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import sp_ref as R
import wl_ref
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd.finetune import finetune as FT, graph_baselines as GB

ROOT = Path(__file__).resolve().parents[1]
BASE = ["--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1", "--seed", "1"]
DISTS = (1, 2, 5, 1023)


@functools.lru_cache(maxsize=None)
def _fixed():
    b = R.make_batch(R.fixed_graphs())
    return b, R.batch_distances(b)


# ---------------------------------------------------------------------------- 1. two routes to the distances
def test_bfs_and_floyd_warshall_agree_on_the_fixed_set():
    b, dist = _fixed()
    fw = R.batch_distances(b, R.floyd_warshall_distances)
    assert all(np.array_equal(x, y) for x, y in zip(dist, fw))
    for md in DISTS:
        for use_labels in (True, False):
            a, c = R.features(b, md, 100, use_labels, dist=dist), R.features(b, md, 100, use_labels, dist=fw)
            assert all(np.array_equal(x, y) for x, y in zip(a, c)) and not a.status.any()
    full = R.features(b, 1023, 256, dist=dist)
    c = R.INDEX["cycle1024"]
    assert full.nuniq[c] == 512 and full.counts[c, :512].sum() == 523776                  # one key per distance; every pair counted
    assert full.counts[c, :511].tolist() == [1024] * 511 and full.counts[c, 511] == 512   # the antipodal pairs
    assert [R.unpack(k)[2] for k in full.keys[c, :512].tolist()] == list(range(1, 513))
    assert R.features(b, 5, 256, dist=dist).nuniq[c] == 5
    k40 = R.INDEX["k40"]
    assert R.row(full, k40) == {R.pack(0, 0, 1): 780}
    assert full.nuniq[R.INDEX["empty"]] == full.nuniq[R.INDEX["single"]] == full.nuniq[R.INDEX["two_isolated"]] == 0
    assert R.row(full, R.INDEX["edge"]) == {R.pack(0, 1, 1): 1}


def test_key_packing_round_trips():
    assert R.unpack(R.pack(5, 3, 7)) == (3, 5, 7)
    top = R.pack(2 ** 24 - 1, 2 ** 24 - 1, 1023)
    assert R.unpack(top) == (2 ** 24 - 1, 2 ** 24 - 1, 1023) and top < 2 ** 59
    assert R.pack(1, 0, 1) == R.pack(0, 1, 1) == (1 << 11) | 1


# ---------------------------------------------------------------------------- 2. node numbering does not matter
def test_reference_is_invariant_under_node_permutations():
    a, dist = _fixed()
    b = R.make_batch(R.permuted(R.fixed_graphs(), 3))
    db = R.batch_distances(b)
    assert not all(np.array_equal(x, y) for x, y in zip(dist, db))                         # (the permutation did move something)
    for use_labels in (True, False):
        fa, fb = R.features(a, 1023, 100, use_labels, dist=dist), R.features(b, 1023, 100, use_labels, dist=db)
        assert all(np.array_equal(x, y) for x, y in zip(fa, fb))
        assert np.array_equal(R.gram(fa, fa), R.gram(fb, fa))


# ---------------------------------------------------------------------------- 3. what 1-WL cannot tell apart
def test_c6_and_two_triangles_differ_where_wl_sees_no_difference():
    b, dist = _fixed()
    f = R.features(b, 1023, 256, dist=dist)
    c6, c3c3 = R.INDEX["c6"], R.INDEX["c3c3"]
    assert R.row(f, c6) == {R.pack(0, 0, 1): 6, R.pack(0, 0, 2): 6, R.pack(0, 0, 3): 3}
    assert R.row(f, c3c3) == {R.pack(0, 0, 1): 6}
    assert not np.array_equal(f.hist[c6], f.hist[c3c3])
    K = R.gram(f, f)
    sim = R.normalised_similarity(K, np.diag(K), np.diag(K))
    assert K[c6, c3c3] == 36 and sim[c6, c3c3] < 1.0 and sim[c6, c6] == 1.0
    wl = wl_ref.refine(b, 7, 256)
    assert np.array_equal(wl_ref.segment(wl.sorted, b.ptr, c6, 7), wl_ref.segment(wl.sorted, b.ptr, c3c3, 7))


def test_histogram_rows_sum_to_the_pair_count():
    b, dist = _fixed()
    for md in DISTS:
        for dim in (1, 100, 256):
            f = R.features(b, md, dim, dist=dist)
            pairs = np.array([sum(R.row(f, g).values()) for g in range(f.nuniq.size)])
            assert np.array_equal(f.hist.sum(axis=1), pairs)
            if md == 1:                                                                    # distance 1: the edges
                assert np.array_equal(pairs, [np.count_nonzero(np.triu(D, 1) == 1) for D in dist])
    assert np.array_equal(np.diag(R.gram(f, f)), R.self_similarity(f))


# ---------------------------------------------------------------------------- 4. the separable set
@pytest.mark.parametrize("use_labels,least_gap,half_digit", [(True, 0.0109, 5e-5), (False, 0.36, 5e-3)], ids=["zero labels", "degrees"])
def test_the_baseline_set_has_no_near_tie_at_the_kth_neighbour(use_labels, least_gap, half_digit):
    """The condition under which the device's top-k indices are pinned by numpy's: no query's k-th and (k + 1)-th similarities lie close
    (the smallest gap over the queries is 0.0109 with all-zero labels and 0.36 with degree labels), and the vote separates the classes."""
    graphs, y = R.baseline_graphs()
    nt, k = wl_ref.BASELINE_TRAIN, wl_ref.BASELINE_K
    ft, fe = R.features(R.make_batch(graphs[:nt]), 1023, 256, use_labels), R.features(R.make_batch(graphs[nt:]), 1023, 256, use_labels)
    sim = R.normalised_similarity(R.gram(fe, ft), R.self_similarity(fe), R.self_similarity(ft))
    assert sim.shape == (wl_ref.BASELINE_EVAL, nt) and k < nt
    top = -np.sort(-sim, axis=1)
    gap = float((top[:, k - 1] - top[:, k]).min())
    print("smallest gap at the k-th neighbour", gap)
    assert gap > 1e-9                                                                      # (fp64 rounding of a similarity: ~1e-16)
    assert abs(gap - least_gap) <= half_digit                                              # the recorded figure, to the digits it was recorded with
    idx = R.top_k(sim, k)
    weight = np.exp(np.take_along_axis(sim, idx, axis=1) / 0.07)                           # the vote of ops.knn_vote at its default temperature
    score = np.stack([(weight * (y[:nt][idx] == c)).sum(axis=1) for c in (0, 1)], axis=1)
    assert np.array_equal(score.argmax(axis=1), y[nt:])                                    # k-NN accuracy 1.0


# ---------------------------------------------------------------------------- 5. flag and config
def _argv(domain, value):
    return ["--domain_name", domain, "--sp-baseline", str(value)] + BASE


def test_flag_parses_into_the_config_and_is_off_by_default():
    assert (ops.SP_MAX_DIST, ops.SP_MAX_GRAPH_NODES, ops.SP_MAX_DIM, ops.SP_MAX_LABEL) == (1023, 1024, 256, 2 ** 24)
    cfg = FT.config_from_args(FT.build_parser().parse_args(_argv("PTC_MR", 8)))
    assert cfg.sp_baseline == 8 and type(cfg.sp_baseline) is int
    assert not cfg.gc_engine and not cfg.wl_baseline and not any(getattr(cfg, p.field) for p in FT.PROBES)
    assert not any(getattr(cfg, b.field) for b in FT.BASELINES if b.field != "sp_baseline")
    assert FT.config_from_args(FT.build_parser().parse_args(["--domain_name", "PTC_MR"] + BASE)).sp_baseline == 0
    assert FT.FinetuneConfig("ENZYMES", "full_finetune", "b1", 1).sp_baseline == 0
    assert FT.FinetuneConfig("ENZYMES", "full_finetune", "b1", 1, sp_baseline=ops.SP_MAX_DIST).sp_baseline == 1023
    both = FT.config_from_args(FT.build_parser().parse_args(
        ["--domain_name", "ENZYMES", "--gc-engine", "--sp-baseline", "1023", "--wl-baseline", "3", "--knn-probe", "5"] + BASE))
    assert (both.sp_baseline, both.wl_baseline, both.knn_probe, both.gc_engine) == (1023, 3, 5, True)
    assert "--sp-baseline" in FT.__doc__


def test_flag_is_bounded():
    for bad in (-1, ops.SP_MAX_DIST + 1):
        with pytest.raises(ValueError, match=f"sp_baseline={bad} .*<= {ops.SP_MAX_DIST}"):
            FT.FinetuneConfig("PTC_MR", "full_finetune", "b1", 1, sp_baseline=bad)
    for bad in (0, ops.SP_MAX_DIST + 1):                                                   # the API has no "off": distance 0 is refused there
        with pytest.raises(ValueError, match="sp_baseline"):
            GB.sp_baseline([], [], 2, bad)


@pytest.mark.parametrize("domain", ["Cora_NC", "Cora_LP"])
def test_flag_is_refused_off_its_task_type_with_the_tables_message(domain):
    with pytest.raises(ValueError, match="sp_baseline"):
        FT.config_from_args(FT.build_parser().parse_args(_argv(domain, 8)))
    with pytest.raises(ValueError, match=f"sp_baseline applies to the graph-classification domains \\(ENZYMES / PTC_MR\\), not to {domain}"):
        FT.FinetuneConfig(domain_name=domain, finetune_strategy="full_finetune", pretrained_scheme="b1", seed=1, sp_baseline=8)
    assert FT.FinetuneConfig(domain, "full_finetune", "b1", 1).sp_baseline == 0


def test_the_row_is_in_the_table_and_the_field_before_wl_baseline():
    assert [b.field for b in FT.BASELINES].index("sp_baseline") == 5 and isinstance(FT.BASELINES[5], FT.Baseline)   # after the five older rows
    assert [b.field for b in FT.BASELINES].count("sp_baseline") == 1
    fields = list(FT.FinetuneConfig.__dataclass_fields__)
    assert fields[-3:] == ["feat_baseline", "sp_baseline", "wl_baseline"]
    assert "sp_baseline" not in {p.field for p in FT.PROBES}


# ---------------------------------------------------------------------------- 6. the new symbols
def test_symbols_are_declared_bound_and_exported():
    for name, count in (("gmp_sp_workspace_bytes", 2), ("gmp_sp_max_unique", 1), ("gmp_sp_features", 19), ("gmp_sp_gram", 12)):
        assert count == len(L._SIGS[name][1]), name
    lib = L.lib()
    assert lib.gmp_sp_workspace_bytes(600, 1024) == 0                                      # everything lives in LDS
    assert lib.gmp_sp_max_unique(256) >= 4096 and lib.gmp_sp_max_unique(1024) >= 1024
    assert [lib.gmp_sp_max_unique(n) for n in (0, 39, 256, 257, 1024)] == [R.max_unique(n) for n in (0, 39, 256, 257, 1024)]
    assert ops.sp_max_unique(620) == R.max_unique(620)


def test_ops_refuse_host_tensors():
    b, _ = _fixed()
    ptr, rowptr, col = torch.from_numpy(b.ptr), torch.from_numpy(b.rowptr), torch.from_numpy(b.col)
    with pytest.raises(L.GnnmpError, match="GPU"):
        ops.sp_features(ptr, rowptr, col, None, 5, 256, 1024)
    k, c, n = torch.zeros(2, 4, dtype=torch.int64), torch.zeros(2, 4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32)
    with pytest.raises(L.GnnmpError, match="GPU"):
        ops.sp_gram(k, c, n, k, c, n)


def test_sp_kernel_source_is_integer_only():
    csrc = ROOT / "gnn_pretraining_amd" / "csrc"
    src = "".join((csrc / name).read_text() for name in ("sp.hip", "bit_bfs.h", "graph_block.h"))
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(float|double|__half)\b", code)
    assert not re.search(r"\basm\b", code)
    names = [m.group(1) for m in re.finditer(r"atomic(?:Add|Or|CAS)\(&?([\w.]+)", code)]
    assert names and set(names) <= {"tb.key", "tb.count", "tb.used", "A", "skipped", "bins"}, names   # integer LDS atomics only
