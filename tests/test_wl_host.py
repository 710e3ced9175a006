"""Host-side checks of the Weisfeiler-Lehman subtree baseline (csrc/wl.hip, finetune/graph_baselines.py, --wl-baseline): that the hashed
definition of tests/wl_ref.py IS Weisfeiler-Lehman on every graph set the GPU tests use, the reference's own invariances, initial_labels,
the flag and the config, and the new symbols.  The kernels themselves are compared against wl_ref bit for bit in test_gpu_wl.py."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import wl_ref as R
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd.finetune import finetune as FT, graph_baselines as GB

ROOT = Path(__file__).resolve().parents[1]
H = ops.WL_MAX_ITERS


@functools.lru_cache(maxsize=None)
def _sets():
    """name -> (batch, use_labels): every graph set and label mode a GPU test refines."""
    fixed = R.fixed_graphs()
    base, _ = R.baseline_graphs()
    return {"fixed/labels": (R.make_batch(fixed), True), "fixed/degrees": (R.make_batch(fixed), False),
            "fixed/wide labels": (R.make_batch(R.with_wide_labels(fixed)), True),
            "fixed/permuted": (R.make_batch(R.permuted(fixed, 3)), True), "baseline/degrees": (R.make_batch(base), False)}


# ---------------------------------------------------------------------------- 1. the hash is Weisfeiler-Lehman on these graphs
@pytest.mark.parametrize("name", ["fixed/labels", "fixed/degrees", "fixed/wide labels", "fixed/permuted", "baseline/degrees"])
def test_hashed_partition_is_the_classical_one_and_no_colour_repeats_across_iterations(name):
    batch, use_labels = _sets()[name]
    ref, ids = R.refine(batch, H, 256, use_labels), R.classical(batch, H, use_labels)
    for t in range(H + 1):
        assert R.same_partition(ref.colors[t], ids[t]), (name, t)
    seen = [set(ref.colors[t].tolist()) for t in range(H + 1)]
    assert not any(seen[i] & seen[j] for i in range(H + 1) for j in range(i)), name
    assert not ref.status.any()


def test_mix_matches_splitmix64_by_hand():
    # splitmix64 seeded with 0: the first output is mix(0 + K1)
    assert int(R.mix(np.array([0x9E3779B97F4A7C15], dtype=np.uint64))[0]) == 0xE220A8397B1DCDAF
    assert int(R.mix(np.array([0], dtype=np.uint64))[0]) == 0


# ---------------------------------------------------------------------------- 2. the Gram is the subtree kernel
def test_reference_gram_is_the_classical_subtree_kernel():
    batch, _ = _sets()["fixed/labels"]
    h = 3
    ref, ids = R.refine(batch, h, 256), R.classical(batch, h)
    K = R.gram(ref.sorted, batch.ptr, ref.sorted, batch.ptr, h)
    assert np.array_equal(K, R.classical_gram(ids, batch.ptr, ids, batch.ptr))
    assert np.array_equal(K, K.T)
    for g in range(batch.ptr.size - 1):
        _, counts = np.unique(R.segment(ref.sorted, batch.ptr, g, h), return_counts=True)
        assert K[g, g] == int(np.sum(counts.astype(np.int64) ** 2))
    c = R.INDEX["cycle1024"]
    assert K[c, c] == 1024 * 1024 * (h + 1) and not K[R.INDEX["empty"]].any()
    k40 = R.INDEX["k40"]
    assert K[k40, k40] == 40 * 40 * (h + 1)


# ---------------------------------------------------------------------------- 3. node numbering does not matter
def test_reference_is_invariant_under_node_permutations():
    fixed = R.fixed_graphs()
    a, b = R.make_batch(fixed), R.make_batch(R.permuted(fixed, 3))
    h = 3
    for use_labels in (True, False):
        ra, rb = R.refine(a, h, 100, use_labels), R.refine(b, h, 100, use_labels)
        assert np.array_equal(ra.sorted, rb.sorted) and np.array_equal(ra.hist, rb.hist)
        assert np.array_equal(R.gram(ra.sorted, a.ptr, ra.sorted, a.ptr, h), R.gram(rb.sorted, b.ptr, ra.sorted, a.ptr, h))
    assert not np.array_equal(R.refine(a, h, 100).colors, R.refine(b, h, 100).colors)      # (the permutation did move something)


# ---------------------------------------------------------------------------- 4. what 1-WL cannot tell apart
def test_c6_and_two_triangles_have_equal_segments():
    batch, _ = _sets()["fixed/labels"]
    ref = R.refine(batch, H, 256)
    a, b = R.segment(ref.sorted, batch.ptr, R.INDEX["c6"], H), R.segment(ref.sorted, batch.ptr, R.INDEX["c3c3"], H)
    assert a.size == 6 * (H + 1) and np.array_equal(a, b)
    assert np.array_equal(ref.hist[R.INDEX["c6"]], ref.hist[R.INDEX["c3c3"]])
    assert not np.array_equal(ref.hist[R.INDEX["c6"]], ref.hist[R.INDEX["k40"]])


def test_histogram_rows_count_every_colour_once():
    batch, _ = _sets()["fixed/labels"]
    for dim in (1, 100, 256):
        ref = R.refine(batch, 3, dim)
        assert np.array_equal(ref.hist.sum(axis=1), 4 * np.diff(batch.ptr))


def test_the_baseline_set_has_no_near_tie_at_the_kth_neighbour():
    """The condition under which the device's top-k indices are pinned by numpy's: in the reference no query's k-th and (k + 1)-th
    similarities lie within 1e-9 relative of each other."""
    graphs, y = R.baseline_graphs()
    nt, h, k = R.BASELINE_TRAIN, R.BASELINE_ITERS, R.BASELINE_K
    tb, eb = R.make_batch(graphs[:nt]), R.make_batch(graphs[nt:])
    rt, re_ = R.refine(tb, h, 256, False), R.refine(eb, h, 256, False)
    sim = R.normalised_similarity(R.gram(re_.sorted, eb.ptr, rt.sorted, tb.ptr, h), np.diag(R.gram(re_.sorted, eb.ptr, re_.sorted, eb.ptr, h)),
                                  np.diag(R.gram(rt.sorted, tb.ptr, rt.sorted, tb.ptr, h)))
    assert sim.shape == (R.BASELINE_EVAL, nt) and k < nt
    top = -np.sort(-sim, axis=1)
    assert np.all(top[:, k - 1] - top[:, k] > 1e-9 * np.abs(top[:, k - 1]))
    assert set(y[:nt].tolist()) == set(y[nt:].tolist()) == {0, 1}


# ---------------------------------------------------------------------------- 5. initial_labels
def test_initial_labels_reads_one_hot_rows_only():
    one_hot = torch.eye(5)[torch.tensor([3, 0, 4, 4, 1])]
    assert GB.initial_labels(one_hot).tolist() == [3, 0, 4, 4, 1] and GB.initial_labels(one_hot).dtype == torch.int64
    x = torch.randn(7, 5, generator=torch.Generator().manual_seed(0))
    assert GB.initial_labels((x - x.mean(0)) / x.std(0)) is None                          # standardised features: degrees
    two = one_hot.clone()
    two[2, 0] = 1.0
    assert GB.initial_labels(two) is None                                                 # a row with two ones
    zero = one_hot.clone()
    zero[1] = 0.0
    assert GB.initial_labels(zero) is None                                                # an all-zero row
    half = one_hot.clone() * 0.5
    assert GB.initial_labels(half) is None                                                # one non-zero, but not 1
    assert GB.initial_labels(torch.zeros(3, 0)) is None


# ---------------------------------------------------------------------------- 6. flag and config
def test_wl_baseline_rounds_are_bounded():
    assert (ops.WL_MAX_ITERS, ops.WL_MAX_DIM, ops.WL_MAX_GRAPH_NODES) == (7, 256, 1024)
    for bad in (-1, H + 1):
        with pytest.raises(ValueError, match="wl_baseline"):
            FT.FinetuneConfig("PTC_MR", "full_finetune", "b1", 1, wl_baseline=bad)
    for bad in (0, H + 1):                                                                # the API has no "off": zero rounds are refused there
        with pytest.raises(ValueError, match="wl_baseline"):
            GB.wl_baseline([], [], 2, bad)


def test_ops_refuse_host_tensors():
    b, _ = _sets()["fixed/labels"]
    ptr, rowptr, col = torch.from_numpy(b.ptr), torch.from_numpy(b.rowptr), torch.from_numpy(b.col)
    with pytest.raises(L.GnnmpError, match="GPU"):
        ops.wl_refine(ptr, rowptr, col)
    with pytest.raises(L.GnnmpError, match="GPU"):
        ops.wl_gram(torch.zeros(4, dtype=torch.int64), ptr, torch.zeros(4, dtype=torch.int64), ptr, 3)


# ---------------------------------------------------------------------------- 7. the new symbols
def test_wl_kernel_source_is_integer_only():
    csrc = ROOT / "gnn_pretraining_amd" / "csrc"
    src = (csrc / "wl.hip").read_text() + (csrc / "graph_block.h").read_text()              # the header holds the row walk, the hash, the frames
    code = re.sub(r"//[^\n]*", "", src)
    assert not re.search(r"\b(float|double|__half)\b", code)
    assert not re.search(r"\basm\b|__builtin_amdgcn", code)
    names = [m.group(1) for m in re.finditer(r"atomicAdd\(&(\w+)", code)]
    assert names and set(names) <= {"bins", "skipped"}, names                             # integer LDS counters only
    header = re.sub(r"//[^\n]*", "", (csrc / "graph_block.h").read_text())                 # the shared header on its own: no float, no atomic
    assert not re.search(r"\b(float|double|__half)\b", header) and "atomic" not in header.replace("std::atomic", "")
