"""Host-side contract of the structural link baselines (csrc/lp_heuristics.hip, finetune/link_heuristics.py, --lp-heuristics): the CPU
reference of tests/lp_heur_ref.py on a graph small enough to score by hand, the node weights, the flag and its precondition, the
declaration / binding / export of the five C-ABI entry points, the workspace size, and a kernel source without float atomics."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lp_heur_ref as R
from gnn_pretraining_amd import _lib as L

ROOT = Path(__file__).resolve().parents[1]

# a triangle 0-1-2, the path 2-3-4 hanging off it (4 is a pendant node), 5 isolated.  Given one way round, once doubled, with a loop.
EDGES = np.array([[0, 0, 1, 2, 3, 1, 5], [1, 2, 2, 3, 4, 0, 5]])
# N(0) = {1, 2}, N(1) = {0, 2}, N(2) = {0, 1, 3}, N(3) = {2, 4}, N(4) = {3}, N(5) = {}: degrees 2 2 3 2 1 0
LN2, LN3 = math.log(2.0), math.log(3.0)


def _graph():
    return R.simple_csr(EDGES, 6)


def test_reference_builds_the_simple_graph():
    rowptr, col = _graph()
    assert rowptr.tolist() == [0, 2, 4, 7, 9, 10, 10]
    assert col.tolist() == [1, 2, 0, 2, 0, 1, 3, 2, 4, 3]


def test_reference_scores_three_pairs_by_hand():
    rowptr, col = _graph()
    src, dst = [0, 2, 4], [1, 4, 5]                      # common neighbours {2}, {3}, {}
    want = {"cn": [1.0, 1.0, 0.0],
            "jaccard": [1 / 3, 1 / 3, 0.0],             # 1 / (2 + 2 - 1), 1 / (3 + 1 - 1), 0 / (1 + 0 - 0)
            "aa": [float(np.float32(1 / LN3)), float(np.float32(1 / LN2)), 0.0],   # 1 / ln deg(2), 1 / ln deg(3)
            "ra": [float(np.float32(1 / 3)), 0.5, 0.0]}
    for kind in R.KINDS:
        got = R.pair_scores(rowptr, col, src, dst, R.weights(rowptr, kind), "jaccard" if kind == "jaccard" else "sum")[0]
        assert got.tolist() == want[kind], kind
    assert R.pair_scores(rowptr, col, [5, 9], [5, 0], None, "jaccard")[0].tolist() == [0.0, 0.0]      # the empty union; a node outside the graph


def test_reference_ranks_by_hand_with_zero_ties_and_the_half_tie_rule():
    rowptr, col = _graph()
    # (0, 3), common neighbours: the candidates 1, 2, 4, 5 score 1, 1, 0, 0 against the true 1: rank 1 + 0 + 2 / 2
    st, ng, ne = R.ranks(rowptr, col, [0], [3])
    assert (st.tolist(), ng.tolist(), ne.tolist(), R.rank_of(ng, ne).tolist()) == ([1.0], [0], [2], [2.0])
    # (0, 5): the true pair scores 0 and ties with candidate 4, below 1, 2 and 3: rank 1 + 3 + 1 / 2
    st, ng, ne = R.ranks(rowptr, col, [0], [5])
    assert (st.tolist(), ng.tolist(), ne.tolist(), R.rank_of(ng, ne).tolist()) == ([0.0], [3], [1], [4.5])
    # the filter takes 1 and 2 (and, ignored, 77) out of the first query: 4 and 5 are left, both below
    st, ng, ne = R.ranks(rowptr, col, [0], [3], filt=R.filter_rows([[0, 0, 0], [1, 2, 77]], 6))
    assert (ng.tolist(), ne.tolist()) == ([0], [0])
    # (2, 4): Adamic-Adar 1 / ln 2 through z = 3; candidates 0 and 1 reach 2 through a degree-2 node too, 3 and 5 score 0
    for kind, true in (("aa", np.float32(1 / LN2)), ("ra", np.float32(0.5))):
        st, ng, ne = R.ranks(rowptr, col, [2], [4], R.weights(rowptr, kind))
        assert (st.tolist(), ng.tolist(), ne.tolist()) == ([float(true)], [0], [2]), kind
    # Jaccard of (2, 4) is 1 / 3; candidates 0 and 1 have 1 / (3 + 2 - 1) = 1 / 4: nothing above, nothing equal
    st, ng, ne = R.ranks(rowptr, col, [2], [4], None, "jaccard")
    assert (st.tolist(), ng.tolist(), ne.tolist()) == ([1 / 3], [0], [0])
    # equal quotients from different counts: with the true pair (4, 5) at 0 / 1 every candidate 0 / k ties
    st, ng, ne = R.ranks(rowptr, col, [5], [4], None, "jaccard")
    assert (ng.tolist(), ne.tolist()) == ([0], [4])


def test_node_weights_follow_the_float64_rule_rounded_once():
    from gnn_pretraining_amd.finetune.link_heuristics import KINDS, node_weights
    assert KINDS == ("cn", "jaccard", "aa", "ra")
    deg = torch.tensor([0, 1, 2, 3, 7, 168, 100000], dtype=torch.int32)
    assert node_weights(deg, "cn") is None and node_weights(deg, "jaccard") is None
    aa, ra = node_weights(deg, "aa"), node_weights(deg, "ra")
    assert aa.dtype == torch.float32 and ra.dtype == torch.float32 and aa.device.type == "cpu"
    assert aa[:2].tolist() == [0.0, 0.0] and ra[0].item() == 0.0 and ra[1].item() == 1.0
    for i, d in enumerate(deg.tolist()):
        if d >= 2:
            assert aa[i].item() == float(np.float32(1.0 / math.log(d))), d
        if d >= 1:
            assert ra[i].item() == float(np.float32(1.0 / d)), d
    rowptr = np.concatenate([[0], np.cumsum(deg.numpy().astype(np.int64))])
    assert np.array_equal(aa.numpy(), R.weights(rowptr, "aa")) and np.array_equal(ra.numpy(), R.weights(rowptr, "ra"))
    with pytest.raises(ValueError):
        node_weights(deg, "katz")


def test_tile_size_is_exported_and_sane():
    tc = L.lib().gmp_lp_cn_tile_nodes()
    assert tc >= 64 and tc % 32 == 0 and tc * 4 <= 64 * 1024                               # a bitmap of whole words, an accumulator inside static LDS


def test_rank_workspace_is_linear_in_queries_plus_nodes():
    size = L.lib().gmp_lp_cn_rank_workspace_bytes
    assert size(1024, 100000) < 16 * 2 ** 20                   # the dense scores alone would be 1024 * 100000 * 4 B = 400 MB
    for Q, N in ((1, 1000), (64, 2708), (1024, 100000), (4096, 50000)):
        small, big = size(Q, N), size(2 * Q, 2 * N)
        assert big <= 2 * small + 4096, (Q, N, small, big)
        assert small <= 4096 * (Q + N) + 4096, (Q, N, small)


def test_heuristics_kernel_source_has_no_float_atomics():
    src = "".join((ROOT / "gnn_pretraining_amd" / "csrc" / f).read_text() for f in ("lp_heuristics.hip", "csr_graph.h"))     # the kernels and their row helper
    names = [m.group(1) for m in re.finditer(r"atomicAdd\(&(\w+)", src)]
    assert names and set(names) <= {"cnt", "n_greater", "n_equal", "violations"}, names    # integer counts only
    assert not re.search(r"__hip_atomic|unsafeAtomic|atomicAdd\([^&]|atomicExch|atomicCAS", src)
    assert "__shared__ int cnt[" in src and not re.search(r"float\s*\*\s*(__restrict__\s+)?(n_greater|n_equal|violations)\b", src)
