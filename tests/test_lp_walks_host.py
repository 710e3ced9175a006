"""Host-side contract of the walk-based link baselines (csrc/lp_walk.hip, finetune/link_walks.py, --lp-walks): the CPU reference of
tests/lp_walk_ref.py on a graph small enough to work by hand, its subnormal case, the three parametrisations, the flag and its
refusals, the declaration / binding / export of the five C-ABI entry points, the storage limits and the workspace rule, and a kernel
source without float atomics."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import lp_walk_ref as W
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd.finetune import finetune as FT

ROOT = Path(__file__).resolve().parents[1]

# the graph of test_lp_heuristics_host.py: a triangle 0-1-2, the path 2-3-4 hanging off it, 5 isolated
EDGES = np.array([[0, 0, 1, 2, 3, 1, 5], [1, 2, 2, 3, 4, 0, 5]])


def _graph():
    return W.simple_csr(EDGES, 6)


def test_reference_walk_sum_by_hand():
    """From 4 with damping 1/2: y_1 = e_3 / 2; y_2 = (e_2 + e_4) / 4; y_3 = (e_0 + e_1 + e_3 + e_3) / 8 (3 is reached from 2 and from 4)."""
    rowptr, col = _graph()
    acc = W.walk_acc(rowptr, col, [4], 3, 0.5)
    assert acc.dtype == np.float32 and acc.tolist() == [[0.125, 0.125, 0.25, 0.75, 0.25, 0.0]]
    assert W.walk_acc(rowptr, col, [4], 1, 0.5).tolist() == [[0.0, 0.0, 0.0, 0.5, 0.0, 0.0]]
    assert W.walk_acc(rowptr, col, [5, -1, 6], 3, 0.5).tolist() == [[0.0] * 6] * 3        # isolated; outside the graph
    assert W.pair_scores(rowptr, col, [4, 4, 4, 9], [3, 5, 6, 3], 3, 0.5).tolist() == [0.75, 0.0, 0.0, 0.0]


def test_reference_hops_by_hand():
    rowptr, col = _graph()
    dist = W.hop_dist(rowptr, col, 4)
    assert dist[:5].tolist() == [3, 3, 2, 1, 0] and dist[5] == W.FAR
    assert W.cut_dist(dist, 3).tolist() == [3, 3, 2, 1, 0, 4]
    assert W.hop_scores(dist, 3).tolist() == [-3.0, -3.0, -2.0, -1.0, 0.0, -4.0]           # 5 is unreachable: -(R + 1)
    assert W.hop_scores(dist, 2).tolist() == [-3.0, -3.0, -2.0, -1.0, 0.0, -3.0]           # at R = 2 the nodes 0 and 1 are as far as 5
    assert W.all_scores(rowptr, col, [7], 3, mode="hops").tolist() == [[-4.0] * 6]         # a source outside the graph
    assert W.pair_scores(rowptr, col, [4, 4], [0, 6], 3, mode="hops").tolist() == [-3.0, -4.0]


def test_reference_ranks_by_hand_with_a_tie():
    rowptr, col = _graph()
    # (4, 0): the true pair scores 1/8; of the candidates 1, 2, 3, 5 (4 is the source) 2 and 3 are above (1/4, 3/4), 1 ties, 5 is below:
    # rank 1 + 2 + 1 / 2
    st, ng, ne = W.ranks(rowptr, col, [4], [0], 3, 0.5)
    assert (st.tolist(), ng.tolist(), ne.tolist(), W.rank_of(ng, ne).tolist()) == ([0.125], [2], [1], [3.5])
    # the same in hops: -3 against -3 (1), -2 (2), -1 (3), -4 (5)
    st, ng, ne = W.ranks(rowptr, col, [4], [0], 3, mode="hops")
    assert (st.tolist(), ng.tolist(), ne.tolist()) == ([-3.0], [2], [1])
    # the filter takes 2 (and, ignored, 77 and another source's row) out
    filt = W.filter_rows([[4, 4, 3], [2, 77, 1]], 6)
    st, ng, ne = W.ranks(rowptr, col, [4], [0], 3, 0.5, filt=filt)
    assert (ng.tolist(), ne.tolist()) == ([1], [1])
    # (4, 5): the true pair scores 0, every candidate 0 .. 3 is above
    st, ng, ne = W.ranks(rowptr, col, [4], [5], 3, 0.5)
    assert (st.tolist(), ng.tolist(), ne.tolist()) == ([0.0], [4], [0])


def test_reference_keeps_subnormals():
    """A path 0 - 1 - ... - 6 and the isolated node 7, damping 2^-26, five rounds from 0: node 5 is first reached by the one walk of
    length 5 and holds 2^-130, below the smallest normal float32 (2^-126)."""
    rowptr, col = W.simple_csr([list(range(6)), list(range(1, 7))], 8)
    acc = W.walk_acc(rowptr, col, [0], 5, 2.0 ** -26)[0]
    assert acc[5] == np.float32(2.0 ** -130) and 0 < acc[5] < np.finfo(np.float32).tiny
    assert acc[6] == 0.0 and acc[7] == 0.0
    st, ng, ne = W.ranks(rowptr, col, [0, 0, 0], [5, 6, 7], 5, 2.0 ** -26)
    assert ng.tolist() == [4, 5, 5] and ne.tolist() == [0, 1, 1]                           # 5 stands above 6 and 7, which tie at 0
    assert W.all_scores(rowptr, col, [0], 5, mode="hops")[0].tolist() == [0.0, -1.0, -2.0, -3.0, -4.0, -5.0, -6.0, -6.0]


def test_three_kinds_are_parametrisations_rounded_once():
    from gnn_pretraining_amd.finetune import link_heuristics as LH, link_walks as LW
    assert LW.KINDS == ("katz", "ppr", "hops") == W.KINDS and LH.KINDS == ("cn", "jaccard", "aa", "ra")
    assert LW.KATZ_BETA == 0.05 == W.KATZ_BETA and LW.PPR_ALPHA == 0.15 == W.PPR_ALPHA
    assert LW.damping_of("katz") == float(np.float32(0.05)) and LW.damping_of("ppr") == float(np.float32(1.0 - 0.15))
    assert LW.damping_of("katz") != 0.05 and LW.damping_of("ppr") != 0.85                # the fp32 values, as Python floats
    with pytest.raises(ValueError):
        LW.damping_of("cn")
    rowptr, _ = _graph()
    w, a, mode = W.params(rowptr, "ppr")
    assert mode == "sum" and float(a) == LW.damping_of("ppr")
    deg = torch.as_tensor(np.diff(rowptr))
    assert np.array_equal(LH.node_weights(deg, "ra").numpy(), w) and w.tolist() == [0.5, 0.5, float(np.float32(1 / 3)), 0.5, 1.0, 0.0]
    assert W.params(rowptr, "katz")[0] is None and float(W.params(rowptr, "katz")[1]) == LW.damping_of("katz")
    assert W.params(rowptr, "hops")[0] is None and W.params(rowptr, "hops")[2] == "hops"
    assert ops.LP_WALK_MAX_ROUNDS == 64 and ops.LP_WALK_MODES == {"sum": 0, "hops": 1}


def test_katz_is_the_truncated_power_series():
    """sum over l <= R of beta^l (A^l)[s, c] in float64 agrees with the float32 fold to float32 precision."""
    rowptr, col = _graph()
    A = np.zeros((6, 6))
    for v in range(6):
        A[v, col[rowptr[v]:rowptr[v + 1]]] = 1.0
    want = sum(0.05 ** l * np.linalg.matrix_power(A, l) for l in range(1, 5))
    got = W.walk_acc(rowptr, col, np.arange(6), 4, np.float32(0.05)).astype(np.float64)
    assert np.allclose(got, want, rtol=1e-6, atol=0.0)
    # rooted PageRank over alpha: y_l = ((1 - alpha) A D^-1)^l e_s
    w, a, _ = W.params(rowptr, "ppr")
    P = A * w.astype(np.float64)[None, :]
    want = sum(0.85 ** l * np.linalg.matrix_power(P, l) for l in range(1, 5)).T           # row s: the scores of source s
    assert np.allclose(W.walk_acc(rowptr, col, np.arange(6), 4, a, w).astype(np.float64), want, rtol=1e-6, atol=0.0)


@pytest.mark.parametrize("rounds", [-1, 65])
def test_lp_walks_rounds_out_of_range_are_refused(rounds):
    with pytest.raises(ValueError, match="lp_walks"):
        FT.FinetuneConfig("Cora_LP", "full_finetune", "b1", 1, lp_walks=rounds)


def test_walk_kinds_stay_out_of_link_heuristics():
    from gnn_pretraining_amd.finetune import link_heuristics as LH, link_walks as LW
    with pytest.raises(ValueError):
        LH.node_weights(torch.tensor([1, 2]), "katz")
    with pytest.raises(ValueError):
        LW.walk_scores(torch.zeros(2, 0, dtype=torch.int64), 4, torch.zeros(2, 0, dtype=torch.int64), "aa", 3)


def test_storage_limits():
    lds, blocks = L.lib().gmp_lp_walk_lds_nodes(), L.lib().gmp_lp_walk_resident_blocks()
    assert lds >= 8192
    assert 1 <= blocks <= 1024
    assert 2 * 4 * lds + lds // 8 <= 160 * 1024                                          # y_prev, y_next and the filter bitmap inside one CU's LDS


def test_workspace_rule():
    size = L.lib().gmp_lp_walk_workspace_bytes
    lds, blocks = L.lib().gmp_lp_walk_lds_nodes(), L.lib().gmp_lp_walk_resident_blocks()
    for Q in (1, 97, blocks, 10 * blocks):
        for N in (0, 1, 2708, lds):
            assert size(Q, N) == 0, (Q, N)                                               # served from LDS
    for N in (lds + 1, 2 * lds + 77, 65535, 1000003):
        for Q in (1, 5, blocks - 1, blocks, blocks + 1, 1000 * blocks):
            got = size(Q, N)
            assert got == size(min(Q, blocks), N), (Q, N)                                # no growth with Q beyond the resident blocks
            assert 12 * N * min(Q, blocks) <= got <= blocks * (16 * N + 4096), (Q, N, got)       # room for three vectors a block
        assert size(1, N) < size(2, N) < size(blocks, N)


def test_walk_kernel_source_has_no_float_atomics():
    src = "".join((ROOT / "gnn_pretraining_amd" / "csrc" / f).read_text() for f in ("lp_walk.hip", "csr_graph.h"))     # the kernels and their row helper
    names = [m.group(1) for m in re.finditer(r"atomicAdd\(&(\w+)", src)]
    assert names and set(names) <= {"cnt"}, names                                        # integer counts in LDS only
    assert not re.search(r"__hip_atomic|unsafeAtomic|atomicAdd\([^&]|atomicExch|atomicCAS", src)
    assert "__shared__ int cnt[" in src and not re.search(r"float\s*\*\s*(__restrict__\s+)?(n_greater|n_equal)\b", src)
    assert not re.search(r"hipMemsetAsync|atomic\w*\(&?(score|n_greater|n_equal)", src)     # one block per query stores its outputs: no memset, no output atomics
