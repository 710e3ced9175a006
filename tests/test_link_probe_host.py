"""Host-side contract of the embedding link probe (csrc/emb_link.hip, finetune/link_probe.py, --link-probe): the CPU reference of
tests/link_probe_ref.py on four nodes worked by hand -- every exclusion and the half tie -- the AUC with a tie, the flag and its
refusals, the declaration / binding / export of the three C-ABI entry points, and the Python layer's refusals."""
import math

import numpy as np
import pytest
import torch

import link_probe_ref as R
from gnn_pretraining_amd import _lib as L, ops
from gnn_pretraining_amd._lib import GnnmpError
from gnn_pretraining_amd.finetune import finetune as FT

BASE = ["--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1", "--seed", "1"]

# four nodes in the plane; inner products        cosines (r = sqrt(1/2))
#   0 (1, 0)      1 2 1 0                        1 1 r 0
#   1 (2, 0)      2 4 2 0                        1 1 r 0
#   2 (1, 1)      1 2 2 3                        r r 1 r
#   3 (0, 3)      0 0 3 9                        0 0 r 1
H = np.array([[1.0, 0.0], [2.0, 0.0], [1.0, 1.0], [0.0, 3.0]])


def _counts(src, dst, mode="dot", filt=None):
    st, ng, ne = R.ranks(R.scores(H, mode), src, dst, filt)
    return st.tolist(), ng.tolist(), ne.tolist()


def test_reference_scores_by_hand():
    assert R.scores(H, "dot").tolist() == [[1, 2, 1, 0], [2, 4, 2, 0], [1, 2, 2, 3], [0, 0, 3, 9]]
    r = math.sqrt(0.5)
    assert np.allclose(R.scores(H, "cos"), [[1, 1, r, 0], [1, 1, r, 0], [r, r, 1, r], [0, 0, r, 1]], rtol=0, atol=1e-15)
    assert R.scores(np.zeros((2, 3)), "cos").tolist() == [[0, 0], [0, 0]]                   # a zero row scores 0, not nan
    assert R.pair_scores(H, [0, 3, -1, 2, 4], [1, 3, 0, 9, 4], "dot").tolist() == [2, 9, 0, 0, 0]        # outside [0, N): a zero row


def test_reference_ranks_by_hand_every_exclusion_counts():
    # (0, 2): the true pair scores 1.  Row 0 is 1 2 1 0: node 1 is above, node 3 below.  The source's own entry (c == src) is 1 and
    # the destination's (c == dst) is 1 as well: counting either would make n_equal 1, counting both 2.
    assert _counts([0], [2]) == ([1.0], [1], [0])
    assert R.rank_of([1], [0]).tolist() == [2.0]
    # (1, 0): the true pair scores 2 and node 2 scores 2 too: a tie, half a rank.  The source's own 4 would be a "greater".
    assert _counts([1], [0]) == ([2.0], [0], [1])
    assert R.rank_of([0], [1]).tolist() == [1.5]
    # (2, 0): 1 against 2 (node 1) and 3 (node 3): both above
    assert _counts([2], [0]) == ([1.0], [2], [0])
    # the filter takes node 1 out of (2, 0); listed twice it is still taken out once: 1, not 0
    assert _counts([2], [0], filt=[[2], [1]]) == ([1.0], [1], [0])
    assert _counts([2], [0], filt=[[2, 2], [1, 1]]) == ([1.0], [1], [0])
    # entries outside [0, N), another source's row, (s, s) and (s, dst) take nothing out: still 2
    assert _counts([2], [0], filt=[[2, 2, 3, 2, 2, 77], [77, -1, 1, 2, 0, 1]]) == ([1.0], [2], [0])
    # a row that covers every candidate leaves nothing to count
    assert _counts([2], [0], filt=[[2, 2], [3, 1]]) == ([1.0], [0], [0])
    # a source outside the graph is a zero row without a filter row: every candidate but the destination ties at 0
    assert _counts([9], [0], filt=[[9], [1]]) == ([0.0], [0], [3])
    # a destination outside: the true score is 0; from source 3 (0 0 3 9) node 2 is above, 0 and 1 tie
    assert _counts([3], [-4]) == ([0.0], [1], [2])
    # the cosine sees the direction only: 0 and 1 are the same point, so (0, 2) has node 1 above and nothing else
    st, ng, ne = R.ranks(R.scores(H, "cos"), [0, 0], [2, 1])
    assert ng.tolist() == [1, 0] and ne.tolist() == [0, 0]
    # replayed on someone else's matrix, row q = query q
    st, ng, ne = R.ranks(None, [1, 2], [0, 0], similarity=np.array([[2.0, 4, 2, 0], [1, 2, 2, 3]], dtype=np.float32))
    assert (st.tolist(), ng.tolist(), ne.tolist()) == ([2.0, 1.0], [0, 2], [1, 0]) and st.dtype == np.float32


def test_auc_by_hand_with_a_tie():
    """positives 0.9, 0.5, 0.7 against negatives 0.5, 0.2, 0.1: 3 + 2.5 + 3 wins of 9."""
    from gnn_pretraining_amd.finetune import link_probe as LPR
    s, y = [0.9, 0.5, 0.5, 0.2, 0.7, 0.1], [1, 1, 0, 0, 1, 0]
    assert R.auc(s, y) == 8.5 / 9
    assert LPR.pair_auc(torch.tensor(s), torch.tensor(y)) == 8.5 / 9
    assert LPR.pair_auc(torch.tensor(s), torch.tensor(y, dtype=torch.float32)) == 8.5 / 9
    assert R.auc([1.0, 1.0], [1, 0]) == 0.5 == LPR.pair_auc(torch.tensor([1.0, 1.0]), torch.tensor([1, 0]))
    assert math.isnan(R.auc(s, [1] * 6)) and math.isnan(LPR.pair_auc(torch.tensor(s), torch.ones(6)))
    assert math.isnan(R.auc([], [])) and math.isnan(LPR.pair_auc(torch.tensor(s), torch.zeros(6)))
    rng = np.random.default_rng(3)
    s, y = rng.integers(0, 5, size=200).astype(np.float32), rng.integers(0, 2, size=200)      # masses of ties
    assert LPR.pair_auc(torch.from_numpy(s), torch.from_numpy(y)) == pytest.approx(R.auc(s, y), abs=1e-15)


def test_kinds_and_modes():
    from gnn_pretraining_amd.finetune import link_probe as LPR
    assert LPR.KINDS == ("cos", "dot") == R.KINDS and ops.EMB_LINK_MODES == {"cos": 0, "dot": 1}
    with pytest.raises(ValueError):
        LPR.embedding_scores(torch.zeros(3, 4), torch.zeros(2, 0, dtype=torch.int64), "katz")
    with pytest.raises(ValueError):
        LPR.embedding_ranks(torch.zeros(3, 4), torch.zeros(2, 0, dtype=torch.int64), "l2")


def test_link_probe_flag_parses_into_the_config():
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--lp-engine", "--link-probe"] + BASE)
    cfg = FT.config_from_args(a)
    assert cfg.link_probe and cfg.lp_engine and not cfg.lp_ranking and not cfg.repr_stats
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--lp-engine"] + BASE)
    assert not FT.config_from_args(a).link_probe                                         # opt-in
    assert FT.FinetuneConfig("CiteSeer_LP", "full_finetune", "b1", 1, lp_engine=True, link_probe=True, repr_stats=True, lp_ranking=True).link_probe
    assert len(FT.PROBES) == 3                                                           # not a class-label probe: the table is untouched


def test_link_probe_needs_the_engine():
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--link-probe"] + BASE)
    with pytest.raises(ValueError, match="link_probe needs an active fine-tune engine.*--lp-engine"):
        FT.config_from_args(a)
    with pytest.raises(ValueError, match="link_probe needs"):
        FT.FinetuneConfig("CiteSeer_LP", "full_finetune", "b1", 1, link_probe=True, lp_heuristics=True)


@pytest.mark.parametrize("domain,engine", [("Cora_NC", {}), ("CiteSeer_NC", {}), ("ENZYMES", {}), ("PTC_MR", {"gc_engine": True})])
def test_link_probe_is_refused_off_link_prediction(domain, engine):
    with pytest.raises(ValueError, match="link_probe applies to the link-prediction domains"):
        FT.FinetuneConfig(domain, "full_finetune", "b1", 1, link_probe=True, **engine)
    assert not FT.FinetuneConfig(domain, "full_finetune", "b1", 1, **engine).link_probe


def test_workspace_rule():
    """256 + the padded copy of h rounded up to 256 bytes, whatever the number of queries; 0 outside the ranges."""
    size = L.lib().gmp_emb_link_workspace_bytes
    for N, d in ((0, 8), (1, 1), (31, 6), (2708, 256), (65535, 100)):
        want = 256 + (4 * N * ((d + 3) // 4 * 4) + 255) // 256 * 256
        assert size(N, 1, d) == size(N, 10 ** 6, d) == size(N, 0, d) == want, (N, d)
    assert size(10, 10, 0) == size(10, 10, 257) == size(-1, 10, 8) == size(2 ** 31, 10, 8) == size(10, -1, 8) == 0


def test_python_layer_refuses_cpu_tensors_and_bad_modes():
    h, e = torch.zeros(4, 8), torch.zeros(3, dtype=torch.int64)
    with pytest.raises(GnnmpError, match="GPU tensor"):
        ops.emb_link_rank(h, e, e)
    with pytest.raises(GnnmpError, match="GPU tensor"):
        ops.emb_link_score(h, e, e, "dot")
    with pytest.raises(GnnmpError, match="mode='l2' is not one of"):
        ops.emb_link_rank(h, e, e, mode="l2")
    with pytest.raises(GnnmpError, match="mode=0 is not one of"):
        ops.emb_link_score(h, e, e, mode=0)
