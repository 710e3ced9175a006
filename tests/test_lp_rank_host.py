"""Host-side contract of all-candidate link ranking: ranking_metrics, the --lp-ranking flag and its precondition, the declaration /
binding / export of the new C-ABI entry points, and the workspace sizes (O(Q + N), never the dense Q x N logits)."""
import re
from pathlib import Path

import pytest

from gnn_pretraining_amd import _lib as L
from gnn_pretraining_amd.finetune import finetune as FT
from gnn_pretraining_amd.finetune.metrics import ranking_metrics

ROOT = Path(__file__).resolve().parents[1]
BASE = ["--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1", "--seed", "1"]


def test_ranking_metrics_on_hand_made_ranks():
    m = ranking_metrics([1, 2, 4, 100])
    assert m == {"mrr": pytest.approx((1 + 0.5 + 0.25 + 0.01) / 4), "hits@1": 0.25, "hits@10": 0.75, "hits@50": 0.75}
    # the half-tie rule: a true edge tied with one candidate sits at rank 1.5 -- not a hit at 1, reciprocal rank 2 / 3
    m = ranking_metrics([1.5, 1.0], ks=(1, 2))
    assert m == {"mrr": pytest.approx((2 / 3 + 1) / 2), "hits@1": 0.5, "hits@2": 1.0}
    # 1 + n_greater + n_equal / 2 with n_greater = 9, n_equal = 3: rank 11.5, outside hits@10 and inside hits@50
    m = ranking_metrics([1 + 9 + 3 / 2])
    assert m["hits@10"] == 0.0 and m["hits@50"] == 1.0 and m["mrr"] == pytest.approx(1 / 11.5)
    import torch
    assert ranking_metrics(torch.tensor([1.0, 2.0]))["mrr"] == pytest.approx(0.75)
    with pytest.raises(ValueError):
        ranking_metrics([])
    with pytest.raises(ValueError):
        ranking_metrics([0.5])


def test_lp_ranking_flag_parses_into_the_config():
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--lp-engine", "--engine-eval", "--lp-ranking"] + BASE)
    cfg = FT.config_from_args(a)
    assert cfg.lp_ranking and cfg.lp_engine and cfg.engine_eval
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--lp-engine", "--engine-eval"] + BASE)
    assert FT.config_from_args(a).lp_ranking is False                                   # opt-in


def test_lp_ranking_is_refused_without_the_lp_engine():
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--lp-ranking"] + BASE)
    with pytest.raises(ValueError, match="lp_ranking"):
        FT.config_from_args(a)
    with pytest.raises(ValueError, match="lp_ranking"):
        FT.FinetuneConfig("Cora_NC", "full_finetune", "b1", 1, lp_ranking=True)
    assert FT.FinetuneConfig("Cora_LP", "full_finetune", "b1", 1, lp_engine=True, lp_ranking=True).lp_ranking


def test_ranking_kernel_source_keeps_the_scorers_products_and_has_no_float_atomics():
    csrc = ROOT / "gnn_pretraining_amd" / "csrc"
    src = (csrc / "lp_rank.hip").read_text()
    assert '#include "lp_tile.h"' in src and '#include "lp_filter.h"' in src            # the scorer's tile code and the filter bitmap
    assert '#include "lp_tile.h"' in (csrc / "lp_score.hip").read_text()                # ... which the training forward runs too
    src += (csrc / "lp_tile.h").read_text() + (csrc / "lp_filter.h").read_text()
    assert "mfma_f32_32x32x2f32" in src
    for m in re.finditer(r"atomicAdd\(&(\w+)", src):                                   # integer counts only
        assert m.group(1) in ("cnt", "n_greater", "n_equal"), m.group(0)
    assert not re.search(r"__hip_atomic|unsafeAtomic|atomicAdd\([^&]", src)


@pytest.mark.parametrize("fn", ["gmp_lp_rank_workspace_bytes", "gmp_lp_topk_workspace_bytes"])
def test_workspaces_are_linear_in_queries_plus_nodes(fn):
    size = getattr(L.lib(), fn)
    assert size(1024, 100000) < 16 * 2 ** 20                   # the dense logits alone would be 1024 * 100000 * 4 B = 400 MB
    for Q, N in ((1, 1000), (64, 2708), (1024, 100000), (4096, 50000)):
        small, big = size(Q, N), size(2 * Q, 2 * N)
        assert big <= 2 * small + 4096, (Q, N, small, big)     # at most linear growth (plus alignment)
        assert small <= 4096 * (Q + N) + 4096, (Q, N, small)   # and a per-element cost that is a constant, not N or Q
