"""Host-side contract of the link-prediction engine option: the config flag, the CLI flag and the fused scorer's C ABI."""
import re
from pathlib import Path

import pytest

from gnn_pretraining_amd.finetune import finetune as FT

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("domain", ["Cora_NC", "CiteSeer_NC", "ENZYMES", "PTC_MR"])
def test_lp_engine_is_rejected_outside_link_prediction(domain):
    with pytest.raises(ValueError, match="lp_engine"):
        FT.FinetuneConfig(domain, "full_finetune", "b1", 0, lp_engine=True)


@pytest.mark.parametrize("domain", ["Cora_LP", "CiteSeer_LP"])
def test_lp_engine_is_accepted_for_link_prediction(domain):
    cfg = FT.FinetuneConfig(domain, "linear_probe", "b1", 0, lp_engine=True)
    assert cfg.lp_engine and cfg.task_type == "link_prediction"
    assert not FT.FinetuneConfig(domain, "linear_probe", "b1", 0).lp_engine          # the module path stays the default


def test_cli_accepts_lp_engine():
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1",
                                      "--seed", "1", "--lp-engine"])
    assert FT.config_from_args(a).lp_engine
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1", "--seed", "1"])
    assert not FT.config_from_args(a).lp_engine


def test_scorer_kernel_source_has_no_float_atomics():
    src = (ROOT / "gnn_pretraining_amd" / "csrc" / "lp_score.hip").read_text()
    assert "v_mfma_f32_32x32x2_f32" in src or "mfma_f32_32x32x2f32" in src
    assert not re.search(r"atomicAdd|__hip_atomic|unsafeAtomic", src)
