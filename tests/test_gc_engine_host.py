"""Host-side contract of the graph-classification engine option: the config flag, the CLI flag and the fused head's C ABI."""
import re
from pathlib import Path

import pytest

from gnn_pretraining_amd.finetune import finetune as FT

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("domain", ["Cora_NC", "CiteSeer_NC", "Cora_LP", "CiteSeer_LP"])
def test_gc_engine_is_rejected_outside_graph_classification(domain):
    with pytest.raises(ValueError, match="gc_engine"):
        FT.FinetuneConfig(domain, "full_finetune", "b1", 0, gc_engine=True)


@pytest.mark.parametrize("domain", ["ENZYMES", "PTC_MR"])
def test_gc_engine_is_accepted_for_graph_classification(domain):
    cfg = FT.FinetuneConfig(domain, "linear_probe", "b1", 0, gc_engine=True)
    assert cfg.gc_engine and cfg.task_type == "graph_classification"
    assert not FT.FinetuneConfig(domain, "linear_probe", "b1", 0).gc_engine          # the module path stays the default


def test_cli_accepts_gc_engine():
    base = ["--domain_name", "ENZYMES", "--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1", "--seed", "1"]
    assert FT.config_from_args(FT.build_parser().parse_args(base + ["--gc-engine"])).gc_engine
    assert not FT.config_from_args(FT.build_parser().parse_args(base)).gc_engine


def test_head_kernel_source_has_no_float_atomics():
    src = (ROOT / "gnn_pretraining_amd" / "csrc" / "gc_head.hip").read_text()
    assert "gmp_gc_head_fwd" in src and "gmp_gc_head_bwd" in src
    assert not re.search(r"atomicAdd|__hip_atomic|unsafeAtomic", src)
