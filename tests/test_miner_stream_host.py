"""Host-side contract of the streaming hard-negative miner (csrc/hardneg_stream.hip): declaration / binding / export of its two
C-ABI entry points, a workspace that is O(n d + E) plus a small constant (never the n x n matrix), the --miner flag and its
precondition, the impl argument of ops.hard_negative_topk, and the kernel source's arithmetic (fp32 MFMA, integer atomics only)."""
import re
from pathlib import Path

import pytest
import torch

from gnn_pretraining_amd import _lib as L
from gnn_pretraining_amd import ops
from gnn_pretraining_amd.finetune import finetune as FT

ROOT = Path(__file__).resolve().parents[1]
BASE = ["--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1", "--seed", "1"]


def test_workspace_is_linear_with_a_bounded_constant_and_far_below_the_matrix():
    ws = L.lib().gmp_hard_negative_stream_workspace_bytes
    for n, d, E in ((1500, 4, 500), (2708, 256, 10556), (19717, 256, 88648), (65535, 256, 10 ** 6), (2 ** 19, 64, 10 ** 6)):
        small, big = ws(n, d, E), ws(2 * n, d, 2 * E)
        assert small > 0 and big <= 2 * small + 4096, (n, d, E, small, big)
    # the constant part (state + candidate buffer) stays far below the 2.25 M tied keys of the identical-rows GPU test
    assert ws(1500, 4, 500) <= 8 * 2 ** 20
    assert ws(65535, 256, 10 ** 6) <= L.lib().gmp_hard_negative_workspace_bytes(65535, 256) // 16
    # sizes the entry point does not take
    assert ws(2 ** 20 + 1, 8, 0) == 0 and ws(100, 257, 0) == 0 and ws(0, 8, 0) == 0


def test_miner_flag_parses_into_the_config_and_defaults_to_matrix():
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP"] + BASE)
    assert FT.config_from_args(a).miner_impl == "matrix"
    for impl in ("matrix", "stream", "auto"):
        a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--miner", impl] + BASE)
        assert FT.config_from_args(a).miner_impl == impl
        a = FT.build_parser().parse_args(["--domain_name", "CiteSeer_LP", "--lp-engine", "--miner", impl] + BASE)
        cfg = FT.config_from_args(a)
        assert cfg.miner_impl == impl and cfg.lp_engine
    with pytest.raises(SystemExit):
        FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--miner", "nope"] + BASE)
    assert FT.FinetuneConfig("Cora_LP", "full_finetune", "b1", 1).miner_impl == "matrix"
    assert FT.LinkPredictionHardNegativeMiner().impl == "matrix"
    assert FT.LinkPredictionHardNegativeMiner(impl="stream").impl == "stream"


@pytest.mark.parametrize("domain", ["Cora_NC", "ENZYMES"])
def test_miner_impl_is_refused_outside_link_prediction(domain):
    a = FT.build_parser().parse_args(["--domain_name", domain, "--miner", "stream"] + BASE)
    with pytest.raises(ValueError, match="miner_impl"):
        FT.config_from_args(a)
    with pytest.raises(ValueError, match="miner_impl"):
        FT.FinetuneConfig(domain, "full_finetune", "b1", 1, miner_impl="auto")
    assert FT.FinetuneConfig(domain, "full_finetune", "b1", 1).miner_impl == "matrix"      # the default is no request


def test_unknown_impl_raises():
    emb, ex = torch.zeros(8, 4), torch.zeros(2, 0, dtype=torch.long)
    with pytest.raises(ValueError, match="impl"):
        ops.hard_negative_topk(emb, ex, 2, impl="nope")
    with pytest.raises(ValueError, match="impl"):
        FT.LinkPredictionHardNegativeMiner(impl="nope")
    with pytest.raises(ValueError, match="miner_impl"):
        FT.FinetuneConfig("Cora_LP", "full_finetune", "b1", 1, miner_impl="nope")


def test_stream_kernel_source_uses_the_fp32_mfma_and_no_float_atomics():
    csrc = ROOT / "gnn_pretraining_amd" / "csrc"                   # the file, the tile core and the helpers it is built on
    src = "".join((csrc / f).read_text() for f in ("hardneg_stream.hip", "sim_tile.h", "gnnmp_internal.h"))
    assert "mfma_f32_32x32x2f32" in src
    for m in re.finditer(r"atomicAdd\(&([\w>-]+)", src):                               # integer counts only
        assert m.group(1) in ("h", "st->hist", "st->out_count"), m.group(0)
    for m in re.finditer(r"atomicOr\(&(\w+)", src):
        assert m.group(1) == "bm", m.group(0)
    assert not re.search(r"__hip_atomic|unsafeAtomic|atomicAdd\([^&]|atomicMax|atomicMin|atomicExch|atomicCAS", src)
    # the integer types behind those names
    assert re.search(r"__shared__ unsigned int h\[", src) and re.search(r"__shared__ unsigned int bm\[", src)
    assert re.search(r"u64 hist\[BINS\]", src) and re.search(r"unsigned int out_count", src)
