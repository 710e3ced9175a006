"""Host side of the device classification metrics: metrics_from_counts against the scikit-learn calls of compute_batch_metrics (counts made
on the CPU with torch integer ops, cls_metrics_ref.cpu_counts), the declaration / binding / export of the new C-ABI entry points, the
--device-metrics flag, and the kernel source's atomics (integer count arrays only)."""
import re
from pathlib import Path

import pytest
import torch

from cls_metrics_ref import DOMAIN_OF, cpu_counts, cpu_counts_sorted, make_inputs
from gnn_pretraining_amd import _lib as L
from gnn_pretraining_amd.finetune import finetune as FT
from gnn_pretraining_amd.finetune import metrics as M

ROOT = Path(__file__).resolve().parents[1]
BASE = ["--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1", "--seed", "1"]
KEYS = ["t/accuracy", "t/f1", "t/precision", "t/recall", "t/auc", "num_samples"]

CASES = [(500, 7, "random"), (32, 6, "random"), (2110, 2, "random"), (140, 7, "random"),
         (300, 7, "absent_target"), (300, 6, "absent_both"),
         (200, 7, "one_class"), (64, 2, "one_class"),
         (250, 7, "all_wrong"), (100, 2, "all_wrong"),
         (1000, 7, "ties"), (400, 6, "ties"), (600, 2, "ties"),
         (300, 7, "dup"), (300, 2, "dup")]


@pytest.mark.parametrize("n,C,kind", CASES)
def test_metrics_from_counts_equal_the_sklearn_scores(n, C, kind):
    t, p, pr = make_inputs(n, C, 100 + n + C, kind)
    want = M.compute_batch_metrics(DOMAIN_OF[C], t, p, pr, torch.tensor(0.25), "t")
    conf, auc, status = cpu_counts(t, p, pr, C)
    assert status == 0
    got = M.metrics_from_counts(conf.numpy(), auc.numpy(), C == 2, "t")
    assert sorted(got.keys()) == sorted(KEYS)
    for k in KEYS:
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    # the case is what its name says
    if kind in ("one_class", "absent_target"):
        assert got["t/auc"] == 0.0
    elif kind != "absent_both":
        assert 0.0 < got["t/auc"] <= 1.0
    if kind == "all_wrong":
        assert got["t/accuracy"] == 0.0 and got["t/f1"] == 0.0
    if kind == "ties":
        assert int(auc[:, 3].sum()) > n                       # many equal pairs
    if kind == "absent_target":
        assert int(conf[C - 1].sum()) == 0 and int(conf[:, C - 1].sum()) > 0
    if kind == "absent_both":
        assert int(conf[1].sum()) == 0 and int(conf[:, 1].sum()) == 0 and got["t/auc"] == 0.0


@pytest.mark.parametrize("n,C,kind", [(1000, 7, "ties"), (777, 2, "ties"), (500, 6, "dup"), (300, 32, "random")])
def test_the_two_cpu_yardsticks_agree(n, C, kind):
    t, p, pr = make_inputs(n, C, n + C, kind)
    t[5], pr[7, 0] = -1, float("nan")
    a, b = cpu_counts(t, p, pr, C), cpu_counts_sorted(t, p, pr, C)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and a[2] == b[2] == 2


def test_metrics_from_counts_refuses_empty_or_misshapen_counts():
    with pytest.raises(ValueError):
        M.metrics_from_counts(torch.zeros(3, 3, dtype=torch.int64).numpy(), torch.zeros(3, 4, dtype=torch.int64).numpy(), False, "t")
    with pytest.raises(ValueError):
        M.metrics_from_counts(torch.ones(3, 3, dtype=torch.int64).numpy(), torch.zeros(2, 4, dtype=torch.int64).numpy(), False, "t")


def test_cls_counts_refuses_out_of_range_sizes_before_touching_a_pointer():
    """Null pointers throughout: a range error must come back before anything is dereferenced or launched (no GPU here)."""
    lib = L.lib()
    assert lib.gmp_cls_counts_workspace_bytes(1000, 7) >= 4000
    for n, classes in ((262145, 7), (0, 7), (100, 33), (100, 1)):
        assert lib.gmp_cls_counts(None, None, None, n, classes, None, None, None, None, 1 << 30, None) == -1, (n, classes)


def test_device_metrics_flag_parses_into_the_config_and_defaults_to_off():
    a = FT.build_parser().parse_args(["--domain_name", "Cora_NC", "--device-metrics"] + BASE)
    assert FT.config_from_args(a).device_metrics is True
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--lp-engine", "--engine-eval", "--device-metrics"] + BASE)
    cfg = FT.config_from_args(a)
    assert cfg.device_metrics and cfg.lp_engine and cfg.engine_eval
    a = FT.build_parser().parse_args(["--domain_name", "Cora_NC"] + BASE)
    assert FT.config_from_args(a).device_metrics is False
    assert FT.FinetuneConfig("ENZYMES", "full_finetune", "b1", 1).device_metrics is False


def test_device_metrics_function_never_imports_sklearn():
    src = (ROOT / "gnn_pretraining_amd" / "finetune" / "metrics.py").read_text()
    body = src.split("def compute_batch_metrics_device(")[1].split("\ndef ")[0] + src.split("def metrics_from_counts(")[1].split("\ndef ")[0]
    assert "sklearn" not in body
    assert not re.search(r"^(import|from)\s+sklearn", src, flags=re.M)                       # and no module-level import of it


def test_cls_metrics_kernel_source_adds_to_integer_count_arrays_only():
    src = (ROOT / "gnn_pretraining_amd" / "csrc" / "cls_metrics.hip").read_text()
    code = re.sub(r"//[^\n]*", "", src)
    targets = [m.group(1) for m in re.finditer(r"atomicAdd\(&(\w+)", code)]
    assert targets and len(targets) == code.count("atomicAdd")                               # every atomicAdd has the &name form
    integer_arrays = {"hist", "nval", "nbad", "cnt", "confusion", "auc_counts", "status"}
    assert set(targets) <= integer_arrays, targets
    for name in set(targets):                                                               # each is declared with an integer type
        decl = re.search(r"\b(int|int32_t|u64)\s*\*?\s*(?:__restrict__\s+)?" + name + r"\b", code)
        assert decl, name
    assert re.search(r"typedef unsigned long long u64;", code)
    assert not re.search(r"__hip_atomic|unsafeAtomic|atomicCAS|atomicExch", code)
    assert not re.search(r"atomic\w*\([^)]*\b(float|double)\b", code)
