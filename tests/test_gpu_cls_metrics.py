"""Device classification metrics (csrc/cls_metrics.hip: gmp_cls_counts; ops.cls_counts; metrics.compute_batch_metrics_device;
--device-metrics).

The yardstick of the counts is cls_metrics_ref.cpu_counts -- torch integer ops on the CPU over the same fp32 values -- and every
comparison of counts is exact.  The scores are compared with compute_batch_metrics (scikit-learn on host copies of the same GPU
tensors) within 1e-12: both see identical fp32 values, so no pair can flip and only float64 rounding of the final ratios differs."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from cls_metrics_ref import DOMAIN_OF, cpu_counts, cpu_counts_sorted, make_inputs                     # noqa: E402
from gnn_pretraining_amd import _lib as L, ops                                     # noqa: E402
from gnn_pretraining_amd.finetune import finetune as FT, metrics as M              # noqa: E402

DEV = torch.device("cuda:0")
TILE = 256                                                                        # rows per tile of both kernels (cls_metrics.hip T)
SCORES = ("accuracy", "f1", "precision", "recall", "auc", "loss")


def _check(t, p, pr, C, want_status=0):
    conf, auc, status = ops.cls_counts(t.to(DEV), p.to(DEV), pr.to(DEV))
    assert conf.dtype == auc.dtype == torch.int64 and status.dtype == torch.int32
    assert conf.shape == (C, C) and auc.shape == (C, 4) and status.shape == (1,) and conf.is_cuda
    w_conf, w_auc, w_status = cpu_counts(t, p, pr, C)
    assert w_status == want_status
    assert int(status.item()) == w_status
    assert torch.equal(conf.cpu(), w_conf)
    assert torch.equal(auc.cpu(), w_auc), (auc.cpu(), w_auc)
    return conf, auc


@pytest.mark.parametrize("C", [2, 6, 7])
@pytest.mark.parametrize("n", [1, 2, TILE - 1, TILE, TILE + 1, 1000])
def test_counts_equal_the_cpu_reference(n, C):
    _check(*make_inputs(n, C, 7 * n + C), C)


@pytest.mark.parametrize("n,C,kind", [(300, 32, "random"), (4099, 7, "random"), (1000, 7, "ties"), (700, 2, "ties"), (600, 6, "dup"),
                                      (500, 7, "one_class"), (300, 2, "one_class"), (513, 32, "ties")])
def test_counts_on_wide_large_tied_duplicated_and_one_class_inputs(n, C, kind):
    conf, auc = _check(*make_inputs(n, C, 11 * n + C, kind), C)
    if kind == "ties":
        assert int(auc[:, 3].sum()) > n
    if kind == "one_class":
        assert int(auc[:, 2:].sum()) == 0 and int(auc[C - 1, 0]) == n and int(auc[C - 1, 1]) == 0


def test_counts_at_the_row_limit_need_64_bit_sums():
    """n = 262144, the largest accepted: 1,024 i-tiles against two chunks of 512 j-tiles, and with probabilities in quarters the equal pairs
    alone pass 2^32 (70/256 of 131069 * 131075 pairs per class; in eighths, 12870/65536 of them, they would not), as do the greater
    pairs.  The yardstick is the sort-and-search form (n^2 booleans would not fit)."""
    n, C = ops.CLS_MAX_ROWS, 2
    t, p, pr = make_inputs(n, C, 17, "ties", steps=4)
    conf, auc, status = ops.cls_counts(t.to(DEV), p.to(DEV), pr.to(DEV))
    w_conf, w_auc, w_status = cpu_counts_sorted(t, p, pr, C)
    assert int(status.item()) == w_status == 0
    assert torch.equal(conf.cpu(), w_conf) and torch.equal(auc.cpu(), w_auc)
    assert int(w_auc[:, 2:].min()) > 1 << 32


def _with_three_bad_rows(n, C):
    t, p, pr = make_inputs(n, C, 5)
    t[3], p[n // 2], pr[n - 2, C - 1] = C, -1, float("nan")       # an out-of-range target, an out-of-range prediction, a NaN probability
    return t, p, pr


@pytest.mark.parametrize("n,C", [(40, 7), (600, 2)])
def test_bad_rows_are_counted_in_status_and_left_out(n, C):
    t, p, pr = _with_three_bad_rows(n, C)
    conf, auc = _check(t, p, pr, C, want_status=3)
    assert int(conf.sum()) == n - 3 and int(auc[0, 0] + auc[0, 1]) == n - 3
    pr[0, 0] = float("inf")                                      # a fourth row: infinite is non-finite too
    t[3] = 1 << 40                                               # far outside int32
    _check(t, p, pr, C, want_status=4)


def test_device_function_raises_on_bad_rows_and_on_too_many_rows():
    t, p, pr = _with_three_bad_rows(40, 7)
    with pytest.raises(ValueError, match="3 of 40 rows"):
        M.compute_batch_metrics_device("Cora_NC", t.to(DEV), p.to(DEV), pr.to(DEV), torch.tensor(0.5), "val")
    n = ops.CLS_MAX_ROWS + 1
    big_t = torch.zeros(n, dtype=torch.int64, device=DEV)
    with pytest.raises(ValueError, match="rows"):
        M.compute_batch_metrics_device("Cora_LP", big_t, big_t, torch.zeros(n, 2, device=DEV), torch.tensor(0.5), "val")


def test_two_calls_give_identical_integers():
    t, p, pr = (x.to(DEV) for x in make_inputs(1500, 7, 3, "ties"))
    a, b = ops.cls_counts_packed(t, p, pr), ops.cls_counts_packed(t, p, pr)
    assert torch.equal(a, b) and int(a.view(-1)[-1]) == 0


def test_out_of_range_sizes_return_the_error_code_without_launching():
    lib, out = L.lib(), torch.full((32 * 32 + 4 * 32 + 1,), -7, dtype=torch.int64, device=DEV)
    t = torch.zeros(16, dtype=torch.int64, device=DEV)
    pr, ws = torch.zeros(16, 33, device=DEV), torch.empty(4 << 20, dtype=torch.uint8, device=DEV)
    args = lambda n, c, nbytes: (ops._ptr(t), ops._ptr(t), ops._ptr(pr), n, c, ops._ptr(out), ops._ptr(out[1024:]), ops._ptr(out[-1:]),   # noqa: E731
                                 ops._ptr(ws), nbytes, ops._stream(t))
    assert lib.gmp_cls_counts(*args(262145, 7, ws.numel())) == -1
    assert b"262145" in lib.gmp_last_error_string()
    assert lib.gmp_cls_counts(*args(16, 33, ws.numel())) == -1
    assert lib.gmp_cls_counts(*args(16, 1, ws.numel())) == -1
    assert lib.gmp_cls_counts(*args(16, 7, 16)) == -3                        # workspace too small: GMP_ERR_WORKSPACE
    torch.cuda.synchronize()
    assert bool((out == -7).all())                                           # nothing ran: the outputs were not even zeroed
    with pytest.raises(L.GnnmpError):
        ops.cls_counts(t, t, pr)                                             # 33 classes through the binding


@pytest.mark.parametrize("n,C,kind", [(500, 7, "random"), (1000, 7, "ties"), (2110, 2, "random"), (64, 2, "ties"), (32, 6, "random")])
def test_device_function_equals_the_host_function(n, C, kind):
    t, p, pr = (x.to(DEV) for x in make_inputs(n, C, 13 * n + C, kind))
    loss = torch.tensor(0.375, device=DEV)
    want = M.compute_batch_metrics(DOMAIN_OF[C], t, p, pr, loss, "val")
    got = M.compute_batch_metrics_device(DOMAIN_OF[C], t, p, pr, loss, "val")
    assert list(got.keys()) == list(want.keys())
    for k in want:
        assert abs(got[k] - want[k]) <= 1e-12, (k, got[k], want[k])
    assert got["num_samples"] == n and isinstance(got["num_samples"], int)


@pytest.mark.parametrize("domain,kw,node_engine", [("Cora_NC", {}, "1"), ("Cora_LP", {"lp_engine": True, "engine_eval": True}, "1"),
                                                   ("ENZYMES", {"gc_engine": True}, "1"), ("Cora_NC", {}, "0")])
def test_finetune_with_device_metrics_reports_the_host_values_and_calls_no_host_metric(domain, kw, node_engine, tmp_path, monkeypatch):
    """finetune() for 2 epochs on scaled-down synthetic data with device_metrics and a log: every batch score comes from the device
    function (the host function is patched to raise wherever finetune.py or metrics.py would reach it) and equals the host function's
    on the same arguments.  The last case runs the module loop (no engine): compute_training_metrics and compute_loss_and_metrics."""
    import json
    monkeypatch.setenv("GMP_FINETUNE_ENGINE", node_engine)
    monkeypatch.setattr(FT, "OUTPUT_DIR", tmp_path / "finetune")
    host_fn, device_fn, seen = M.compute_batch_metrics, M.compute_batch_metrics_device, []

    def checked(domain_name, targets, predictions, probabilities, loss, prefix):
        got = device_fn(domain_name, targets, predictions, probabilities, loss, prefix)
        want = host_fn(domain_name, targets, predictions, probabilities, loss, prefix)
        assert list(got.keys()) == list(want.keys())
        for k in want:
            assert abs(got[k] - want[k]) <= 1e-12, (prefix, k, got[k], want[k])
        seen.append(prefix)
        return got

    def refuse(*a, **k):
        raise AssertionError("compute_batch_metrics called on the --device-metrics path")

    for mod in (FT, M):
        monkeypatch.setattr(mod, "compute_batch_metrics_device", checked)
        monkeypatch.setattr(mod, "compute_batch_metrics", refuse)
    log = tmp_path / "log.jsonl"
    cfg = FT.FinetuneConfig(domain, "full_finetune", "b1", 3, device_metrics=True, **kw)
    test = FT.finetune(cfg, epochs=2, data_root=str(tmp_path / "data"), data_scale=0.1, log_path=str(log))
    for prefix in ("train", "val", "test"):
        assert seen.count(prefix) >= 1, seen
    for k in SCORES:
        assert f"test/{k}" in test
    for k in ("test/convergence_epochs", "test/training_time", "test/total_parameters", "test/trainable_parameters"):
        assert k in test
    rows = [json.loads(line) for line in log.read_text().splitlines()]
    assert any("train/auc" in r for r in rows) and any("val/auc" in r for r in rows) and any("test/auc" in r for r in rows)
