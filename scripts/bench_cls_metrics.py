"""Per-batch cost of the fine-tuning scores, two routes in one process on the same GPU tensors:

  host     metrics.compute_batch_metrics: three device-to-host copies, five scikit-learn calls
  device   metrics.compute_batch_metrics_device: gmp_cls_counts (csrc/cls_metrics.hip), one read-back, float64 arithmetic on the counts

    python scripts/bench_cls_metrics.py [--reps 200] [--warmup 10] [--epochs 20] [--rounds 3] [--out profiles/cls_metrics.json]

Shapes (rows, classes) are the batches the six fine-tuning domains produce, from seeded synthetic inputs.  Every call is timed on its
own by a host clock between two device synchronises (both routes end in a read-back, so the clock sees all of the work); the routes
alternate call by call and the median and the minimum over --reps calls are reported.  The two routes' values are compared (1e-12).
Then gmp_cls_counts alone at the row limit (device events), and the wall time of finetune() on Cora_NC for --epochs epochs with a log
(so every training step is scored), device_metrics off and on alternately, --rounds times after one discarded run of each."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import tempfile
import time
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchkit import DEV, emit, require_gpu  # noqa: E402
from gnn_pretraining_amd import ops  # noqa: E402
from gnn_pretraining_amd.constants import NUM_CLASSES  # noqa: E402
from gnn_pretraining_amd.finetune import finetune as FT, metrics as M  # noqa: E402

SHAPES = [(500, "Cora_NC"), (1000, "Cora_NC"), (140, "Cora_NC"), (32, "ENZYMES"), (2110, "Cora_LP"), (64, "PTC_MR")]


def inputs(n: int, c: int, seed: int):
    g = torch.Generator().manual_seed(seed)
    targets = torch.randint(0, c, (n,), generator=g)
    prob = torch.softmax(torch.randn(n, c, generator=g) + 1.5 * torch.nn.functional.one_hot(targets, c), dim=1)
    return targets.to(DEV), prob.argmax(dim=1).to(DEV), prob.to(DEV).contiguous()


def one_call_ms(fn) -> float:
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def bench_shape(n: int, domain: str, reps: int, warmup: int) -> dict:
    c = NUM_CLASSES[domain]
    t, p, pr = inputs(n, c, 1000 * c + n)
    loss = torch.tensor(0.5, device=DEV)
    host = lambda: M.compute_batch_metrics(domain, t, p, pr, loss, "val")
    device = lambda: M.compute_batch_metrics_device(domain, t, p, pr, loss, "val")
    want, got = host(), device()
    worst = max(abs(got[k] - want[k]) for k in want)
    for _ in range(warmup):
        host(), device()
    ht, dt = [], []
    for _ in range(reps):                                           # alternate: neither route owns a quiet or a noisy stretch
        ht.append(one_call_ms(host))
        dt.append(one_call_ms(device))
    r = lambda x: round(x, 4)
    return {"rows": n, "classes": c, "host_ms_median": r(statistics.median(ht)), "host_ms_min": r(min(ht)),
            "device_ms_median": r(statistics.median(dt)), "device_ms_min": r(min(dt)),
            "host_over_device": round(statistics.median(ht) / statistics.median(dt), 2), "max_abs_difference": worst}


def limit_ms(c: int, reps: int = 5) -> dict:
    """gmp_cls_counts alone at the largest accepted n (ops.CLS_MAX_ROWS): device events around `reps` calls after one warm-up call."""
    n = ops.CLS_MAX_ROWS
    t, p, pr = inputs(n, c, 7)
    ops.cls_counts_packed(t, p, pr)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        ops.cls_counts_packed(t, p, pr)
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / reps
    return {"rows": n, "classes": c, "counts_event_ms": round(ms, 3), "compares_per_s": round(n * n / (ms * 1e-3), -9)}


def finetune_wall_s(device_metrics: bool, epochs: int, root: Path, tag: str) -> float:
    FT.OUTPUT_DIR = root / "finetune"
    cfg = FT.FinetuneConfig("Cora_NC", "full_finetune", "b1", 42, device_metrics=device_metrics)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    FT.finetune(cfg, epochs=epochs, data_root=str(root / "data"), log_path=str(root / f"log_{tag}.jsonl"))
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    require_gpu("bench_cls_metrics.py")
    res = {"per_batch": [bench_shape(n, d, a.reps, a.warmup) for n, d in SHAPES], "reps": a.reps, "warmup": a.warmup}
    res["row_limit"] = [limit_ms(c) for c in (2, 7, 32)]
    with tempfile.TemporaryDirectory() as tmp:
        root = Path(tmp)
        finetune_wall_s(False, a.epochs, root, "warm_off"), finetune_wall_s(True, a.epochs, root, "warm_on")      # discarded
        off, on = [], []
        for i in range(a.rounds):
            off.append(finetune_wall_s(False, a.epochs, root, f"off{i}"))
            on.append(finetune_wall_s(True, a.epochs, root, f"on{i}"))
    res["finetune_cora_nc"] = {"epochs": a.epochs, "host_metrics_wall_s": [round(x, 4) for x in off], "device_metrics_wall_s": [round(x, 4) for x in on],
                               "host_metrics_wall_s_median": round(statistics.median(off), 4),
                               "device_metrics_wall_s_median": round(statistics.median(on), 4),
                               "what": "whole finetune() call: loaders, model, epochs x (one logged step + one validation batch), checkpoints, test"}
    emit(res, a.out)
    if max(s["max_abs_difference"] for s in res["per_batch"]) > 1e-12:
        raise SystemExit("the two routes disagree")


if __name__ == "__main__":
    main()
