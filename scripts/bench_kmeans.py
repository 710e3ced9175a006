"""Time per Lloyd iteration and peak memory of the spherical k-means fit (ops.kmeans_fit: csrc/kmeans.hip) beside the two routes a user
has without it: the same loop in torch (F.normalize, x @ c.T which allocates the n x kc matrix, max, index_add_), and the loop with the
assignment from ops.knn_topk(x, c, 1) and the update in torch -- what not having the dedicated kernels costs.  Cases (n, kc) at d = 256:
(2,708, 7), (19,717, 64), (65,535, 1,024), seeded randn rows, the initial centroids rows of a permutation, a fixed number of iterations
(none of the routes reads anything back inside the loop; the fit's one read-back at the end is inside its time).  Per case and route:
the median over alternated rounds of the mean call time after warm-up divided by the iterations run, the spread over the rounds, and
torch.cuda.max_memory_allocated over one call (absolute, and above what was allocated before the call: the inputs); plus how many labels
of the routes agree after the last pass.  No bar on time or memory.
    python scripts/bench_kmeans.py --out profiles/kmeans.json"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gnn_pretraining_amd import ops                                               # noqa: E402

CASES = [(2708, 7), (19717, 64), (65535, 1024)]


def torch_update(xn, labels, c):
    sums = torch.zeros_like(c).index_add_(0, labels, xn)            # (floating-point atomics: the order of the sum is not fixed)
    counts = torch.bincount(labels, minlength=c.size(0))
    return torch.where(counts[:, None] > 0, F.normalize(sums, dim=1), c)


def torch_route(x, init, iters):
    xn, c = F.normalize(x, dim=1), F.normalize(init, dim=1)
    for _ in range(iters):
        sim, labels = (xn @ c.t()).max(dim=1)
        c = torch_update(xn, labels, c)
    return c, labels, sim


def knn_route(x, init, iters):
    xn, c = F.normalize(x, dim=1), F.normalize(init, dim=1)
    for _ in range(iters):
        idx, sim = ops.knn_topk(x, c, 1)                            # normalises all rows again on every call
        labels = idx[:, 0]
        c = torch_update(xn, labels, c)
    return c, labels, sim[:, 0]


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e3          # us


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    before = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    del out
    return peak, peak - before


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", type=str, default=None, help="also write the rows to this JSON file")
    p.add_argument("--d", type=int, default=256)
    p.add_argument("--iterations", type=int, default=10, help="Lloyd iterations per call")
    p.add_argument("--rounds", type=int, default=3, help="alternated rounds per case")
    p.add_argument("--reps", type=int, default=10, help="calls per round at fewer than 10,000 rows (3 above)")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_kmeans.py measures on the GPU: no device found")
    rows = []
    for n, kc in CASES:
        g = torch.Generator().manual_seed(0)
        x = torch.randn(n, a.d, generator=g)
        init = x[torch.randperm(n, generator=g)[:kc]].contiguous().cuda()
        x = x.cuda()
        routes = {"kmeans_fit": lambda: ops.kmeans_fit(x, init, a.iterations), "torch": lambda: torch_route(x, init, a.iterations),
                  "knn_topk": lambda: knn_route(x, init, a.iterations)}
        reps = a.reps if n < 10000 else 3
        ran = routes["kmeans_fit"]().n_iter                           # (the fit stops early when it converges; randn rows do not in 10)
        times = {r: [] for r in routes}
        for _ in range(a.rounds):
            for r, fn in routes.items():
                times[r].append(timed(fn, reps) / (ran if r == "kmeans_fit" else a.iterations))
        row = {"n": n, "clusters": kc, "d": a.d, "iterations": a.iterations, "iterations_run_by_kmeans_fit": ran, "reps": reps, "rounds": a.rounds,
               "matrix_bytes": 4 * n * kc}
        for r, fn in routes.items():
            t = sorted(times[r])
            row[f"{r}_us_per_iteration"] = round(t[len(t) // 2], 1)
            row[f"{r}_us_per_iteration_rounds"] = [round(v, 1) for v in times[r]]
            row[f"{r}_peak_bytes"], row[f"{r}_peak_bytes_above_inputs"] = peak_bytes(fn)
        fit, (_, tl, _), (_, kl, _) = routes["kmeans_fit"](), routes["torch"](), routes["knn_topk"]()
        row["same_labels_share_torch"] = round(float((fit.labels == tl).float().mean()), 6)      # (the torch sums are in another order)
        row["same_labels_share_knn_topk"] = round(float((fit.labels == kl).float().mean()), 6)
        row["kmeans_over_torch_time"] = round(row["kmeans_fit_us_per_iteration"] / row["torch_us_per_iteration"], 3)
        row["kmeans_over_knn_topk_time"] = round(row["kmeans_fit_us_per_iteration"] / row["knn_topk_us_per_iteration"], 3)
        row["kmeans_over_torch_peak_above_inputs"] = round(row["kmeans_fit_peak_bytes_above_inputs"] / row["torch_peak_bytes_above_inputs"], 4)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del x, init, routes, fit
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
