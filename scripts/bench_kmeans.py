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
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchkit import alternate, emit, peak, require_gpu                           # noqa: E402
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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", type=str, default=None, help="also write the rows to this JSON file")
    p.add_argument("--d", type=int, default=256)
    p.add_argument("--iterations", type=int, default=10, help="Lloyd iterations per call")
    p.add_argument("--rounds", type=int, default=3, help="alternated rounds per case")
    p.add_argument("--reps", type=int, default=10, help="calls per round at fewer than 10,000 rows (3 above)")
    a = p.parse_args()
    require_gpu("bench_kmeans.py")
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
        times = {r: [1e3 * t.event_ms / (ran if r == "kmeans_fit" else a.iterations) for t in ts]                  # us per iteration
                 for r, ts in alternate(routes, reps, rounds=a.rounds, route_warmup=2).items()}
        row = {"n": n, "clusters": kc, "d": a.d, "iterations": a.iterations, "iterations_run_by_kmeans_fit": ran, "reps": reps, "rounds": a.rounds,
               "matrix_bytes": 4 * n * kc}
        for r, fn in routes.items():
            t = sorted(times[r])
            row[f"{r}_us_per_iteration"] = round(t[len(t) // 2], 1)
            row[f"{r}_us_per_iteration_rounds"] = [round(v, 1) for v in times[r]]
            above, total = peak(fn)[:2]                                           # (the output dies here, before the next route's peak)
            row[f"{r}_peak_bytes"], row[f"{r}_peak_bytes_above_inputs"] = total, above
        fit, tl, kl = routes["kmeans_fit"](), routes["torch"]()[1], routes["knn_topk"]()[1]       # (labels only: nothing else outlives the case)
        row["same_labels_share_torch"] = round(float((fit.labels == tl).float().mean()), 6)      # (the torch sums are in another order)
        row["same_labels_share_knn_topk"] = round(float((fit.labels == kl).float().mean()), 6)
        row["kmeans_over_torch_time"] = round(row["kmeans_fit_us_per_iteration"] / row["torch_us_per_iteration"], 3)
        row["kmeans_over_knn_topk_time"] = round(row["kmeans_fit_us_per_iteration"] / row["knn_topk_us_per_iteration"], 3)
        row["kmeans_over_torch_peak_above_inputs"] = round(row["kmeans_fit_peak_bytes_above_inputs"] / row["torch_peak_bytes_above_inputs"], 4)
        emit(row, None)
        rows.append(row)
        del x, init, routes, fit
    emit({"device": torch.cuda.get_device_name(0), "rows": rows}, a.out, indent=1)


if __name__ == "__main__":
    main()
