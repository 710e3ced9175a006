"""Time and peak memory of the streaming k-nearest-neighbour search (ops.knn_topk: csrc/knn.hip) beside the torch route a user has
without it (F.normalize, q @ db.T, torch.topk), which allocates the nq x ndb similarity matrix.  Cases: leave-one-out over 2,708, 19,717
and 65,535 rows and 1,000 queries against 140 database rows, d = 256, k = 20.  Per case and route: the median over alternated rounds
(round r times one route, then the other) of the mean call time after warm-up, the spread over the rounds, and
torch.cuda.max_memory_allocated over one call (absolute, and above what was allocated before the call: the inputs); plus whether the
two routes return the same neighbours.  No speed bar is set: the condition is that the kernel's peak memory at 19,717 and at 65,535 rows
lies below the torch route's (exit status 1 otherwise).
    python scripts/bench_knn.py --out profiles/knn.json"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchkit import alternate, emit, peak, require_gpu                           # noqa: E402
from gnn_pretraining_amd import ops                                               # noqa: E402

CASES = [("leave_one_out", 2708, 2708), ("leave_one_out", 19717, 19717), ("leave_one_out", 65535, 65535), ("queries", 1000, 140)]
MEMORY_BAR_ROWS = (19717, 65535)


def torch_route(q, db, k, exclude_self):
    sim = F.normalize(q, dim=1) @ F.normalize(db, dim=1).t()
    if exclude_self:
        sim.fill_diagonal_(float("-inf"))
    val, idx = torch.topk(sim, k, dim=1)
    return idx, val


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", type=str, default=None, help="also write the rows to this JSON file")
    p.add_argument("--d", type=int, default=256)
    p.add_argument("--k", type=int, default=20)
    p.add_argument("--rounds", type=int, default=3, help="alternated rounds per case")
    p.add_argument("--iters", type=int, default=50, help="calls per round at fewer than 10,000 queries (a tenth of it above, at least 3)")
    a = p.parse_args()
    require_gpu("bench_knn.py")
    rows, ok = [], True
    for kind, nq, ndb in CASES:
        g = torch.Generator().manual_seed(0)
        loo = kind == "leave_one_out"
        db = torch.randn(ndb, a.d, generator=g).cuda()
        q = db if loo else torch.randn(nq, a.d, generator=g).cuda()
        routes = {"knn_topk": lambda: ops.knn_topk(q, db, a.k, exclude_self=loo), "torch": lambda: torch_route(q, db, a.k, loo)}
        iters = a.iters if nq < 10000 else max(a.iters // 10, 3)
        times = {r: [1e3 * t.event_ms for t in ts] for r, ts in alternate(routes, iters, rounds=a.rounds, route_warmup=3).items()}      # us
        row = {"case": kind, "nq": nq, "ndb": ndb, "d": a.d, "k": a.k, "iters": iters, "rounds": a.rounds,
               "matrix_bytes": 4 * nq * ndb}
        for r, fn in routes.items():
            t = sorted(times[r])
            row[f"{r}_us"] = round(t[len(t) // 2], 1)
            row[f"{r}_us_rounds"] = [round(x, 1) for x in times[r]]
            above, total = peak(fn)[:2]                                           # (the output dies here, before the next route's peak)
            row[f"{r}_peak_bytes"], row[f"{r}_peak_bytes_above_inputs"] = total, above
        (ki, ks), (ti, ts) = routes["knn_topk"](), routes["torch"]()
        row["same_neighbours_share"] = round(float((ki == ti).float().mean()), 6)      # (torch.topk leaves the order of ties open)
        row["max_similarity_diff"] = float((ks - ts).abs().max())
        row["knn_over_torch_time"] = round(row["knn_topk_us"] / row["torch_us"], 3)
        row["knn_over_torch_peak_above_inputs"] = round(row["knn_topk_peak_bytes_above_inputs"] / row["torch_peak_bytes_above_inputs"], 4)
        if nq in MEMORY_BAR_ROWS:
            row["memory_below_torch"] = row["knn_topk_peak_bytes"] < row["torch_peak_bytes"]
            ok = ok and row["memory_below_torch"]
        emit(row, None)
        rows.append(row)
        del q, db, routes
    emit({"device": torch.cuda.get_device_name(0), "memory_condition_met": ok, "rows": rows}, a.out, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
