"""Time and peak memory of the label-free embedding statistics (ops.repr_pair_stats and ops.repr_gram: csrc/repr_stats.hip) beside the
matrix form a user has without them in torch: F.normalize, zn @ zn.T, exp and a triu sum for the pair statistics (which allocates
n x n arrays), z.double().T @ z.double() for the Gram matrix (which allocates an fp64 copy of z).  Sizes: the ladder of the other
probes, 2,708 / 19,717 / 65,535 rows at d = 256.  Per size, statistic and route: the median over alternated rounds (round r times
one route, then the other) of the mean call time after warm-up on the GPU clock (events), the spread over the rounds, and
torch.cuda.max_memory_allocated over one call (absolute, and above what was allocated before the call: the input); plus how far the
two routes' results lie apart.  No speed bar is set: the condition is the memory claim, that the kernel route's peak above the input
holds no n x n array (it stays below 4 n^2 bytes at 19,717 and 65,535 rows; exit status 1 otherwise).
    python scripts/bench_repr_stats.py --out profiles/repr_stats.json"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchkit import alternate, emit, peak, require_gpu                           # noqa: E402
from gnn_pretraining_amd import ops                                               # noqa: E402

SIZES = (2708, 19717, 65535)
MEMORY_BAR_ROWS = (19717, 65535)


def torch_pair_stats(z, t):
    zn = F.normalize(z, dim=1)
    sim = zn @ zn.t()
    e = torch.exp(2.0 * t * (sim - 1.0))
    return torch.stack([torch.triu(e, diagonal=1).sum(dtype=torch.float64), torch.triu(sim, diagonal=1).sum(dtype=torch.float64)])


def torch_gram(z):
    zd = z.double()
    return zd.t() @ zd, zd.sum(dim=0)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", type=str, default=None, help="also write the rows to this JSON file")
    p.add_argument("--d", type=int, default=256)
    p.add_argument("--t", type=float, default=2.0)
    p.add_argument("--rounds", type=int, default=3, help="alternated rounds per case")
    p.add_argument("--iters", type=int, default=20, help="calls per round at fewer than 10,000 rows (a fifth of it above, at least 2)")
    a = p.parse_args()
    require_gpu("bench_repr_stats.py")
    rows, ok = [], True
    for n in SIZES:
        z = torch.randn(n, a.d, generator=torch.Generator().manual_seed(0)).cuda()
        iters = a.iters if n < 10000 else max(a.iters // 5, 2)
        if torch.cuda.mem_get_info()[0] < 5 * 4 * n * n:                    # sim, sim - 1, its product, exp and triu live together at the peak
            raise SystemExit(f"bench_repr_stats.py: the torch route needs about {5 * 4 * n * n >> 30} GiB of free device memory at n = {n}")
        for stat, routes in (("pair_stats", {"kernel": lambda: ops.repr_pair_stats(z, a.t), "torch": lambda: torch_pair_stats(z, a.t)}),
                             ("gram", {"kernel": lambda: ops.repr_gram(z), "torch": lambda: torch_gram(z)})):
            times = {r: [1e3 * t.event_ms for t in ts] for r, ts in alternate(routes, iters, rounds=a.rounds, route_warmup=2).items()}      # us
            row = {"statistic": stat, "n": n, "d": a.d, "iters": iters, "rounds": a.rounds, "matrix_bytes": 4 * n * n}
            for r, fn in routes.items():
                ts = sorted(times[r])
                row[f"{r}_us"] = round(ts[len(ts) // 2], 1)
                row[f"{r}_us_rounds"] = [round(x, 1) for x in times[r]]
                above, total = peak(fn)[:2]                                       # (the output dies here, before the next route's peak)
                row[f"{r}_peak_bytes"], row[f"{r}_peak_bytes_above_input"] = total, above
            k, ref = routes["kernel"](), routes["torch"]()
            if stat == "pair_stats":
                pairs = n * (n - 1) / 2
                row["uniformity_diff"] = abs(float(torch.log(k[0] / pairs)) - float(torch.log(ref[0] / pairs)))
                row["mean_cosine_diff"] = abs(float(k[1] - ref[1])) / pairs
            else:
                row["gram_max_rel_diff"] = float((k[0] - ref[0]).abs().max() / ref[0].abs().max())
            row["kernel_over_torch_time"] = round(row["kernel_us"] / row["torch_us"], 3)
            if n in MEMORY_BAR_ROWS:
                row["no_n_by_n_array"] = row["kernel_peak_bytes_above_input"] < 4 * n * n
                ok = ok and row["no_n_by_n_array"]
            emit(row, None)
            rows.append(row)
            del routes, k, ref
        del z
    emit({"device": torch.cuda.get_device_name(0), "memory_condition_met": ok, "rows": rows}, a.out, indent=1)
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
