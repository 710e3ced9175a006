"""T rounds of label spreading, F <- alpha S F + (1 - alpha) Y with S = D^-1/2 A D^-1/2, on random graphs of Cora, PubMed and 65,535-node
size and on a star-plus-noise graph whose hub has 10,000 neighbours, two routes in one process:

  kernel   ops.label_propagate: gmp_label_propagate, one launch per round, all rounds enqueued by one call, a lane group per row
  torch    the same loop in torch: S as a sparse CSR tensor (values left[i] * right[j]), per round torch.sparse.mm(S, F) and one
           torch.add(beta * Y, S F, alpha=alpha)

    python scripts/bench_label_propagation.py [--rounds 50] [--reps 20] [--warmup 3] [--out profiles/label_propagation.json]

The simple graph, the scales, Y and (for torch) S and beta * Y are built before the clock starts.  Routes run alternately and are timed
by a host clock around work that ends in a synchronise and by device events; the time per round is the call's time over the rounds.  Peak
memory is torch's allocator peak over a route's first call, above what was allocated before it (the kernel route's outputs and its
two-buffer workspace included).  The torch form sums a row in another order and fuses nothing away, so the two results agree to rounding,
not bit for bit; the largest difference is recorded and bounded.  The star graph measures the accepted cost of the sequential row sum: the
hub's row is walked by one lane group."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchkit import DEV, alternate, attempt, emit, peak, random_graph, require_gpu  # noqa: E402
from gnn_pretraining_amd import ops  # noqa: E402
from gnn_pretraining_amd.finetune import link_heuristics as LH, node_baselines as NB  # noqa: E402

ALPHA = 0.9
SHAPES = (("cora", 2708, 5429, 7, 0), ("pubmed", 19717, 44324, 3, 0), ("n65535", 65535, 200000, 32, 0), ("star", 20000, 40000, 7, 10000))


def torch_route(rowptr, col, left, right, f0, rounds: int):
    N = rowptr.numel() - 1
    row = torch.repeat_interleave(torch.arange(N, device=DEV), (rowptr[1:] - rowptr[:-1]).to(torch.int64))
    S = torch.sparse_csr_tensor(rowptr.to(torch.int64), col.to(torch.int64), left[row] * right[col.to(torch.int64)], size=(N, N))
    by = (1.0 - ALPHA) * f0

    def run():
        F = f0
        for _ in range(rounds):
            F = torch.add(by, torch.sparse.mm(S, F), alpha=ALPHA)
        return F

    return run


def bench_shape(name: str, N: int, E: int, classes: int, hub: int, a) -> dict:
    gen = torch.Generator().manual_seed(N)
    rowptr, col = LH.simple_graph(random_graph(N, E, hub, gen), N)
    left, right = NB.degree_scales(rowptr, "sym")
    seeds = torch.randperm(N, generator=gen)[: max(N // 20, 1)].to(DEV)
    f0 = torch.zeros(N, classes, device=DEV)
    f0[seeds, torch.randint(0, classes, (seeds.numel(),), generator=gen).to(DEV)] = 1.0
    res = {"graph": name, "nodes": N, "edges": E + hub, "nnz": int(col.numel()), "classes": classes, "rounds": a.rounds,
           "max_degree": int((rowptr[1:] - rowptr[:-1]).max())}

    def kernel():
        return ops.label_propagate(rowptr, col, f0, a.rounds, ALPHA, 1.0 - ALPHA, left=left, right=right).out

    kernel()
    above, _, got = peak(kernel)
    res["kernel_peak_mb"] = round(above / 2 ** 20, 3)
    routes = {"kernel": kernel}

    def first():
        run = torch_route(rowptr, col, left, right, f0, a.rounds)
        run()
        return (run,) + peak(run)
    out, err = attempt(first)
    if err is not None:
        res["torch_error"] = err
        torch.cuda.empty_cache()
    else:
        run, above, _, want = out
        routes["torch"] = run
        res["torch_peak_mb"] = round(above / 2 ** 20, 3)
        res["max_abs_diff"] = float((got - want).abs().max())
        res["max_abs_value"] = float(want.abs().max())
    times = alternate(routes, a.reps, warmup=a.warmup)                              # alternated: the order does not decide the result
    for k, ts in times.items():                                                     # (record_min's keys with *_us_per_round between them)
        res[f"{k}_ms"] = round(min(t.host_ms for t in ts), 4)
        res[f"{k}_event_ms"] = round(min(t.event_ms for t in ts), 4)
        res[f"{k}_us_per_round"] = round(1e3 * min(t.event_ms for t in ts) / a.rounds, 3)
        res[f"{k}_ms_runs"] = [round(t.host_ms, 4) for t in ts]
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=50)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    require_gpu("bench_label_propagation.py")
    res = {"what": "label spreading (alpha 0.9, symmetric scaling) for `rounds` rounds; kernel = gmp_label_propagate (one launch per round, a "
                   "lane group per row, sequential row sums), torch = torch.sparse.mm on a CSR of S plus one axpy per round; *_us_per_round = "
                   "device-event time of a call over its rounds",
           "rounds": a.rounds, "reps": a.reps, "warmup": a.warmup, "shapes": [bench_shape(*s, a) for s in SHAPES]}
    emit(res, a.out)
    bad = [s["graph"] for s in res["shapes"] if s.get("max_abs_diff", 0.0) > 1e-5]             # entries lie in [0, 1]: rounding leaves ~1e-7
    if bad:
        raise SystemExit(f"the kernel's result differs from the torch form's beyond rounding on {bad}")


if __name__ == "__main__":
    main()
