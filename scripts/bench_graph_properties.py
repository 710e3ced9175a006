"""Cost of the 12 graph-property targets of a dataset, two routes over the same graphs:

  host     GraphPropertyCalculator.compute_for_dataset(graphs): scipy per graph (sparse A @ A, connected_components, all-pairs Dijkstra)
  device   GraphPropertyCalculator.compute_for_dataset(graphs, device="cuda"): collation, gmp_graph_props (csrc/graph_props.hip), one
           read-back of [B, 16] integers per chunk, properties_from_counts on the host

    python scripts/bench_graph_properties.py [--reps 5] [--graphs 512] [--step-timeout 300] [--out profiles/graph_properties.json]

Cases: synthetic datasets with the public size statistics of the four pre-training domains (data_setup.TU_STATS: MUTAG, PROTEINS, NCI1,
ENZYMES; --graphs graphs each, at most the public count) and one 620-node graph (the largest PROTEINS graph).  Every case runs as a
process of its own under --step-timeout (this script with --case NAME) and the parent stops at the first case that fails or runs out of
time.  Per case: wall time of each route (host clock, device synchronised, median and minimum over --reps after one discarded call),
the kernel alone (device events around ops.graph_properties on the collated batch) and the largest |difference| of the two routes'
float32 targets."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = ["MUTAG", "PROTEINS", "NCI1", "ENZYMES", "one_graph_620"]


def case_graphs(name: str, count: int):
    import torch
    from gnn_pretraining_amd import synthetic
    from gnn_pretraining_amd.constants import DOMAIN_DIMENSIONS
    from gnn_pretraining_amd.data.data_setup import TU_STATS
    gen = torch.Generator().manual_seed(1234)
    if name == "one_graph_620":
        return [_fixed_size_graph(gen, 620, 1200)]          # synthetic.random_graph clips n at 126
    total, mean_nodes, mean_edges, classes = TU_STATS[name]
    return [synthetic.random_graph(gen, DOMAIN_DIMENSIONS[name], mean_nodes, mean_edges, classes) for _ in range(min(count, total))]


def _fixed_size_graph(gen, nodes: int, edges: int):
    import torch
    from gnn_pretraining_amd.graph import Data
    src, dst = torch.randint(0, nodes, (edges,), generator=gen), torch.randint(0, nodes, (edges,), generator=gen)
    return Data(torch.zeros(nodes, 1), torch.stack([torch.cat([src, dst]), torch.cat([dst, src])]))


def run_case(name: str, count: int, reps: int) -> dict:
    import numpy as np
    import torch
    from gnn_pretraining_amd import ops
    from gnn_pretraining_amd.data.graph_properties import GraphPropertyCalculator
    graphs, calc = case_graphs(name, count), GraphPropertyCalculator()

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), out

    host = lambda: calc.compute_for_dataset(graphs)
    device = lambda: calc.compute_for_dataset(graphs, device="cuda")
    want, got = host(), device()                                     # also the discarded first call of each route
    ht, dt = [], []
    for _ in range(reps):                                            # alternate: neither route owns a quiet or a noisy stretch
        ht.append(wall_ms(host)[0])
        dt.append(wall_ms(device)[0])

    sizes = np.array([int(g.num_nodes) for g in graphs], dtype=np.int64)
    ptr = torch.from_numpy(np.concatenate([[0], np.cumsum(sizes)])).cuda()
    eptr = torch.from_numpy(np.concatenate([[0], np.cumsum([int(g.edge_index.size(1)) for g in graphs])]).astype(np.int64)).cuda()
    ei = torch.cat([g.edge_index + int(o) for g, o in zip(graphs, ptr[:-1].tolist())], dim=1).contiguous().cuda()
    big = int(sizes.max())
    ops.graph_properties(ptr, eptr, ei, max_graph_nodes=big)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        ops.graph_properties(ptr, eptr, ei, max_graph_nodes=big)
    e1.record()
    torch.cuda.synchronize()
    r = lambda x: round(x, 4)
    return {"case": name, "graphs": len(graphs), "nodes": int(sizes.sum()), "largest_graph": big, "reps": reps,
            "host_ms_median": r(statistics.median(ht)), "host_ms_min": r(min(ht)),
            "device_ms_median": r(statistics.median(dt)), "device_ms_min": r(min(dt)),
            "host_over_device": round(statistics.median(ht) / statistics.median(dt), 2),
            "kernel_event_ms": r(e0.elapsed_time(e1) / reps),
            "max_abs_difference_float32": float((got.double() - want.double()).abs().max())}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--graphs", type=int, default=512)
    ap.add_argument("--step-timeout", type=float, default=300.0)
    ap.add_argument("--case", default=None, help="run one case in this process and print its JSON line (what the parent starts)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from benchkit import emit, require_gpu                            # (brings torch: imported where this script imports torch)
    if a.case:
        require_gpu("bench_graph_properties.py")                      # in the case's process: the parent opens no device, it only starts them
        emit(run_case(a.case, a.graphs, a.reps), None)
        return
    results = []
    for name in CASES:
        cmd = [sys.executable, os.path.abspath(__file__), "--case", name, "--reps", str(a.reps), "--graphs", str(a.graphs)]
        try:
            done = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
        except subprocess.TimeoutExpired:
            raise SystemExit(f"case {name}: no result within {a.step_timeout} s; stopping")
        if done.returncode != 0:
            sys.stderr.write(done.stderr)
            raise SystemExit(f"case {name}: exit status {done.returncode}; stopping")
        results.append(json.loads(done.stdout.strip().splitlines()[-1]))
    emit({"cases": results}, a.out)


if __name__ == "__main__":
    main()
