"""S^K X with S = D~^-1/2 (A + I) D~^-1/2 and K = 2 -- the features of the SGC baseline -- on random graphs of Cora, CiteSeer and PubMed
size and on a star-plus-noise graph whose hub has 10,000 neighbours, up to four routes in one process:

  kernel_dense    ops.feature_propagate on the dense X: gmp_feature_propagate, one launch per round, a wave per (row, 256-column strip)
  kernel_sparse   the same call on X as graph.SparseFeatures: round 1 reads the CSR directly (a wave and an LDS strip per row)
  torch_dense     torch.sparse.mm(S, torch.sparse.mm(S, X)) with S a sparse CSR tensor (values scale[i] * scale[j]) and X dense
  torch_sparse    round 1 as torch.sparse.mm(S, X) with X a sparse CSR tensor too, densified, then torch.sparse.mm(S, H) for round 2

    python scripts/bench_sgc.py [--reps 20] [--warmup 3] [--out profiles/sgc.json]

The graph, the scales, X in both forms and (for torch) S are built before the clock starts.  The sparse routes run where X is sparse (bag
of words, rows normalised to sum 1 as NormalizeFeatures leaves them); PubMed-size X is dense.  Routes run alternately and are timed by a
host clock around work that ends in a synchronise and by device events.  Peak memory is torch's allocator peak over a route's first call,
above what was allocated before it (the kernel routes' output and workspace included).  The torch forms sum a row in another order, so the
results agree to rounding, not bit for bit; the largest difference is recorded and bounded.  The two kernel routes must agree bit for bit.
The star graph measures the accepted cost of the sequential row sum: the hub's row is walked by one wave per strip."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchkit import DEV, alternate, attempt, emit, peak, random_graph, record_min, require_gpu  # noqa: E402
from gnn_pretraining_amd import ops  # noqa: E402
from gnn_pretraining_amd.finetune import node_baselines as NB  # noqa: E402
from gnn_pretraining_amd.graph import SparseFeatures  # noqa: E402

ROUNDS = 2
# name, nodes, random edges, features, density (0 = dense), hub neighbours
SHAPES = (("cora", 2708, 5429, 1433, 0.0127, 0), ("citeseer", 3327, 4552, 3703, 0.0086, 0), ("pubmed", 19717, 44324, 500, 0.0, 0),
          ("star", 20000, 40000, 1433, 0.0127, 10000))


def make_features(N: int, d: int, density: float, gen: torch.Generator):
    if not density:
        return torch.randn(N, d, generator=gen).to(DEV), None
    x = (torch.rand(N, d, generator=gen) < density).float()
    x = (x / x.sum(dim=1, keepdim=True).clamp(min=1.0)).to(DEV)
    return x, SparseFeatures.from_dense(x)


def bench_shape(name: str, N: int, E: int, d: int, density: float, hub: int, a) -> dict:
    gen = torch.Generator().manual_seed(N)
    rowptr, col, scale = NB.sgc_graph(random_graph(N, E, hub, gen), N)
    x, xs = make_features(N, d, density, gen)
    res = {"graph": name, "nodes": N, "edges": E + hub, "nnz": int(col.numel()), "features": d, "rounds": ROUNDS,
           "feature_nnz": int(xs.nnz) if xs is not None else N * d, "max_degree": int((rowptr[1:] - rowptr[:-1]).max())}
    row = torch.repeat_interleave(torch.arange(N, device=DEV), (rowptr[1:] - rowptr[:-1]).to(torch.int64))
    S = torch.sparse_csr_tensor(rowptr.to(torch.int64), col.to(torch.int64), scale[row] * scale[col.to(torch.int64)], size=(N, N))

    def kernel_dense():
        return ops.feature_propagate(rowptr, col, x, ROUNDS, left=scale, right=scale).out

    def torch_dense():
        return torch.sparse.mm(S, torch.sparse.mm(S, x))

    candidates = {"kernel_dense": kernel_dense, "torch_dense": torch_dense}
    if xs is not None:
        xt = torch.sparse_csr_tensor(xs.rowptr.to(torch.int64), xs.col.to(torch.int64), xs.val, size=(N, d))

        def kernel_sparse():
            return ops.feature_propagate(rowptr, col, xs, ROUNDS, left=scale, right=scale).out

        def torch_sparse():
            return torch.sparse.mm(S, torch.sparse.mm(S, xt).to_dense())

        candidates = {"kernel_dense": kernel_dense, "kernel_sparse": kernel_sparse, "torch_dense": torch_dense, "torch_sparse": torch_sparse}
    routes, outs = {}, {}
    for k, fn in candidates.items():
        def first(fn=fn):
            fn()
            return peak(fn)
        got, err = attempt(first)
        if err is not None:
            res[f"{k}_error"] = err
            torch.cuda.empty_cache()
            continue
        routes[k], outs[k] = fn, got.out
        res[f"{k}_peak_mb"] = round(got.above_bytes / 2 ** 20, 3)
    want = outs["kernel_dense"]
    res["max_abs_value"] = float(want.abs().max())
    if "kernel_sparse" in outs:
        res["kernel_sparse_equals_kernel_dense_bitwise"] = bool(torch.equal(outs["kernel_sparse"].view(torch.int32), want.view(torch.int32)))
    for k in ("torch_dense", "torch_sparse"):
        if k in outs:
            res[f"{k}_max_abs_diff"] = float((outs[k] - want).abs().max())
    outs.clear()
    record_min(res, alternate(routes, a.reps, warmup=a.warmup), 4)                  # alternated: the order does not decide the result
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    require_gpu("bench_sgc.py")
    res = {"what": "S^2 X, S = D~^-1/2 (A + I) D~^-1/2; kernel_* = gmp_feature_propagate (one launch per round, sequential row sums) on the "
                   "dense / the CSR X, torch_* = torch.sparse.mm on a CSR of S with the dense / the CSR X; *_event_ms = device-event time "
                   "of a call, *_peak_mb = allocator peak above the inputs",
           "rounds": ROUNDS, "reps": a.reps, "warmup": a.warmup, "shapes": [bench_shape(*s, a) for s in SHAPES]}
    emit(res, a.out)
    bad = [s["graph"] for s in res["shapes"] if not s.get("kernel_sparse_equals_kernel_dense_bitwise", True)
           or any(s.get(f"{k}_max_abs_diff", 0.0) > 1e-5 * max(s["max_abs_value"], 1.0) for k in ("torch_dense", "torch_sparse"))]
    if bad:
        raise SystemExit(f"the kernel's result differs from the torch form's beyond rounding on {bad}")


if __name__ == "__main__":
    main()
