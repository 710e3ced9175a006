"""Filtered ranking of Q = 1,000 true edges against all nodes under the walk-based baselines -- rooted PageRank with 20 rounds and Katz
with 6 -- on random graphs of Cora, PubMed and 65,535-node size, three routes in one process:

  kernel     link_walks.walk_ranks: gmp_lp_walk_rank, one launch, one workgroup per query with its three vectors in LDS (or, beyond
             gmp_lp_walk_lds_nodes() nodes, in a bounded workspace), no Q x N array
  spmm       the natural torch form: Y <- a * torch.sparse.mm(A diag(w), Y) on a dense N x Q one-hot, accumulated per round; then
             comparisons against the true pair's score under a dense Q x N mask of the known edges, and row sums
  labelprop  the same through ops.label_propagate, 32 one-hot columns at a time, one launch per round and an N x 32 matrix per chunk,
             then the same mask, compare and count per chunk in torch -- the only way to these baselines before the kernel

    python scripts/bench_lp_walks.py [--queries 1000] [--reps 5] [--warmup 1] [--out profiles/lp_walks.json]

The simple graph, the weights and the filter CSR are built before the clock starts (all routes start from them).  Routes run alternately
and are timed by a host clock around work that ends in a synchronise and by device events.  Peak memory is torch's allocator peak over a
route's first call, above what was allocated before it.  A route that cannot run (out of memory, an operator the installed torch lacks)
is recorded with the error instead of a time.  The labelprop route makes the kernel's operations in the kernel's order, so its counts
must equal the kernel's; spmm adds in another order, so its counts may differ in ties and the comparison is recorded, not required."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchkit import DEV, alternate, attempt, emit, keep_mask, peak, record_min, require_gpu  # noqa: E402
from gnn_pretraining_amd import _lib as L, ops  # noqa: E402
from gnn_pretraining_amd.finetune import link_heuristics as LH, link_walks as LW  # noqa: E402
from gnn_pretraining_amd.operators import csr_of  # noqa: E402

SHAPES = ((2708, 5429), (19717, 44324), (65535, 200000))
CASES = (("ppr", 20), ("katz", 6))
CHUNK = ops.LABELPROP_MAX_CLASSES


def count(acc_t, src, dst, frp, fcl, N):
    """(n_greater, n_equal) from scores [Q, N] (a view of the N x Q accumulator)."""
    true = acc_t[torch.arange(src.numel(), device=DEV), dst][:, None]
    keep = keep_mask(src, dst, frp, fcl, N)
    return ((acc_t > true) & keep).sum(1).to(torch.int32), ((acc_t == true) & keep).sum(1).to(torch.int32)


def spmm_route(rowptr, col, weight, damping, rounds, pos, frp, fcl, N):
    """The closure of the torch.sparse.mm form; the matrix A diag(w) is built here, outside the clock, and counted as its input."""
    rp, cl = rowptr.to(torch.int64), col.to(torch.int64)
    row = torch.repeat_interleave(torch.arange(N, device=DEV), rp[1:] - rp[:-1])
    val = torch.ones(cl.numel(), device=DEV) if weight is None else weight[cl]
    W = torch.sparse_coo_tensor(torch.stack([row, cl]), val, size=(N, N)).coalesce()
    src, dst = pos[0], pos[1]
    Q = src.numel()

    def run():
        y = torch.zeros(N, Q, device=DEV)
        y[src, torch.arange(Q, device=DEV)] = 1.0
        acc = torch.zeros(N, Q, device=DEV)
        for _ in range(rounds):
            y = damping * torch.sparse.mm(W, y)
            acc += y
        return count(acc.t(), src, dst, frp, fcl, N)

    return run


def labelprop_route(rowptr, col, weight, damping, rounds, pos, frp, fcl, N):
    """The closure of the route through ops.label_propagate: 32 sources a chunk, one call (one launch) per round, accumulated in torch."""
    src, dst = pos[0], pos[1]
    Q = src.numel()

    def run():
        greater, equal = [], []
        for lo in range(0, Q, CHUNK):
            s, d = src[lo:lo + CHUNK], dst[lo:lo + CHUNK]
            y = torch.zeros(N, CHUNK, device=DEV)
            y[s, torch.arange(s.numel(), device=DEV)] = 1.0
            acc = torch.zeros(N, CHUNK, device=DEV)
            for _ in range(rounds):
                y = ops.label_propagate(rowptr, col, y, 1, damping, 0.0, right=weight).out
                acc += y
            g, e = count(acc.t()[:s.numel()], s, d, frp, fcl, N)
            greater.append(g); equal.append(e)
        return torch.cat(greater), torch.cat(equal)

    return run


def bench_case(graph, N, pos, known, kind: str, rounds: int, a) -> dict:
    rowptr, col, weight, damping, _ = LW._kernel_args(graph, N, kind)
    csr = csr_of(known, N)
    frp, fcl = csr.rowptr_t.to(torch.int64), csr.col_t.to(torch.int64)
    res = {"kind": kind, "rounds": rounds}

    def kernel():
        r = LW.walk_ranks(graph, N, pos, kind, rounds, filter_edges=known)
        return r.n_greater, r.n_equal

    kernel()                                                                        # the cached graph, weights and filter CSR exist from here on
    above, _, got = peak(kernel)
    res["kernel_peak_mb"] = round(above / 2 ** 20, 3)
    routes = {"kernel": kernel}
    for name, make in (("spmm", spmm_route), ("labelprop", labelprop_route)):
        def first(make=make):
            run = make(rowptr, col, weight, damping, rounds, pos, frp, fcl, N)
            return (run,) + peak(run)
        out, err = attempt(first)
        if err is not None:
            res[f"{name}_error"] = err
            torch.cuda.empty_cache()
            continue
        run, above, _, want = out
        routes[name] = run
        res[f"{name}_peak_mb"] = round(above / 2 ** 20, 3)
        res[f"{name}_counts_equal"] = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
        res[f"{name}_queries_with_other_counts"] = int(((got[0] != want[0]) | (got[1] != want[1])).sum())
    reps = {k: a.reps if k == "kernel" else max(a.reps // 5, 1) for k in routes}
    record_min(res, alternate(routes, reps, warmup=a.warmup), 3)                    # alternated: the order does not decide the result
    return res


def bench_shape(N: int, E: int, a) -> dict:
    gen = torch.Generator().manual_seed(N)
    graph = torch.randint(0, N, (2, E), generator=gen).to(DEV).contiguous()
    rowptr, col = LH.simple_graph(graph, N)
    pick = torch.randperm(E, generator=gen)[:a.queries].to(DEV)
    pos = graph[:, pick].contiguous()
    pos = pos[:, pos[0] != pos[1]].contiguous()
    known = torch.cat([graph, graph.flip(0)], dim=1).contiguous()
    return {"nodes": N, "edges": E, "nnz": int(col.numel()), "queries": int(pos.size(1)), "max_degree": int((rowptr[1:] - rowptr[:-1]).max()),
            "kernel_storage": "lds" if N <= L.lib().gmp_lp_walk_lds_nodes() else "workspace",
            "kernel_workspace_mb": round(L.lib().gmp_lp_walk_workspace_bytes(int(pos.size(1)), N) / 2 ** 20, 3),
            "cases": [bench_case(graph, N, pos, known, kind, rounds, a) for kind, rounds in CASES]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    require_gpu("bench_lp_walks.py")
    res = {"what": "filtered ranking of true edges against all nodes under rooted PageRank (20 rounds) and Katz (6 rounds) on uniform random "
                   "graphs; kernel = gmp_lp_walk_rank (one workgroup per query), spmm = torch.sparse.mm on an N x Q one-hot per round, "
                   "labelprop = ops.label_propagate on 32 columns at a time, both then compare and count under a dense mask",
           "reps": a.reps, "warmup": a.warmup, "lds_nodes": L.lib().gmp_lp_walk_lds_nodes(),
           "resident_blocks": L.lib().gmp_lp_walk_resident_blocks(), "shapes": [bench_shape(N, E, a) for N, E in SHAPES]}
    emit(res, a.out)
    bad = [(s["nodes"], c["kind"]) for s in res["shapes"] for c in s["cases"] if c.get("labelprop_counts_equal") is False]
    if bad:
        raise SystemExit(f"the kernel's counts differ from the label_propagate route's at {bad}")


if __name__ == "__main__":
    main()
