"""Filtered ranking of Q = 1,000 true edges against all nodes under the Adamic-Adar baseline, on random graphs of Cora, PubMed and
65,535-node size, two routes in one process:

  kernel   link_heuristics.heuristic_ranks: gmp_lp_cn_rank, two launches, an accumulator per candidate tile in LDS, no Q x N array
  torch    the natural torch form: the sparse rows A[src] (Q x N) times diag(w) A -- as a sparse N x N matrix (torch_sparse) and as a
           dense one (torch_dense) -- gives the dense Q x N scores; then comparisons against the true pair's score under a dense Q x N
           mask of the known edges, and row sums

    python scripts/bench_lp_heuristics.py [--queries 1000] [--reps 10] [--warmup 2] [--out profiles/lp_heuristics.json]

The simple graph, the weights and the filter CSR are built before the clock starts (both routes start from them).  Routes run
alternately and are timed by a host clock around work that ends in a synchronise and by device events.  Peak memory is torch's
allocator peak over a route's first call, above what was allocated before it.  A route that cannot run (out of memory, an operator
the installed torch lacks) is recorded with the error instead of a time.  The torch form adds in another order, so its Adamic-Adar
counts may differ from the kernel's in ties; the cross-check that must hold is on common neighbours, whose sums are exact integers."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchkit import DEV, alternate, attempt, emit, peak, record_min, require_gpu  # noqa: E402
from gnn_pretraining_amd.finetune import link_heuristics as LH  # noqa: E402
from gnn_pretraining_amd.operators import csr_of  # noqa: E402

SHAPES = ((2708, 5429), (19717, 44324), (65535, 200000))


def torch_route(rowptr, col, weight, pos, known, N, dense: bool):
    """Returns the closure of the torch form; what it needs besides the inputs (the matrix diag(w) A, the row index of every entry) is
    built here, outside the clock, and counted as its input."""
    rp, cl = rowptr.to(torch.int64), col.to(torch.int64)
    deg = rp[1:] - rp[:-1]
    row = torch.repeat_interleave(torch.arange(N, device=DEV), deg)
    w = torch.ones(N, device=DEV) if weight is None else weight
    W = torch.sparse_coo_tensor(torch.stack([row, cl]), w[row], size=(N, N)).coalesce()
    if dense:
        W = W.to_dense()
    src, dst = pos[0], pos[1]
    Q = src.numel()
    qs = torch.arange(Q, device=DEV)
    csr = csr_of(known, N)
    frp, fcl = csr.rowptr_t.to(torch.int64), csr.col_t.to(torch.int64)

    def run():
        d = deg[src]
        qrow = torch.repeat_interleave(qs, d)                                       # A[src] as a sparse Q x N matrix
        start = torch.cumsum(d, 0) - d
        within = torch.arange(qrow.numel(), device=DEV) - start[qrow]
        a_src = torch.sparse_coo_tensor(torch.stack([qrow, cl[rp[src][qrow] + within]]), torch.ones(qrow.numel(), device=DEV), size=(Q, N))
        scores = torch.sparse.mm(a_src, W)
        if scores.layout != torch.strided:
            scores = scores.to_dense()
        keep = torch.ones(Q, N, dtype=torch.bool, device=DEV)
        keep[qs, src] = False
        keep[qs, dst] = False
        fd = frp[src + 1] - frp[src]                                                # the filter rows of the sources
        frow = torch.repeat_interleave(qs, fd)
        fwithin = torch.arange(frow.numel(), device=DEV) - (torch.cumsum(fd, 0) - fd)[frow]
        keep[frow, fcl[frp[src][frow] + fwithin]] = False
        true = scores[qs, dst][:, None]
        return ((scores > true) & keep).sum(1).to(torch.int32), ((scores == true) & keep).sum(1).to(torch.int32)

    return run


def bench_shape(N: int, E: int, a) -> dict:
    gen = torch.Generator().manual_seed(N)
    graph = torch.randint(0, N, (2, E), generator=gen).to(DEV).contiguous()
    rowptr, col = LH.simple_graph(graph, N)
    pick = torch.randperm(E, generator=gen)[:a.queries].to(DEV)
    pos = graph[:, pick].contiguous()
    pos = pos[:, pos[0] != pos[1]].contiguous()
    known = torch.cat([graph, graph.flip(0)], dim=1).contiguous()
    weight = LH.node_weights(rowptr[1:] - rowptr[:-1], "aa").to(DEV)
    res = {"nodes": N, "edges": E, "nnz": int(col.numel()), "queries": int(pos.size(1)), "max_degree": int((rowptr[1:] - rowptr[:-1]).max())}

    def kernel(kind="aa"):
        r = LH.heuristic_ranks(graph, N, pos, kind, filter_edges=known)
        return r.n_greater, r.n_equal

    kernel()                                                                        # the cached graph, weights and filter CSR exist from here on
    above, _, got = peak(kernel)
    res["kernel_peak_mb"] = round(above / 2 ** 20, 3)
    routes = {"kernel": kernel}
    for name, dense in (("torch_sparse", False), ("torch_dense", True)):
        def first(dense=dense):
            run = torch_route(rowptr, col, weight, pos, known, N, dense)
            return (run,) + peak(run)
        out, err = attempt(first)
        if err is not None:
            res[f"{name}_error"] = err
            torch.cuda.empty_cache()
            continue
        run, above, _, want = out
        routes[name] = run
        res[f"{name}_peak_mb"] = round(above / 2 ** 20, 3)
        res[f"{name}_aa_counts_equal"] = bool(torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]))
        cn_run, err = attempt(lambda dense=dense: torch_route(rowptr, col, None, pos, known, N, dense)())
        if err is None:
            cn = kernel("cn")
            res[f"{name}_cn_counts_equal"] = bool(torch.equal(cn[0], cn_run[0]) and torch.equal(cn[1], cn_run[1]))
    reps = {k: a.reps if k == "kernel" else max(a.reps // 5, 1) for k in routes}
    record_min(res, alternate(routes, reps, warmup=a.warmup), 3)                    # alternated: the order does not decide the result
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    require_gpu("bench_lp_heuristics.py")
    res = {"what": "Adamic-Adar filtered ranking of true edges against all nodes on uniform random graphs; kernel = gmp_lp_cn_rank (push form, "
                   "the only form built), torch = sparse A[src] times sparse / dense diag(w) A, then compare and count under a dense mask",
           "reps": a.reps, "warmup": a.warmup, "shapes": [bench_shape(N, E, a) for N, E in SHAPES]}
    emit(res, a.out)
    bad = [s["nodes"] for s in res["shapes"] for k, v in s.items() if k.endswith("_cn_counts_equal") and not v]
    if bad:
        raise SystemExit(f"the kernel's common-neighbour counts differ from the torch form's at N = {bad}")


if __name__ == "__main__":
    main()
