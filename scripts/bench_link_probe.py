"""Filtered ranking of Q = 1,000 true edges against all nodes by the cosine and by the inner product of random d = 256 embeddings, on
random graphs of Cora, PubMed and 65,535-node size, three routes in one process:

  kernel   link_probe.embedding_ranks: gmp_emb_link_rank -- a normalise / pad pass, the true pairs' scores, then one streaming launch
           that compares and counts in registers; no Q x N array
  torch    the natural torch form: F.normalize (cos), the sources' rows gathered, one Q x N matmul, a dense Q x N mask of the known
           edges, compare with the true pair's score and row sums
  scorer   operators.lp_rank, what LinkPredictionEngine.rank launches, on the same embeddings and pairs with random 768 -> 256 -> 1
           weights: not an alternative, the context -- what ranking with the trained scorer costs at the same Q and N

    python scripts/bench_link_probe.py [--queries 1000] [--reps 20] [--warmup 3] [--out profiles/link_probe.json]

The filter CSR is built before the clock starts (all routes start from it).  Routes run alternately and are timed by a host clock around
work that ends in a synchronise and by device events.  Peak memory is torch's allocator peak over a route's first call, above what was
allocated before it (the inputs).  A route that cannot run (out of memory) is recorded with the error instead of a time.  The torch
route adds in another order than the MFMA chain, so its counts may differ where scores tie to the last bit: the comparison is recorded,
not required.  No time is a pass criterion."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from benchkit import DEV, alternate, attempt, emit, keep_mask, peak, record_min, require_gpu  # noqa: E402
from gnn_pretraining_amd import _lib as L, operators as O  # noqa: E402
from gnn_pretraining_amd.finetune import link_probe as LPR  # noqa: E402
from gnn_pretraining_amd.operators import csr_of  # noqa: E402

SHAPES = ((2708, 5429), (19717, 44324), (65535, 200000))
DIM = 256


def torch_route(h, pos, frp, fcl, kind):
    src, dst = pos[0], pos[1]
    N = h.size(0)

    def run():
        z = F.normalize(h, dim=1) if kind == "cos" else h
        S = z[src] @ z.t()
        true = S[torch.arange(src.numel(), device=src.device), dst][:, None]
        keep = keep_mask(src, dst, frp, fcl, N)
        return ((S > true) & keep).sum(1).to(torch.int32), ((S == true) & keep).sum(1).to(torch.int32)

    return run


def bench_kind(h, pos, known, frp, fcl, kind: str, scorer, a) -> dict:
    res = {"kind": kind}

    def kernel():
        r = LPR.embedding_ranks(h, pos, kind, filter_edges=known)
        return r.n_greater, r.n_equal

    kernel()                                                                        # the cached filter CSR exists from here on
    above, _, got = peak(kernel)
    res["kernel_peak_mb"] = round(above / 2 ** 20, 3)
    routes = {"kernel": kernel}

    def first():
        run = torch_route(h, pos, frp, fcl, kind)
        return (run,) + peak(run)
    out, err = attempt(first)
    if err is not None:
        res["torch_error"] = err
        torch.cuda.empty_cache()
    else:
        run, above, _, want = out
        routes["torch"] = run
        res["torch_peak_mb"] = round(above / 2 ** 20, 3)
        res["torch_queries_with_other_counts"] = int(((got[0] != want[0]) | (got[1] != want[1])).sum())
        res["torch_max_rank_difference"] = float(((got[0] - want[0]).float() + 0.5 * (got[1] - want[1]).float()).abs().max())
    if scorer is not None:                                                          # once per shape: it does not depend on the kind
        routes["scorer"] = scorer
        res["scorer_peak_mb"] = round(peak(scorer).above_bytes / 2 ** 20, 3)
    reps = {k: max(a.reps // 5, 1) if k == "scorer" else a.reps for k in routes}
    record_min(res, alternate(routes, reps, warmup=a.warmup), 3)                    # alternated: the order does not decide the result
    return res


def bench_shape(N: int, E: int, a) -> dict:
    gen = torch.Generator().manual_seed(N)
    graph = torch.randint(0, N, (2, E), generator=gen).to(DEV).contiguous()
    h = torch.randn(N, DIM, generator=gen).to(DEV)
    pick = torch.randperm(E, generator=gen)[:a.queries].to(DEV)
    pos = graph[:, pick].contiguous()
    pos = pos[:, pos[0] != pos[1]].contiguous()
    known = torch.cat([graph, graph.flip(0)], dim=1).contiguous()
    csr = csr_of(known, N)
    frp, fcl = csr.rowptr_t.to(torch.int64), csr.col_t.to(torch.int64)
    w0, b0 = torch.randn(256, 768, generator=gen).to(DEV) / 28, torch.zeros(256, device=DEV)
    w3, b3 = torch.randn(1, 256, generator=gen).to(DEV) / 16, torch.zeros(1, device=DEV)
    scorer = lambda: O.lp_rank(h, pos, w0, b0, w3, b3, filter_edges=known)                          # noqa: E731
    Q = int(pos.size(1))
    return {"nodes": N, "edges": E, "queries": Q, "dim": DIM, "filter_entries": int(fcl.numel()),
            "kernel_workspace_mb": round(L.lib().gmp_emb_link_workspace_bytes(N, Q, DIM) / 2 ** 20, 3),
            "dense_scores_mb": round(4 * Q * N / 2 ** 20, 3),
            "kinds": [bench_kind(h, pos, known, frp, fcl, kind, scorer if kind == "cos" else None, a) for kind in LPR.KINDS]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--queries", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    require_gpu("bench_link_probe.py")
    res = {"what": "filtered ranking of true edges against all nodes by the cosine / the inner product of random d = 256 embeddings on uniform "
                   "random graphs; kernel = gmp_emb_link_rank (streaming, no Q x N array), torch = normalize + gather + Q x N matmul + dense "
                   "mask + compare and count, scorer = gmp_lp_rank with the 768 -> 256 -> 1 MLP on the same pairs (context, timed beside cos)",
           "reps": a.reps, "warmup": a.warmup, "shapes": [bench_shape(N, E, a) for N, E in SHAPES]}
    emit(res, a.out)


if __name__ == "__main__":
    main()
