"""The Weisfeiler-Lehman subtree baseline on synthetic batches of ENZYMES, NCI1 and PROTEINS shape, two routes in one process:

  kernel   ops.wl_refine (gmp_wl_refine: one launch per batch, colours, sorted lists and histograms made in LDS) and ops.wl_gram
           (gmp_wl_gram: one wave per Gram entry, equal runs counted by binary searches)
  torch    the same definition written in torch: the int64 wrap-around mix, one index_add_ per round and a scatter for the histogram; for
           the Gram torch.unique(return_inverse=True) over all colours, a dense [G, colours] count matrix and its product with itself

    python scripts/bench_wl.py [--iters 3] [--dim 256] [--reps 10] [--warmup 2] [--out profiles/wl.json]

The simple CSR is built before the clock starts (both routes start from it).  Routes run alternately and are timed by a host clock around
work that ends in a synchronise and by device events.  Peak memory is torch's allocator peak over a route's first call, above what was
allocated before it.  A route that cannot run (out of memory) is recorded with the error instead of a time.  Both routes are exact integer
arithmetic: the colours, the histograms and the Gram must be equal, and the script fails when they are not."""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchkit import DEV, GRAPH_SHAPES, alternate, attempt, emit, peak, record_min, require_gpu, synthetic_batch  # noqa: E402
from gnn_pretraining_amd import ops  # noqa: E402
from gnn_pretraining_amd.finetune.link_heuristics import simple_graph  # noqa: E402


def _s64(v: int) -> int:
    return v - (1 << 64) if v >= (1 << 63) else v


K1, K2, M1, M2 = (_s64(v) for v in (0x9E3779B97F4A7C15, 0xD1B54A32D192ED03, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB))


def _lsr(z, s: int):
    return (z >> s) & ((1 << (64 - s)) - 1)                                       # a logical shift of the two's-complement word


def mix(z):
    z = z ^ _lsr(z, 30)
    z = z * M1
    z = z ^ _lsr(z, 27)
    z = z * M2
    return z ^ _lsr(z, 31)


def torch_refine(ptr, rowptr, col, labels, iters: int, dim: int):
    """(colors [iters + 1, N], hist [G, dim]) of the definition in torch; the row index of every entry is made here, outside the clock."""
    N, G = rowptr.numel() - 1, ptr.numel() - 1
    rp, cl = rowptr.to(torch.int64), col.to(torch.int64)
    deg = rp[1:] - rp[:-1]
    row = torch.repeat_interleave(torch.arange(N, device=DEV), deg)
    gid = torch.repeat_interleave(torch.arange(G, device=DEV), ptr[1:] - ptr[:-1])
    start = deg if labels is None else labels

    def run():
        colors = torch.empty(iters + 1, N, dtype=torch.int64, device=DEV)
        colors[0] = mix(start + K1)
        for t in range(iters):
            s = torch.zeros(N, dtype=torch.int64, device=DEV)
            s.index_add_(0, row, mix(colors[t])[cl])
            colors[t + 1] = mix(colors[t] * K1 + s + _s64(((t + 1) * K2) % (1 << 64)))         # the round's constant, wrapped on the host
        bucket = (_lsr(colors, 32) * dim) >> 32
        hist = torch.zeros(G * dim, dtype=torch.int32, device=DEV)
        hist.index_add_(0, (gid[None, :] * dim + bucket).reshape(-1), torch.ones(colors.numel(), dtype=torch.int32, device=DEV))
        return colors, hist.view(G, dim)

    return run, gid


def torch_gram(colors, gid, G: int):
    def run():
        uniq, inv = torch.unique(colors.reshape(-1), return_inverse=True)
        counts = torch.zeros(G, uniq.numel(), device=DEV)
        counts.index_put_((gid.repeat(colors.size(0)), inv), torch.ones(inv.numel(), device=DEV), accumulate=True)
        return (counts @ counts.t()).to(torch.int64)

    return run


def bench_shape(name: str, graphs: int, mean_nodes: float, mean_edges: float, big: int, num_labels: int, a) -> dict:
    gen = torch.Generator().manual_seed(graphs)
    ptr, edge_index, N, labels = synthetic_batch(graphs, mean_nodes, mean_edges, big, num_labels, gen)
    rowptr, col = simple_graph(edge_index, N)
    mgn = int((ptr[1:] - ptr[:-1]).max())
    res = {"name": name, "graphs": graphs, "nodes": N, "nnz": int(col.numel()), "max_graph_nodes": mgn, "labels": num_labels or "degrees"}

    def k_refine():
        return ops.wl_refine(ptr, rowptr, col, labels, a.iters, a.dim, max_graph_nodes=mgn, return_colors=True)

    k_refine()
    above, _, ref = peak(lambda: ops.wl_refine(ptr, rowptr, col, labels, a.iters, a.dim, max_graph_nodes=mgn))
    res["refine_kernel_peak_mb"] = round(above / 2 ** 20, 3)
    ref = k_refine()
    assert not bool(ref.status.any())

    def k_gram():
        return ops.wl_gram(ref.sorted, ptr, ref.sorted, ptr, a.iters)

    above, _, K = peak(k_gram)
    res["gram_kernel_peak_mb"] = round(above / 2 ** 20, 3)
    routes = {"refine_kernel": lambda: ops.wl_refine(ptr, rowptr, col, labels, a.iters, a.dim, max_graph_nodes=mgn), "gram_kernel": k_gram}
    t_refine, gid = torch_refine(ptr, rowptr, col, labels, a.iters, a.dim)
    out, err = attempt(lambda: peak(t_refine))
    if err is not None:
        res["refine_torch_error"] = err
    else:
        res["refine_torch_peak_mb"] = round(out.above_bytes / 2 ** 20, 3)
        res["refine_equal"] = bool(torch.equal(out.out[0], ref.colors) and torch.equal(out.out[1], ref.hist))
        routes["refine_torch"] = t_refine
    t_gram = torch_gram(ref.colors, gid, graphs)
    out, err = attempt(lambda: peak(t_gram))
    if err is not None:
        res["gram_torch_error"] = err
        torch.cuda.empty_cache()
    else:
        res["gram_torch_peak_mb"] = round(out.above_bytes / 2 ** 20, 3)
        res["gram_equal"] = bool(torch.equal(out.out, K))
        routes["gram_torch"] = t_gram
    del out
    reps = {k: a.reps if k.endswith("kernel") else max(a.reps // 5, 1) for k in routes}
    record_min(res, alternate(routes, reps, warmup=a.warmup), 3)                  # alternated: the order does not decide the result
    return res


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=3)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    require_gpu("bench_wl.py")
    res = {"what": "WL subtree refinement (colours, sorted lists, histograms) of one batch and the Gram of the batch with itself; kernel = "
                   "gmp_wl_refine / gmp_wl_gram, torch = int64 mix + index_add_ per round, torch.unique + dense count-matrix product",
           "iters": a.iters, "dim": a.dim, "reps": a.reps, "warmup": a.warmup, "shapes": [bench_shape(*s, a) for s in GRAPH_SHAPES]}
    emit(res, a.out)
    bad = [s["name"] for s in res["shapes"] for k, v in s.items() if k.endswith("_equal") and not v]
    if bad:
        raise SystemExit(f"the kernel and the torch form disagree on {bad}")


if __name__ == "__main__":
    main()
