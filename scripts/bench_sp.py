"""The shortest-path kernel baseline on the synthetic batches of ENZYMES, NCI1 and PROTEINS shape that scripts/bench_wl.py uses, two routes
in one process:

  kernel   ops.sp_features (gmp_sp_features: one launch per batch, a bit-set BFS per source and the key table in LDS) and ops.sp_gram
           (gmp_sp_gram: one wave per Gram entry, the shorter key row binary-searched in the longer)
  torch    the same definition written in torch: the padded dense adjacency [G, P, P], distances by repeated boolean products (one batched
           matrix product per level, until no level finds a pair), torch.unique over the (graph, key) rows; for the Gram torch.unique
           over all keys, a dense [G, keys] count matrix in fp64 and its product with itself

    python scripts/bench_sp.py [--max-dist 1023] [--dim 256] [--reps 10] [--warmup 2] [--out profiles/sp.json]

The simple CSR, and for the torch route the dense adjacency, are built before the clock starts.  The row stride of the kernel's outputs is
the one finetune/graph_baselines.py takes: the node pairs of the largest graph, up to gmp_sp_max_unique.  Routes run alternately and are
timed per call by a host clock around work that ends in a synchronise and by device events.  Peak memory is torch's allocator peak over
a route's first call, above what was allocated before it.  A route that cannot run (out of memory) is recorded with the error instead of
a time.  The status words are recorded, not asserted: a graph with more distinct keys than the stride (status bit 1) is reported as such,
and is left out of the comparison.  Both routes are exact integer arithmetic: the keys, the counts and the Gram must be equal, and the
script fails when they are not."""
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


def dense_batch(ptr, rowptr, col, labels):
    """(A bool [G, P, P], lab int64 [G, P], upper bool [G, P, P] = the pairs u < v of real nodes), P = the largest graph."""
    G, N = ptr.numel() - 1, rowptr.numel() - 1
    sizes = ptr[1:] - ptr[:-1]
    P = int(sizes.max())
    gid = torch.repeat_interleave(torch.arange(G, device=DEV), sizes)
    local = torch.arange(N, device=DEV) - ptr[gid]
    deg = (rowptr[1:] - rowptr[:-1]).to(torch.int64)
    row = torch.repeat_interleave(torch.arange(N, device=DEV), deg)
    A = torch.zeros(G, P, P, dtype=torch.bool, device=DEV)
    A[gid[row], local[row], local[col.to(torch.int64)]] = True
    A = A | A.transpose(1, 2)
    lab = torch.zeros(G, P, dtype=torch.int64, device=DEV)
    lab[gid, local] = deg if labels is None else labels
    idx = torch.arange(P, device=DEV)
    upper = (idx[None, :, None] < idx[None, None, :]) & (idx[None, None, :] < sizes[:, None, None])
    return A, lab, upper


def torch_features(A, lab, upper, max_dist: int):
    """(graph int64 [K], key int64 [K], count int64 [K]) sorted by (graph, key): the definition in torch."""
    Af = A.to(torch.float32)

    def run():
        dist = A.to(torch.int16)
        reach = A | torch.eye(A.size(1), dtype=torch.bool, device=DEV)[None]
        for d in range(2, max_dist + 1):
            new = (torch.bmm(reach.to(torch.float32), Af) > 0) & ~reach
            if not bool(new.any()):                                               # (one read-back per level: how torch knows where to stop)
                break
            dist[new] = d
            reach |= new
        g, u, v = torch.nonzero(upper & (dist > 0), as_tuple=True)
        la, lb = lab[g, u], lab[g, v]
        key = (torch.minimum(la, lb) << 35) | (torch.maximum(la, lb) << 11) | dist[g, u, v].to(torch.int64)
        rows, counts = torch.unique(torch.stack([g, key], dim=1), dim=0, return_counts=True)
        return rows[:, 0], rows[:, 1], counts

    return run


def kernel_rows(feat):
    """The kernel's live (graph, key, count) entries in the torch route's order."""
    live = torch.arange(feat.keys.size(1), device=DEV)[None, :] < feat.nuniq[:, None]
    g = torch.nonzero(live, as_tuple=True)[0]
    return g, feat.keys[live], feat.counts[live].to(torch.int64)


def torch_gram(g, key, count, G: int):
    def run():
        uniq, inv = torch.unique(key, return_inverse=True)
        counts = torch.zeros(G, uniq.numel(), dtype=torch.float64, device=DEV)
        counts[g, inv] = count.to(torch.float64)
        return (counts @ counts.t()).to(torch.int64)

    return run


def bench_shape(name: str, graphs: int, mean_nodes: float, mean_edges: float, big: int, num_labels: int, a) -> dict:
    gen = torch.Generator().manual_seed(graphs)
    ptr, edge_index, N, labels = synthetic_batch(graphs, mean_nodes, mean_edges, big, num_labels, gen)
    rowptr, col = simple_graph(edge_index, N)
    mgn = int((ptr[1:] - ptr[:-1]).max())
    cap = max(1, min(ops.sp_max_unique(mgn), mgn * (mgn - 1) // 2))
    res = {"name": name, "graphs": graphs, "nodes": N, "nnz": int(col.numel()), "max_graph_nodes": mgn, "labels": num_labels or "degrees", "cap": cap}

    def k_features():
        return ops.sp_features(ptr, rowptr, col, labels, a.max_dist, a.dim, max_graph_nodes=mgn, cap=cap)

    k_features()
    above, _, feat = peak(k_features)
    res["features_kernel_peak_mb"] = round(above / 2 ** 20, 3)
    status = feat.status.cpu()
    res["status_bits"] = {"too_large": int((status & 1).ne(0).sum()), "key_overflow": int((status & 2).ne(0).sum()),
                          "label_range": int((status & 4).ne(0).sum()), "skipped_entries": int((status >> 8).sum())}
    res["max_distinct_keys"] = int(feat.nuniq.max())
    sizes = (ptr[1:] - ptr[:-1]).cpu()
    res["largest_graph"] = {"nodes": int(sizes.max()), "distinct_keys": int(feat.nuniq[int(sizes.argmax())]), "status": int(status[int(sizes.argmax())])}
    accepted = (feat.status & 7) == 0

    def k_gram():
        return ops.sp_gram(feat.keys, feat.counts, feat.nuniq, feat.keys, feat.counts, feat.nuniq)

    above, _, K = peak(k_gram)
    res["gram_kernel_peak_mb"] = round(above / 2 ** 20, 3)
    routes = {"features_kernel": k_features, "gram_kernel": k_gram}
    kg, kk, kc = kernel_rows(feat)

    out, err = attempt(lambda: dense_batch(ptr, rowptr, col, labels))
    if err is not None:
        res["features_torch_error"] = err
    else:
        t_features = torch_features(*out, a.max_dist)
        out, err = attempt(lambda: peak(t_features))
        if err is not None:
            res["features_torch_error"] = err
            torch.cuda.empty_cache()
        else:
            res["features_torch_peak_mb"] = round(out.above_bytes / 2 ** 20, 3)
            tg, tk, tc = out.out
            keep = accepted[tg]                                                   # (a graph the kernel refused has no rows to compare)
            res["features_equal"] = bool(torch.equal(tg[keep], kg) and torch.equal(tk[keep], kk) and torch.equal(tc[keep], kc))
            routes["features_torch"] = t_features
    t_gram = torch_gram(kg, kk, kc, graphs)
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
    ap.add_argument("--max-dist", type=int, default=ops.SP_MAX_DIST)
    ap.add_argument("--dim", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    require_gpu("bench_sp.py")
    res = {"what": "shortest-path features (sorted distinct (label, label, distance) keys with counts, histograms) of one batch and the Gram of "
                   "the batch with itself; kernel = gmp_sp_features / gmp_sp_gram, torch = dense adjacency + one bmm per level + torch.unique, "
                   "torch.unique + dense fp64 count-matrix product",
           "max_dist": a.max_dist, "dim": a.dim, "reps": a.reps, "warmup": a.warmup, "shapes": [bench_shape(*s, a) for s in GRAPH_SHAPES]}
    emit(res, a.out)
    bad = [s["name"] for s in res["shapes"] for k, v in s.items() if k.endswith("_equal") and not v]
    if bad:
        raise SystemExit(f"the kernel and the torch form disagree on {bad}")


if __name__ == "__main__":
    main()
