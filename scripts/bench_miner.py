"""Timing of the hard-negative miner.
Without --impl: the dense form (csrc/hardneg.hip) at Cora / CiteSeer size, beside (a) the reference's own sequence of torch ops run
on the same GPU (finetune.py:45-75 as written: dense mask, torch.where, torch.topk) and (b) the CPU oracle.
    python scripts/bench_miner.py [--n 2708] [--k 256]
With --impl {matrix,stream,both}: the dense form against the streaming form (csrc/hardneg_stream.hip) at 2,708 and 3,327 nodes (Cora,
CiteSeer), 19,717 and 65,535, d = 256, k = 256, in alternated rounds (round r times one form, then the other); per size both times
with their spread over the rounds, both workspace sizes, whether the two selections agree, and the number of histogram tile passes the
streaming form ran (its device counter, read back after the timed loops).  At 65,535 nodes the dense form needs a 16 GiB workspace:
only the streaming form runs there.
    python scripts/bench_miner.py --impl both --out profiles/miner_stream.json"""
import argparse
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from benchkit import alternate, emit, require_gpu, timed                          # noqa: E402
from gnn_pretraining_amd import ops                                               # noqa: E402


def torch_sequence(emb, edges, k):
    import torch.nn.functional as F
    n = emb.size(0)
    zn = F.normalize(emb, dim=1)
    sim = torch.mm(zn, zn.t())
    mask = torch.zeros(n, n, device=emb.device, dtype=torch.bool)
    mask[edges[0], edges[1]] = True
    mask[edges[1], edges[0]] = True
    mask.fill_diagonal_(True)
    pot = ~mask
    scores = sim[pot]
    idx = torch.where(pot)
    _, top = torch.topk(scores, k, largest=True)
    return torch.stack([idx[0][top], idx[1][top]])


SIZES = [(2708, 8446), (3327, 7283), (19717, 70918), (65535, 262140)]     # (nodes, directed training-edge entries: 80 % of the public counts; 4 n at 65,535)
DENSE_MAX_N = 20000                                                          # above: the dense form's 4 n^2-byte workspace is not asked for


def stream_passes(emb, edges, k):
    """One direct call with a workspace of our own; the entry point leaves its histogram-pass count in the first int32."""
    from gnn_pretraining_amd import _lib as L
    l = L.lib()
    n, d = emb.shape
    E = edges.size(1)
    ws = torch.empty(l.gmp_hard_negative_stream_workspace_bytes(n, d, E), dtype=torch.uint8, device=emb.device)
    out = torch.empty(2, k, dtype=torch.int64, device=emb.device)
    L.check(l.gmp_hard_negative_topk_stream(ops._ptr(emb), n, d, ops._ptr(edges), E, k, ops._ptr(out), None, None, ops._ptr(ws), ws.numel(),
                                            ops._stream(emb)), "gmp_hard_negative_topk_stream")
    torch.cuda.synchronize()
    return int(ws[:4].view(torch.int32).item())


def compare(a):
    from gnn_pretraining_amd import _lib as L
    l = L.lib()
    sizes = [(a.n, a.edges)] if a.n_given else SIZES
    rows = []
    for n, E in sizes:
        g = torch.Generator().manual_seed(0)
        emb = torch.randn(n, a.d, generator=g).cuda()
        edges = torch.randint(0, n, (2, E), generator=g).cuda()
        impls = [i for i in ("matrix", "stream") if a.impl in (i, "both") and (i == "stream" or n <= DENSE_MAX_N)]
        iters = a.iters if n < 10000 else max(a.iters // 5, 3)
        routes = {i: lambda i=i: ops.hard_negative_topk(emb, edges, a.k, impl=i) for i in impls}
        times = {i: [1e3 * t.event_ms for t in ts]                           # us; alternated: matrix, stream, matrix, stream, ...
                 for i, ts in alternate(routes, iters, rounds=a.rounds, route_warmup=3).items()}
        row = {"n": n, "d": a.d, "E": E, "k": a.k, "iters": iters, "rounds": a.rounds}
        for i in impls:
            t = sorted(times[i])
            row[f"{i}_us"] = round(t[len(t) // 2], 1)
            row[f"{i}_us_rounds"] = [round(x, 1) for x in times[i]]
        row["matrix_workspace_bytes"] = int(l.gmp_hard_negative_workspace_bytes(n, a.d))
        row["stream_workspace_bytes"] = int(l.gmp_hard_negative_stream_workspace_bytes(n, a.d, E))
        if "matrix" not in impls and a.impl != "stream":
            row["matrix_skipped"] = "the dense form's workspace at this size is not allocated"
        if "stream" in impls:
            row["stream_hist_passes"] = stream_passes(emb, edges, a.k)
            row["stream_tile_passes"] = row["stream_hist_passes"] + 1         # + the gather
        if len(impls) == 2:
            m, ms = ops.hard_negative_topk(emb, edges, a.k, return_scores=True, impl="matrix")
            s, ss = ops.hard_negative_topk(emb, edges, a.k, return_scores=True, impl="stream")
            row["same_pairs"] = bool(torch.equal(m, s))
            row["max_score_diff"] = float((ms - ss).abs().max())
            row["stream_over_matrix"] = round(row["stream_us"] / row["matrix_us"], 3)
        emit(row, None)
        rows.append(row)
    emit({"device": torch.cuda.get_device_name(0), "rows": rows}, a.out, indent=1)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--impl", choices=["matrix", "stream", "both"], default=None, help="compare the miner's two forms over the size ladder")
    p.add_argument("--out", type=str, default=None, help="with --impl: also write the rows to this JSON file")
    p.add_argument("--rounds", type=int, default=3, help="with --impl: alternated rounds per size")
    p.add_argument("--n", type=int, default=2708)
    p.add_argument("--d", type=int, default=256)
    p.add_argument("--edges", type=int, default=8446)        # 80 % of Cora's 10,556 directed entries
    p.add_argument("--k", type=int, default=256)
    p.add_argument("--iters", type=int, default=50)
    a = p.parse_args()
    require_gpu("bench_miner.py")
    a.n_given = any(x == "--n" or x.startswith("--n=") for x in sys.argv[1:])
    if a.impl is not None:
        return compare(a)
    g = torch.Generator().manual_seed(0)
    emb = torch.randn(a.n, a.d, generator=g).cuda()
    edges = torch.randint(0, a.n, (2, a.edges), generator=g).cuda()
    t_hip = 1e3 * timed(lambda: ops.hard_negative_topk(emb, edges, a.k), a.iters, warmup=3).event_ms                  # us
    t_torch = 1e3 * timed(lambda: torch_sequence(emb, edges, a.k), max(a.iters // 5, 3), warmup=3).event_ms
    from oracle import miner as OM
    t0 = time.time()
    OM.mine_hard_negatives_for_edges(emb.cpu(), edges[:, :a.k].cpu(), a.k, edges.cpu())
    t_cpu = (time.time() - t0) * 1e6
    # algorithmic traffic: write S once (n^2*4), read it 7 times (6 select passes + gather), read emb twice
    alg = a.n * a.n * 4 * 8 + 2 * a.n * a.d * 4
    emit({"n": a.n, "d": a.d, "k": a.k, "hip_us": round(t_hip, 1), "torch_gpu_us": round(t_torch, 1),
          "cpu_oracle_us": round(t_cpu, 1), "speedup_vs_torch_gpu": round(t_torch / t_hip, 2),
          "algorithmic_GBps": round(alg / t_hip / 1e3, 1), "gemm_TFLOPs_if_alone": round(2 * a.n * a.n * a.d / t_hip / 1e6, 2)}, None)


if __name__ == "__main__":
    main()
