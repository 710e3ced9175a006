"""What drawing the link-prediction negatives on the device (StepEngine(rng_mode="device", device_negatives=True); csrc/augment.hip
gmp_aug_negative_edges) costs and saves on bench.py's s4 workload (4 domains x 8 synthetic ENZYMES-shaped graphs per step):

    python scripts/bench_device_negatives.py [--steps 300] [--rounds 3] [--out profiles/device_negatives.json]

  host_negatives_ms_per_step    host clock around StepEngine._negatives over the four domain batches of a step, mean over the input pool:
                                native (csrc_host/hostdraw.cpp PyRandom) and python (pretrain/tasks.py sample_negative_edges)
  engine_ms_per_step            the engine's optimisation step through StepPrefetcher with rng_mode="device", the flag off and on: ONE engine
                                whose flag is flipped between rounds, the two arms interleaved (off, on, off, on, ...), --steps steps per
                                round after a warm-up, host clock around steps that end in a device synchronise
  kernel_us_per_ticket          device events around gmp_aug_negative_edges_batch (both launches, the four jobs of a step) alone on an idle
                                stream: what a ticket adds to the aux stream, not what it costs beside a running step
No speed bar: the mode is opt-in whichever way the numbers fall."""
from __future__ import annotations

import argparse
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    import bench as B                          # (first: it sets the process environment bench.py runs under)
    import torch
    from benchkit import emit, require_gpu
    require_gpu("bench_device_negatives.py")
    from gnn_pretraining_amd import _lib as L, ops
    from gnn_pretraining_amd._host import limit_host_threads
    from gnn_pretraining_amd.engine import StepEngine, StepPrefetcher, hostdraw
    from gnn_pretraining_amd.models import PretrainableGNN
    from gnn_pretraining_amd.pretrain import pretrain as PT
    from gnn_pretraining_amd.pretrain.control import TemperatureScheduler
    from gnn_pretraining_amd.pretrain.tasks import sample_negative_edges
    limit_host_threads(1)
    device = torch.device("cuda:0")
    torch.cuda.set_device(device)
    seed = 42
    torch.manual_seed(seed)
    tasks, domains = PT.ACTIVE_TASKS[B.SCHEME], PT.PRETRAIN_DOMAINS[B.SCHEME]
    model = PretrainableGNN(device, domains, tasks)
    model.train()
    engine = StepEngine(model, tasks, domains, device, seed=seed, shuffle_rng=random.Random(seed), rng_mode="device", device_negatives=True)
    pool = B.make_pool(seed, device, engine.dpad)
    gen = torch.Generator().manual_seed(seed)
    temperature = TemperatureScheduler(total_steps=462 * PT.EPOCHS)
    res = {"workload": f"bench.py {B.SCHEME}: {len(domains)} domains x 8 synthetic ENZYMES-shaped graphs per step, pool of {len(pool)} inputs",
           "steps_per_round": a.steps, "warmup_steps": a.warmup, "rounds": a.rounds}

    # ---- what a step's negatives are
    negs = [sum(int(engine._negatives(inp.host[d]).shape[1]) for d in domains) for inp in pool]
    res["negatives_per_step_mean"] = statistics.mean(negs)
    res["positive_edge_columns_per_step_mean"] = statistics.mean(sum(inp.host[d].num_edges for d in domains) for inp in pool)

    # ---- host time of the sampler
    def host_ms(fn, reps=20):
        fn()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        return (time.perf_counter() - t0) * 1e3 / reps / len(pool)

    rng = random.Random(1)
    res["host_negatives_ms_per_step"] = {
        "native": host_ms(lambda: [engine._negatives(inp.host[d]) for inp in pool for d in domains]) if hostdraw() is not None else None,
        "python": host_ms(lambda: [sample_negative_edges(inp.host[d], rng) for inp in pool for d in domains], reps=5)}

    # ---- engine, flag off / on, interleaved
    def round_ms(flag: bool) -> float:
        engine.device_negatives = flag
        it = iter(StepPrefetcher(engine, (pool[i % len(pool)] for i in range(a.warmup + a.steps)), gen))
        B.advance(engine, temperature, gen, it, a.warmup)
        torch.cuda.synchronize(device)
        t0 = time.perf_counter()
        B.advance(engine, temperature, gen, it, a.steps)
        torch.cuda.synchronize(device)
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        for _ in it:
            pass
        return ms

    round_ms(False); round_ms(True)                         # set-up: code objects, workspaces, clocks
    runs = {"off": [], "on": []}
    for _ in range(a.rounds):
        runs["off"].append(round_ms(False))
        runs["on"].append(round_ms(True))
    engine.check_gates()
    res["engine_ms_per_step"] = {k: {"median": statistics.median(v), "runs": [round(x, 4) for x in v]} for k, v in runs.items()}
    res["losses_finite"] = all(v == v and abs(v) != float("inf") for v in engine.losses().values())

    # ---- the kernels alone
    lib = L.lib()
    keep, per_input = [], []
    for inp in pool:
        jobs, nmax = [], 1
        for i, d in enumerate(domains):
            hb = inp.host[d]
            ptr, eptr, ei, *_ = inp.dev_graph(d)
            nmax = max(nmax, max(int(y - x) for x, y in zip(hb.ptr_host[:-1], hb.ptr_host[1:])))
            jobs.append((hb, ptr, eptr, ei, i))
        cj = []
        for hb, ptr, eptr, ei, i in jobs:
            cap = max(ops.negative_capacity(hb.ptr_host, hb.num_edges), 1)
            neg = torch.empty(2, cap, dtype=torch.int64, device=device)
            counts, total = torch.empty(hb.num_graphs, dtype=torch.int32, device=device), torch.empty(1, dtype=torch.int32, device=device)
            ws = torch.empty(lib.gmp_aug_negative_edges_workspace_bytes(hb.num_nodes, nmax, cap), dtype=torch.uint8, device=device)
            keep += [neg, counts, total, ws]
            cj.append(L.AugNegJob(ptr.data_ptr(), eptr.data_ptr(), ei.data_ptr(), hb.num_nodes, hb.num_edges, hb.num_graphs, 2 * i + 1, hb.num_edges,
                                  neg.data_ptr(), cap, counts.data_ptr(), total.data_ptr(), ws.data_ptr(), ws.numel()))
        per_input.append(((L.AugNegJob * len(cj))(*cj), len(cj), nmax))
    st = torch.cuda.current_stream(device).cuda_stream

    def tickets(n: int) -> None:
        for k in range(n):
            arr, cnt, nmax = per_input[k % len(per_input)]
            L.check(lib.gmp_aug_negative_edges_batch(arr, cnt, nmax, 1234 + k, st), "gmp_aug_negative_edges_batch")

    tickets(50)
    torch.cuda.synchronize(device)
    ev = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); tickets(400); e1.record()
        torch.cuda.synchronize(device)
        ev.append(e0.elapsed_time(e1) * 1e3 / 400)
    res["kernel_us_per_ticket"] = {"median": statistics.median(ev), "runs": [round(x, 2) for x in ev],
                                   "note": "back-to-back tickets on an idle stream, two launches each: includes launch gaps"}
    emit(res, a.out)


if __name__ == "__main__":
    main()
