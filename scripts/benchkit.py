"""The measurement protocol of the bench_* scripts, defined once (tests/test_benchkit_host.py, tests/test_gpu_benchkit.py):

  require_gpu   a measurement path that finds no GPU fails, with one message
  timed         `reps` calls between a host clock and a device-event pair, per call, after `warmup` calls and a synchronise
  peak          torch's allocator peak over one call, absolute and above what was allocated before it
  attempt       a route that cannot run is recorded with its error instead of a time
  alternate     every route timed once per round, round after round: the order of the routes does not decide the result
  record_min    the minimum over the rounds, as <name>_ms / <name>_event_ms / <name>_ms_runs
  emit          one JSON line on stdout, and the record file

and the synthetic workloads that more than one script builds.  A bench script imports this module and carries only its routes.  Nothing
here touches a device at import time."""
from __future__ import annotations

import json
import os
import sys
import time
from typing import Any, Callable, Mapping, NamedTuple

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gnn_pretraining_amd import ops  # noqa: E402

DEV = torch.device("cuda")
# name, graphs, mean nodes, mean edges, one graph of this many nodes (0: none), discrete labels (0: start from degrees)
GRAPH_SHAPES = (("ENZYMES", 600, 32.6, 62.1, 0, 0), ("NCI1", 4110, 29.9, 32.3, 0, 37), ("PROTEINS", 1113, 39.1, 72.8, 620, 0))


class Timing(NamedTuple):
    host_ms: float                                                                # per call, host clock around work that ends in a synchronise
    event_ms: float                                                               # per call, between two device events on the current stream


class Peak(NamedTuple):
    above_bytes: int                                                              # the peak above what was allocated before the call
    total_bytes: int                                                              # torch.cuda.max_memory_allocated over the call
    out: Any                                                                      # what the call returned (alive as long as this tuple is)


def require_gpu(script: str) -> None:
    if not torch.cuda.is_available():
        raise SystemExit(f"{script} measures on the GPU: no device found")


def timed(fn: Callable[[], Any], reps: int, warmup: int = 0) -> Timing:
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return Timing(1e3 * (time.perf_counter() - t0) / reps, e0.elapsed_time(e1) / reps)


def peak(fn: Callable[[], Any]) -> Peak:
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    total = torch.cuda.max_memory_allocated()
    return Peak(total - base, total, out)


def attempt(fn: Callable[[], Any]):
    try:
        return fn(), None
    except Exception as e:                                                        # noqa: BLE001  (recorded, not hidden)
        torch.cuda.synchronize()
        return None, f"{type(e).__name__}: {str(e).splitlines()[0][:160]}"


def alternate(routes: Mapping[str, Callable[[], Any]], reps, rounds: int = 3, warmup: int = 0, route_warmup: int = 0) -> dict:
    """{name: [Timing per round]}.  reps: an int, or {name: int} where the routes differ; warmup: calls of every route before the first
    round; route_warmup: calls of a route before each of its timed runs."""
    for _ in range(warmup):
        for fn in routes.values():
            fn()
    times = {k: [] for k in routes}
    for _ in range(rounds):
        for k, fn in routes.items():
            times[k].append(timed(fn, reps[k] if isinstance(reps, Mapping) else reps, route_warmup))
    return times


def record_min(res: dict, times: Mapping[str, list], digits: int) -> None:
    for k, ts in times.items():
        res[f"{k}_ms"] = round(min(t.host_ms for t in ts), digits)
        res[f"{k}_event_ms"] = round(min(t.event_ms for t in ts), digits)
        res[f"{k}_ms_runs"] = [round(t.host_ms, digits) for t in ts]


def emit(res, out, indent=None) -> None:
    """Prints res as one JSON line; with `out`, writes the file too: the same line, or with `indent` the indented form."""
    line = json.dumps(res)
    print(line, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write((line if indent is None else json.dumps(res, indent=indent)) + "\n")


def synthetic_batch(graphs: int, mean_nodes: float, mean_edges: float, big: int, num_labels: int, gen: torch.Generator, device=DEV):
    """(ptr, edge_index, N, labels or None) of one batch of random graphs: Poisson sizes, uniform endpoints within a graph."""
    sizes = torch.poisson(torch.full((graphs,), mean_nodes - 2.0), generator=gen).to(torch.int64) + 2
    sizes = sizes.clamp(max=ops.WL_MAX_GRAPH_NODES)
    if big:
        sizes[graphs // 2] = big
    ptr = torch.zeros(graphs + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(sizes, 0)
    edges = torch.round(sizes.double() * (mean_edges / mean_nodes)).to(torch.int64)
    owner = torch.repeat_interleave(torch.arange(graphs), edges)
    u = (torch.rand(owner.numel(), generator=gen) * sizes[owner]).to(torch.int64) + ptr[owner]
    v = (torch.rand(owner.numel(), generator=gen) * sizes[owner]).to(torch.int64) + ptr[owner]
    N = int(ptr[-1])
    labels = torch.randint(0, num_labels, (N,), generator=gen) if num_labels else None
    return ptr.to(device), torch.stack([u, v]).to(device).contiguous(), N, None if labels is None else labels.to(device)


def random_graph(N: int, E: int, hub: int, gen: torch.Generator, device=DEV):
    """edge_index [2, E + hub]: E uniform random edges and, with `hub`, a star from node 0 to nodes 1 .. hub."""
    edges = torch.randint(0, N, (2, E), generator=gen)
    if hub:
        edges = torch.cat([edges, torch.stack([torch.zeros(hub, dtype=torch.int64), torch.arange(1, hub + 1)])], dim=1)
    return edges.to(device).contiguous()


def keep_mask(src, dst, frp, fcl, N):
    """bool [len(src), N]: the candidates of every query -- all nodes but the source, the destination and the source's filter row."""
    Q = src.numel()
    qs = torch.arange(Q, device=src.device)
    keep = torch.ones(Q, N, dtype=torch.bool, device=src.device)
    keep[qs, src] = False
    keep[qs, dst] = False
    fd = frp[src + 1] - frp[src]
    frow = torch.repeat_interleave(qs, fd)
    fwithin = torch.arange(frow.numel(), device=src.device) - (torch.cumsum(fd, 0) - fd)[frow]
    keep[frow, fcl[frp[src][frow] + fwithin]] = False
    return keep
