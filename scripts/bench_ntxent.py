"""NT-Xent forward + backward: the matrix form (gmp_nt_xent_fwd / _bwd, the [2n, 2n] similarity matrix in the workspace) against the
streaming form (gmp_nt_xent_stream_fwd / _bwd, similarity tiles in registers), d = 128, T = 0.2, in one process.

    python scripts/bench_ntxent.py [--reps 20] [--warmup 5] [--rounds 3] [--out profiles/ntxent_stream.json]

Both forms at n in {512, 2048, 8192}, the stream form alone at n in {16384, 32768} (the matrix form refuses n > 8192).  Every figure is
the time between two device events on one stream around `reps` forward + backward calls, after `warmup` calls of the same shape; the two
forms alternate over `rounds` rounds and the median round is reported with the spread (min, max).  The workspace is allocated once per
shape outside the timed window, as a training loop's caching allocator would hand it back.  For the stream form the rate is
6 R^2 d / time (R = 2n: the three GEMM-sized products) as a fraction of the 157.3 TFLOP/s fp32 MFMA peak; it is a whole-call rate, not a
kernel's.  Per-kernel times: run under `rocprofv3 --kernel-trace --stats -- python scripts/bench_ntxent.py --rounds 1`."""
from __future__ import annotations

import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchkit import DEV, alternate, emit, require_gpu  # noqa: E402
from gnn_pretraining_amd import _lib as L, ops  # noqa: E402

D, T = 128, 0.2
PEAK_F32_MFMA = 157.3e12
BOTH, STREAM_ONLY = (512, 2048, 8192), (16384, 32768)


def make_call(form: str, z1, z2, gs):
    """One forward + backward on preallocated buffers, straight on the C ABI."""
    lib = L.lib()
    n, d = z1.shape
    pre = "gmp_nt_xent_stream" if form == "stream" else "gmp_nt_xent"
    ws = torch.empty(getattr(lib, pre + "_workspace_bytes")(n, d), dtype=torch.uint8, device=DEV)
    loss = torch.empty(1, device=DEV)
    g1, g2 = torch.empty_like(z1), torch.empty_like(z2)
    fwd, bwd = getattr(lib, pre + "_fwd"), getattr(lib, pre + "_bwd")
    p = ops._ptr

    def call():
        st = ops._stream(z1)
        L.check(fwd(p(z1), p(z2), n, d, T, p(loss), p(ws), ws.numel(), st), pre + "_fwd")
        L.check(bwd(p(z1), p(z2), n, d, T, p(gs), p(g1), p(g2), p(ws), ws.numel(), st), pre + "_bwd")
    return call, (loss, g1, g2), ws.numel()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    require_gpu("bench_ntxent.py")
    gs = torch.full((1,), 0.25, device=DEV)
    rows = []
    for n in BOTH + STREAM_ONLY:
        gen = torch.Generator().manual_seed(n)
        z1, z2 = torch.randn(n, D, generator=gen).to(DEV), torch.randn(n, D, generator=gen).to(DEV)
        forms = ("matrix", "stream") if n in BOTH else ("stream",)
        reps = a.reps if n <= 8192 else max(a.reps // 4, 3)
        calls, outs, row = {}, {}, {"n": n, "d": D, "T": T, "reps": reps}
        for f in forms:
            calls[f], outs[f], row[f + "_workspace_bytes"] = make_call(f, z1, z2, gs)
            for _ in range(a.warmup):
                calls[f]()
        times = {f: [t.event_ms for t in ts] for f, ts in alternate(calls, reps, rounds=a.rounds).items()}
        for f in forms:
            row[f + "_ms"] = statistics.median(times[f])
            row[f + "_ms_min_max"] = [min(times[f]), max(times[f])]
        flops = 6.0 * (2 * n) ** 2 * D
        row["stream_tflops"] = flops / (row["stream_ms"] * 1e-3) / 1e12
        row["stream_fraction_of_f32_mfma_peak"] = flops / (row["stream_ms"] * 1e-3) / PEAK_F32_MFMA
        if "matrix" in forms:
            row["stream_over_matrix_time"] = row["stream_ms"] / row["matrix_ms"]
            (ml, m1, m2), (sl, s1, s2) = outs["matrix"], outs["stream"]
            row["stream_vs_matrix"] = {"loss_rel": abs(sl.item() - ml.item()) / abs(ml.item()),
                                       "g_z1_rel_to_max": ((s1 - m1).abs().max() / m1.abs().max()).item(),
                                       "g_z2_rel_to_max": ((s2 - m2).abs().max() / m2.abs().max()).item()}
        rows.append(row)
        emit(row, None)
        del calls, outs
        torch.cuda.empty_cache()
    res = {"bench": "nt_xent forward + backward, matrix form vs stream form", "device": torch.cuda.get_device_name(0),
           "warmup": a.warmup, "rounds": a.rounds, "peak_f32_mfma_flops": PEAK_F32_MFMA, "rows": rows}
    emit(res, a.out, indent=1)


if __name__ == "__main__":
    main()
