"""Sparse (CSR) input encoder against the dense one, on the Cora and CiteSeer shapes (MI355X).

    python scripts/bench_sparse_encoder.py [--reps 200] [--steps 100] [--out profiles/sparse_encoder.json]

1. the encoder alone: forward (dense: the NT GEMM on the K-padded x; sparse: W transposed + one wave per row) and weight gradient
   (dense: the grouped TN GEMM with the bias column sums; sparse: gmp_sparse_linear_wgrad + gmp_colsum), the launches the fine-tune
   engine makes, timed between device events, the two forms alternating in one process, median and spread over the rounds;
2. the Cora_NC / CiteSeer_NC engine step (finetune/engine.py, eager default), dense x against sparse x;
3. bytes and FLOPs counted from the shapes, so that each rate is named against the bound it is held to.
Per-kernel times: run the script under `rocprofv3 --kernel-trace --stats -- python scripts/bench_sparse_encoder.py --reps 20 --steps 20`."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchkit import alternate, emit, require_gpu  # noqa: E402
from gnn_pretraining_amd import _lib as L, synthetic as S  # noqa: E402
from gnn_pretraining_amd.finetune.engine import NodeClassificationEngine  # noqa: E402
from gnn_pretraining_amd.graph import SparseFeatures  # noqa: E402
from gnn_pretraining_amd.models import FinetuneGNN  # noqa: E402

H = 256
SHAPES = {"Cora_NC": dict(num_nodes=2708, undirected_edges=5278, dim=1433, density=0.0127, num_classes=7),
          "CiteSeer_NC": dict(num_nodes=3327, undirected_edges=4552, dim=3703, density=0.0085, num_classes=6)}
HBM_TBS, MFMA_F32_TFLOPS = 8.0, 157.0          # MI355X: HBM3E peak, dense fp32 MFMA peak


def encoder_legs(dense: NodeClassificationEngine, sparse: NodeClassificationEngine):
    """The engine's own encoder launches, forward and weight gradient, for both forms (same shapes, same gradient input)."""
    lib, N, K, dpad = dense.lib, dense.N, dense.d_in, dense.dpad
    st = torch.cuda.current_stream().cuda_stream
    g = torch.randn(N, H, device="cuda")

    def d_fwd():
        P = dense._P
        dense._gemm(st, 0, dense.x.data_ptr(), P("input_encoder.linear.weight"), P("input_encoder.linear.bias"), dense.z0.data_ptr(), N, H, dpad,
                    dpad, dpad, H, ws=dense.gemm_ws)

    def d_wgrad():
        dense._wgrad(st, g.data_ptr(), dense.x.data_ptr(), "input_encoder.linear.weight", "input_encoder.linear.bias", H, dpad, dpad)

    def s_fwd():
        xs, P = sparse.xs, sparse._P
        L.check(lib.gmp_sparse_linear_fwd(xs.rowptr.data_ptr(), xs.col.data_ptr(), xs.val.data_ptr(), N, K, P("input_encoder.linear.weight"), dpad,
                                          P("input_encoder.linear.bias"), sparse.z0.data_ptr(), H, H, sparse.sp_status.data_ptr(),
                                          sparse.sp_wt.data_ptr(), sparse.sp_wt.numel(), st), "sparse fwd")

    def s_wgrad():
        colptr, row, val_t = sparse.x_csc
        gb = sparse.grad.data_ptr()
        L.check(lib.gmp_sparse_linear_wgrad(colptr.data_ptr(), row.data_ptr(), val_t.data_ptr(), N, K, g.data_ptr(), H,
                                            gb + 4 * sparse._G("input_encoder.linear.weight"), dpad, sparse.sp_status.data_ptr(), st), "sparse wgrad")
        L.check(lib.gmp_colsum(g.data_ptr(), gb + 4 * sparse._G("input_encoder.linear.bias"), N, H, H, 0, sparse.colsum_ws.data_ptr(),
                               sparse.colsum_ws.numel(), st), "colsum")

    return {"dense_fwd": d_fwd, "sparse_fwd": s_fwd, "dense_wgrad": d_wgrad, "sparse_wgrad": s_wgrad}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200, help="launches per timed round")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=100, help="engine steps per timed round")
    ap.add_argument("--out", type=str, default=None)
    a = ap.parse_args()
    require_gpu("bench_sparse_encoder.py")
    dev = torch.device("cuda:0")
    report = {"device": torch.cuda.get_device_name(dev), "legs": {}}
    for domain, shp in SHAPES.items():
        gen = torch.Generator().manual_seed(0)
        c = S.cora_like(gen, **shp)
        sp = SparseFeatures.from_dense(c.x)
        idx = torch.randperm(c.num_nodes, generator=gen)[:140]
        y, idx_d = c.y[idx].to(dev), idx.to(dev)
        engines = {}
        for kind, x in (("dense", c.x), ("sparse", sp)):
            torch.manual_seed(0)
            m = FinetuneGNN(dev, domain, "full_finetune")
            m.train()
            engines[kind] = NodeClassificationEngine(m, x, c.edge_index, dev, seed=0)
        legs = encoder_legs(engines["dense"], engines["sparse"])
        for fn in legs.values():                              # warm-up: code objects, LDS attributes, caches
            for _ in range(10):
                fn()
        samples = {k: [1e3 * t.event_ms for t in ts]          # us per call; the forms alternate within each round
                   for k, ts in alternate(legs, a.reps, rounds=a.rounds).items()}
        # engine step, eager default, dense and sparse alternating
        for e in engines.values():
            for _ in range(10):
                e.step(idx_d, y)
        torch.cuda.synchronize()
        step_ms = {k: [] for k in engines}
        for _ in range(a.rounds):
            for k, e in engines.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    e.step(idx_d, y)
                torch.cuda.synchronize()
                step_ms[k].append((time.perf_counter() - t0) / a.steps * 1e3)
        losses = {k: round(e.loss(), 5) for k, e in engines.items()}
        N, K, dpad, nnz = c.num_nodes, shp["dim"], engines["dense"].dpad, sp.nnz
        # counted from the shapes: the dense GEMMs' algorithmic FLOPs (padding excluded) against the fp32 MFMA peak; the sparse kernels
        # move one 1 KB row of W^T (forward) / G (weight gradient) per non-zero, mostly from L2 -- counted against HBM as an upper bound
        fl_dense = 2.0 * N * K * H
        bytes_fwd = nnz * (H * 4 + 8) + 2 * K * H * 4 + N * H * 4            # gathers + transpose read/write + output
        bytes_wg = nnz * (H * 4 + 8) + dpad * H * 4 + N * H * 4              # gathers + dW + colsum read of G
        med = {k: statistics.median(v) for k, v in samples.items()}
        leg = {"N": N, "K": K, "nnz": nnz, "density": round(nnz / (N * K), 5)}
        for k, v in samples.items():
            leg[k + "_us"] = {"median": round(med[k], 2), "min": round(min(v), 2), "max": round(max(v), 2)}
        leg["dense_fwd_rate"] = {"TFLOP/s": round(fl_dense / med["dense_fwd"] / 1e6, 2), "of_mfma_peak": round(fl_dense / med["dense_fwd"] / 1e6 / MFMA_F32_TFLOPS, 3)}
        leg["dense_wgrad_rate"] = {"TFLOP/s": round(fl_dense / med["dense_wgrad"] / 1e6, 2), "of_mfma_peak": round(fl_dense / med["dense_wgrad"] / 1e6 / MFMA_F32_TFLOPS, 3)}
        leg["sparse_fwd_rate"] = {"useful_GFLOP/s": round(2.0 * nnz * H / med["sparse_fwd"] / 1e3, 1), "bytes": bytes_fwd,
                                  "TB/s": round(bytes_fwd / med["sparse_fwd"] / 1e6, 2), "of_hbm_peak": round(bytes_fwd / med["sparse_fwd"] / 1e6 / HBM_TBS, 3)}
        leg["sparse_wgrad_rate"] = {"useful_GFLOP/s": round(2.0 * nnz * H / med["sparse_wgrad"] / 1e3, 1), "bytes": bytes_wg,
                                    "TB/s": round(bytes_wg / med["sparse_wgrad"] / 1e6, 2), "of_hbm_peak": round(bytes_wg / med["sparse_wgrad"] / 1e6 / HBM_TBS, 3)}
        leg["encoder_total_us"] = {"dense": round(med["dense_fwd"] + med["dense_wgrad"], 2), "sparse": round(med["sparse_fwd"] + med["sparse_wgrad"], 2)}
        for k, v in step_ms.items():
            leg[f"step_ms_{k}"] = {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}
        leg["loss_after"] = losses
        report["legs"][domain] = leg
        emit({domain: leg}, None)
        del engines
        torch.cuda.empty_cache()
    emit(report, a.out, indent=1)


if __name__ == "__main__":
    main()
