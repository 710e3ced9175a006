"""Link-prediction fine-tune step: the module path (finetune.py process_batch on autograd + torch.optim.AdamW) against the explicit-kernel
LinkPredictionEngine (finetune/engine.py), on a Cora_LP-shaped synthetic graph (2,708 x 1,433, the splits of data_setup, 256 positives per
batch + as many mined hard negatives), in one process.

    python scripts/bench_lp_finetune.py [--steps 50] [--warmup 10] [--scorer-reps 50] [--out profiles/lp_finetune.json]

Per path: wall ms per training step (mining pass + miner + step, synchronised at the end of the timed run) and the same span between device
events; for the engine also the fused scorer alone (gmp_lp_score_fwd + _bwd at K = 512) between device events.  Per-kernel times: run it
under `rocprofv3 --kernel-trace --stats -- python scripts/bench_lp_finetune.py --steps 20 --warmup 5`."""
from __future__ import annotations

import argparse
import itertools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from benchkit import DEV, emit, require_gpu, timed  # noqa: E402
from gnn_pretraining_amd import ops, synthetic as S  # noqa: E402
from gnn_pretraining_amd.data.data_setup import create_link_prediction_splits  # noqa: E402
from gnn_pretraining_amd.finetune import finetune as FT  # noqa: E402
from gnn_pretraining_amd.finetune.engine import LinkPredictionEngine  # noqa: E402
from gnn_pretraining_amd.models import FinetuneGNN  # noqa: E402

def counted(step):
    """step(i) as a call without arguments, i counting the calls from 0: every timed run walks the batches from the first one."""
    i = itertools.count()
    return lambda: step(next(i))


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--scorer-reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    require_gpu("bench_lp_finetune.py")
    gen = torch.Generator().manual_seed(0)
    torch.manual_seed(0)
    c = S.cora_like(gen)
    train_pos = create_link_prediction_splits(c)["train_pos"].contiguous()
    mp = train_pos.to(DEV)
    batches = [train_pos[:, s:s + 256].to(DEV).contiguous() for s in range(0, train_pos.size(1), 256)]
    cd = c.to(DEV)

    model = FinetuneGNN(DEV, "Cora_LP", "full_finetune")
    opt = torch.optim.AdamW(model.param_groups)
    miner = FT.LinkPredictionHardNegativeMiner()
    model.train()

    def module_step(i):
        loss, *_ = FT.process_batch(model, (cd, batches[i % len(batches)], None), DEV, "link_prediction", "Cora_LP", miner, mp)
        opt.zero_grad()
        loss.backward()
        opt.step()

    emodel = FinetuneGNN(DEV, "Cora_LP", "full_finetune")
    emodel.train()
    eng = LinkPredictionEngine(emodel, c.x, train_pos, DEV, seed=0)
    eminer = FT.LinkPredictionHardNegativeMiner()

    def engine_step(i):
        pos = batches[i % len(batches)]
        emb = eng.mining_forward()
        neg = eminer.mine_hard_negatives_for_edges(emb, pos, pos.size(1), mp)
        eng.step(pos, neg)

    mod_wall, mod_gpu = timed(counted(module_step), a.steps, a.warmup)
    eng_wall, eng_gpu = timed(counted(engine_step), a.steps, a.warmup)
    mod_wall2, mod_gpu2 = timed(counted(module_step), a.steps, 0)  # second module run: the order of the two legs does not decide the result

    # the fused scorer alone at the step's K = 512
    h = torch.randn(c.num_nodes, 256, device=DEV)
    src, dst = (torch.randint(0, c.num_nodes, (512,), device=DEV) for _ in range(2))
    hd = "classification_head.predictor.mlp."
    p = dict(emodel.named_parameters())
    w0, b0, w3, b3 = p[hd + "0.weight"].detach(), p[hd + "0.bias"].detach(), p[hd + "3.weight"].detach(), p[hd + "3.bias"].detach()
    act, logit = ops.lp_score_fwd(h, src, dst, w0, b0, w3, b3, 0.2, 1, 40)
    g = torch.randn(512, device=DEV) / 512
    fwd_wall, fwd_gpu = timed(lambda: ops.lp_score_fwd(h, src, dst, w0, b0, w3, b3, 0.2, 1, 40), a.scorer_reps, 3)
    bwd_wall, bwd_gpu = timed(lambda: ops.lp_score_bwd(h, src, dst, w0, w3, act, g, 0.2, 1, 40), a.scorer_reps, 3)

    res = {"shape": "Cora_LP synthetic: 2708 x 1433, 256 positives + 256 mined negatives per step",
           "module_ms_per_step": round(min(mod_wall, mod_wall2), 3), "module_event_ms_per_step": round(min(mod_gpu, mod_gpu2), 3),
           "engine_ms_per_step": round(eng_wall, 3), "engine_event_ms_per_step": round(eng_gpu, 3),
           "speedup": round(min(mod_wall, mod_wall2) / eng_wall, 2),
           "scorer_fwd_event_ms_K512": round(fwd_gpu, 4), "scorer_bwd_event_ms_K512": round(bwd_gpu, 4),
           "engine_loss_finite": bool(torch.isfinite(torch.tensor(eng.loss())).item()),
           "steps": a.steps, "warmup": a.warmup}
    emit(res, a.out)


if __name__ == "__main__":
    main()
