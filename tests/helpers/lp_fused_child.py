"""Child of tests/test_gpu_lp_fused.py: three seeded s4 StepEngine steps on the synthetic batches of tests/test_gpu_engine.py, with the
link-prediction head as GMP_LP_FUSED (set by the parent) says.  argv[1]: "step" (the 8-graph batches of tests/test_gpu_engine.py) or "tiny" (two 14-node
graphs per domain: fewer than 1,024 merged pairs, the step's two-launch fallback), argv[2]: output file (torch.save of the flat parameters,
task_grads, the loss sums, the number of merged link-prediction pairs K of every step and how many fused launches the process made)."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]

from gnn_pretraining_amd import synthetic as S                                    # noqa: E402
from gnn_pretraining_amd.engine import StepEngine, StepInputs                      # noqa: E402
from gnn_pretraining_amd.models import PretrainableGNN                             # noqa: E402
from gnn_pretraining_amd.pretrain import pretrain as PT                            # noqa: E402

mode, out = sys.argv[1], sys.argv[2]
dev = torch.device("cuda:0")
tasks, domains = PT.ACTIVE_TASKS["s4"], PT.PRETRAIN_DOMAINS["s4"]
torch.manual_seed(41)
gen = torch.Generator().manual_seed(41)
hm = PretrainableGNN(torch.device("cpu"), domains, tasks)
hm.device = dev
hm.to(dev)
hm.train()
eng = StepEngine(hm, tasks, domains, dev, seed=41)
assert eng.native, "the step executor (csrc/step.hip) is what reads GMP_LP_FUSED"
if mode == "tiny":
    host = {d: S.domain_batch(gen, S.DOMAIN_SHAPES[d][0], 2, 14.0, 20.0) for d in domains}
else:
    host = S.pretrain_step_batches(gen, domains)
inp = StepInputs(host, dev, eng.dpad)
Ks = []
for _ in range(3):
    eng.step(inp, gen, order=list(tasks))          # a fixed PCGrad order: the default draws one per step from an unseeded stream
    Ks.append(int(eng.last_plan.lp_K))
torch.cuda.synchronize()
torch.save({"flat": eng.flat.cpu(), "task_grads": eng.task_grads.cpu(), "loss_sums": eng.loss_sums.cpu(),
            "losses": eng.losses(), "K": Ks, "fused_launches": int(eng.lib.gmp_lp_feat_gemm_launch_count())}, out)
