"""GPU time of the s4 step with the host taken out of the picture: main spins for 90 ms while the host enqueues `reps` prepared steps behind it
(every other stream waits for main through the step's own gates), then the queued steps run at the GPU's pace.  For A/B runs of executor
switches (GMP_STEP_WG1, GMP_STEP_BWD2, ...) whose launch counts differ: bench.py's number includes whatever the launcher cannot hide."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import bench as B
from gnn_pretraining_amd import _lib as L
from gnn_pretraining_amd.engine import StepEngine
from gnn_pretraining_amd.models.pretrain_model import PretrainableGNN
from gnn_pretraining_amd.pretrain import pretrain as PT

dev = torch.device("cuda:0")
torch.set_num_threads(1)
model = PretrainableGNN(device=dev, domain_names=PT.PRETRAIN_DOMAINS["s4"], task_names=PT.ACTIVE_TASKS["s4"])
model.train()
eng = StepEngine(model, PT.ACTIVE_TASKS["s4"], PT.PRETRAIN_DOMAINS["s4"], dev, seed=0, rng_mode="vectorized")
pool = B.make_pool(0, dev, eng.dpad)
gen = torch.Generator().manual_seed(0)
for k in range(20):
    eng.step(pool[k % len(pool)], gen)
p, inp = eng.last_plan, pool[19 % len(pool)]
main_h = torch.cuda.current_stream(dev).cuda_stream
torch.cuda.synchronize()
main = torch.cuda.current_stream(dev)
reps = int(sys.argv[1]) if len(sys.argv) > 1 else 40
for trial in range(3):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    L.check(L.lib().gmp_spin_us(90000, main.cuda_stream), "spin")
    a.record()
    t0 = time.perf_counter()
    for _ in range(reps):
        eng._forward_backward_native(p, inp)
        eng._optimizer(p, None, True, main_h)
    t1 = time.perf_counter()
    b.record()
    torch.cuda.synchronize()
    print(f"{reps} queued steps: GPU {a.elapsed_time(b) / reps:.3f} ms/step (host enqueued them in {(t1 - t0) * 1e3:.1f} ms, {(t1 - t0) / reps * 1e3:.3f} each)")
