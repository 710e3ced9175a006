"""The modes of the step executor (csrc/step.hip) that are read once per process and that no other test reaches: one enqueue thread instead
of two (GMP_STEP_LANES=0), every weight-gradient GEMM of the backward on the aux stream (GMP_STEP_WG1=0), phase timing on (GMP_STEP_TIMING=1:
one thread, timing events on every stream).  Each walks the same launch sequence over the same buffers, so three seeded s4 steps leave the
same bits as the default.  And what the executor requires of its descriptor is refused before anything is enqueued."""
import ctypes as C
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from gnn_pretraining_amd import synthetic as S                                    # noqa: E402
from gnn_pretraining_amd.engine import StepEngine, StepInputs                      # noqa: E402
from gnn_pretraining_amd.models import PretrainableGNN                             # noqa: E402
from gnn_pretraining_amd.pretrain import pretrain as PT                            # noqa: E402

DEV = torch.device("cuda:0")
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "lp_fused_child.py")
SETTINGS = [("default", {}), ("one lane", {"GMP_STEP_LANES": "0"}), ("dW1 on aux", {"GMP_STEP_WG1": "0"}), ("phase timing", {"GMP_STEP_TIMING": "1"})]


def run_child(extra, path):
    env = {k: v for k, v in os.environ.items() if k not in ("GMP_STEP_LANES", "GMP_STEP_WG1", "GMP_STEP_TIMING")}
    env.update(extra)
    r = subprocess.run([sys.executable, CHILD, "step", path], env=env, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, f"{extra}: exit status {r.returncode}\n" + r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(path)


def test_lanes_second_weight_gradient_stream_and_timing_give_the_same_bits(tmp_path):
    """three seeded s4 steps on the 8-graph synthetic batches (tests/helpers/lp_fused_child.py), one child process per setting, one after
    the other: a child that faults, aborts or runs into its timeout fails the test there and no further child is started"""
    ref = None
    for i, (name, extra) in enumerate(SETTINGS):
        out = run_child(extra, str(tmp_path / f"{i}.pt"))
        if ref is None:
            ref = out
            assert ref["task_grads"].abs().sum().item() > 0 and len(ref["losses"]) == 5
            continue
        assert out["K"] == ref["K"]
        for k in ("flat", "task_grads", "loss_sums"):
            assert torch.equal(out[k], ref[k]), f"{name}: {k}: {(out[k] != ref[k]).sum().item()} elements differ from the default"


def test_a_missing_per_layer_buffer_is_refused_and_nothing_is_enqueued():
    """gu_l / gz1_l are required: with gu_l[0] = NULL the call returns GMP_ERR_ARG (-1) before it touches a stream -- no gradient, no loss
    sum and no gate flag is written (the buffers a step fills first are cleared beforehand, the epoch is a new one)"""
    tasks, domains = PT.ACTIVE_TASKS["s4"], PT.PRETRAIN_DOMAINS["s4"]
    torch.manual_seed(41)
    gen = torch.Generator().manual_seed(41)
    hm = PretrainableGNN(torch.device("cpu"), domains, tasks)
    hm.device = DEV
    hm.to(DEV)
    hm.train()
    eng = StepEngine(hm, tasks, domains, DEV, seed=41)
    assert eng.native
    inp = StepInputs(S.pretrain_step_batches(gen, domains), DEV, eng.dpad)
    eng.step(inp, gen, order=list(tasks))
    torch.cuda.synchronize()
    assert eng.task_grads.abs().sum().item() > 0 and eng.loss_sums.abs().sum().item() > 0
    d = eng._desc
    eng.task_grads.zero_()
    eng.loss_sums.zero_()
    eng.gA.fill_(1.0)                      # (the heads start from a cleared gA)
    flags = eng.sync_flags.clone()
    d.gu_l[0] = None
    eng._epoch += 1
    d.epoch = eng._epoch
    rc = eng.lib.gmp_pretrain_step_fwd_bwd(C.byref(d), torch.cuda.current_stream(DEV).cuda_stream, eng._stream_arr, eng.aux_stream.cuda_stream)
    msg = eng.lib.gmp_last_error_string().decode()
    torch.cuda.synchronize()
    assert rc == -1, (rc, msg)
    assert "gu_l" in msg, msg
    assert not eng.task_grads.any() and not eng.loss_sums.any() and bool((eng.gA == 1.0).all())
    assert torch.equal(eng.sync_flags, flags), "a gate flag was written"
