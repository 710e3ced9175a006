"""What the GPU tests of the node baselines share (test_gpu_labelprop.py, test_gpu_sgc.py): tensors on the device, float bits, the sentinel
of the error-path tests, and the command-line run."""
import json
import sys

import numpy as np
import torch

from gnn_pretraining_amd.graph import SparseFeatures

DEV = "cuda"
SENTINEL = -7.0


def t(a, dtype=None):
    if a is None or isinstance(a, (torch.Tensor, SparseFeatures)):
        return a
    x = torch.as_tensor(np.ascontiguousarray(a))
    return (x if dtype is None else x.to(dtype)).to(DEV).contiguous()


def bits(x):
    return np.ascontiguousarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.float32).view(np.uint32)


def run_cli(root, monkeypatch, name, extra):
    """python -m gnn_pretraining_amd.finetune.finetune on the synthetic Cora_NC stand-in, in process, one epoch: (the log's records, the
    checkpoint's state dict)."""
    from gnn_pretraining_amd import operators as O
    from gnn_pretraining_amd.finetune import finetune as FT
    monkeypatch.setattr(FT, "OUTPUT_DIR", root / name)
    monkeypatch.setattr(O.DROPOUT, "count", 0)                                    # the module path's dropout counter is process-wide
    log = root / f"{name}.jsonl"
    monkeypatch.setattr(sys, "argv", ["finetune", "--domain_name", "Cora_NC", "--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1",
                                      "--seed", "5", "--epochs", "1", "--data-root", str(root / "data"), "--data-scale", "0.1",
                                      "--log", str(log)] + extra)
    FT.main()
    rec = [json.loads(line) for line in log.read_text().splitlines()]
    state = torch.load(next((root / name).glob("model_*.pt")), map_location="cpu", weights_only=True)["model_state_dict"]
    return rec, state
