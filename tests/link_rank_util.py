"""What the GPU tests of the link rankers share (test_gpu_link_rankers.py, test_gpu_lp_heuristics.py, test_gpu_lp_walks.py): tensors on the
device, a filter CSR written out verbatim, the seeded 700-node graph with its queries, and the command-line run."""
import functools
import json
import sys

import numpy as np
import torch

from lp_heur_ref import simple_csr

DEV = "cuda"
N_BIG, HUB = 700, 0


def t(a, dtype):
    return torch.as_tensor(np.ascontiguousarray(a)).to(dtype).to(DEV).contiguous()


def filter_csr(rows, n):
    """The filter CSR (int32, on the device) with row s holding rows[s] verbatim: any order, duplicates, entries out of range."""
    rowptr, col = [0], []
    for s in range(n):
        col += list(rows.get(s, []))
        rowptr.append(len(col))
    return t(rowptr, torch.int32), t(np.asarray(col, dtype=np.int64), torch.int32)


def run_cli(tmp_path, monkeypatch, name, extra):
    """python -m gnn_pretraining_amd.finetune.finetune on the synthetic Cora_LP stand-in, in process, one epoch: (the log's records, the
    checkpoint's state dict)."""
    from gnn_pretraining_amd.finetune import finetune as FT
    monkeypatch.setattr(FT, "OUTPUT_DIR", tmp_path / name)
    log = tmp_path / f"{name}.jsonl"
    monkeypatch.setattr(sys, "argv", ["finetune", "--domain_name", "Cora_LP", "--finetune_strategy", "full_finetune", "--pretrained_scheme", "b1",
                                      "--seed", "5", "--epochs", "1", "--data-root", str(tmp_path / "data"), "--data-scale", "0.1",
                                      "--log", str(log)] + extra)
    FT.main()
    rec = [json.loads(line) for line in log.read_text().splitlines()]
    state = torch.load(next((tmp_path / name).glob("model_*.pt")), map_location="cpu", weights_only=True)["model_state_dict"]
    return rec, state


@functools.lru_cache(maxsize=None)
def big():
    """700 nodes: node 0 a hub of degree 300 (longer than a 256-thread stride), 690 .. 694 of degree 1, 695 .. 699 isolated, about 2,100
    random edges; 97 queries -- the hub and an isolated node as sources, an isolated destination, 48 destinations at distance two,
    duplicates -- and known edges to filter."""
    rng = np.random.RandomState(20240607)
    hub = [(HUB, int(v)) for v in rng.choice(np.arange(1, 690), 300, replace=False)]
    pend = [(690 + i, int(rng.randint(1, 690))) for i in range(5)]
    rnd = rng.randint(1, 690, size=(1800, 2)).tolist()
    edges = np.asarray(hub + pend + rnd, dtype=np.int64).T                       # one direction only, with the odd loop and duplicate
    rowptr, col = simple_csr(edges, N_BIG)
    deg = np.diff(rowptr)
    assert deg[HUB] == 300 and bool((deg[690:695] == 1).all()) and bool((deg[695:] == 0).all())
    src, dst = [], []
    for _ in range(10):
        src.append(HUB); dst.append(int(rng.randint(1, N_BIG)))
    for _ in range(3):
        src.append(695); dst.append(int(rng.randint(0, 690)))
    for _ in range(2):
        src.append(int(rng.randint(1, 690))); dst.append(697)
    while len(src) < 63:                                                         # 48 at distance two
        s = int(rng.randint(0, 690))
        if deg[s] == 0:
            continue
        z = int(rng.choice(col[rowptr[s]:rowptr[s + 1]]))
        d = int(rng.choice(col[rowptr[z]:rowptr[z + 1]]))
        if d != s:
            src.append(s); dst.append(d)
    while len(src) < 92:
        s, d = (int(v) for v in rng.randint(0, N_BIG, size=2))
        if s != d:
            src.append(s); dst.append(d)
    src += src[:5]; dst += dst[:5]                                               # duplicates
    assert len(src) == 97
    half = edges[:, rng.rand(edges.shape[1]) < 0.5]
    known = np.concatenate([half, half[::-1], rng.randint(0, N_BIG, size=(2, 300))], axis=1)
    return edges, rowptr, col, np.asarray(src), np.asarray(dst), known
