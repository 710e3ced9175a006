"""scripts/benchkit.py without a device: it imports, it refuses to measure, its synthetic workloads are the streams the committed records
were measured on, and no bench script keeps a private copy of what it defines."""
import ast
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPTS = os.path.join(ROOT, "scripts")
if SCRIPTS not in sys.path:
    sys.path.insert(0, SCRIPTS)

import benchkit  # noqa: E402

IN_SCOPE = ("wl", "sp", "graph_feat", "label_propagation", "sgc", "lp_heuristics", "lp_walks", "link_probe", "lp_rank",
            "knn", "kmeans", "logreg", "repr_stats", "miner", "gc_finetune", "lp_finetune", "ntxent", "sparse_encoder",
            "cls_metrics", "device_negatives", "graph_properties")
TOOLKIT_NAMES = {"timed", "timeit", "time_ms", "peak_mb", "peak_bytes", "attempt", "make_graph", "keep_mask", "synthetic_batch"}
# name -> (N, raw edges, sum of edge_index, label sum or None): the parent's bench_wl.synthetic_batch on the CPU, gen seeded by the graph count;
# the three N are the `nodes` of profiles/wl.json, sp.json and graph_feat.json
BATCHES = {"ENZYMES": (19518, 37172, 725580369, None), "NCI1": (123377, 133158, 16429491550, 2220628),
           "PROTEINS": (43953, 81811, 3595735524, None)}


def test_imports_without_a_device_and_names_the_device():
    assert benchkit.DEV == torch.device("cuda")
    assert [s[0] for s in benchkit.GRAPH_SHAPES] == list(BATCHES)


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is present: nothing to refuse")
def test_require_gpu_refuses_without_a_device():
    with pytest.raises(SystemExit) as e:
        benchkit.require_gpu("x.py")
    assert str(e.value) == "x.py measures on the GPU: no device found"


@pytest.mark.parametrize("shape", benchkit.GRAPH_SHAPES, ids=lambda s: s[0])
def test_synthetic_batch_draws_the_streams_of_the_committed_records(shape):
    name, graphs = shape[0], shape[1]
    ptr, edge_index, N, labels = benchkit.synthetic_batch(*shape[1:], torch.Generator().manual_seed(graphs), device="cpu")
    want_n, want_e, want_sum, want_labels = BATCHES[name]
    assert (N, int(ptr[-1]), ptr.numel()) == (want_n, want_n, graphs + 1)
    assert tuple(edge_index.shape) == (2, want_e) and edge_index.is_contiguous() and int(edge_index.sum()) == want_sum
    assert (labels is None) == (want_labels is None)
    if labels is not None:
        assert labels.numel() == N and int(labels.sum()) == want_labels


def test_random_graph_is_the_star_of_the_propagation_records():
    # the parent's make_graph (bench_label_propagation and bench_sgc: the same function) for the `star` shape, gen seeded by N
    e = benchkit.random_graph(20000, 40000, 10000, torch.Generator().manual_seed(20000), device="cpu")
    assert tuple(e.shape) == (2, 50000) and e.is_contiguous() and e.dtype == torch.int64
    assert int(e.sum()) == 851017192 and int((e[0] * 3 + e[1]).sum()) == 1651861870
    assert int((e * torch.arange(1, 50001)).sum()) == 18355861330611                # position-weighted: the order of the columns too
    assert torch.equal(e[:, 40000:], torch.stack([torch.zeros(10000, dtype=torch.int64), torch.arange(1, 10001)]))
    plain = benchkit.random_graph(20000, 40000, 0, torch.Generator().manual_seed(20000), device="cpu")
    assert torch.equal(plain, e[:, :40000])


def test_keep_mask_drops_the_source_the_destination_and_the_filter_row():
    # 5 nodes; filter rows (CSR): 0 -> {1, 2}, 1 -> {}, 2 -> {4}, 3 -> {}, 4 -> {0}
    frp, fcl = torch.tensor([0, 2, 2, 3, 3, 4]), torch.tensor([1, 2, 4, 0])
    keep = benchkit.keep_mask(torch.tensor([0, 2, 3]), torch.tensor([3, 1, 4]), frp, fcl, 5)
    assert keep.tolist() == [[False, False, False, False, True], [True, False, False, True, False], [True, True, True, False, False]]


def test_no_bench_script_keeps_a_private_copy_or_imports_another():
    for name in IN_SCOPE:
        with open(os.path.join(SCRIPTS, f"bench_{name}.py")) as f:
            tree = ast.parse(f.read())
        private = {n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.ClassDef))}
        private |= {t.id for n in tree.body if isinstance(n, ast.Assign) for t in n.targets if isinstance(t, ast.Name)}
        assert not private & TOOLKIT_NAMES, (name, private & TOOLKIT_NAMES)
        for n in ast.walk(tree):
            modules = [al.name for al in n.names] if isinstance(n, ast.Import) else [n.module or ""] if isinstance(n, ast.ImportFrom) else []
            assert not [m for m in modules if m.startswith("bench_")], (name, modules)
