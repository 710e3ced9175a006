"""Host side of the device graph-property targets: the declaration / binding / export of the new C-ABI entry points, the formulas of
properties_from_counts (guards included) against the existing GraphPropertyCalculator on counts made by graph_props_ref.ref_counts
(pure Python integers), and compute_for_dataset(device=None) against the per-graph loop it always was.  No GPU."""
import sys

import numpy as np
import pytest
import torch

import graph_props_ref as R
from graph_props_ref import as_data, within_float_bar
from gnn_pretraining_amd import _lib as L
from gnn_pretraining_amd.data import data_setup as DS
from gnn_pretraining_amd.data.graph_properties import GRAPH_PROPERTY_DIM, GraphPropertyCalculator, properties_from_counts



def from_ref(n, pairs):
    slots, csum = R.ref_counts(n, R.both_directions(pairs))
    return properties_from_counts(torch.tensor([slots], dtype=torch.int64), torch.tensor([float(csum)], dtype=torch.float64))[0]


FORMULA_GRAPHS = {
    "regular": R.cubic(12),
    "regular_plus_isolated": R.cubic(12, 5),                # deg variance != 0 but every edge joins equal degrees: vx = 0
    "star": R.star(9),
    "path": R.path(11),
    "complete": R.complete(7),
    "two_components_path_first": R.two_components(True),
    "two_components_star_first": R.two_components(False),
    "n1": R.empty(1),
    "n2": R.path(2),
    "n2_no_edge": R.empty(2),
    "n3_path": R.path(3),
    "n3_triangle": R.complete(3),
    "no_edges": R.empty(6),
    "random_sparse": R.gnp(40, 0.08, 1),
    "random_dense": R.gnp(30, 0.4, 2),
}


def test_graph_props_symbols_are_declared_bound_and_exported():
    header = open(L.HEADER_PATH).read()
    doc = header.split("size_t gmp_graph_props_workspace_bytes")[0].rsplit("/* ----", 1)[1]
    for word in ("max degree", "T2", "Pr", "Sxy", "Sxx", "connected components", "diameter", "status", "reserved", "clustering_sum"):
        assert word in doc, f"the slot table in gnnmp.h does not mention {word!r}"


def test_graph_props_refuses_bad_sizes_before_touching_a_pointer():
    """Null pointers throughout: a size error must come back before anything is dereferenced or launched (no GPU here)."""
    lib = L.lib()
    assert lib.gmp_graph_props_workspace_bytes(37, 1024) == 0
    for nodes, edges, graphs, biggest in ((-1, 0, 1, 1), (0, -1, 1, 1), (0, 0, -1, 1), (0, 0, 1, -1)):
        assert lib.gmp_graph_props(None, None, None, nodes, edges, graphs, biggest, None, None, None, 0, None) == -1
    assert lib.gmp_graph_props(None, None, None, 10, 10, 3, 5, None, None, None, 0, None) == -1          # null pointers
    assert lib.gmp_graph_props(None, None, None, 0, 0, 0, 0, None, None, None, 0, None) == 0             # no graphs: nothing to do


@pytest.mark.parametrize("name", sorted(FORMULA_GRAPHS))
def test_properties_from_counts_equal_the_calculator(name):
    """The CPU-only pin of the formulas.  Measured worst |difference| over these graphs and the end-to-end graphs of the GPU test, both
    float32: 0.0 (graph_props_ref.MEASURED_WORST), so the bar is its floor, one float32 ulp of the calculator's value."""
    n, pairs = FORMULA_GRAPHS[name]
    want = GraphPropertyCalculator()(as_data(n, pairs))
    got = from_ref(n, pairs)
    assert got.dtype == torch.float32 and got.shape == (GRAPH_PROPERTY_DIM,)
    print(name, "max |diff| =", float((got.double() - want.double()).abs().max()))
    assert within_float_bar(got, want), (name, got, want)
    # the integer-valued targets are exact whatever the bar
    for k in (0, 1, 5, 8, 9):
        assert got[k] == want[k], (name, k)
    if name in ("regular", "regular_plus_isolated", "n1", "n2", "n2_no_edge", "no_edges", "complete", "n3_triangle"):
        assert got[10] == 0.0                                # the assortativity guards: zero variance of deg, or of deg over the edges
    if name == "two_components_path_first":
        assert got[9] == 3.0
    if name == "two_components_star_first":
        assert got[9] == 2.0


def test_ref_counts_treats_a_messy_list_like_the_clean_one():
    n, pairs = R.gnp(50, 0.1, 5)
    clean = R.ref_counts(n, pairs)
    assert R.ref_counts(*R.messy(n, pairs, 9)) == clean
    slots, _ = R.ref_counts(n, pairs + [(3, n), (-1, 4)])
    assert slots[12] == 2 << 8 and slots[:12] == clean[0][:12]


def test_properties_from_counts_leaves_a_refused_graph_as_zeros():
    row = [0] * 16
    row[12] = 1
    ok, _ = R.ref_counts(*R.star(5))
    out = properties_from_counts(torch.tensor([row, ok], dtype=torch.int64), torch.zeros(2, dtype=torch.float64))
    assert torch.count_nonzero(out[0]) == 0 and out[1, 0] == 5.0 and out[1, 5] == 4.0


def test_compute_for_dataset_without_a_device_is_the_per_graph_loop():
    graphs = [as_data(*g) for g in FORMULA_GRAPHS.values()]
    calc = GraphPropertyCalculator()
    want = torch.stack([calc(g) for g in graphs])
    for got in (calc.compute_for_dataset(graphs), calc.compute_for_dataset(graphs, device=None)):
        assert got.dtype == torch.float32 and torch.equal(got, want)
    idx = np.arange(0, len(graphs), 2)
    assert torch.equal(calc.compute_and_standardize_for_dataset(graphs, idx), calc.compute_and_standardize_for_dataset(graphs, idx, device=None))


def test_device_properties_flag_defaults_to_off(monkeypatch, tmp_path):
    seen = {}
    monkeypatch.setattr(DS, "process_synthetic", lambda root, scale, device_properties: seen.update(dp=device_properties))
    monkeypatch.setattr(sys, "argv", ["data_setup", "--root", str(tmp_path)])
    DS.main()
    assert seen["dp"] is False
    monkeypatch.setattr(sys, "argv", ["data_setup", "--root", str(tmp_path), "--device-properties"])
    DS.main()
    assert seen["dp"] is True
