"""Host side of the device-drawn link-prediction negatives: the numpy checker (negatives_ref) against the host sampler
pretrain.tasks.sample_negative_edges -- exact where the sampler makes no draw, subset / size / no duplicates where it samples --, the
declaration and export of the new C-ABI entry points, and the opt-in switches (engine argument, pretrain command line).  No GPU."""
import ctypes
import random

import numpy as np
import pytest

import negatives_ref as R
from gnn_pretraining_amd import _lib as L
from gnn_pretraining_amd.graph import Batch
from gnn_pretraining_amd.pretrain.tasks import sample_negative_edges



def test_checker_agrees_with_the_host_sampler():
    rng = np.random.default_rng(5)
    no_draw = sampled = 0
    for k in range(300):
        graphs = []
        for _ in range(int(rng.integers(1, 6))):
            n = int(rng.integers(1, 14))
            graphs.append(R.pairs_graph(n, R.density_pairs(n, rng.choice([0.0, 0.1, 0.3, 0.6, 0.9, 1.0]), rng), rng))
        if k % 3 == 0:
            graphs.append(R.filler(int(rng.integers(1, 200))))           # a wide range of num_neg (= the batch's edge columns)
        b = Batch.from_data_list(graphs)
        num_neg = b.num_edges
        host = R.split_per_graph(b, sample_negative_edges(b, random.Random(k)).numpy())
        for (cnt, M, nd, codes), got in zip(R.batch_ref(b, num_neg), host):
            if nd:
                assert np.array_equal(got, codes[:min(M, num_neg)])
                no_draw += 1
            else:
                assert len(got) <= num_neg and len(np.unique(got)) == len(got) and np.isin(got, codes).all()
                sampled += 1
    assert no_draw > 300 and sampled > 100, (no_draw, sampled)


def test_threshold_search_finds_both_sides():
    tr = R.threshold_triples()
    assert any(nd for *_, nd in tr) and any(not nd for *_, nd in tr)
    assert any(nd and num_neg < n * n - n - cnt for n, cnt, num_neg, nd in tr)
    for n, cnt, num_neg, nd in tr:
        assert (n * n - n <= int(1.1 * num_neg / (1.0 - cnt / (n * n - n)))) == nd


def test_new_entry_points_are_declared_bound_and_exported():
    assert ctypes.sizeof(L.AugNegJob) == 13 * 8
    wsb = L.lib().gmp_aug_negative_edges_workspace_bytes
    assert wsb(100, 64, 50) >= 100 * 2 * 4 + 50 * 4 and wsb(-1, 64, 50) == 0


def test_device_negatives_needs_the_device_rng_mode():
    from gnn_pretraining_amd.engine import StepEngine
    for mode in ("reference", "vectorized"):
        with pytest.raises(ValueError, match="device_negatives"):
            StepEngine(None, [], [], "cpu", rng_mode=mode, device_negatives=True)


def test_pretrain_parser_takes_the_flag_only_with_rng_device(capsys):
    from gnn_pretraining_amd.pretrain import pretrain as PT
    a = PT.parse_args(["--exp_name", "s4", "--seed", "1", "--rng", "device", "--device-negatives"])
    assert a.rng == "device" and a.device_negatives
    assert not PT.parse_args(["--exp_name", "s4", "--seed", "1", "--rng", "device"]).device_negatives
    for extra in ([], ["--rng", "vectorized"]):
        with pytest.raises(SystemExit):
            PT.parse_args(["--exp_name", "s4", "--seed", "1", "--device-negatives"] + extra)
    assert "--device-negatives needs --rng device" in capsys.readouterr().err
