"""Device-side link-prediction negatives (csrc/augment.hip: gmp_aug_negative_edges / _batch, ops.batched_negative_sampling) against
the numpy checker negatives_ref and the host sampler pretrain.tasks.sample_negative_edges.  Where the sampler makes no random draw the
device must equal it bit for bit; where it samples, the device's own Philox draw is held to the structure (exactly min(M, num_neg)
distinct non-edges of the right graph, ascending) and to the distribution (a uniform subset)."""
import ctypes as C
import math
import random

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import negatives_ref as R                                                  # noqa: E402
from gnn_pretraining_amd import _lib as L, ops                             # noqa: E402
from gnn_pretraining_amd.graph import Batch, Data                          # noqa: E402
from gnn_pretraining_amd.pretrain.tasks import negative_sampling_local, sample_negative_edges   # noqa: E402

DEV = torch.device("cuda:0")
NUM_NEGS = (1, 7, 240, 2000)


def on_dev(b: Batch):
    return (b.edge_index.to(DEV).contiguous(), torch.tensor(b.ptr_host, dtype=torch.long, device=DEV),
            torch.tensor(b.edge_ptr_host, dtype=torch.long, device=DEV))


def draw(b: Batch, num_neg: int, seed: int = 7, stream: int = 3):
    neg, counts = ops.batched_negative_sampling(*on_dev(b), num_neg, seed, stream)
    return neg.cpu().numpy(), counts.cpu().numpy()


_STRUCT = {}


def structure_batch() -> Batch:
    if "b" not in _STRUCT:
        rng = np.random.default_rng(3)
        graphs = [R.pairs_graph(1, R.random_pairs(1, 0, rng), rng), R.pairs_graph(2, np.array([[0, 1]]), rng, messy=False),
                  R.pairs_graph(2, R.random_pairs(2, 0, rng), rng)]
        for n in (3, 5, 12, 28, 63, 64, 65, 100):
            for density in ("empty", "sparse", 0.6, "complete"):
                graphs.append(R.pairs_graph(n, R.density_pairs(n, density, rng), rng))
        _STRUCT["b"] = Batch.from_data_list(graphs)
    return _STRUCT["b"]


def check_structure(b: Batch, neg: np.ndarray, counts: np.ndarray, num_neg: int):
    """The rules every output obeys; returns the per-graph (reference, device codes)."""
    ref = R.batch_ref(b, num_neg)
    assert neg.dtype == np.int64 and neg.shape[0] == 2 and neg.shape[1] == int(counts.sum())
    got = R.split_per_graph(b, neg)                          # every pair inside one graph, graphs in batch order
    for g, ((cnt, M, nd, codes), mine) in enumerate(zip(ref, got)):
        assert counts[g] == len(mine) == min(M, num_neg), (g, counts[g], len(mine), M, num_neg)
        assert (np.diff(mine) > 0).all(), g                  # ascending codes: unique too
        assert np.isin(mine, codes).all(), g                 # non-edges only (no self pair, no edge in either direction)
    return ref, got


@pytest.mark.parametrize("num_neg", NUM_NEGS)
def test_structure_and_no_draw_graphs_equal_the_host(num_neg):
    b = structure_batch()
    n = np.diff(np.asarray(b.ptr_host))
    neg, counts = draw(b, num_neg)
    ref, got = check_structure(b, neg, counts, num_neg)
    ei = b.edge_index.numpy()
    seen = {True: 0, False: 0}
    for g, ((cnt, M, nd, codes), mine) in enumerate(zip(ref, got)):
        if n[g] < 2 or cnt >= n[g] * (n[g] - 1):
            assert counts[g] == 0
            continue
        seen[nd] += 1
        if nd:                                               # the host's own routine on this graph: no draw happens, so any rng will do
            loc = ei[:, b.edge_ptr_host[g]:b.edge_ptr_host[g + 1]] - b.ptr_host[g]
            und = np.unique(np.concatenate([loc[0] * n[g] + loc[1], loc[1] * n[g] + loc[0]]))
            want = negative_sampling_local(np.stack([und // n[g], und % n[g]]), int(n[g]), num_neg, None)
            assert np.array_equal(mine, want[0] * n[g] + want[1]), g
    # (num_neg = 1: 1.1 / prob never reaches a population of 2 or more, every graph samples; from 7 on both kinds are present)
    assert seen[False] > 0 and (num_neg == 1 or seen[True] > 0), seen


def test_no_draw_equals_sample_negative_edges_on_both_sides_of_the_threshold():
    """Batches whose edge-column count (the num_neg sample_negative_edges takes) is set by a filler graph, holding graphs found by CPU search
    right at pop == int(1.1 * num_neg / prob), one step to either side of it, and in the no-draw band with num_neg < M."""
    triples = R.threshold_triples()
    assert sum(nd for *_, nd in triples) >= 6 and sum(not nd for *_, nd in triples) >= 3
    assert any(nd and num_neg < n * n - n - cnt for n, cnt, num_neg, nd in triples)
    rng = np.random.default_rng(17)
    exact = 0
    for n, cnt, num_neg, nd in triples:
        g = R.pairs_graph(n, R.random_pairs(n, cnt // 2, rng), rng, messy=False)
        b = Batch.from_data_list([g] + ([R.filler(num_neg - g.num_edges)] if num_neg > g.num_edges else []))
        assert b.num_edges == num_neg
        host = R.split_per_graph(b, sample_negative_edges(b, random.Random(1)).numpy())
        neg, counts = draw(b, num_neg)
        ref, got = check_structure(b, neg, counts, num_neg)
        assert ref[0][0] == cnt and ref[0][2] == nd, (n, cnt, num_neg)
        if nd:
            assert np.array_equal(got[0], host[0]), (n, cnt, num_neg)
            exact += 1
    assert exact >= 6


def test_same_seed_same_bytes_other_seed_or_stream_other_sample():
    b = structure_batch()
    base = draw(b, 7, seed=11, stream=5)
    again = draw(b, 7, seed=11, stream=5)
    assert base[0].tobytes() == again[0].tobytes() and base[1].tobytes() == again[1].tobytes()
    sampled = np.array([not nd for (_, _, nd, _) in R.batch_ref(b, 7)])
    assert sampled.any()
    for other in (draw(b, 7, seed=12, stream=5), draw(b, 7, seed=11, stream=6)):
        assert np.array_equal(other[1], base[1])
        a, o = R.split_per_graph(b, base[0]), R.split_per_graph(b, other[0])
        differs = np.array([not np.array_equal(x, y) for x, y in zip(a, o)])
        assert (differs & sampled).any() and not (differs & ~sampled).any()


def test_batched_launch_equals_the_per_job_calls():
    """gmp_aug_negative_edges_batch: more jobs than one launch carries (8), a job without graphs, different num_neg per job."""
    rng = np.random.default_rng(23)
    bs = [structure_batch()]
    for k in range(9):
        graphs = [R.pairs_graph(n, R.density_pairs(n, d, rng), rng) for n, d in zip(rng.integers(1, 40, size=6), (0.0, 0.2, 0.5, 0.8, 1.0, 0.3))]
        bs.append(Batch.from_data_list(graphs))
    bs.insert(4, Batch.empty(4))
    devs = [on_dev(b) for b in bs]
    jobs = [(d[0], d[1], d[2], (3, 40, 900)[i % 3], 2 * i + 1) for i, d in enumerate(devs)]
    got = ops.batched_negative_sampling_batch(jobs, 515)
    for i, (b, d) in enumerate(zip(bs, devs)):
        neg, counts = ops.batched_negative_sampling(d[0], d[1], d[2], (3, 40, 900)[i % 3], 515, 2 * i + 1)
        assert torch.equal(got[i][0], neg) and torch.equal(got[i][1], counts), i
    assert sum(int(g[0].size(1)) for g in got) > 1000


def test_sampled_graphs_draw_a_uniform_subset():
    """2,000 copies of one 12-node graph with cnt = 40 (M = 92), num_neg = 10, one launch: every copy samples.  A non-edge is chosen with
    p = 10 / 92 per copy, independently across copies (each ordered pair of the batch has a key of its own), so its count over the
    copies is Binomial(2000, p): it must lie within 5 standard deviations, 2000 p +- 5 sqrt(2000 p (1 - p)) (a derived bound: for 92
    counts the chance of one honest miss is below 1e-4)."""
    rng = np.random.default_rng(29)
    g = R.pairs_graph(12, R.random_pairs(12, 20, rng), rng)
    copies = 2000
    b = Batch.from_data_list([g] * copies)
    cnt, M, nd, codes = R.graph_ref(g.edge_index.numpy(), 12, 10)
    assert (cnt, M, nd) == (40, 92, False)
    neg, counts = draw(b, 10, seed=77, stream=9)
    assert (counts == 10).all()
    per = np.stack(R.split_per_graph(b, neg))                                      # [2000, 10] codes
    assert (np.diff(per, axis=1) > 0).all() and np.isin(per, codes).all()
    hits = np.bincount(per.reshape(-1), minlength=144)[codes]
    p = 10 / 92
    lo, hi = copies * p - 5 * math.sqrt(copies * p * (1 - p)), copies * p + 5 * math.sqrt(copies * p * (1 - p))
    print("hits per non-edge: min %d max %d (bounds %.1f .. %.1f)" % (hits.min(), hits.max(), lo, hi))
    assert (hits >= lo).all() and (hits <= hi).all(), (hits.min(), hits.max(), lo, hi)
    assert len({row.tobytes() for row in per}) > copies // 2                       # the copies do not all pick the same set


def _ring(n: int) -> Data:
    i = torch.arange(n)
    return Data(torch.zeros(n, 4), torch.stack([i, (i + 1) % n]), torch.zeros(1, dtype=torch.long), torch.zeros(12))


def test_limits_1024_nodes_accepted_1025_refused_no_graphs_no_op():
    rng = np.random.default_rng(31)
    b = Batch.from_data_list([R.pairs_graph(5, R.random_pairs(5, 3, rng), rng), _ring(1024), R.pairs_graph(9, R.random_pairs(9, 30, rng), rng)])
    for num_neg in (50, 1200000):                            # sampled among a million pairs | no draw: every non-edge of the ring
        neg, counts = draw(b, num_neg)
        ref, _ = check_structure(b, neg, counts, num_neg)
        assert ref[1][2] == (num_neg == 1200000) and counts[1] == min(num_neg, 1024 * 1023 - 2048)
    # one node more: a return code with a message, nothing is launched
    big = Batch.from_data_list([_ring(1025)])
    ei, ptr, eptr = on_dev(big)
    out, counts, total = torch.zeros(2, 8, dtype=torch.long, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    ws = torch.zeros(1 << 20, dtype=torch.uint8, device=DEV)
    lib = L.lib()
    rc = lib.gmp_aug_negative_edges(ptr.data_ptr(), eptr.data_ptr(), ei.data_ptr(), 1025, 1025, 1, 1025, 4, 1, 0, out.data_ptr(), 8, counts.data_ptr(),
                                    total.data_ptr(), ws.data_ptr(), ws.numel(), None)
    assert rc == -1 and b"1025 nodes (limit 1024)" in lib.gmp_last_error_string()          # GMP_ERR_ARG
    job = L.AugNegJob(ptr.data_ptr(), eptr.data_ptr(), ei.data_ptr(), 1025, 1025, 1, 0, 4, out.data_ptr(), 8, counts.data_ptr(), total.data_ptr(),
                      ws.data_ptr(), ws.numel())
    assert lib.gmp_aug_negative_edges_batch((L.AugNegJob * 1)(job), 1, 1025, 1, None) == -1
    with pytest.raises(L.GnnmpError, match="limit 1024"):
        ops.batched_negative_sampling(ei, ptr, eptr, 4, 1)
    torch.cuda.synchronize()
    assert int(out.abs().sum()) == 0
    # no graphs: a no-op, also with null pointers
    assert lib.gmp_aug_negative_edges(None, None, None, 0, 0, 0, 0, 4, 1, 0, None, 0, None, None, None, 0, None) == 0
    assert lib.gmp_aug_negative_edges_batch(None, 0, 0, 1, None) == 0
    e = Batch.empty(4)
    neg, counts = ops.batched_negative_sampling(e.edge_index.to(DEV), torch.zeros(1, dtype=torch.long, device=DEV), torch.zeros(1, dtype=torch.long, device=DEV), 5, 1)
    assert tuple(neg.shape) == (2, 0) and counts.numel() == 0
