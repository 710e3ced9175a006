"""StepEngine(rng_mode="device", device_negatives=True): the link-prediction negatives ride the draw ticket with the masks and views
(csrc/augment.hip gmp_aug_negative_edges_batch) instead of being sampled on the host, graph by graph.  The artefacts obey the sampler's
rules, the step they feed matches the oracle on the same artefacts, the draws are a function of (engine seed, draw sequence), the
prefetcher runs with them, and a domain batch with a graph over the kernel's limit falls back to the host for that domain alone."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import negatives_ref as R                                                           # noqa: E402
from gnn_pretraining_amd import synthetic as S                                    # noqa: E402
from gnn_pretraining_amd.engine import StepEngine, StepInputs, StepPrefetcher      # noqa: E402
from gnn_pretraining_amd.graph import Batch, Data                                  # noqa: E402
from gnn_pretraining_amd.models import PretrainableGNN                             # noqa: E402
from gnn_pretraining_amd.pretrain import pretrain as PT                            # noqa: E402
from oracle import models as OM, tasks as OTk                                      # noqa: E402
from oracle.harness import oracle_artefacts                                        # noqa: E402
from parity_util import copy_state, set_dropout, to_oracle                         # noqa: E402
from test_gpu_modules import perturb_bn                                            # noqa: E402

DEV = torch.device("cuda:0")


def build(scheme, seed, rng_mode="device", make_host=None, **engine_kw):
    tasks, domains = PT.ACTIVE_TASKS[scheme], PT.PRETRAIN_DOMAINS[scheme]
    torch.manual_seed(seed)
    gen = torch.Generator().manual_seed(seed)
    om = OM.PretrainableGNN(torch.device("cpu"), domains, tasks)
    perturb_bn(om, gen)
    for l in om.gnn_backbone.layers:
        l.gin_conv.eps.data.fill_(0.05)
    hm = PretrainableGNN(torch.device("cpu"), domains, tasks)
    copy_state(hm, om)
    hm.device = DEV
    hm.to(DEV)
    set_dropout(om, 0.0)
    om.train(); hm.train()
    eng = StepEngine(hm, tasks, domains, DEV, seed=seed, rng_mode=rng_mode, **engine_kw)
    eng.dropout_p = eng.da_dropout = 0.0
    host = make_host(gen, domains) if make_host is not None else S.pretrain_step_batches(gen, domains)
    inp = StepInputs(host, DEV, eng.dpad)
    return om, hm, eng, host, inp, gen, tasks, domains


def check_negatives(b: Batch, neg: np.ndarray):
    """The structure rules of tests/test_gpu_negatives.py for one domain batch, num_neg = its edge-column count."""
    num_neg = b.num_edges
    assert neg.dtype == np.int64 and neg.shape[0] == 2
    got = R.split_per_graph(b, neg)
    for g, ((cnt, M, nd, codes), mine) in enumerate(zip(R.batch_ref(b, num_neg), got)):
        assert len(mine) == min(M, num_neg), (g, len(mine), M, num_neg)
        assert (np.diff(mine) > 0).all() and np.isin(mine, codes).all(), g


def no_host_sampler(eng):
    def boom(b):
        raise AssertionError("the host sampler ran although the negatives ride the ticket")
    eng._negatives = boom


def test_negatives_ride_the_ticket_and_the_step_matches_the_oracle():
    om, hm, eng, host, inp, gen, tasks, domains = build("s4", 191, device_negatives=True)
    no_host_sampler(eng)
    art = eng.draw(inp, gen)
    for d, b in host.items():
        check_negatives(b, art["link_pred"][d])
        assert art["link_pred"][d].shape[1] > 0
    eng.temperature = 0.37
    eng.step(inp, gen, art=art, order=list(tasks), apply_update=False)
    got = eng.losses()
    otasks = OTk.instantiate_tasks(om, tasks, None, lambda: 0.37)
    o_art, o_b = oracle_artefacts(art, host), {d: to_oracle(b) for d, b in host.items()}
    for t in tasks:
        want = otasks[t].loss(o_b, o_art.get(t))[0].item()
        print(t, got[t], want, abs(got[t] - want) / abs(want))
        assert abs(got[t] - want) <= 1e-4 * abs(want), (t, got[t], want)


def _sampled_host(gen, domains):
    """Step batches in which some graphs are large and sparse enough for the sampler to draw (TUDataset-sized graphs never are)."""
    host = S.pretrain_step_batches(gen, domains)
    rng = np.random.default_rng(5)
    d = domains[0]
    F = int(host[d].x.size(1))
    big = R.pairs_graph(90, R.random_pairs(90, 60, rng), rng)
    big = Data(torch.randn(90, F, generator=gen), big.edge_index, torch.zeros(1, dtype=torch.long), torch.rand(12, generator=gen))
    host[d] = Batch.from_data_list(host[d].to_data_list()[:3] + [big])
    return host


def test_equal_seeds_draw_equal_negatives_and_the_rng_state_replays_them():
    _, _, e1, host, inp, gen, tasks, domains = build("s4", 77, make_host=_sampled_host, device_negatives=True)
    _, _, e2, _, _, _, _, _ = build("s4", 77, make_host=_sampled_host, device_negatives=True)
    d0 = domains[0]
    assert any(not nd for (_, _, nd, _) in R.batch_ref(host[d0], host[d0].num_edges)), "the test needs a graph that samples"
    inp2 = StepInputs(host, DEV, e2.dpad)
    first = []
    for k in range(3):
        a1, a2 = e1.draw(inp, gen), e2.draw(inp2, gen)
        for d in domains:
            check_negatives(host[d], a1["link_pred"][d])
            assert np.array_equal(a1["link_pred"][d], a2["link_pred"][d]), (k, d)
        first.append(a1["link_pred"][d0].copy())
    assert not np.array_equal(first[0], first[1]) and not np.array_equal(first[1], first[2])      # every ticket draws anew
    st = e1.rng_state()
    nxt = [e1.draw(inp, gen)["link_pred"][d0].copy() for _ in range(3)]
    e1.set_rng_state(st)
    again = [e1.draw(inp, gen)["link_pred"][d0].copy() for _ in range(3)]
    assert all(np.array_equal(a, b) for a, b in zip(nxt, again))
    assert not np.array_equal(nxt[0], first[2])


def test_prefetcher_run_stays_finite_with_clean_gates():
    om, hm, eng, host, inp, gen, tasks, domains = build("s4", 192, device_negatives=True)
    no_host_sampler(eng)
    pool = [StepInputs(S.pretrain_step_batches(gen, domains), DEV, eng.dpad) for _ in range(3)]
    steps = 0
    for inp_k, prepared in StepPrefetcher(eng, (pool[i % 3] for i in range(12)), gen):
        eng.step(inp_k, gen, prepared=prepared)
        steps += 1
    torch.cuda.synchronize()
    eng.check_gates()
    assert steps == 12 and all(np.isfinite(v) for v in eng.losses().values())


def test_a_graph_over_the_limit_sends_only_its_domain_to_the_host():
    def make(gen, domains):
        host = S.pretrain_step_batches(gen, domains)
        d = domains[1]
        F = int(host[d].x.size(1))
        i = torch.arange(1100)
        ring = Data(torch.randn(1100, F, generator=gen), torch.stack([i, (i + 1) % 1100]), torch.zeros(1, dtype=torch.long), torch.rand(12, generator=gen))
        host[d] = Batch.from_data_list(host[d].to_data_list()[:2] + [ring])
        return host
    om, hm, eng, host, inp, gen, tasks, domains = build("s4", 193, make_host=make, device_negatives=True)
    asked = []
    real = eng._negatives
    eng._negatives = lambda b: (asked.append(b), real(b))[1]
    ticket = eng.enqueue_draws(inp)
    assert sorted(d for (t, d, _) in ticket.layout if t == "link_pred") == sorted(d for d in domains if d != domains[1])
    art = eng.collect_draws(inp, ticket)
    assert len(asked) == 1 and asked[0] is inp.host[domains[1]]
    for d in domains:
        neg = art["link_pred"][d]
        if d != domains[1]:
            check_negatives(host[d], neg)
        else:                                       # the host sampler's own output: distinct non-edges, at most num_neg per graph
            ref = R.batch_ref(host[d], host[d].num_edges)
            for (cnt, M, nd, codes), mine in zip(ref, R.split_per_graph(host[d], neg)):
                assert len(np.unique(mine)) == len(mine) <= min(M, host[d].num_edges) and np.isin(mine, codes).all()
    eng.step(inp, gen, art=art, order=list(tasks), apply_update=False)
    torch.cuda.synchronize()
    eng.check_gates()
    assert all(np.isfinite(v) for v in eng.losses().values())
