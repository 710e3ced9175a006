"""The graph-classification fine-tune step on explicit kernels (finetune/engine.py GraphClassificationEngine) and its fused head
(csrc/gc_head.hip, gmp_gc_head_fwd / _bwd): the head against fp64 torch, one ENZYMES- and one PTC_MR-shaped step against the oracle,
changing batch sizes with a regrow, linear_probe, determinism with the side-stream fork, evaluation, and the CLI loop end to end.
Parity is against oracle/, whose PyG operators are restated; the batches are synthetic (ENZYMES / PTC_MR shapes)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gnn_pretraining_amd import ops, synthetic as S                                 # noqa: E402
from gnn_pretraining_amd.graph import Batch                                         # noqa: E402
from gnn_pretraining_amd.models import FinetuneGNN                                  # noqa: E402
from oracle import models as OM                                                     # noqa: E402
from parity_util import assert_close, assert_grad_tight, copy_state, set_dropout, to_oracle   # noqa: E402

DEV = torch.device("cuda:0")
SCORER_TOL = 2e-5          # fp32 kernel vs fp64 torch: max |err| / max |fp64 value| per tensor (the project's bar for the fused scorer)
CLASSES = {"ENZYMES": 6, "PTC_MR": 2}
DIMS = {"ENZYMES": 21, "PTC_MR": 18}


def _batch(gen, domain, graphs):
    """A synthetic batch of the domain's shape: ENZYMES 33 nodes / 62 edges per graph, PTC_MR 14 / 15, labels in 0 .. C - 1."""
    mn, me = (33.0, 62.0) if domain == "ENZYMES" else (14.0, 15.0)
    return Batch.from_data_list([S.random_graph(gen, DIMS[domain], mn, me, num_classes=CLASSES[domain]) for _ in range(graphs)])


def _loss64(logits, y, C):
    """The reference's classification_loss (finetune.py:110-114) as a SUM over the batch."""
    if C == 2:
        return F.binary_cross_entropy_with_logits(logits[:, 1], y.to(logits.dtype), reduction="sum")
    return F.cross_entropy(logits, y, reduction="sum")


@pytest.mark.parametrize("B", [1, 5, 32, 300])
@pytest.mark.parametrize("C", [2, 6])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_fused_head_matches_fp64_torch(B, C, p):
    gen = torch.Generator().manual_seed(1000 * B + 10 * C + int(p * 10))
    Hd, Hh = 256, 128
    if B == 1:
        sizes = [37]
    else:                                                     # ragged: one node, no node, more than 256 nodes
        sizes = torch.randint(2, 60, (B,), generator=gen).tolist()
        sizes[0], sizes[1], sizes[2] = 1, 0, 300
    ptr = torch.tensor([0] + np.cumsum(sizes).tolist(), dtype=torch.int32)
    N = int(ptr[-1])
    h = torch.randn(N, Hd, generator=gen)
    w0, b0 = torch.randn(Hh, Hd, generator=gen) * 0.08, torch.randn(Hh, generator=gen) * 0.1
    w3, b3 = torch.randn(C, Hh, generator=gen) * 0.1, torch.randn(C, generator=gen) * 0.1
    y = torch.randint(0, C, (B,), generator=gen)
    seed, site = 7654321, 41
    d = lambda t: t.to(DEV).contiguous()
    g_scale = torch.full((1,), 1.0 / B, device=DEV)
    pooled, act, logits, loss, g_logits = ops.gc_head_fwd(d(h), d(ptr), d(w0), d(b0), d(w3), d(b3), d(y), g_scale, p, seed, site)
    g_w0, g_b0, g_w3, g_b3, g_h = ops.gc_head_bwd(d(ptr), N, d(w0), d(w3), pooled, act, g_logits, p, seed, site)
    # the kernel's own dropout mask and ReLU gates on the fp64 side
    mask = ops.dropout_fwd(torch.ones(B, Hh, device=DEV), p, seed, site).cpu().double() if p > 0 else torch.ones(B, Hh, dtype=torch.float64)
    gates = (act.cpu() > 0).double()
    h64 = h.double().requires_grad_(True)
    W0, B0, W3, B3 = (t.double().requires_grad_(True) for t in (w0, b0, w3, b3))
    rows = []
    for b in range(B):
        a, e = int(ptr[b]), int(ptr[b + 1])
        rows.append(h64[a:e].sum(dim=0) / max(e - a, 1))
    pool64 = torch.stack(rows)
    z = pool64 @ W0.T + B0
    yy = ((z * gates) * mask) @ W3.T + B3
    lo = _loss64(yy, y, C)
    (lo / B).backward()
    assert_close(pooled, pool64.detach(), SCORER_TOL, "pooled")
    assert_close(act, torch.relu(z).detach() * gates, SCORER_TOL, "act")
    assert_close(logits, yy.detach(), SCORER_TOL, "logits")
    print(f"B={B} C={C} p={p}: loss {loss.item():.7f} fp64 {lo.item():.7f}")
    assert abs(loss.item() - lo.item()) <= SCORER_TOL * abs(lo.item())
    if C == 2:
        assert torch.count_nonzero(g_logits[:, 0]).item() == 0 and torch.count_nonzero(g_w3[0]).item() == 0 and g_b3[0].item() == 0.0
    for got, ref, n in ((g_w0, W0.grad, "dW0"), (g_b0, B0.grad, "db0"), (g_w3, W3.grad, "dW3"), (g_b3, B3.grad, "db3"), (g_h, h64.grad, "g_h")):
        assert_close(got, ref, SCORER_TOL, n)
    # deterministic: a second run is bitwise the same
    f2 = ops.gc_head_fwd(d(h), d(ptr), d(w0), d(b0), d(w3), d(b3), d(y), g_scale, p, seed, site)
    for a1, a2 in zip((pooled, act, logits, loss, g_logits), f2):
        assert torch.equal(a1, a2)
    r2 = ops.gc_head_bwd(d(ptr), N, d(w0), d(w3), pooled, act, g_logits, p, seed, site)
    for a1, a2 in zip((g_w0, g_b0, g_w3, g_b3, g_h), r2):
        assert torch.equal(a1, a2)


def _twin(m, domain, strategy="full_finetune"):
    t = FinetuneGNN(DEV, domain, strategy)
    t.load_state_dict(m.state_dict())
    return t


@pytest.mark.parametrize("domain", ["ENZYMES", "PTC_MR"])
def test_gc_engine_step_matches_the_oracle_step(domain):
    """One 32-graph step (full fine-tune, dropout 0, learning rates x 100) on the engine against the oracle model + torch.optim.AdamW,
    with the engine's 12 ReLU gate masks (encoder, inner / outer of five layers, head) imposed on the oracle (oracle/gates.py).
    Bars of the link-prediction engine's step test."""
    from gnn_pretraining_amd.finetune.engine import GraphClassificationEngine
    from oracle import gates as OGt
    C = CLASSES[domain]
    gen = torch.Generator().manual_seed(61 + C)
    torch.manual_seed(61 + C)
    batch = _batch(gen, domain, 32)
    N, B = batch.num_nodes, batch.num_graphs
    om = OM.FinetuneGNN(torch.device("cpu"), domain, "full_finetune")
    hm = FinetuneGNN(torch.device("cpu"), domain, "full_finetune")
    copy_state(hm, om); hm.device = DEV; hm.to(DEV)
    set_dropout(om, 0.0)
    om.train(); hm.train()
    eng = GraphClassificationEngine(hm, DEV, seed=5)
    eng.dropout_p = 0.0
    keys_before = list(hm.state_dict().keys())
    oopt = torch.optim.AdamW(om.param_groups)
    for g in oopt.param_groups:
        g["lr"] *= 100
    eng.lr.mul_(100)
    before = {k: v.clone() for k, v in om.state_dict().items()}
    eng.step(batch.to(DEV))
    torch.cuda.synchronize()
    masks = [(eng.h[0][:N] > 0).cpu()]
    for l in range(5):
        masks += [(eng.r1[l][:N] > 0).cpu(), (eng.h[l + 1][:N] > 0).cpu()]
    masks.append((eng.act[:B] > 0).cpu())
    assert len(masks) == 12
    tape = OGt.GateTape(masks)
    with OGt.use_tape(tape):
        logits = om(to_oracle(batch))
    assert tape.done()
    lo = _loss64(logits, batch.y, C) / B
    oopt.zero_grad(); lo.backward(); oopt.step()
    print(f"{domain}: engine loss {eng.loss():.7f} oracle {lo.item():.7f}")
    assert abs(eng.loss() - lo.item()) <= 1e-4 * abs(lo.item())
    assert_close(eng.logits(), logits.detach(), 1e-4, "logits")
    og = dict(om.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in og.values() if p.grad is not None)
    bn_fed = lambda n: n.endswith("linear.bias") or n.endswith("gin_conv.nn.0.bias") or n.endswith("gin_conv.nn.3.bias")
    frozen = [n for n, p in og.items() if not p.requires_grad]
    assert (domain == "ENZYMES") == bool(frozen) and all(n.startswith("input_encoder.") for n in frozen)
    for n, p in og.items():
        if n in frozen:
            assert p.grad is None and torch.count_nonzero(eng.gradient(n)).item() == 0, n
        elif bn_fed(n):
            assert eng.gradient(n).abs().max().item() <= 1e-4 * gmax and p.grad.abs().max().item() <= 1e-3 * gmax, n
        else:
            assert_grad_tight(eng.gradient(n), p.grad, gmax, f"grad {n}")
    eng.flush_counters()
    after_o, after_h = om.state_dict(), hm.state_dict()
    assert list(after_h.keys()) == keys_before
    num = den = 0.0
    for k, v in after_o.items():
        if "running_" in k:
            assert_close(after_h[k], v, 1e-4, f"buffer {k}")
        elif k.endswith("num_batches_tracked"):
            assert int(after_h[k]) == int(v) == 1, k
        elif k in frozen:                                     # the frozen encoder: bitwise what it was, on both sides
            assert torch.equal(after_h[k].cpu(), before[k]) and torch.equal(v, before[k]), k
        elif bn_fed(k):
            assert (after_h[k].cpu() - before[k]).abs().max().item() <= 1.01 * 100 * 1e-3
        else:
            num += ((after_h[k].cpu() - v).double() ** 2).sum().item()
            den += ((v - before[k]).double() ** 2).sum().item()
    print(f"{domain}: relative update error {(num / den) ** 0.5:.3e}")
    assert (num / den) ** 0.5 <= 2e-2, f"relative update error {(num / den) ** 0.5:.3e}"
    if C == 2:                                                # logits[:, 0] has no gradient: its row moves by weight decay only
        decay = 1.0 - (1e-3 * 100) * 0.01
        for k in ("classification_head.mlp.3.weight", "classification_head.mlp.3.bias"):
            for side, name in ((after_h[k].cpu(), "engine"), (after_o[k], "oracle")):
                assert_close(side[0], before[k][0] * decay, 1e-6, f"{name} {k}[0]")


def test_changing_batches_and_regrow():
    """Three consecutive steps on batches of different N, E and B -- a large one, a smaller one (rows of the larger batch stay behind in
    the buffers), one beyond the initial capacity -- each against the module path on a twin model holding the weights of before the step."""
    from gnn_pretraining_amd.finetune import finetune as FT
    from gnn_pretraining_amd.finetune.engine import GraphClassificationEngine
    gen = torch.Generator().manual_seed(71)
    torch.manual_seed(71)
    hm = FinetuneGNN(DEV, "ENZYMES", "full_finetune")
    hm.train()
    eng = GraphClassificationEngine(hm, DEV, seed=3, max_nodes=600, max_edges=2500, max_graphs=16)
    eng.dropout_p = 0.0
    twin = _twin(hm, "ENZYMES")
    twin.train()
    set_dropout(twin, 0.0)
    batches = [_batch(gen, "ENZYMES", g).to(DEV) for g in (12, 5, 40)]
    assert batches[2].num_nodes > 600 and batches[2].num_graphs > 16 and batches[1].num_nodes < batches[0].num_nodes <= 600
    for i, b in enumerate(batches):
        twin.load_state_dict(hm.state_dict())
        lg = twin(b)
        lo = FT.classification_loss(lg, b.y, 6)
        eng.step(b)
        torch.cuda.synchronize()
        print(f"step {i}: N={b.num_nodes} E={b.num_edges} B={b.num_graphs} engine loss {eng.loss():.7f} module {lo.item():.7f}")
        assert abs(eng.loss() - lo.item()) <= 1e-4 * abs(lo.item()), i
        assert_close(eng.logits(), lg.detach(), 1e-4, f"logits of step {i}")
    assert eng.cap_n >= batches[2].num_nodes and eng.cap_b >= 40 and eng.cap_e >= batches[2].num_edges


def test_linear_probe_keeps_the_backbone():
    from gnn_pretraining_amd.finetune.engine import GraphClassificationEngine
    gen = torch.Generator().manual_seed(73)
    torch.manual_seed(73)
    hm = FinetuneGNN(DEV, "ENZYMES", "linear_probe")
    hm.train()
    before = {n: p.detach().clone() for n, p in hm.named_parameters()}
    eng = GraphClassificationEngine(hm, DEV, seed=2)
    for s in range(3):
        eng.step(_batch(gen, "ENZYMES", 32).to(DEV))
    torch.cuda.synchronize()
    assert np.isfinite(eng.loss())
    for n, p in hm.named_parameters():
        if n.startswith("classification_head."):
            assert not torch.equal(p.detach(), before[n]), n
        else:                                                 # ENZYMES: the encoder is frozen too
            assert torch.equal(p.detach(), before[n]), n


def test_gc_engine_is_deterministic_with_the_side_stream():
    from gnn_pretraining_amd.finetune.engine import GraphClassificationEngine
    gen = torch.Generator().manual_seed(75)
    torch.manual_seed(75)
    m1 = FinetuneGNN(DEV, "PTC_MR", "full_finetune")
    m2 = _twin(m1, "PTC_MR")
    engines = []
    for m in (m1, m2):
        m.train()
        e = GraphClassificationEngine(m, DEV, seed=11)
        e.dropout_p = 0.2
        engines.append(e)
    batches = [_batch(gen, "PTC_MR", g).to(DEV) for g in (32, 32, 17, 32, 9)]
    for e in engines:
        for b in batches:
            e.step(b)
    torch.cuda.synchronize()
    e1, e2 = engines
    assert e1.fork_wgrads == e2.fork_wgrads
    for a, b, n in ((e1.flat, e2.flat, "parameters"), (e1.exp_avg, e2.exp_avg, "exp_avg"), (e1.exp_avg_sq, e2.exp_avg_sq, "exp_avg_sq")):
        assert torch.equal(a, b), n
    assert e1.loss() == e2.loss()


def test_evaluation_goes_through_the_module():
    from gnn_pretraining_amd.finetune.engine import GraphClassificationEngine
    gen = torch.Generator().manual_seed(77)
    torch.manual_seed(77)
    hm = FinetuneGNN(DEV, "ENZYMES", "full_finetune")
    hm.train()
    eng = GraphClassificationEngine(hm, DEV, seed=4)
    eng.step(_batch(gen, "ENZYMES", 32).to(DEV))
    b = _batch(gen, "ENZYMES", 20).to(DEV)
    hm.eval()
    with torch.no_grad():
        lg_mod = hm(b)
    lg_eng = eng.evaluate(b)
    torch.cuda.synchronize()
    assert_close(lg_eng, lg_mod, 1e-4, "module eval forward vs engine")
    assert np.isfinite(eng.loss())                            # (raises if a gate or a BatchNorm slab wait timed out)
    assert int(eng.sync_flags[63].item()) == 0 and (eng.bn_sync is None or int(eng.bn_sync[0].item()) == 0)
    hm.train()


def test_pretrain_then_graph_classification_finetune_on_the_engine(tmp_path, monkeypatch):
    from gnn_pretraining_amd.finetune import finetune as FT
    from gnn_pretraining_amd.models import finetune_model as FM
    from gnn_pretraining_amd.pretrain import pretrain as PT
    monkeypatch.setattr(PT, "OUTPUT_DIR", tmp_path / "pretrain")
    monkeypatch.setattr(FM, "PRETRAIN_OUTPUT_DIR", tmp_path / "pretrain")
    monkeypatch.setattr(FT, "OUTPUT_DIR", tmp_path / "finetune")
    PT.pretrain(PT.PretrainConfig(exp_name="s4", seed=7), epochs=1, steps_per_epoch=3, data_root=str(tmp_path / "data"), data_scale=0.03)
    monkeypatch.setattr(FM.load_pretrained_weights, "__defaults__", (tmp_path / "pretrain",))
    log = tmp_path / "log.jsonl"
    test = FT.finetune(FT.FinetuneConfig("ENZYMES", "full_finetune", "s4", 7, gc_engine=True), epochs=2, data_root=str(tmp_path / "data"),
                       data_scale=0.03, log_path=str(log))
    assert np.isfinite(test["test/accuracy"]) and 0.0 <= test["test/accuracy"] <= 1.0
    assert any('"train/' in line for line in log.read_text().splitlines()), "no training metrics logged"


def test_an_engine_without_a_loaded_batch_refuses_forward_embed_and_evaluate(monkeypatch):
    """Construction sets up no graph of its own (no placeholder, no csr_build), so there is nothing to run on until a batch is loaded."""
    from gnn_pretraining_amd.finetune.engine import GraphClassificationEngine, NodeClassificationEngine
    assert NodeClassificationEngine not in GraphClassificationEngine.__mro__
    monkeypatch.setattr(ops, "csr_build", lambda *a, **k: pytest.fail("csr_build at construction"))
    eng = GraphClassificationEngine(FinetuneGNN(DEV, "PTC_MR", "full_finetune"), DEV, max_nodes=8, max_edges=8, max_graphs=2)
    for call in (eng.forward, eng.embed, eng.evaluate):
        with pytest.raises(ValueError, match="no batch has been loaded"):
            call()
    assert eng._fwd_gen == 0                                  # (refused before anything was launched)
