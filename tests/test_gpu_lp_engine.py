"""The link-prediction fine-tune step on explicit kernels (finetune/engine.py LinkPredictionEngine) and its fused scorer
(csrc/lp_score.hip, gmp_lp_score_fwd / _bwd): the scorer against fp64 torch, one Cora_LP-shaped step against the oracle, the mining
pass, linear_probe, sparse features, determinism with the side-stream fork, and the CLI loop end to end."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from gnn_pretraining_amd import _lib as L, ops, synthetic as S                     # noqa: E402
from gnn_pretraining_amd.graph import Batch, SparseFeatures                        # noqa: E402
from gnn_pretraining_amd.models import FinetuneGNN                                 # noqa: E402
from oracle import models as OM                                                    # noqa: E402
from parity_util import assert_close, assert_grad_close, assert_grad_tight, copy_state, set_dropout, to_oracle   # noqa: E402

DEV = torch.device("cuda:0")
SCORER_TOL = 2e-5          # fp32 kernel vs fp64 torch: max |err| / max |fp64 value| per tensor (sums of 768-256 products, up to 3,000 pairs)


def _bce_lib(logit, labels):
    """The engine's loss launch (gmp_sigmoid_bce_sum_fwd_bwd) on a logit vector: (mean loss, probabilities, d mean loss / d logit)."""
    lib, K = L.lib(), logit.numel()
    g_scale = torch.full((1,), 1.0 / K, device=DEV)
    loss, prob, g = torch.zeros(1, device=DEV), torch.empty(K, device=DEV), torch.empty(K, device=DEV)
    ws = torch.empty(max(lib.gmp_loss_workspace_bytes(K), 16), dtype=torch.uint8, device=DEV)
    L.check(lib.gmp_sigmoid_bce_sum_fwd_bwd(logit.data_ptr(), labels.data_ptr(), K, g_scale.data_ptr(), loss.data_ptr(), prob.data_ptr(),
                                            g.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream), "bce")
    return loss / K, prob, g


@pytest.mark.parametrize("K", [1, 238, 512, 3000])
@pytest.mark.parametrize("p", [0.0, 0.2])
def test_fused_scorer_matches_fp64_torch(K, p):
    gen = torch.Generator().manual_seed(K + int(p * 10))
    N, Hd = 300, 256
    h = torch.randn(N, Hd, generator=gen)
    h[:, 7] = 0.25                                            # an exact hs == hd column: |hs - hd| sits at 0 for every pair
    src, dst = torch.randint(0, N, (K,), generator=gen), torch.randint(0, N, (K,), generator=gen)
    if K > 4:
        src[1], dst[1] = src[0], dst[0]                       # a repeated pair
        dst[2] = src[2]                                       # src == dst
        src[3] = N                                            # outside [0, N): reads as a zero row
    w0 = torch.randn(Hd, 3 * Hd, generator=gen) * 0.05
    b0, w3, b3 = torch.randn(Hd, generator=gen) * 0.1, torch.randn(1, Hd, generator=gen) * 0.1, torch.randn(1, generator=gen) * 0.1
    labels = (torch.rand(K, generator=gen) < 0.5).float()
    seed, site = 1234567, 40
    d = lambda t: t.to(DEV).contiguous()
    act, logit = ops.lp_score_fwd(d(h), d(src), d(dst), d(w0), d(b0), d(w3), d(b3), p, seed, site)
    loss, prob, g_logit = _bce_lib(logit, d(labels))
    g_w0, g_b0, g_w3, g_b3, g_hs, g_hd = ops.lp_score_bwd(d(h), d(src), d(dst), d(w0), d(w3), act, g_logit, p, seed, site)
    g_h = ops.lp_score_node_grad(g_hs, g_hd, d(torch.stack([src, dst])), N)
    # the kernel's own dropout mask: the library's dropout kernel draws it for the same (seed, site) over a [K, 256] activation
    mask = ops.dropout_fwd(torch.ones(K, Hd, device=DEV), p, seed, site).cpu().double() if p > 0 else torch.ones(K, Hd, dtype=torch.float64)
    gates = (act.cpu() > 0).double()                          # the kernel's ReLU gates (a pre-activation within rounding of 0 may differ)
    # fp64 reference
    hd64 = h.double().requires_grad_(True)
    W0, B0, W3, B3 = (t.double().requires_grad_(True) for t in (w0, b0, w3, b3))
    zero = torch.zeros(1, Hd, dtype=torch.float64)
    rows = lambda i: torch.where((i < N).unsqueeze(1), torch.cat([hd64, zero])[i.clamp(max=N)], zero)
    hs, hdd = rows(src), rows(dst)
    # the node scatter (csr_build + segment_sum, as in the module path's backward) drops a pair with an endpoint outside [0, N)
    valid = ((src < N) & (dst < N)).unsqueeze(1)
    hs, hdd = torch.where(valid, hs, hs.detach()), torch.where(valid, hdd, hdd.detach())
    feat = torch.cat([hs + hdd, hs * hdd, (hs - hdd).abs()], dim=1)
    z = feat @ W0.T + B0
    a = z * gates
    y = (a * mask) @ W3[0] + B3[0]
    pr = torch.sigmoid(y)
    lo = F.binary_cross_entropy(pr, labels.double())
    lo.backward()
    assert_close(act, torch.relu(z).detach() * gates, SCORER_TOL, "act")
    assert_close(logit, y.detach(), SCORER_TOL, "logit")
    assert_close(prob, pr.detach(), SCORER_TOL, "probabilities")
    assert abs(loss.item() - lo.item()) <= SCORER_TOL * abs(lo.item())
    for got, ref, n in ((g_w0, W0.grad, "dW0"), (g_b0, B0.grad, "db0"), (g_w3, W3.grad[0], "dw3"), (g_b3, B3.grad, "db3"), (g_h, hd64.grad, "g_h")):
        assert_close(got, ref, SCORER_TOL, n)
    # deterministic: a second run is bitwise the same
    r2 = ops.lp_score_bwd(d(h), d(src), d(dst), d(w0), d(w3), act, g_logit, p, seed, site)
    for a1, a2 in zip((g_w0, g_b0, g_w3, g_b3, g_hs, g_hd), r2):
        assert torch.equal(a1, a2)


def _lp_setup(seed, domain="Cora_LP", strategy="full_finetune", num_nodes=2708, dim=1433):
    from gnn_pretraining_amd.data.data_setup import create_link_prediction_splits
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    c = S.cora_like(gen, num_nodes=num_nodes, dim=dim)
    splits = create_link_prediction_splits(c)
    return gen, c, splits["train_pos"].contiguous()


def _twin(m, domain):
    t = FinetuneGNN(DEV, domain, "full_finetune")
    t.load_state_dict(m.state_dict())
    return t


def _neg(gen, n, k):
    return torch.stack([torch.randint(0, n, (k,), generator=gen), torch.randint(0, n, (k,), generator=gen)])


def test_lp_engine_step_matches_the_oracle_step():
    """One Cora_LP-shaped step (2,708 x 1,433, 256 positives + mined negatives, dropout 0) on the engine against the oracle model +
    torch.optim.AdamW, with the engine's ReLU gates and |x| signs imposed on the oracle's training forward (oracle/gates.py); the oracle's
    mining pass runs outside the tape for its BatchNorm side effect.  Bars of the node-classification engine test."""
    from gnn_pretraining_amd.finetune.engine import LinkPredictionEngine
    from gnn_pretraining_amd.finetune.finetune import LinkPredictionHardNegativeMiner
    from oracle import gates as OGt
    gen, c, train_pos = _lp_setup(41)
    om = OM.FinetuneGNN(torch.device("cpu"), "Cora_LP", "full_finetune")
    hm = FinetuneGNN(torch.device("cpu"), "Cora_LP", "full_finetune")
    copy_state(hm, om); hm.device = DEV; hm.to(DEV)
    set_dropout(om, 0.0)
    om.train(); hm.train()
    eng = LinkPredictionEngine(hm, c.x, train_pos, DEV, seed=5)
    eng.dropout_p = 0.0
    keys_before = list(hm.state_dict().keys())
    oopt = torch.optim.AdamW(om.param_groups)
    for g in oopt.param_groups:
        g["lr"] *= 100
    eng.lr.mul_(100)
    before = {k: v.clone() for k, v in om.state_dict().items()}
    pos = train_pos[:, :256].contiguous()
    mp = train_pos.to(DEV)
    emb = eng.mining_forward()
    neg = LinkPredictionHardNegativeMiner().mine_hard_negatives_for_edges(emb, pos.to(DEV), 256, mp)
    eng.step(pos.to(DEV), neg)
    torch.cuda.synchronize()
    K = 256 + neg.size(1)
    all_edges = torch.cat([pos, neg.cpu()], dim=1)
    labels = torch.cat([torch.ones(256), torch.zeros(neg.size(1))])
    hL = eng.h[5].cpu()
    masks = [(eng.h[0] > 0).cpu()]
    for l in range(5):
        masks += [(eng.r1[l] > 0).cpu(), (eng.h[l + 1] > 0).cpu()]
    masks += [torch.sign(hL[all_edges[0]] - hL[all_edges[1]]), (eng.act[:K] > 0).cpu()]
    ob = to_oracle(Batch.from_data_list([c]))
    with torch.no_grad():                                     # the mining pass: BatchNorm statistics only
        om.gnn_backbone(om.input_encoder(ob.x), train_pos)
    tape = OGt.GateTape(masks)
    with OGt.use_tape(tape):
        probs = om(ob, edge_index=all_edges, message_passing_edges=train_pos)
    assert tape.done()
    lo = F.binary_cross_entropy(probs, labels)
    oopt.zero_grad(); lo.backward(); oopt.step()
    assert abs(eng.loss() - lo.item()) <= 1e-4 * abs(lo.item())
    assert_close(eng.probabilities(), probs.detach(), 1e-4, "probabilities")
    og = dict(om.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in og.values())
    bn_fed = lambda n: n.endswith("linear.bias") or n.endswith("gin_conv.nn.0.bias") or n.endswith("gin_conv.nn.3.bias")
    for n, p in og.items():
        if bn_fed(n):
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
            assert int(after_h[k]) == int(v) == 2, k
        elif bn_fed(k):
            assert (after_h[k].cpu() - before[k]).abs().max().item() <= 1.01 * 100 * 1e-3
        else:
            num += ((after_h[k].cpu() - v).double() ** 2).sum().item()
            den += ((v - before[k]).double() ** 2).sum().item()
    assert (num / den) ** 0.5 <= 2e-2, f"relative update error {(num / den) ** 0.5:.3e}"
    # evaluation goes through the module: its eval forward agrees with the engine's
    hm.eval()
    with torch.no_grad():
        h_mod = hm.gnn_backbone(hm.input_encoder(c.x.to(DEV)), mp)
    h_eng = eng.forward()
    torch.cuda.synchronize()
    assert_close(h_eng, h_mod, 1e-4, "module eval forward vs engine")
    hm.train()


def test_mining_pass_equals_the_module_forward_and_draws_its_own_masks():
    from gnn_pretraining_amd.finetune.engine import LinkPredictionEngine
    gen, c, train_pos = _lp_setup(43)
    hm = FinetuneGNN(DEV, "Cora_LP", "full_finetune")
    hm.train()
    mp = train_pos.to(DEV)
    eng = LinkPredictionEngine(hm, c.x, train_pos, DEV, seed=9)
    eng.dropout_p = 0.0
    set_dropout(hm, 0.0)
    with torch.no_grad():
        h_mod = hm.gnn_backbone(hm.input_encoder(c.x.to(DEV)), mp).clone()
    h_eng = eng.mining_forward().clone()
    assert_close(h_eng, h_mod, 1e-5, "mining pass vs module no_grad train-mode forward")
    eng.dropout_p = 0.2
    eng.mining_forward()
    mine_h0 = eng.h[0].clone()
    eng.step(train_pos[:, :64].to(DEV), _neg(gen, c.num_nodes, 64).to(DEV))
    torch.cuda.synchronize()
    assert not torch.equal(mine_h0 == 0, eng.h[0] == 0), "mining and training forward drew the same dropout masks"
    assert np.isfinite(eng.loss())


def test_linear_probe_keeps_the_backbone():
    from gnn_pretraining_amd.finetune.engine import LinkPredictionEngine
    gen, c, train_pos = _lp_setup(45)
    hm = FinetuneGNN(DEV, "Cora_LP", "linear_probe")
    hm.train()
    before = {n: p.detach().clone() for n, p in hm.named_parameters()}
    eng = LinkPredictionEngine(hm, c.x, train_pos, DEV, seed=2)
    for s in range(3):
        eng.mining_forward()
        eng.step(train_pos[:, 256 * s:256 * s + 238].to(DEV), _neg(gen, c.num_nodes, 238).to(DEV))   # 238: Cora's ragged last batch
    torch.cuda.synchronize()
    assert np.isfinite(eng.loss())
    for n, p in hm.named_parameters():
        if n.startswith("gnn_backbone."):
            assert torch.equal(p.detach(), before[n]), n
        elif not n.endswith("linear.bias"):                   # (the encoder Linear's bias feeds a BatchNorm: gradient ~0)
            assert not torch.equal(p.detach(), before[n]), n


def test_sparse_features_agree_with_dense():
    """CiteSeer_LP shape (3,327 x 3,703): the engine on graph.SparseFeatures against the dense engine, one step, dropout 0."""
    from gnn_pretraining_amd.finetune.engine import LinkPredictionEngine
    gen, c, train_pos = _lp_setup(47, "CiteSeer_LP", num_nodes=3327, dim=3703)
    domain = "CiteSeer_LP"
    m1 = FinetuneGNN(DEV, domain, "full_finetune")
    m2 = _twin(m1, domain)
    m1.train(); m2.train()
    e1 = LinkPredictionEngine(m1, c.x, train_pos, DEV, seed=4)
    e2 = LinkPredictionEngine(m2, SparseFeatures.from_dense(c.x), train_pos, DEV, seed=4)
    pos, neg = train_pos[:, :256].to(DEV), _neg(gen, c.num_nodes, 256).to(DEV)
    for e in (e1, e2):
        e.dropout_p = 0.0
        e.mining_forward()
        e.step(pos, neg)
    torch.cuda.synchronize()
    assert abs(e1.loss() - e2.loss()) <= 1e-5 * abs(e1.loss())
    assert_close(e2.probabilities(), e1.probabilities(), 1e-4, "probabilities")
    gmax = e1.final_grad.abs().max().item()
    for n in e1.names:
        assert_grad_close(e2.gradient(n), e1.gradient(n), gmax, n)


def test_lp_engine_is_deterministic_with_the_side_stream():
    from gnn_pretraining_amd.finetune.engine import LinkPredictionEngine
    gen, c, train_pos = _lp_setup(49)
    domain = "Cora_LP"
    m1 = FinetuneGNN(DEV, domain, "full_finetune")
    m2 = _twin(m1, domain)
    engines = []
    for m in (m1, m2):
        m.train()
        e = LinkPredictionEngine(m, c.x, train_pos, DEV, seed=11)
        e.dropout_p = 0.2
        engines.append(e)
    batches = [(train_pos[:, 256 * s:256 * (s + 1)].to(DEV), _neg(gen, c.num_nodes, 256).to(DEV)) for s in range(5)]
    for e in engines:
        for pos, neg in batches:
            e.mining_forward()
            e.step(pos, neg)
    torch.cuda.synchronize()
    e1, e2 = engines
    assert e1.fork_wgrads == e2.fork_wgrads
    for a, b, n in ((e1.flat, e2.flat, "parameters"), (e1.exp_avg, e2.exp_avg, "exp_avg"), (e1.exp_avg_sq, e2.exp_avg_sq, "exp_avg_sq")):
        assert torch.equal(a, b), n
    assert e1.loss() == e2.loss()


def test_pretrain_then_link_prediction_finetune_on_the_engine(tmp_path, monkeypatch):
    from gnn_pretraining_amd.finetune import finetune as FT
    from gnn_pretraining_amd.models import finetune_model as FM
    from gnn_pretraining_amd.pretrain import pretrain as PT
    monkeypatch.setattr(PT, "OUTPUT_DIR", tmp_path / "pretrain")
    monkeypatch.setattr(FM, "PRETRAIN_OUTPUT_DIR", tmp_path / "pretrain")
    monkeypatch.setattr(FT, "OUTPUT_DIR", tmp_path / "finetune")
    PT.pretrain(PT.PretrainConfig(exp_name="s4", seed=7), epochs=1, steps_per_epoch=3, data_root=str(tmp_path / "data"), data_scale=0.03)
    monkeypatch.setattr(FM.load_pretrained_weights, "__defaults__", (tmp_path / "pretrain",))
    log = tmp_path / "log.jsonl"
    test = FT.finetune(FT.FinetuneConfig("Cora_LP", "full_finetune", "s4", 7, lp_engine=True), epochs=2, data_root=str(tmp_path / "data"),
                       data_scale=0.1, log_path=str(log))
    assert np.isfinite(test["test/auc"]) and 0.0 <= test["test/auc"] <= 1.0
    assert any('"train/' in line for line in log.read_text().splitlines()), "no training metrics logged"
