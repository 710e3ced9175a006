"""Sparse (CSR) node features on the GPU: the gmp_sparse_linear_* kernels against fp64, the module path (one Cora_LP train step), the
Cora_NC / CiteSeer_NC node engine against the oracle step and three ways bitwise, and the fine-tune loop end to end."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gnn_pretraining_amd import ops, synthetic as S                              # noqa: E402
from gnn_pretraining_amd._lib import GnnmpError                                 # noqa: E402
from gnn_pretraining_amd.graph import Batch, SparseFeatures                     # noqa: E402
from gnn_pretraining_amd.models import FinetuneGNN                              # noqa: E402
from oracle import models as OM                                                 # noqa: E402
from parity_util import assert_close, assert_grad_close, assert_grad_tight, copy_state, set_dropout, to_oracle   # noqa: E402

DEV = torch.device("cuda:0")
OUT_RTOL = 1e-4
SHAPES = {"cora": (2708, 1433, 1440, 0.0127), "citeseer": (3327, 3703, 3712, 0.0085)}


def _features(name, seed):
    """Bag-of-words-like X [N, K] plus edge rows: row 0 empty, row 1 fully dense (K terms); N is not a multiple of 4 rows per block."""
    N, K, ldw, dens = SHAPES[name]
    gen = torch.Generator().manual_seed(seed)
    x = (torch.rand(N, K, generator=gen) < dens).float() * torch.rand(N, K, generator=gen)
    x[0] = 0.0
    x[1] = torch.rand(K, generator=gen)
    x[:, 5] = 0.0                                                            # a column without entries
    return x, ldw, gen


@pytest.mark.parametrize("name", ["cora", "citeseer"])
def test_sparse_linear_forward_matches_fp64(name):
    x, ldw, gen = _features(name, 11)
    N, K = x.shape
    slot = torch.randn(256, ldw, generator=gen) * 0.05                        # the engine's padded [256, ldw] slot; W is the [256, K] view
    b = torch.randn(256, generator=gen)
    W = slot.to(DEV)[:, :K]
    sp = SparseFeatures.from_dense(x).to(DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    y1 = ops.sparse_linear_fwd(sp, W, b.to(DEV), status=status)
    y2 = ops.sparse_linear_fwd(sp, W, b.to(DEV))
    torch.cuda.synchronize()
    ref = x.double() @ slot[:, :K].double().T + b.double()
    err = (y1.cpu().double() - ref).abs().max().item()
    assert err <= 2e-6 * ref.abs().max().item(), f"{name}: forward err {err:.3e} vs max {ref.abs().max().item():.3e}"
    assert torch.equal(y1.cpu()[0], b)                                       # empty row: exactly the bias
    assert torch.equal(y1, y2), "two launches differ"
    assert int(status.item()) == 0
    # the module dispatch takes the same kernel (row-strided weight view read in place)
    from gnn_pretraining_amd.models.gnn import Linear
    m = Linear(K, 256).to(DEV)
    m.weight.data, m.bias.data = W, b.to(DEV)
    assert torch.equal(m(sp).detach(), y1)


def test_sparse_linear_forward_skips_and_counts_bad_columns_and_checks_shapes():
    x, ldw, gen = _features("cora", 12)
    N, K = x.shape
    sp = SparseFeatures.from_dense(x)
    col = sp.col.clone()
    col[3], col[10] = K, K + 500                                             # two indices out of range
    bad = SparseFeatures(sp.rowptr, col, sp.val, sp.shape).to(DEV)
    W, b = (torch.randn(256, K, generator=gen) * 0.05).to(DEV), torch.zeros(256, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    y = ops.sparse_linear_fwd(bad, W, b, status=status)
    keep = torch.ones(sp.nnz, dtype=torch.bool)
    keep[3] = keep[10] = False
    rows = torch.repeat_interleave(torch.arange(N), sp.rowptr[1:].long() - sp.rowptr[:-1].long())
    xd = torch.zeros(N, K, dtype=torch.float64)
    xd[rows[keep], sp.col.long()[keep]] = sp.val.double()[keep]
    ref = xd @ W.cpu().double().T
    torch.cuda.synchronize()
    assert int(status.item()) == 2
    assert (y.cpu().double() - ref).abs().max().item() <= 2e-6 * ref.abs().max().item()
    with pytest.raises(GnnmpError):
        ops.sparse_linear_fwd(sp.to(DEV), torch.zeros(100, K, device=DEV))   # out_features not a multiple of 64: unsupported


@pytest.mark.parametrize("name", ["cora", "citeseer"])
def test_sparse_linear_weight_gradient_matches_fp64(name):
    x, ldw, gen = _features(name, 13)
    N, K = x.shape
    G = torch.randn(N, 256, generator=gen)
    sp = SparseFeatures.from_dense(x).to(DEV)
    csc = sp.csc()
    host = SparseFeatures.from_dense(x).csc()                                # the device CSC build equals the host's stable sort
    for a, h in zip(csc, host):
        assert torch.equal(a.cpu(), h)
    out = torch.full((256, ldw), float("nan"), device=DEV)                   # garbage: every column must be overwritten
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    dW = ops.sparse_linear_wgrad(csc, N, G.to(DEV), out=out, status=status)
    again = ops.sparse_linear_wgrad(csc, N, G.to(DEV), out=torch.full((256, ldw), 7.0, device=DEV))
    db = ops.colsum(G.to(DEV))
    torch.cuda.synchronize()
    ref = G.double().T @ x.double()
    err = (dW.cpu()[:, :K].double() - ref).abs().max().item()
    assert err <= 2e-6 * ref.abs().max().item(), f"{name}: wgrad err {err:.3e}"
    assert torch.equal(dW.cpu()[:, 5], torch.zeros(256)) and torch.equal(dW.cpu()[:, K:], torch.zeros(256, ldw - K))
    assert (dW.cpu()[:, K:].view(torch.int32) == 0).all()                   # +0.0, bit for bit
    assert torch.equal(dW, again), "weight gradient not reproducible"
    assert int(status.item()) == 0
    dbr = G.double().sum(0)
    assert (db.cpu().double() - dbr).abs().max().item() <= 2e-6 * dbr.abs().max().item()
    # a column index >= K is left out of the CSC (and so of dW) and counted
    host_sp = SparseFeatures.from_dense(x)
    col = host_sp.col.clone()
    col[7] = K + 3
    bad = SparseFeatures(host_sp.rowptr, col, host_sp.val, host_sp.shape).to(DEV)
    colptr, row, val_t, st = ops.sparse_csc_build(bad)
    dW_bad = ops.sparse_linear_wgrad((colptr, row, val_t), N, G.to(DEV), out=torch.full((256, ldw), 3.0, device=DEV))
    r7 = int(torch.searchsorted(host_sp.rowptr.long(), torch.tensor(7), right=True)) - 1
    xd = x.double().clone()
    xd[r7, int(host_sp.col[7])] = 0.0
    ref_bad = G.double().T @ xd
    torch.cuda.synchronize()
    assert int(st.item()) == 1 and int(colptr[-1].item()) == host_sp.nnz - 1
    assert (dW_bad.cpu()[:, :K].double() - ref_bad).abs().max().item() <= 2e-6 * ref_bad.abs().max().item()
    with pytest.raises(ValueError):
        bad.csc()


class _RecordingMiner:
    """The hard-negative miner's result recorded by one run and replayed to another, so that the runs score the same edges (a top-k tie
    cannot decide the comparison)."""

    def __init__(self, fixed=None):
        from gnn_pretraining_amd.finetune import finetune as FT
        self.inner, self.fixed, self.got = FT.LinkPredictionHardNegativeMiner(), fixed, None

    def mine_hard_negatives_for_edges(self, node_embeddings, positive_edges, num_negatives, existing_edges):
        self.got = (self.inner.mine_hard_negatives_for_edges(node_embeddings, positive_edges, num_negatives, existing_edges)
                    if self.fixed is None else self.fixed)
        return self.got


def test_finetune_link_prediction_train_step_with_sparse_features():
    """One Cora_LP train step through FT.process_batch with sparse data.x: against the same step with dense x and against the oracle,
    on the edges the sparse run mined."""
    from gnn_pretraining_amd.data import data_setup as DS
    from gnn_pretraining_amd.data.finetune_data_loaders import LinkLoader, LinkPredictionDataset
    from gnn_pretraining_amd.finetune import finetune as FT
    gen = torch.Generator().manual_seed(78)
    torch.manual_seed(78)
    c = S.cora_like(gen, num_nodes=600, undirected_edges=1500)
    splits = DS.create_link_prediction_splits(c)
    om = OM.FinetuneGNN(torch.device("cpu"), "Cora_LP", "full_finetune")
    runs = {}
    for kind in ("sparse", "dense"):
        data = Batch.from_data_list([c])
        if kind == "sparse":
            data.x = SparseFeatures.from_dense(data.x)
        loader = LinkLoader(LinkPredictionDataset(data, splits, "train"), 256)
        hm = FinetuneGNN(torch.device("cpu"), "Cora_LP", "full_finetune")
        copy_state(hm, om); hm.device = DEV; hm.to(DEV)
        set_dropout(hm, 0.0); hm.train()
        miner = _RecordingMiner(None if kind == "sparse" else runs["sparse"][2])
        batch = next(iter(loader))
        train_edges = splits["train_pos"].to(DEV).contiguous()
        loss, targets, pred, prob = FT.process_batch(hm, batch, DEV, "link_prediction", "Cora_LP", miner, train_edges)
        loss.backward()
        assert targets.numel() == 512 and int(targets.sum()) == 256
        runs[kind] = (hm, loss.detach(), miner.got, batch)
    set_dropout(om, 0.0); om.train()
    with torch.no_grad():
        om.gnn_backbone(om.input_encoder(c.x), splits["train_pos"])
    all_edges = torch.cat([runs["sparse"][3][1], runs["sparse"][2].cpu()], dim=1)
    labels = torch.cat([torch.ones(256), torch.zeros(256)])
    lo = torch.nn.functional.binary_cross_entropy(om(to_oracle(Batch.from_data_list([c])), edge_index=all_edges,
                                                     message_passing_edges=splits["train_pos"]), labels)
    lo.backward()
    hs, hd = runs["sparse"][0], runs["dense"][0]
    assert_close(runs["sparse"][1], lo, OUT_RTOL, "sparse LP loss vs oracle")
    assert_close(runs["sparse"][1], runs["dense"][1], OUT_RTOL, "sparse LP loss vs dense")
    og, sg, dg = dict(om.named_parameters()), dict(hs.named_parameters()), dict(hd.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in og.values())
    for n, p in og.items():
        assert_grad_close(sg[n].grad, p.grad, gmax, f"grad {n} vs oracle")
        assert_grad_close(sg[n].grad, dg[n].grad, gmax, f"grad {n} vs dense")
    for (n, a), (_, o), (_, d) in zip(hs.named_buffers(), om.named_buffers(), hd.named_buffers()):
        assert_close(a, o, 1e-4, f"buffer {n} vs oracle")
        assert_close(a, d, 1e-4, f"buffer {n} vs dense")


def _planetoid(domain, gen):
    if domain == "Cora_NC":
        return S.cora_like(gen)
    return S.cora_like(gen, num_nodes=3327, undirected_edges=4552, dim=3703, density=0.0085, num_classes=6)


@pytest.mark.parametrize("domain", ["Cora_NC", "CiteSeer_NC"])
def test_sparse_node_engine_matches_the_oracle_step(domain):
    """test_gpu_modules.test_finetune_node_classification_engine_matches_the_oracle_step with sparse x: shared ReLU gates, tight gradients,
    relative update error, running statistics; then the module forward (sparse x, the engine's strided encoder weight) against the engine."""
    from gnn_pretraining_amd.finetune.engine import NodeClassificationEngine
    from oracle import gates as OGt
    gen = torch.Generator().manual_seed(34)
    torch.manual_seed(34)
    om = OM.FinetuneGNN(torch.device("cpu"), domain, "full_finetune")
    hm = FinetuneGNN(torch.device("cpu"), domain, "full_finetune")
    copy_state(hm, om); hm.device = DEV; hm.to(DEV)
    set_dropout(om, 0.0)
    om.train(); hm.train()
    c = _planetoid(domain, gen)
    idx = torch.randperm(c.num_nodes, generator=gen)[:140]
    eng = NodeClassificationEngine(hm, SparseFeatures.from_dense(c.x), c.edge_index, DEV, seed=3)
    assert eng.sparse and eng.x is None
    eng.dropout_p = 0.0
    keys_before = list(hm.state_dict().keys())
    oopt = torch.optim.AdamW(om.param_groups)
    for g in oopt.param_groups:
        g["lr"] *= 100
    eng.lr.mul_(100)
    before = {k: v.clone() for k, v in om.state_dict().items()}
    eng.step(idx.to(DEV), c.y[idx].to(DEV))
    torch.cuda.synchronize()
    masks = [(eng.h[0] > 0).cpu()]
    for l in range(5):
        masks += [(eng.r1[l] > 0).cpu(), (eng.h[l + 1] > 0).cpu()]
    tape = OGt.GateTape(masks)
    with OGt.use_tape(tape):
        lo = torch.nn.functional.cross_entropy(om(to_oracle(Batch.from_data_list([c])))[idx], c.y[idx])
    assert tape.done()
    oopt.zero_grad(); lo.backward(); oopt.step()
    assert abs(eng.loss() - lo.item()) <= 1e-4 * abs(lo.item())
    og = dict(om.named_parameters())
    gmax = max(p.grad.abs().max().item() for p in og.values())
    for n, p in og.items():
        if n.endswith("linear.bias") or n.endswith("gin_conv.nn.0.bias") or n.endswith("gin_conv.nn.3.bias"):
            assert eng.gradient(n).abs().max().item() <= 1e-4 * gmax and p.grad.abs().max().item() <= 1e-3 * gmax, n
        else:
            assert_grad_tight(eng.gradient(n), p.grad, gmax, f"grad {n}")
    o = eng.off["input_encoder.linear.weight"]                               # the slot's padding columns got a zero gradient
    assert (eng.final_grad[o:o + 256 * eng.dpad].view(256, eng.dpad)[:, eng.d_in:] == 0).all()
    eng.flush_counters()
    after_o, after_h = om.state_dict(), hm.state_dict()
    assert list(after_h.keys()) == keys_before
    num = den = 0.0
    for k, v in after_o.items():
        assert after_h[k].shape == v.shape, k
        if "running_" in k:
            assert_close(after_h[k], v, 1e-4, f"buffer {k}")
        elif k.endswith("num_batches_tracked"):
            assert int(after_h[k]) == int(v)
        elif k.endswith("linear.bias") or k.endswith("gin_conv.nn.0.bias") or k.endswith("gin_conv.nn.3.bias"):
            assert (after_h[k].cpu() - before[k]).abs().max().item() <= 1.01 * 100 * 1e-3
        else:
            num += ((after_h[k].cpu() - v).double() ** 2).sum().item()
            den += ((v - before[k]).double() ** 2).sum().item()
    assert (num / den) ** 0.5 <= 2e-2, f"relative update error {(num / den) ** 0.5:.3e}"
    eng.step(idx.to(DEV), c.y[idx].to(DEV))
    assert np.isfinite(eng.loss())
    hm.eval()
    b = Batch.from_data_list([c])
    b.x = SparseFeatures.from_dense(c.x)
    with torch.no_grad():
        logits_mod = hm(b.to(DEV))
    assert not hm.input_encoder.linear.weight.is_contiguous()
    logits_eng = eng.forward()
    torch.cuda.synchronize()
    assert_close(logits_mod, logits_eng.cpu(), 1e-4, "module forward (sparse x) on the engine's strided encoder weight")


def test_sparse_node_engine_graph_replay_fork_and_one_stream_are_bitwise_equal():
    from gnn_pretraining_amd.finetune.engine import NodeClassificationEngine
    gen = torch.Generator().manual_seed(36)
    c = S.cora_like(gen)
    sp = SparseFeatures.from_dense(c.x)
    idx = torch.randperm(c.num_nodes, generator=gen)[:140].to(DEV)
    y = c.y[idx.cpu()].to(DEV)
    outs = []
    for use_graph, fork in ((True, False), (False, True), (False, False)):
        torch.manual_seed(36)
        hm = FinetuneGNN(torch.device("cpu"), "Cora_NC", "full_finetune")
        hm.device = DEV; hm.to(DEV); hm.train()
        eng = NodeClassificationEngine(hm, sp, c.edge_index, DEV, seed=9)
        eng.use_graph, eng.fork_wgrads = use_graph, fork
        eng.lr.mul_(30)
        losses = []
        for k in range(5):
            eng.step(idx, y)
            losses.append(eng.loss())
        assert (eng._graph is not None) == use_graph
        eng.flush_counters()
        torch.cuda.synchronize()
        outs.append((eng.flat.clone(), eng.exp_avg.clone(), eng.exp_avg_sq.clone(), {k: v.clone() for k, v in hm.state_dict().items()}, losses, eng.step_count))
    a = outs[0]
    assert len(set(a[4])) == 5
    for b in outs[1:]:
        assert a[5] == b[5] == 5 and a[4] == b[4], (a[4], b[4])
        for i in range(3):
            assert torch.equal(a[i], b[i])
        for k in a[3]:
            assert torch.equal(a[3][k], b[3][k]), k


@pytest.mark.parametrize("domain", ["CiteSeer_NC", "Cora_LP"])
def test_finetune_end_to_end_with_sparse_features(tmp_path, monkeypatch, domain):
    from gnn_pretraining_amd.data.finetune_data_loaders import create_finetune_data_loader
    from gnn_pretraining_amd.finetune import finetune as FT
    monkeypatch.setattr(FT, "OUTPUT_DIR", tmp_path / "finetune")
    root = tmp_path / "data"
    cfg = FT.FinetuneConfig(domain, "full_finetune", "b1", 7, sparse_features=True)
    test = FT.finetune(cfg, epochs=3, data_root=str(root), data_scale=0.1)
    assert all(np.isfinite(v) for k, v in test.items() if isinstance(v, float)), test
    saved = torch.load(tmp_path / "finetune" / f"model_{cfg.exp_name}_7.pt", map_location=DEV, weights_only=True)["model_state_dict"]
    dense = FinetuneGNN(DEV, domain, "full_finetune")
    ref = dense.state_dict()
    assert list(saved.keys()) == list(ref.keys()) and all(saved[k].shape == ref[k].shape for k in ref)
    dense.load_state_dict(saved)
    sparse = FinetuneGNN(DEV, domain, "full_finetune")
    sparse.load_state_dict(saved)
    dense.eval(); sparse.eval()
    data = create_finetune_data_loader(domain, "test", -1, torch.Generator(), root).dataset.data
    bd = data.to(DEV)
    bs = Batch(SparseFeatures.from_dense(data.x), data.edge_index, data.batch, data.ptr, data.ptr_host, data.edge_ptr_host).to(DEV)
    mp = bd.edge_index
    with torch.no_grad():
        if domain.endswith("_NC"):
            ld, ls = dense(bd), sparse(bs)
        else:
            e = mp[:, :64].contiguous()
            ld, ls = dense(bd, edge_index=e, message_passing_edges=mp), sparse(bs, edge_index=e, message_passing_edges=mp)
    assert_close(ls, ld, 1e-4, f"{domain}: eval logits, sparse x vs dense x")
