"""The inference path: gmp_bn_fold, gmp_linear_affine_fwd (csrc/infer.hip + the affine epilogue of both GEMM families), the engines'
embed / predict (finetune/engine.py) and the --engine-eval loop (finetune/finetune.py).

Kernel bars are derived, not measured.  u = 2^-24 (half an ulp, relative).
  bn_fold        scale = fl(gamma / fl(sqrt(fl(var + eps)))): three correctly rounded operations, the first halved by the root: 2.5 u.
                 shift = fma(-scale, mean, beta): 2.5 u |scale mean| from the scale + one rounding.  Asserted: 4 u and 4 u (|beta| + |scale mean|).
  linear_affine  a K-term fp32 running sum is within K u sum|a_k w_k| of the exact one; bias, residual, scale and shift add one rounding
                 each (and scale / shift multiply what came before): (K + 6) u (|scale| (sum|a_k w_k| + |bias| + |residual|) + |shift|).

Engine bars are measured against the same float64 oracle (oracle/models.py, eval mode, double) on the same inputs and state: the new path
gets 4 x the error of the existing unfused eval forward (engine.forward() under model.eval(); evaluate() for graph classification), capped
by the project's 1e-4 relative bar for fp32 outputs.  Error = max |got - fp64| / max |fp64| per tensor.  Measured on MI355X:

  case                                   unfused eval forward    embed / predict
  Cora_NC dense, logits of 500 nodes     4.41e-07                5.05e-07
  Cora_NC dense, embeddings              6.74e-07                9.79e-07
  Cora_NC sparse, logits / embeddings    5.73e-07 / 8.46e-07     5.72e-07 / 9.43e-07
  Cora_LP, embeddings                    6.45e-07                5.86e-07   (probabilities of 600 pairs: 3.34e-07)
  ENZYMES B = 1 / 5 / 32, logits         0.77 / 1.55 / 1.29e-07  0.77 / 1.55 / 1.10e-07
  ENZYMES B = 1 / 5 / 32, embeddings     2.66 / 4.14 / 2.98e-07  2.07 / 1.97 / 2.67e-07
  PTC_MR B = 1 / 5 / 32, logits          1.36 / 1.36 / 2.09e-07  1.36 / 1.13 / 1.30e-07
  PTC_MR B = 1 / 5 / 32, embeddings      3.61 / 5.07 / 4.54e-07  2.31 / 1.65 / 1.87e-07
  bn_fold: worst scale error 1.93 u, worst shift error 2.20 u; linear_affine: worst error / derived bound 0.025 (256 -> 512), 0.013
  (512 -> 256), 0.004 (1,440 -> 256), 0.142 (32 -> 256), 0.130 (37 -> 256).
"""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from gnn_pretraining_amd import _lib as L, ops, synthetic as S                     # noqa: E402
from gnn_pretraining_amd.graph import Batch, SparseFeatures                        # noqa: E402
from gnn_pretraining_amd.models import FinetuneGNN                                 # noqa: E402
from oracle import models as OM                                                    # noqa: E402
from parity_util import copy_state, rel_err, to_oracle                             # noqa: E402

DEV = torch.device("cuda:0")
U = 2.0 ** -24
FP32_BAR = 1e-4
CLASSES = {"ENZYMES": 6, "PTC_MR": 2}
DIMS = {"ENZYMES": 21, "PTC_MR": 18}


# --------------------------------------------------------------------------- the fold table
def test_bn_fold_against_float64():
    gen = torch.Generator().manual_seed(5)
    chans = [256, 512, 256, 7, 512, 256, 512, 256, 512, 256, 512]               # eleven layers, one launch
    eps = 1e-5
    eps32 = float(np.float32(eps))
    layers = []
    for i, c in enumerate(chans):
        g, b, m = torch.randn(c, generator=gen), torch.randn(c, generator=gen), torch.randn(c, generator=gen) * 3
        v = torch.rand(c, generator=gen) * 2 + 0.01
        if i == 1:
            v[:8] = torch.tensor([0.0, 1e-30, 1e-12, 1e-8, 1e-6, 1e-5, 3e-5, 1e-4])      # tiny variances: eps decides
        if i == 2:
            v[:6] = torch.tensor([1e4, 1e6, 1e9, 1e12, 1e20, 1e30])                         # large ones
            m[:6] = torch.tensor([1e3, -1e3, 1e5, 0.0, 1e8, -1e10])
        if i == 3:
            b[:3] = 0.0                                                                     # shift = -scale * mean alone
        layers.append(tuple(t.to(DEV) for t in (g, b, m, v)))
    table, pairs = ops.bn_fold(layers, eps)
    assert table.numel() == 2 * sum(chans)
    worst_s = worst_h = 0.0
    for (g, b, m, v), (sc, sh) in zip(layers, pairs):
        g, b, m, v = (t.cpu().double() for t in (g, b, m, v))
        s64 = g / torch.sqrt(v + eps32)
        h64 = b - s64 * m
        es = ((sc.cpu().double() - s64).abs() / s64.abs().clamp_min(1e-300)).max().item()
        eh = ((sh.cpu().double() - h64).abs() / (b.abs() + (s64 * m).abs()).clamp_min(1e-300)).max().item()
        worst_s, worst_h = max(worst_s, es), max(worst_h, eh)
    print(f"bn_fold: worst scale error {worst_s / U:.2f} u, worst shift error {worst_h / U:.2f} u (|beta| + |scale mean|)")
    assert worst_s <= 4 * U and worst_h <= 4 * U
    table2, _ = ops.bn_fold(layers, eps)
    assert torch.equal(table.view(torch.int32), table2.view(torch.int32))
    # gamma / beta absent: 1 / 0
    _, ((sc, sh),) = ops.bn_fold([(None, None, layers[0][2], layers[0][3])], eps)
    s64 = 1.0 / torch.sqrt(layers[0][3].cpu().double() + eps32)
    assert ((sc.cpu().double() - s64).abs() / s64).max().item() <= 4 * U
    with pytest.raises(L.GnnmpError):
        ops.bn_fold([tuple(t.cpu() for t in layers[0])])
    with pytest.raises(L.GnnmpError):
        ops.linear_affine(torch.zeros(4, 8), torch.zeros(4, 8), None, torch.ones(4), torch.zeros(4))


# --------------------------------------------------------------------------- linear_affine against float64, every element
ROWS = [1, 31, 450, 1000, 1024, 2708, 7400, 70000]


@pytest.mark.parametrize("K,N", [(256, 512), (512, 256), (1440, 256), (32, 256), (37, 256)])
def test_linear_affine_against_float64(K, N):
    gen = torch.Generator().manual_seed(K * 1000 + N)
    w = (torch.randn(N, K, generator=gen) / K ** 0.5).to(DEV)
    bias, scale, shift = (torch.randn(N, generator=gen).to(DEV) for _ in range(3))           # negative scales among them
    assert (scale < 0).any() and (scale > 0).any()
    w64, b64, s64, h64 = w.double(), bias.double(), scale.double(), shift.double()
    SENT, PAD = -12345.0, 3
    worst = 0.0
    for M in ROWS:
        a = torch.randn(M, K, generator=gen).to(DEV)
        resid = torch.randn(M, N, generator=gen).to(DEV)
        a64, r64 = a.double(), resid.double()
        prod = a64 @ w64.T                                                                    # fp64 on the device: 70,000 x 1,440 x 256 on a CPU takes seconds
        mag = a64.abs() @ w64.abs().T
        for use_bias in (False, True):
            for use_res in (False, True):
                for relu in (False, True):
                    buf = torch.full((M + PAD, N), SENT, device=DEV)
                    out = ops.linear_affine(a, w, bias if use_bias else None, scale, shift, resid if use_res else None, relu, out=buf[:M])
                    v, inner = prod, mag
                    if use_bias:
                        v, inner = v + b64, inner + b64.abs()
                    if use_res:
                        v, inner = v + r64, inner + r64.abs()
                    v = v * s64 + h64
                    if relu:
                        v = torch.relu(v)
                    bound = (K + 6) * U * (s64.abs() * inner + h64.abs())
                    ratio = ((out.double() - v).abs() / bound).max().item()
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, f"M={M} K={K} N={N} bias={use_bias} residual={use_res} relu={relu}: error / bound = {ratio:.3f}"
                    assert (buf[M:] == SENT).all(), f"M={M}: rows beyond M were written"
                    buf2 = torch.full((M + PAD, N), SENT, device=DEV)
                    ops.linear_affine(a, w, bias if use_bias else None, scale, shift, resid if use_res else None, relu, out=buf2[:M])
                    assert torch.equal(buf.view(torch.int32), buf2.view(torch.int32)), f"M={M}: a second run differs"
        del a, resid, a64, r64, prod, mag
    print(f"linear_affine K={K} N={N}: worst error / derived bound {worst:.3f}")


def test_linear_affine_takes_the_engines_leading_dimensions():
    """Row-strided operands: A and W as [., 1433] views of K-padded [., 1440] buffers (the encoder), the residual and the output as views
    of wider buffers."""
    gen = torch.Generator().manual_seed(77)
    M, K, Kp, N = 2708, 1433, 1440, 256
    abuf, wbuf = torch.zeros(M, Kp), torch.zeros(N, Kp)
    abuf[:, :K], wbuf[:, :K] = torch.randn(M, K, generator=gen), torch.randn(N, K, generator=gen) / K ** 0.5
    abuf, wbuf = abuf.to(DEV), wbuf.to(DEV)
    bias, scale, shift = (torch.randn(N, generator=gen).to(DEV) for _ in range(3))
    rbuf, obuf = torch.randn(M, 2 * N, generator=gen).to(DEV), torch.full((M, 2 * N), 7.0, device=DEV)
    a, w, resid = abuf[:, :K], wbuf[:, :K], rbuf[:, N:]
    for A_, W_ in ((a, w), (abuf, wbuf)):                     # the unpadded views (generic loader) and the padded operands (pipelined kernel)
        out = ops.linear_affine(A_, W_, bias, scale, shift, resid, True, out=obuf[:, :N])
        v = torch.relu((abuf.double() @ wbuf.double().T + bias.double() + resid.double()) * scale.double() + shift.double())
        inner = abuf.double().abs() @ wbuf.double().abs().T + bias.double().abs() + resid.double().abs()
        bound = (Kp + 6) * U * (scale.double().abs() * inner + shift.double().abs())
        assert ((out.double() - v).abs() / bound).max().item() <= 1.0
        assert (obuf[:, N:] == 7.0).all()


@pytest.mark.parametrize("M,K,N,family", [(2708, 256, 512, "gemm_pipe_kernel"), (450, 256, 512, "gemm_kernel"), (450, 512, 256, "gemm_kernel, K-slices"),
                                          (1000, 37, 256, "gemm_kernel, generic loader")])
def test_identity_epilogue_equals_gemm_f32_bitwise(M, K, N, family):
    gen = torch.Generator().manual_seed(M + K)
    a, w, bias = torch.randn(M, K, generator=gen).to(DEV), (torch.randn(N, K, generator=gen) / K ** 0.5).to(DEV), torch.randn(N, generator=gen).to(DEV)
    one, zero = torch.ones(N, device=DEV), torch.zeros(N, device=DEV)
    for b in (bias, None):
        for relu in (True, False):
            want = ops.gemm(ops.NT, a, w, b, relu=relu)
            got = ops.linear_affine(a, w, b, one, zero, None, relu)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), f"{family}: bias={b is not None} relu={relu}"


@pytest.mark.parametrize("case", ["scale/shift offset by one float", "bias offset by one float", "residual with an odd leading dimension", "N % 4 != 0"])
def test_pipelined_kernel_scalar_affine_epilogue(case):
    """M >= 1,024 with an operand that is not 16-byte addressable: the pipelined kernel takes its scalar epilogue.  Against float64 under the
    derived bound, and bitwise against the float4 epilogue on aligned copies of the same operands."""
    gen = torch.Generator().manual_seed(len(case))
    M, K, N = 2708, 256, 512
    a = torch.randn(M, K, generator=gen).to(DEV)
    w = (torch.randn(N, K, generator=gen) / K ** 0.5).to(DEV)
    bias, scale, shift = (torch.randn(N, generator=gen).to(DEV) for _ in range(3))
    resid = torch.randn(M, N, generator=gen).to(DEV)
    aligned = ops.linear_affine(a, w, bias, scale, shift, resid, True)
    off = lambda t: torch.cat([torch.zeros(1, device=DEV), t])[1:]
    w2, bias2, scale2, shift2, resid2, cols = w, bias, scale, shift, resid, N
    if case.startswith("scale"):
        scale2, shift2 = off(scale), off(shift)
        assert scale2.data_ptr() % 16 == 4
    elif case.startswith("bias"):
        bias2 = off(bias)
    elif case.startswith("residual"):
        rbuf = torch.zeros(M, N + 1, device=DEV)
        rbuf[:, :N] = resid
        resid2 = rbuf[:, :N]
        assert resid2.stride(0) % 4 == 1
    else:
        cols = N - 2
        w2, bias2, scale2, shift2 = w[:cols], bias[:cols].clone(), scale[:cols].clone(), shift[:cols].clone()
        resid2 = resid[:, :cols]
    got = ops.linear_affine(a, w2, bias2, scale2, shift2, resid2, True)
    assert got.shape == (M, cols)
    assert torch.equal(got.view(torch.int32), aligned[:, :cols].contiguous().view(torch.int32)), case
    a64, w64 = a.double(), w.double()[:cols]
    inner = a64.abs() @ w64.abs().T + bias.double()[:cols].abs() + resid.double()[:, :cols].abs()
    v = torch.relu((a64 @ w64.T + bias.double()[:cols] + resid.double()[:, :cols]) * scale.double()[:cols] + shift.double()[:cols])
    bound = (K + 6) * U * (scale.double()[:cols].abs() * inner + shift.double()[:cols].abs())
    ratio = ((got.double() - v).abs() / bound).max().item()
    print(f"{case}: error / derived bound {ratio:.3f}")
    assert ratio <= 1.0


# --------------------------------------------------------------------------- engines against the float64 oracle
def _oracle64(hm, domain):
    om = OM.FinetuneGNN(torch.device("cpu"), domain, "full_finetune")
    copy_state(om, hm)
    om.double()
    om.eval()
    return om


def _bar(err_old):
    return min(4 * err_old, FP32_BAR)


def _node_setup(seed, sparse):
    from gnn_pretraining_amd.finetune.engine import NodeClassificationEngine
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    c = S.cora_like(gen)
    hm = FinetuneGNN(DEV, "Cora_NC", "full_finetune")
    hm.train()
    eng = NodeClassificationEngine(hm, SparseFeatures.from_dense(c.x) if sparse else c.x, c.edge_index, DEV, seed=seed)
    eng.lr.mul_(30)
    idx = torch.randperm(c.num_nodes, generator=gen)[:140].to(DEV)
    y = c.y[idx.cpu()].to(DEV)
    return gen, c, hm, eng, idx, y


def _oracle_batch64(c):
    ob = to_oracle(Batch.from_data_list([c]))
    ob.x = ob.x.double()
    return ob


@pytest.mark.parametrize("sparse", [False, True])
def test_node_predict_against_the_float64_oracle(sparse):
    gen, c, hm, eng, idx, y = _node_setup(101, sparse)
    for _ in range(3):
        eng.step(idx, y)
    eng.flush_counters()
    val = torch.randperm(c.num_nodes, generator=gen)[:500].to(DEV)
    yv = c.y[val.cpu()].to(DEV)
    assert hm.training
    got = eng.predict(val, yv).clone()                       # always eval mode, whatever model.training is
    loss = eng.loss()
    emb = eng.embed().clone()
    assert hm.training
    hm.eval()
    old = eng.forward()[val].clone()
    old_emb = eng.h[5].clone()
    hm.train()
    om = _oracle64(hm, "Cora_NC")
    with torch.no_grad():
        ob = _oracle_batch64(c)
        want_emb = om.gnn_backbone(om.input_encoder(ob.x), ob.edge_index)
        want = om.classification_head(want_emb)[val.cpu()]
        want_loss = torch.nn.functional.cross_entropy(want, yv.cpu()).item()
    e_old, e_new = rel_err(old, want), rel_err(got, want)
    ee_old, ee_new = rel_err(old_emb, want_emb), rel_err(emb, want_emb)
    print(f"Cora_NC sparse={sparse}: logits unfused {e_old:.3e} predict {e_new:.3e}; embeddings unfused {ee_old:.3e} embed {ee_new:.3e}; "
          f"loss {loss:.7f} fp64 {want_loss:.7f}")
    assert e_new <= _bar(e_old) and ee_new <= _bar(ee_old)
    assert abs(loss - want_loss) <= FP32_BAR * abs(want_loss)


def _lp_setup(seed):
    from gnn_pretraining_amd.data.data_setup import create_link_prediction_splits
    from gnn_pretraining_amd.finetune.engine import LinkPredictionEngine
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    c = S.cora_like(gen)
    train_pos = create_link_prediction_splits(c)["train_pos"].contiguous()
    hm = FinetuneGNN(DEV, "Cora_LP", "full_finetune")
    hm.train()
    eng = LinkPredictionEngine(hm, c.x, train_pos, DEV, seed=seed)
    eng.lr.mul_(30)
    return gen, c, train_pos, hm, eng


def _rand_pairs(gen, n, k):
    return torch.stack([torch.randint(0, n, (k,), generator=gen), torch.randint(0, n, (k,), generator=gen)])


def _lp_steps(eng, gen, c, train_pos, steps=3):
    for s in range(steps):
        eng.mining_forward()
        eng.step(train_pos[:, 256 * s:256 * (s + 1)].to(DEV), _rand_pairs(gen, c.num_nodes, 256).to(DEV))
    eng.flush_counters()


def test_link_prediction_predict_against_the_float64_oracle():
    gen, c, train_pos, hm, eng = _lp_setup(103)
    _lp_steps(eng, gen, c, train_pos)
    edges = torch.cat([train_pos[:, 1000:1300], _rand_pairs(gen, c.num_nodes, 300)], dim=1).contiguous()
    labels = torch.cat([torch.ones(300), torch.zeros(300)])
    assert hm.training
    emb = eng.embed()
    p1 = eng.predict(edges.to(DEV), labels.to(DEV), embeddings=emb).clone()          # one embedding, scored repeatedly
    loss = eng.loss()
    p2 = eng.predict(edges[:, :100].contiguous().to(DEV), embeddings=emb).clone()
    assert torch.equal(p1[:100], p2)
    p3 = eng.predict(edges.to(DEV)).clone()                                            # embeds itself
    assert torch.equal(p1, p3)
    emb = emb.clone()
    hm.eval()
    old_emb = eng.forward().clone()
    hm.train()
    om = _oracle64(hm, "Cora_LP")
    with torch.no_grad():
        ob = _oracle_batch64(c)
        want_emb = om.gnn_backbone(om.input_encoder(ob.x), train_pos)
        want = om.classification_head(want_emb, edges)
        want_loss = torch.nn.functional.binary_cross_entropy(want, labels.double()).item()
    ee_old, ee_new, e_p = rel_err(old_emb, want_emb), rel_err(emb, want_emb), rel_err(p1, want)
    print(f"Cora_LP: embeddings unfused {ee_old:.3e} embed {ee_new:.3e}; probabilities predict {e_p:.3e}; loss {loss:.7f} fp64 {want_loss:.7f}")
    assert ee_new <= _bar(ee_old) and e_p <= FP32_BAR
    assert abs(loss - want_loss) <= FP32_BAR * abs(want_loss)


def _gc_batch(gen, domain, graphs):
    mn, me = (33.0, 62.0) if domain == "ENZYMES" else (14.0, 15.0)
    return Batch.from_data_list([S.random_graph(gen, DIMS[domain], mn, me, num_classes=CLASSES[domain]) for _ in range(graphs)])


@pytest.mark.parametrize("domain", ["ENZYMES", "PTC_MR"])
def test_graph_classification_predict_against_the_float64_oracle(domain):
    from gnn_pretraining_amd.finetune.engine import GraphClassificationEngine
    gen = torch.Generator().manual_seed(105 + CLASSES[domain])
    torch.manual_seed(105)
    hm = FinetuneGNN(DEV, domain, "full_finetune")
    hm.train()
    eng = GraphClassificationEngine(hm, DEV, seed=3, max_nodes=300, max_edges=1200, max_graphs=8)
    eng.lr.mul_(30)
    for _ in range(3):
        eng.step(_gc_batch(gen, domain, 8).to(DEV))
    eng.flush_counters()
    om = _oracle64(hm, domain)
    cap0 = eng.cap_n
    for B in (1, 5, 32):                                     # 32 graphs: beyond the capacities, predict regrows as step does
        b = _gc_batch(gen, domain, B)
        assert hm.training
        got = eng.predict(b.to(DEV)).clone()
        loss = eng.loss()
        emb = eng.embed().clone()                            # the batch already loaded
        hm.eval()
        old = eng.evaluate(b.to(DEV)).clone()
        old_emb = eng.h[5][:b.num_nodes].clone()
        hm.train()
        with torch.no_grad():
            ob = to_oracle(b)
            ob.x = ob.x.double()
            want_emb = om.gnn_backbone(om.input_encoder(ob.x), ob.edge_index)
            want = om(ob)
            if CLASSES[domain] == 2:
                want_loss = torch.nn.functional.binary_cross_entropy_with_logits(want[:, 1], b.y.double()).item()
            else:
                want_loss = torch.nn.functional.cross_entropy(want, b.y).item()
        e_old, e_new, ee_old, ee_new = rel_err(old, want), rel_err(got, want), rel_err(old_emb, want_emb), rel_err(emb, want_emb)
        print(f"{domain} B={B} N={b.num_nodes}: logits evaluate {e_old:.3e} predict {e_new:.3e}; embeddings unfused {ee_old:.3e} embed {ee_new:.3e}; "
              f"loss {loss:.7f} fp64 {want_loss:.7f}")
        assert got.shape == (B, CLASSES[domain])
        assert e_new <= _bar(e_old) and ee_new <= _bar(ee_old)
        assert abs(loss - want_loss) <= FP32_BAR * abs(want_loss)
    assert eng.cap_n > cap0 and eng.cap_b >= 32
    b = _gc_batch(gen, domain, 4)
    b.y = None                                               # embeddings need no labels
    assert eng.embed(b.to(DEV)).shape == (b.num_nodes, 256)


def test_stale_embeddings_are_refused():
    gen, c, train_pos, hm, eng = _lp_setup(119)
    edges = _rand_pairs(gen, c.num_nodes, 64).to(DEV)
    emb = eng.embed()
    eng.predict(edges, embeddings=emb)
    eng.mining_forward()                                     # overwrites the buffer embed() returned
    with pytest.raises(ValueError, match="overwritten"):
        eng.predict(edges, embeddings=emb)
    emb = eng.embed()
    eng.step(train_pos[:, :256].to(DEV), _rand_pairs(gen, c.num_nodes, 256).to(DEV))
    with pytest.raises(ValueError, match="overwritten"):
        eng.predict(edges, embeddings=emb)
    with pytest.raises(ValueError, match="embed"):
        eng.predict(edges, embeddings=emb.clone())
    eng.predict(edges)                                       # embeds itself


def test_graph_classification_predict_without_labels():
    from gnn_pretraining_amd.finetune.engine import GraphClassificationEngine
    gen = torch.Generator().manual_seed(121)
    torch.manual_seed(121)
    hm = FinetuneGNN(DEV, "ENZYMES", "full_finetune")
    hm.train()
    eng = GraphClassificationEngine(hm, DEV, seed=3)
    b = _gc_batch(gen, "ENZYMES", 9)
    want = eng.predict(b.to(DEV)).clone()
    b.y = None
    got = eng.predict(b.to(DEV))
    assert torch.equal(got, want)
    with pytest.raises(L.GnnmpError, match="no labels"):
        eng.loss()
    eng.predict(_gc_batch(gen, "ENZYMES", 3).to(DEV))
    assert np.isfinite(eng.loss())


# --------------------------------------------------------------------------- side effects
def _snapshot(eng):
    eng.flush_counters()
    torch.cuda.synchronize()
    sd = {k: v.clone() for k, v in eng.model.state_dict().items() if "running_" in k or k.endswith("num_batches_tracked")}
    capture = dict(seed_word=eng.seed_word.clone(), graph=eng._graph) if hasattr(eng, "seed_word") else {}   # the node engine's alone
    return dict(flat=eng.flat.clone(), grad=eng.grad.clone(), final_grad=eng.final_grad.clone(), exp_avg=eng.exp_avg.clone(),
                exp_avg_sq=eng.exp_avg_sq.clone(), steps=eng.steps.clone(), buffers=sd, step_count=eng.step_count, bn_calls=eng._bn_calls, **capture)


def _assert_same(a, b, what):
    for k in a:
        if k == "buffers":
            assert a[k].keys() == b[k].keys()
            for n in a[k]:
                assert torch.equal(a[k][n], b[k][n]), f"{what}: {n}"
        elif isinstance(a[k], torch.Tensor):
            assert torch.equal(a[k].view(torch.int32) if a[k].dtype == torch.float32 else a[k], b[k].view(torch.int32) if b[k].dtype == torch.float32 else b[k]), f"{what}: {k}"
        else:
            assert a[k] is b[k] if k == "graph" else a[k] == b[k], f"{what}: {k}"


def test_predict_and_embed_leave_the_training_state_alone():
    gen, c, hm, eng, idx, y = _node_setup(107, False)
    for _ in range(2):
        eng.step(idx, y)
    before = _snapshot(eng)
    pending = eng._bn_calls
    eng.predict(idx, y); eng.embed(); eng.predict(idx[:17])
    assert eng._bn_calls == pending
    _assert_same(before, _snapshot(eng), "node engine")
    gen, c, train_pos, hm, eng = _lp_setup(109)
    _lp_steps(eng, gen, c, train_pos, 2)
    before = _snapshot(eng)
    eng.predict(_rand_pairs(gen, c.num_nodes, 700).to(DEV), torch.ones(700, device=DEV)); eng.embed()     # (700 pairs: beyond max_pairs)
    _assert_same(before, _snapshot(eng), "link-prediction engine")
    from gnn_pretraining_amd.finetune.engine import GraphClassificationEngine
    hm = FinetuneGNN(DEV, "PTC_MR", "full_finetune")
    hm.train()
    eng = GraphClassificationEngine(hm, DEV, seed=3, max_nodes=300, max_edges=1200, max_graphs=8)
    for _ in range(2):
        eng.step(_gc_batch(gen, "PTC_MR", 8).to(DEV))
    before = _snapshot(eng)
    eng.predict(_gc_batch(gen, "PTC_MR", 40).to(DEV)); eng.embed()
    _assert_same(before, _snapshot(eng), "graph-classification engine")


@pytest.mark.parametrize("graph", [False, True])
def test_a_step_after_predict_is_bitwise_the_step_without_it(graph, monkeypatch):
    """Two node engines from the same seed, dropout on: one calls predict / embed between its steps, the other does not.  Default (forked
    weight gradients) and GMP_FINETUNE_GRAPH=1 (the step captured at its second call and replayed at the third)."""
    if graph:
        monkeypatch.setenv("GMP_FINETUNE_GRAPH", "1")
    else:
        monkeypatch.delenv("GMP_FINETUNE_GRAPH", raising=False)
    snaps, losses = [], []
    for with_predict in (True, False):
        gen, c, hm, eng, idx, y = _node_setup(111, False)
        assert eng.use_graph == graph and eng.dropout_p > 0
        val = torch.arange(300, device=DEV)
        ls = []
        for _ in range(3):
            if with_predict:
                eng.predict(val, c.y[:300].to(DEV)); eng.embed()
            eng.step(idx, y)
            ls.append(eng.loss())
        if with_predict:
            eng.predict(val)
        assert (eng._graph is not None) == graph
        snaps.append(_snapshot(eng)); losses.append(ls)
    snaps[0].pop("graph"); snaps[1].pop("graph")
    _assert_same(snaps[0], snaps[1], "with / without predict")
    assert losses[0] == losses[1] and len(set(losses[0])) == 3


def test_lp_and_gc_steps_after_predict_are_bitwise_the_steps_without_it():
    from gnn_pretraining_amd.finetune.engine import GraphClassificationEngine
    snaps = []
    for with_predict in (True, False):
        gen, c, train_pos, hm, eng = _lp_setup(113)
        for s in range(3):
            neg = _rand_pairs(gen, c.num_nodes, 256).to(DEV)
            if with_predict:
                eng.predict(train_pos[:, :900].contiguous().to(DEV))
            eng.mining_forward()
            if with_predict:
                eng.embed()
            eng.step(train_pos[:, 256 * s:256 * (s + 1)].to(DEV), neg)
        snaps.append(_snapshot(eng))
    _assert_same(snaps[0], snaps[1], "link prediction with / without predict")
    snaps = []
    for with_predict in (True, False):
        gen = torch.Generator().manual_seed(115)
        torch.manual_seed(115)
        hm = FinetuneGNN(DEV, "ENZYMES", "full_finetune")
        hm.train()
        eng = GraphClassificationEngine(hm, DEV, seed=5, max_nodes=600, max_edges=2500, max_graphs=16)
        batches = [_gc_batch(gen, "ENZYMES", g).to(DEV) for g in (12, 5, 12, 40)]
        for s in range(3):
            if with_predict:
                eng.predict(batches[3] if s == 1 else batches[1])            # (the 40-graph batch regrows the buffers between two steps)
            eng.step(batches[s])
        snaps.append(_snapshot(eng))
    _assert_same(snaps[0], snaps[1], "graph classification with / without predict")


# --------------------------------------------------------------------------- freshness
def test_predict_reads_the_state_as_it_is_at_the_call():
    gen, c, hm, eng, idx, y = _node_setup(117, False)
    for _ in range(2):
        eng.step(idx, y)
    eng.flush_counters()
    val = torch.arange(400, device=DEV)
    saved = {k: v.clone() for k, v in hm.state_dict().items()}
    p0 = eng.predict(val).clone()

    def check(what):
        got = eng.predict(val).clone()
        om = _oracle64(hm, "Cora_NC")
        with torch.no_grad():
            want = om(_oracle_batch64(c))[val.cpu()]
        e = rel_err(got, want)
        print(f"freshness, {what}: predict vs fp64 on the new state {e:.3e}; moved by {rel_err(got, p0):.3e}")
        assert e <= FP32_BAR
        return got

    with torch.no_grad():
        hm.gnn_backbone.layers[2].batch_norm.running_mean.mul_(1.5).add_(0.1)                # in place
        hm.input_encoder.batch_norm.running_var.mul_(2.0)
    p1 = check("running statistics changed in place")
    assert rel_err(p1, p0) > 1e-3
    for _ in range(2):
        eng.step(idx, y)
    eng.flush_counters()
    p2 = check("two more steps")
    assert rel_err(p2, p1) > 1e-3
    hm.load_state_dict(saved)                                                                # the best checkpoint comes back
    p3 = check("load_state_dict")
    assert torch.equal(p3, p0)


# --------------------------------------------------------------------------- the loop
@pytest.fixture(scope="module")
def pretrained(tmp_path_factory):
    from gnn_pretraining_amd.pretrain import pretrain as PT
    root = tmp_path_factory.mktemp("infer_loop")
    old = PT.OUTPUT_DIR
    PT.OUTPUT_DIR = root / "pretrain"
    try:
        PT.pretrain(PT.PretrainConfig(exp_name="s4", seed=7), epochs=1, steps_per_epoch=3, data_root=str(root / "data"), data_scale=0.03)
    finally:
        PT.OUTPUT_DIR = old
    return root


def _auc_slack(y, p, tol):
    """Largest change of a one-vs-rest AUC when every score moves by at most tol: the share of (positive, negative) pairs whose scores
    are within 2 tol of each other (only those can change order)."""
    worst = 0.0
    for cls in range(p.shape[1]):
        pos, neg = p[y == cls, cls], p[y != cls, cls]
        if len(pos) and len(neg):
            worst = max(worst, float((np.abs(pos[:, None] - neg[None, :]) <= 2 * tol).mean()))
    return worst


@pytest.mark.parametrize("domain,kw", [("Cora_NC", {}), ("Cora_LP", {"lp_engine": True}), ("PTC_MR", {"gc_engine": True})])
def test_finetune_loop_with_engine_eval(domain, kw, pretrained, monkeypatch):
    """finetune() for two epochs on scaled-down synthetic data, engine_eval against the module evaluation from the same seed.  Training is
    bitwise the same in both runs (the tests above), so the two evaluations see the same state and differ by fp32 rounding alone.

    Tolerance.  Both paths hold their logits within 1e-4 max|logit| of fp64 (the predict tests above; the module's own tests), so two
    logit vectors differ by at most d = 2e-4 * Lmax, Lmax = the largest |logit| difference the recorded probabilities show (a softmax
    fixes logits up to a shift; for the sigmoid Lmax = max |logit|).  Softmax and sigmoid move by at most d / 2 per unit of logit
    difference 2 d: every probability is within tol_p = d.  Then
      loss        mean CE / BCE is 2-Lipschitz in the logits' max-norm: 2 d
      accuracy    only samples whose decision margin (top-two gap, or |p - 0.5|) is within 2 tol_p can flip: k of n samples, k / n
      f1, precision, recall   ratios of counts that each move by at most k: 2 k / (m - k), m = the smallest per-class count, true or predicted
      auc         only (positive, negative) pairs with scores within 2 tol_p of each other can change order: their share (_auc_slack)
    and the selected epoch must agree whenever the two epochs' selection metrics are further apart than that metric's tolerance."""
    from gnn_pretraining_amd.finetune import finetune as FT
    from gnn_pretraining_amd.models import finetune_model as FM
    monkeypatch.delenv("GMP_FINETUNE_ENGINE", raising=False)
    monkeypatch.setattr(FM, "PRETRAIN_OUTPUT_DIR", pretrained / "pretrain")
    monkeypatch.setattr(FM.load_pretrained_weights, "__defaults__", (pretrained / "pretrain",))
    real_batch, real_val = FT.compute_batch_metrics, FT.compute_validation_metrics
    runs = []
    for engine_eval in (True, False):
        monkeypatch.setattr(FT, "OUTPUT_DIR", pretrained / f"finetune_{domain}_{int(engine_eval)}")
        rec = {"batches": [], "val": []}

        def batch_metrics(domain_name, targets, predictions, probabilities, loss, prefix, rec=rec):
            m = real_batch(domain_name, targets, predictions, probabilities, loss, prefix)
            rec["batches"].append((prefix, targets.cpu().numpy(), probabilities.detach().cpu().double().numpy(), m))
            return m

        def val_metrics(batch_metrics_, epoch, rec=rec):
            v = real_val(batch_metrics_, epoch)
            rec["val"].append(v)
            return v

        monkeypatch.setattr(FT, "compute_batch_metrics", batch_metrics)
        monkeypatch.setattr(FT, "compute_validation_metrics", val_metrics)
        test = FT.finetune(FT.FinetuneConfig(domain, "full_finetune", "s4", 7, engine_eval=engine_eval, **kw), epochs=2,
                           data_root=str(pretrained / "data"), data_scale=0.1)
        runs.append((test, rec))
    (test_e, rec_e), (test_m, rec_m) = runs
    skip = {"test/training_time"}
    assert test_e.keys() == test_m.keys()
    assert len(rec_e["val"]) == len(rec_m["val"]) == 2 and all(a.keys() == b.keys() for a, b in zip(rec_e["val"], rec_m["val"]))
    assert len(rec_e["batches"]) == len(rec_m["batches"]) > 0
    key = "val/auc" if domain == "Cora_LP" else "val/accuracy"
    tols = {}                                                 # metric name -> tolerance, the worst over the batches that feed it
    for (pre_e, y_e, p_e, m_e), (pre_m, y_m, p_m, m_m) in zip(rec_e["batches"], rec_m["batches"]):
        assert pre_e == pre_m and np.array_equal(y_e, y_m) and m_e.keys() == m_m.keys()
        logp = np.log(np.clip(np.concatenate([p_e, p_m]), 1e-300, None))
        lmax = float((logp.max(axis=1) - logp.min(axis=1)).max())
        d = 2e-4 * max(lmax, 1.0)
        dp = float(np.abs(p_e - p_m).max())
        print(f"{domain} {pre_e} batch of {len(y_e)}: max |p_engine - p_module| = {dp:.3e}, tol_p = {d:.3e}")
        assert dp <= d
        top = np.sort(np.minimum(p_e, p_m), axis=1)
        k = int(((top[:, -1] - top[:, -2]) <= 2 * d).sum()) if p_e.shape[1] > 2 else int((np.abs(np.minimum(p_e[:, 1], p_m[:, 1]) - 0.5) <= 2 * d).sum())
        n = len(y_e)
        counts = []
        for cls in ([1] if p_e.shape[1] == 2 else range(p_e.shape[1])):
            counts += [int((y_e == cls).sum()), int((p_e.argmax(axis=1) == cls).sum()), int((p_m.argmax(axis=1) == cls).sum())]
        m_small = max(min(counts) - k, 1)
        t = {"loss": 2 * d, "accuracy": k / n, "f1": 2 * k / m_small, "precision": 2 * k / m_small, "recall": 2 * k / m_small,
             "auc": max(_auc_slack(y_e, p_e, d), _auc_slack(y_m, p_m, d))}
        for name, tol in t.items():
            tols[f"{pre_e}/{name}"] = max(tols.get(f"{pre_e}/{name}", 0.0), tol + 1e-12)
            assert abs(m_e[f"{pre_e}/{name}"] - m_m[f"{pre_e}/{name}"]) <= tol + 1e-12, (pre_e, name, m_e[f"{pre_e}/{name}"], m_m[f"{pre_e}/{name}"], tol)
    for ve, vm in zip(rec_e["val"], rec_m["val"]):
        for name in ve:
            assert abs(ve[name] - vm[name]) <= tols[name], (name, ve[name], vm[name], tols[name])
    for name in test_e:
        if name in tols:
            assert abs(test_e[name] - test_m[name]) <= tols[name], (name, test_e[name], test_m[name], tols[name])
        elif name not in skip:
            if name != "test/convergence_epochs":
                assert test_e[name] == test_m[name], name
    gap = min(abs(r["val"][0][key] - r["val"][1][key]) for r in (rec_e, rec_m))
    print(f"{domain}: {key} per epoch engine {[v[key] for v in rec_e['val']]} module {[v[key] for v in rec_m['val']]}, tolerance {tols[key]:.3e}")
    if gap > 2 * tols[key]:
        assert test_e["test/convergence_epochs"] == test_m["test/convergence_epochs"]


def test_engine_eval_without_an_engine_raises_in_the_loop(monkeypatch):
    from gnn_pretraining_amd.finetune import finetune as FT
    monkeypatch.setenv("GMP_FINETUNE_ENGINE", "0")
    with pytest.raises(ValueError, match="engine_eval needs an active fine-tune engine"):
        FT.FinetuneConfig("Cora_NC", "full_finetune", "s4", 1, engine_eval=True)
