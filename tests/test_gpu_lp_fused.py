"""The link-prediction head without its K x 768 matrices: the 768 -> 256 GEMM and the weight-gradient GEMM with the edge features generated
in their operand loaders (gmp_lp_feat_gemm_fwd / _wgrad) against gmp_lp_edge_features_fwd + gmp_gemm_f32 (NT) and gmp_gemm_f32_grouped (TN,
column-sum rider), and the input-gradient GEMM with the edge-feature fold in its epilogue (gmp_lp_feat_gemm_bwd_fold) against the
materialised path it replaces -- gmp_gemm_f32 (NN) into a K x 768 matrix, then gmp_lp_edge_features_bwd -- BIT FOR BIT: the fused kernel
keeps the GEMM's accumulation order and the fold's expressions, so torch.equal is the check and no tolerance is involved.

Shapes: F = 256 (the only width), 9 nodes, K just past the pipelined kernel's 1,024-row threshold so that both sides run it: whole 64-row
tiles (1024), one row in the last tile (1025), 63 rows in the last tile (1087), a half-filled last tile (1056)."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from gnn_pretraining_amd import _lib as L, ops                                    # noqa: E402

DEV = torch.device("cuda:0")
F, NODES = 256, 9


def reference(gy1, w0, h, edges):
    """the materialised path: gfeat = gy1 W0 through gmp_gemm_f32, folded by gmp_lp_edge_features_bwd"""
    gfeat = ops.gemm(ops.NN, gy1, w0)
    assert gfeat.shape == (gy1.size(0), 3 * F)
    return ops.lp_edge_features_bwd(gfeat, h, edges)


def operands(K, seed, edges=None):
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(NODES, F, generator=gen)
    h[3, ::5] = h[4, ::5]                      # equal entries in two different rows: |hs - hd| = 0 and sgn = 0 inside an ordinary pair
    gy1 = torch.randn(K, F, generator=gen)
    gy1[:, ::7] = 0.0                          # what the ReLU / dropout gate leaves behind: exact zeros (and -0.0 products) in the reduction
    w0 = torch.randn(F, 3 * F, generator=gen) * 0.05
    if edges is None:
        edges = torch.randint(0, NODES, (2, K), generator=gen)
    return gy1.to(DEV), w0.to(DEV), h.to(DEV), edges.to(DEV).contiguous()


def check(K, seed, edges=None):
    gy1, w0, h, e = operands(K, seed, edges)
    want_s, want_d = reference(gy1, w0, h, e)
    got_s, got_d = ops.lp_feat_gemm_bwd_fold(gy1, w0, h, e)
    torch.cuda.synchronize()
    assert torch.equal(got_s, want_s), f"K={K}: g_hs differs in {(got_s != want_s).sum().item()} elements, max {(got_s - want_s).abs().max().item():.3e}"
    assert torch.equal(got_d, want_d), f"K={K}: g_hd differs in {(got_d != want_d).sum().item()} elements, max {(got_d - want_d).abs().max().item():.3e}"
    assert got_s.abs().sum().item() > 0


@pytest.mark.parametrize("K", [1024, 1025, 1056, 1087])
def test_bwd_fold_equals_gemm_then_fold_bitwise(K):
    check(K, 100 + K)


@pytest.mark.parametrize("case", ["one_node", "src_eq_dst", "out_of_range"])
def test_bwd_fold_index_cases(case):
    K = 1025
    gen = torch.Generator().manual_seed(7)
    if case == "one_node":
        edges = torch.full((2, K), 5, dtype=torch.int64)
    elif case == "src_eq_dst":
        a = torch.randint(0, NODES, (K,), generator=gen)
        edges = torch.stack([a, a])
    else:
        edges = torch.randint(0, NODES, (2, K), generator=gen)
        edges[0, [0, 63, 64, 1024]] = -1          # read as zero rows, each endpoint on its own
        edges[1, [1, 63, 500, 1024]] = NODES
        edges[0, 700] = NODES
        edges[1, 700] = -1
    check(K, 11, edges)


# ---- the two GEMMs that read the features, with the features generated in their loaders ---------------------------------------------------
WS_SIZES = {"one_slice": 64, "many_slices": 32 * (F * 3 * F + F) * 4}          # bytes: no room for a second slice / room for the 32 the rule may pick


def fwd_operands(K, seed, edges=None):
    gen = torch.Generator().manual_seed(seed)
    h = torch.randn(NODES, F, generator=gen)
    h[3, ::5] = h[4, ::5]
    w0 = torch.randn(F, 3 * F, generator=gen) * 0.05
    b0 = torch.randn(F, generator=gen) * 0.1
    gy1 = torch.randn(K, F, generator=gen)
    gy1[:, ::7] = 0.0
    if edges is None:
        edges = torch.randint(0, NODES, (2, K), generator=gen)
    return h.to(DEV), w0.to(DEV), b0.to(DEV), gy1.to(DEV), edges.to(DEV).contiguous()


def reference_wgrad(gy1, feat, ws):
    """gmp_gemm_f32_grouped TN, one group, column-sum rider, the given workspace: the step's materialised weight-gradient call"""
    import ctypes as C
    K = gy1.size(0)
    dW0 = torch.empty(F, 3 * F, device=DEV)
    db0 = torch.empty(F, device=DEV)
    rows = (C.c_int32 * 2)(0, K)
    zero = (C.c_int64 * 1)(0)
    vp = lambda t: C.c_void_p(t.data_ptr())
    L.check(L.lib().gmp_gemm_f32_grouped(2, vp(gy1), vp(feat), None, vp(dW0), 1, rows, None, None, zero, vp(db0), zero, F, 3 * F, 0, F, 3 * F, 3 * F,
                                         1.0, 0, 0, vp(ws), ws.numel(), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "reference TN")
    return dW0, db0


def check_fwd_wgrad(K, seed, edges=None, ws_kinds=("one_slice", "many_slices")):
    h, w0, b0, gy1, e = fwd_operands(K, seed, edges)
    feat = ops.lp_edge_features_fwd(h, e)
    want_y1 = ops.gemm(ops.NT, feat, w0, b0, relu=True)          # w0 [256, 768]: the Linear weight, k-contiguous
    got_y1 = ops.lp_feat_gemm_fwd(h, e, w0, b0)
    torch.cuda.synchronize()
    assert torch.equal(got_y1, want_y1), f"K={K}: y1 differs in {(got_y1 != want_y1).sum().item()} elements, max {(got_y1 - want_y1).abs().max().item():.3e}"
    assert (got_y1 > 0).any() and (got_y1 == 0).any()
    for kind in ws_kinds:
        ws = torch.empty(WS_SIZES[kind], dtype=torch.uint8, device=DEV)
        want_w, want_b = reference_wgrad(gy1, feat, ws)
        got_w, got_b = ops.lp_feat_gemm_wgrad(gy1, h, e, ws)
        torch.cuda.synchronize()
        assert torch.equal(got_w, want_w), f"K={K} {kind}: dW0 differs in {(got_w != want_w).sum().item()} elements, max {(got_w - want_w).abs().max().item():.3e}"
        assert torch.equal(got_b, want_b), f"K={K} {kind}: db0 differs in {(got_b != want_b).sum().item()} elements"
        assert got_w.abs().sum().item() > 0


@pytest.mark.parametrize("K", [1024, 1025, 1056, 1087])
def test_generated_features_fwd_and_wgrad_equal_the_materialised_gemms_bitwise(K):
    """K = 1025: one row in the last row tile and a weight-gradient K-step tail of 1; 1087: 63 rows, tail 31; 1056: the reduction ends on a
    whole K-step; each weight gradient once with a workspace too small for a second row slice and once with room for every slice count"""
    check_fwd_wgrad(K, 200 + K)


@pytest.mark.parametrize("case", ["one_node", "src_eq_dst", "out_of_range"])
def test_generated_features_index_cases(case):
    K = 1025
    gen = torch.Generator().manual_seed(8)
    if case == "one_node":
        edges = torch.full((2, K), 5, dtype=torch.int64)
    elif case == "src_eq_dst":
        a = torch.randint(0, NODES, (K,), generator=gen)
        edges = torch.stack([a, a])
    else:
        edges = torch.randint(0, NODES, (2, K), generator=gen)
        edges[0, [0, 63, 64, 1024]] = -1
        edges[1, [1, 63, 500, 1024]] = NODES
        edges[0, 700] = NODES
        edges[1, 700] = -1
    check_fwd_wgrad(K, 12, edges)


def test_wgrad_without_a_workspace_is_refused():
    """without a workspace gmp_gemm_f32_grouped keeps the weight gradient off the pipelined kernel (another accumulation order): there is
    nothing bit-identical to be, the entry point says so and the step keeps the materialised sequence"""
    h, w0, b0, gy1, e = fwd_operands(1024, 5)
    with pytest.raises(L.GnnmpError):
        ops.lp_feat_gemm_wgrad(gy1, h, e, None)


def test_below_the_row_threshold_is_refused_without_a_launch():
    """K = 1000: gmp_gemm_f32 would not run the pipelined kernel there and the accumulation order would differ, so the entry point refuses
    (the step's fallback at such sizes is the "tiny" case of the engine test below)"""
    gy1, w0, h, e = operands(1000, 3)
    before = L.lib().gmp_lp_feat_gemm_launch_count()
    with pytest.raises(L.GnnmpError):
        ops.lp_feat_gemm_bwd_fold(gy1, w0, h, e)
    assert L.lib().gmp_lp_feat_gemm_launch_count() == before


def run_child(fused, mode, path):
    env = dict(os.environ, GMP_LP_FUSED=fused)
    child = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "lp_fused_child.py")
    r = subprocess.run([sys.executable, child, mode, path], env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return torch.load(path)


@pytest.mark.parametrize("mode,fused,launches", [("step", "1", 3), ("step", "2", 9), ("tiny", "2", 0)])
def test_engine_steps_bitwise_with_and_without_the_fused_head(tmp_path, mode, fused, launches):
    """three seeded s4 steps (PCGrad in a fixed task order, clip and AdamW included), one child process per setting of GMP_LP_FUSED: the
    flat parameters, task_grads and the five loss sums must not differ in a bit.
    GMP_LP_FUSED=1 (the default) folds the input gradient only, 2 generates the features in the forward and weight-gradient GEMMs too.
    "step": the 8-graph batches of tests/test_gpu_engine.py merge to thousands of link-prediction pairs; the fused child must have made
    one (level 1) or three (level 2) fused launches per step (counted by the library) and the other none -- a vacuous pass is a failure.
    "tiny": fewer than 1,024 pairs: both children must have taken the two-launch sequence, and agree."""
    a = run_child("0", mode, str(tmp_path / "mat.pt"))
    b = run_child(fused, mode, str(tmp_path / "fused.pt"))
    assert a["K"] == b["K"] and a["fused_launches"] == 0
    if mode == "step":
        assert min(a["K"]) >= 1024, f"merged link-prediction pairs per step {a['K']}: the fused path needs >= 1024"
        assert b["fused_launches"] == launches, f"{b['fused_launches']} fused launches in three steps at GMP_LP_FUSED={fused}"
    else:
        assert 0 < max(a["K"]) < 1024, f"merged link-prediction pairs per step {a['K']}: the fallback case needs fewer than 1024"
        assert b["fused_launches"] == launches == 0
    assert len(a["losses"]) == 5
    for k in ("loss_sums", "task_grads", "flat"):
        assert torch.equal(a[k], b[k]), f"{k}: {(a[k] != b[k]).sum().item()} elements differ"
    assert a["task_grads"].abs().sum().item() > 0
