"""Host-side checks of the inference path (no GPU): the BatchNorm fold formula against torch.nn.BatchNorm1d.eval() in float64, the
--engine-eval flag and its precondition, and the declaration / binding of the two new C-ABI entry points."""
import pytest
import torch

from gnn_pretraining_amd import _lib as L
from gnn_pretraining_amd.finetune import finetune as FT


def fold64(gamma, beta, mean, var, eps):
    """The float64 twin of gmp_bn_fold: scale = gamma / sqrt(var + eps), shift = beta - scale * mean."""
    scale = gamma / torch.sqrt(var + eps)
    return scale, beta - scale * mean


def linear_affine64(a, w, bias, resid, scale, shift, relu):
    """The float64 twin of gmp_linear_affine_fwd: act(((a w^T + bias) + resid) * scale + shift), in that order."""
    v = a @ w.T
    if bias is not None:
        v = v + bias
    if resid is not None:
        v = v + resid
    v = v * scale + shift
    return torch.relu(v) if relu else v


@pytest.mark.parametrize("with_residual", [False, True])
@pytest.mark.parametrize("K,N", [(256, 512), (512, 256), (37, 256)])
def test_fold_composed_with_a_linear_equals_batchnorm_eval_in_float64(with_residual, K, N):
    gen = torch.Generator().manual_seed(K + N + int(with_residual))
    M = 97
    lin = torch.nn.Linear(K, N).double()
    bn = torch.nn.BatchNorm1d(N).double()
    with torch.no_grad():
        bn.weight.copy_(torch.randn(N, generator=gen, dtype=torch.float64))            # negative scales among them
        bn.bias.copy_(torch.randn(N, generator=gen, dtype=torch.float64))
        bn.running_mean.copy_(torch.randn(N, generator=gen, dtype=torch.float64))
        bn.running_var.copy_(torch.rand(N, generator=gen, dtype=torch.float64) * 4 + 1e-3)
    bn.eval()
    a = torch.randn(M, K, generator=gen, dtype=torch.float64)
    resid = torch.randn(M, N, generator=gen, dtype=torch.float64) if with_residual else None
    with torch.no_grad():
        u = lin(a)
        want = torch.relu(bn(u + resid if with_residual else u))
        scale, shift = fold64(bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
        got = linear_affine64(a, lin.weight, lin.bias, resid, scale, shift, True)
    err = (got - want).abs().max().item() / want.abs().max().item()
    print(f"K={K} N={N} residual={with_residual}: max rel err {err:.3e}")
    assert err <= 1e-12


def test_engine_eval_flag_parses_into_the_config(monkeypatch):
    monkeypatch.delenv("GMP_FINETUNE_ENGINE", raising=False)
    base = ["--finetune_strategy", "full_finetune", "--pretrained_scheme", "s4", "--seed", "1"]
    a = FT.build_parser().parse_args(["--domain_name", "Cora_NC", "--engine-eval"] + base)
    assert FT.config_from_args(a).engine_eval is True
    a = FT.build_parser().parse_args(["--domain_name", "Cora_NC"] + base)
    assert FT.config_from_args(a).engine_eval is False                               # opt-in
    a = FT.build_parser().parse_args(["--domain_name", "Cora_LP", "--lp-engine", "--engine-eval"] + base)
    cfg = FT.config_from_args(a)
    assert cfg.engine_eval and cfg.lp_engine
    a = FT.build_parser().parse_args(["--domain_name", "PTC_MR", "--gc-engine", "--engine-eval"] + base)
    cfg = FT.config_from_args(a)
    assert cfg.engine_eval and cfg.gc_engine


def test_engine_eval_without_an_engine_raises(monkeypatch):
    monkeypatch.delenv("GMP_FINETUNE_ENGINE", raising=False)
    with pytest.raises(ValueError, match="engine_eval needs an active fine-tune engine"):
        FT.FinetuneConfig("Cora_LP", "full_finetune", "s4", 1, engine_eval=True)
    with pytest.raises(ValueError, match="engine_eval needs an active fine-tune engine"):
        FT.FinetuneConfig("ENZYMES", "full_finetune", "s4", 1, engine_eval=True)
    assert FT.FinetuneConfig("Cora_NC", "full_finetune", "s4", 1, engine_eval=True).engine_eval       # the node engine is on by default
    monkeypatch.setenv("GMP_FINETUNE_ENGINE", "0")
    with pytest.raises(ValueError, match="engine_eval needs an active fine-tune engine"):
        FT.FinetuneConfig("Cora_NC", "full_finetune", "s4", 1, engine_eval=True)
    assert FT.FinetuneConfig("Cora_NC", "full_finetune", "s4", 1).engine_eval is False                # without the flag nothing changes


def test_new_symbols_are_declared_and_bound():
    """gmp_bn_fold and gmp_linear_affine_fwd are in test_layout.FEATURE_SYMBOLS; the folded forward runs on this GEMM signature."""
    assert L._SIGS["gmp_gemm_f32"][1] == [L.i32, L.p, L.p, L.p, L.p, L.i64, L.i64, L.i64, L.i64, L.i64, L.i64, L.f32, L.i32, L.i32, L.p, L.sz, L.p]
