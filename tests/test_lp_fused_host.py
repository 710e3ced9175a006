"""Host-side contract of gmp_lp_feat_gemm_bwd_fold: declared, bound, exported, and every bad call is refused with its error code before
anything is launched (so this runs without a GPU)."""
import ctypes

import pytest

from gnn_pretraining_amd import _lib as L

ERR_ARG, ERR_UNSUPPORTED = -1, -4


def call(gy1=0x1000, w0=0x2000, h=0x3000, edges=0x4000, ghs=0x5000, ghd=0x6000, n=9, k=2048, f=256):
    """the pointers are never dereferenced by the host and nothing is launched on a refused call"""
    vp = ctypes.c_void_p
    return L.lib().gmp_lp_feat_gemm_bwd_fold(vp(gy1), vp(w0), vp(h), vp(edges), vp(ghs), vp(ghd), n, k, f, None)


@pytest.mark.parametrize("f", [0, 128, 252, 512])
def test_other_feature_widths_are_unsupported(f):
    assert call(f=f) == ERR_UNSUPPORTED
    assert b"256" in L.lib().gmp_last_error_string()


@pytest.mark.parametrize("k", [-1, 0, 1, 1023])
def test_row_counts_below_the_pipelined_kernels_threshold_are_refused(k):
    assert call(k=k) == ERR_ARG


@pytest.mark.parametrize("which", ["gy1", "w0", "h", "ghs", "ghd"])
def test_misaligned_and_null_float_operands_are_refused(which):
    assert call(**{which: 0x1004}) == ERR_ARG
    assert b"aligned" in L.lib().gmp_last_error_string()
    assert call(**{which: 0}) == ERR_ARG


def test_fwd_and_wgrad_refuse_bad_calls_without_launching():
    vp, lib = ctypes.c_void_p, L.lib()
    fwd = lambda h=0x1000, e=0x2000, w=0x3000, b=0x4000, y=0x5000, k=2048, f=256: lib.gmp_lp_feat_gemm_fwd(vp(h), vp(e), vp(w), vp(b), vp(y), 9, k, f, None)
    wg = lambda g=0x1000, h=0x2000, e=0x3000, w=0x4000, b=0x5000, k=2048, f=256, ws=0x6000: lib.gmp_lp_feat_gemm_wgrad(vp(g), vp(h), vp(e), vp(w), vp(b), 9, k, f, vp(ws), 1 << 20, None)
    assert fwd(f=128) == ERR_UNSUPPORTED and wg(f=128) == ERR_UNSUPPORTED
    for k in (0, 1023):
        assert fwd(k=k) == ERR_ARG and wg(k=k) == ERR_ARG
    for name in ("h", "w", "b", "y"):
        assert fwd(**{name: 0x1004}) == ERR_ARG and fwd(**{name: 0}) == ERR_ARG
    for name in ("g", "h", "w"):
        assert wg(**{name: 0x1004}) == ERR_ARG and wg(**{name: 0}) == ERR_ARG
    assert fwd(e=0) == ERR_ARG and wg(e=0) == ERR_ARG
    assert wg(ws=0) == -3          # GMP_ERR_WORKSPACE


def test_null_edges_and_negative_node_count_are_refused():
    assert call(edges=0) == ERR_ARG
    assert call(n=-1) == ERR_ARG
