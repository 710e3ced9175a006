"""Host-side contract of gmp_gemm_f32, gmp_gemm_f32_grouped and gmp_colsum: every bad call is refused with GMP_ERR_ARG before anything is
enqueued, and the empty problems return GMP_OK without a launch -- so this runs without a GPU, on fake non-null pointers that the host
never dereferences (the pattern of test_lp_fused_host.py)."""
import pytest

import gemm_ref as R
from gnn_pretraining_amd import _lib as L

A, B, BIAS, CP, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
# per mode: the smallest legal (lda, ldb, ldc) of an M x N x K = 5 x 7 x 11 problem (TN: A is [K, M], B is [K, N])
M, N, K = 5, 7, 11
MIN_LD = {R.NT: (K, K, N), R.NN: (K, N, N), R.TN: (M, N, N)}


def single(mode=R.NT, a=A, b=B, c=CP, m=M, n=N, k=K, ld=None):
    lda, ldb, ldc = MIN_LD[mode] if ld is None else ld
    return R.gemm(mode, a, b, None, c, m, n, k, lda, ldb, ldc)


def grouped(mode=R.NT, a=A, b=B, bias=None, c=CP, rows=(0, 3, 9), n=N, k=K, m_tn=0, ld=None, groups=None, offs=True):
    if mode == R.TN and m_tn == 0:
        m_tn = M
    lda, ldb, ldc = MIN_LD[mode] if ld is None else ld
    rows = None if rows is None else list(rows)
    zeros = None if (rows is None or not offs) else [0] * (len(rows) - 1)
    return R.gemm_grouped(mode, a, b, bias, c, rows, zeros, zeros, zeros, None, None, m_tn, n, k, lda, ldb, ldc, groups=groups)


@pytest.mark.parametrize("mode", [-1, 3, 7])
def test_bad_mode_is_refused(mode):
    assert R.gemm(mode, A, B, None, CP, M, N, K, K, K, N) == R.ERR_ARG
    assert b"mode" in R.last_error()
    assert R.gemm_grouped(mode, A, B, None, CP, [0, 3], None, None, None, None, None, M, N, K, K, K, N) == R.ERR_ARG


@pytest.mark.parametrize("which", ["m", "n", "k"])
def test_negative_sizes_are_refused(which):
    assert single(**{which: -1}) == R.ERR_ARG
    assert b"negative" in R.last_error()


@pytest.mark.parametrize("mode", [R.NT, R.NN, R.TN])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_each_too_small_leading_dimension_is_refused(mode, which):
    ld = list(MIN_LD[mode])          # (the legal minimum itself would launch: not called here)
    ld[which] -= 1
    assert single(mode, ld=ld) == R.ERR_ARG
    assert b"leading dims" in R.last_error()


@pytest.mark.parametrize("mode", [R.NT, R.NN, R.TN])
def test_null_pointers_are_refused(mode):
    assert single(mode, c=None) == R.ERR_ARG
    assert single(mode, a=None) == R.ERR_ARG and single(mode, b=None) == R.ERR_ARG
    assert b"null" in R.last_error()


@pytest.mark.parametrize("mode", [R.NT, R.NN, R.TN])
def test_empty_outputs_return_ok_without_a_launch(mode):
    assert single(mode, m=0) == R.OK and single(mode, n=0) == R.OK
    assert single(mode, m=0, c=None) == R.OK             # (nothing is looked at beyond the sizes)
    assert R.gemm_workspace_bytes(mode, 0, N, K) == 0 and R.gemm_workspace_bytes(mode, M, 0, K) == 0 and R.gemm_workspace_bytes(mode, M, N, 0) == 0


@pytest.mark.parametrize("mode", [R.NT, R.NN, R.TN])
def test_grouped_group_counts_row_lists_and_sizes_are_refused(mode):
    assert grouped(mode, groups=0) == R.ERR_ARG
    assert b"groups" in R.last_error()
    assert grouped(mode, rows=list(range(26))) == R.ERR_ARG           # 25 groups: one more than GMP_MAX_GROUPS
    assert grouped(mode, rows=list(range(26)), offs=False) == R.ERR_ARG
    assert grouped(mode, rows=None, groups=2) == R.ERR_ARG            # NULL row list
    assert grouped(mode, rows=(0, 9, 3)) == R.ERR_ARG                 # descending
    assert b"ascending" in R.last_error()
    assert grouped(mode, rows=(-2, 3, 9)) == R.ERR_ARG
    assert grouped(mode, n=0) == R.ERR_ARG and grouped(mode, n=-3) == R.ERR_ARG
    assert grouped(mode, k=-1) == R.ERR_ARG
    for name in ("a", "b", "c"):
        assert grouped(mode, **{name: None}) == R.ERR_ARG


@pytest.mark.parametrize("mode", [R.NT, R.NN, R.TN])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_grouped_refuses_each_too_small_leading_dimension(mode, which):
    """the rules of the single form: NT lda, ldb >= K; NN lda >= K, ldb >= N; TN lda >= M_tn, ldb >= N; always ldc >= N"""
    ld = list(MIN_LD[mode])
    ld[which] -= 1
    assert grouped(mode, ld=ld) == R.ERR_ARG
    assert b"leading dims" in R.last_error()
    assert grouped(mode, ld=ld, offs=False) == R.ERR_ARG


def test_grouped_tn_refuses_a_bias_and_a_negative_output_height():
    assert grouped(R.TN, bias=BIAS) == R.ERR_ARG
    assert b"bias" in R.last_error()
    assert grouped(R.TN, m_tn=-1) == R.ERR_ARG


@pytest.mark.parametrize("mode", [R.NT, R.NN])
def test_grouped_with_every_group_empty_returns_ok_without_a_launch(mode):
    assert grouped(mode, rows=(4, 4, 4)) == R.OK
    assert grouped(mode, rows=(0, 0)) == R.OK


def test_colsum_refusals_and_empty_sizes():
    assert R.colsum(A, CP, 9, N, N - 1, ws=(WS, 1 << 20)) == R.ERR_ARG              # lda < N
    assert b"colsum" in R.last_error()
    assert R.colsum(A, CP, -1, N, N, ws=(WS, 1 << 20)) == R.ERR_ARG and R.colsum(A, CP, 9, -1, N, ws=(WS, 1 << 20)) == R.ERR_ARG
    assert R.colsum(A, CP, 9, 0, 0) == R.OK                                          # N == 0: nothing to do
    assert R.colsum(A, None, 9, N, N, ws=(WS, 1 << 20)) == R.ERR_ARG and R.colsum(None, CP, 9, N, N, ws=(WS, 1 << 20)) == R.ERR_ARG
    assert R.colsum(A, CP, 9, N, N) == R.ERR_WORKSPACE                               # no workspace
    need = L.lib().gmp_colsum_workspace_bytes(600, N)
    assert need == 3 * N * 4 and L.lib().gmp_colsum_workspace_bytes(0, N) == 0
    assert R.colsum(A, CP, 600, N, N, ws=(WS, need - 1)) == R.ERR_WORKSPACE
