"""Host-side contract of the streaming NT-Xent: the C ABI is declared, bound and exported, the public operator takes `impl`,
and the workspace grows linearly with n (the matrix form's grows quadratically)."""
import inspect
import re
from pathlib import Path

import pytest
import torch

from gnn_pretraining_amd import _lib as L, operators as O, ops

ROOT = Path(__file__).resolve().parents[1]


def test_stream_symbols_are_declared_bound_and_exported():
    # same argument lists as the matrix form
    assert L._SIGS["gmp_nt_xent_stream_fwd"] == L._SIGS["gmp_nt_xent_fwd"]
    assert L._SIGS["gmp_nt_xent_stream_bwd"] == L._SIGS["gmp_nt_xent_bwd"]
    assert hasattr(ops, "nt_xent_stream_fwd") and hasattr(ops, "nt_xent_stream_bwd")


def test_operator_takes_impl_and_rejects_unknown_values():
    sig = inspect.signature(O.nt_xent)
    assert sig.parameters["impl"].default == "auto"
    z = torch.zeros(4, 8)
    with pytest.raises(ValueError, match="impl"):
        O.nt_xent(z, z, 0.5, impl="flash")


def test_workspace_is_an_eighth_of_the_matrix_forms_at_the_old_limit():
    lib = L.lib()
    assert lib.gmp_nt_xent_stream_workspace_bytes(8192, 128) * 8 <= lib.gmp_nt_xent_workspace_bytes(8192, 128)


@pytest.mark.parametrize("n", [4096, 16384, 65536])
def test_workspace_is_linear_in_n(n):
    ws = L.lib().gmp_nt_xent_stream_workspace_bytes
    assert ws(n, 128) >= 2 * n * 128 * 4                 # at least the normalised rows
    assert ws(2 * n, 128) <= 2.1 * ws(n, 128)


def test_workspace_of_a_problem_beyond_the_matrix_form():
    lib = L.lib()
    assert lib.gmp_nt_xent_workspace_bytes(32768, 128) > 16 * 2**30      # the matrix alone
    assert 0 < lib.gmp_nt_xent_stream_workspace_bytes(32768, 128) < 2**30
    assert lib.gmp_nt_xent_stream_workspace_bytes(0, 128) == 0
    assert lib.gmp_nt_xent_stream_workspace_bytes(2**30, 128) == 0        # 2n rows no longer index as int32


def test_stream_kernel_source_uses_the_f32_mfma_and_no_float_atomics():
    csrc = ROOT / "gnn_pretraining_amd" / "csrc"                   # the file, the tile core and the helpers it is built on
    src = "".join((csrc / f).read_text() for f in ("ntxent_stream.hip", "sim_tile.h", "gnnmp_internal.h", "ntxent.hip"))
    assert "mfma_f32_32x32x2f32" in src
    assert not re.search(r"atomicAdd|__hip_atomic|unsafeAtomic", src)
