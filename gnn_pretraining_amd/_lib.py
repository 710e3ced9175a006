"""ctypes binding of libgnnmp.so.  Every prototype, struct and constant is read from include/gnnmp.h and
include/gnnmp_step.h by _abi.py: to bind something new, declare it in the header.

The product path has NO fallback: if the shared library is missing or a symbol
is absent this module raises, and every operator in the package goes through it.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Dict, List

from ._abi import HEADER_PATH, STEP_HEADER_PATH, GnnmpError, load  # noqa: F401  (re-exported)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libgnnmp.so")

ABI = load()                    # constants, structs and prototypes of include/gnnmp.h and include/gnnmp_step.h
K: Dict[str, int] = ABI.constants
_SIGS: Dict[str, tuple] = ABI.functions     # name -> (restype, [argtypes])

OK = K["GMP_OK"]
p, i64, i32, f32, sz = C.c_void_p, C.c_int64, C.c_int, C.c_float, C.c_size_t
BnConfig, AugMasksJob, AugViewsJob, AugNegJob = (ABI.structs["gmp_" + n] for n in ("bn_config", "aug_masks_job", "aug_views_job", "aug_neg_job"))
SURGERY_RULES = {"reference": K["GMP_SURGERY_REFERENCE"], "pcgrad": K["GMP_SURGERY_PCGRAD"], "mean": K["GMP_SURGERY_MEAN"]}
SURGERY_SCOPES = {"tensor": K["GMP_SURGERY_SCOPE_TENSOR"], "model": K["GMP_SURGERY_SCOPE_MODEL"]}


def declared_symbols() -> List[str]:
    """Every function name declared in include/gnnmp.h and include/gnnmp_step.h (used by the export test)."""
    return sorted(_SIGS)


_lib = None


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise GnnmpError(
                f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C gnn_pretraining_amd/csrc`). There is no CPU fallback.")
        _lib = C.CDLL(LIB_PATH)
        _declare(_lib)
    return _lib


def _declare(l: C.CDLL) -> None:
    missing = [s for s in _SIGS if not hasattr(l, s)]
    if missing:
        raise GnnmpError(f"libgnnmp.so lacks symbols declared in gnnmp.h: {missing}")
    for name, (res, args) in _SIGS.items():
        fn = getattr(l, name)
        fn.restype = res
        fn.argtypes = args
    desc = ABI.structs["gmp_step_desc"]
    if l.gmp_step_desc_size() != C.sizeof(desc):
        raise GnnmpError(f"gnnmp_step.h and libgnnmp.so disagree: sizeof(gmp_step_desc) = {l.gmp_step_desc_size()} in the library "
                         f"but {C.sizeof(desc)} bytes by the header: rebuild the library")


def check(rc: int, what: str) -> None:
    if rc != OK:
        msg = lib().gmp_last_error_string()
        raise GnnmpError(f"{what} failed with code {rc}: {msg.decode() if msg else ''}")
