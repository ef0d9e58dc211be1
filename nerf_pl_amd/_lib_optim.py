"""ctypes binding of the fused SGD / RAdam / Ranger steps
(include/nerf_pl_amd_optim.h).

The entry points live in the same ``libnerf_pl_amd.so`` as the render path but
are declared in their own header and bound by their own table, so the other
tables stay the images of their headers.  As there, nothing falls back: a
missing symbol or a failed call raises.
"""
from __future__ import annotations

import ctypes

from . import _lib

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_d = ctypes.c_double

# nr_radam_step's ``mode``
RECTIFIED, SGD_LIKE, SKIP = 0, 1, 2

# name -> argtypes; every entry returns int (0 = ok, or a count)
SIGNATURES = {
    "nr_optim_max_tensors": [],
    "nr_sgd_step": [_p, _p, _p, _p, _i, _d, _d, _d, _i, _p],
    "nr_radam_step": [_p, _p, _p, _p, _p, _p, _i, _d, _d, _d, _d, _d, _i64, _i, _d, _i, _p],
}
RESTYPES = {}

_bound = None


def lib():
    """The handle of ``_lib.lib()`` with the optimizer entry points typed."""
    global _bound
    if _bound is None:
        L = _lib.lib()
        for name, args in SIGNATURES.items():
            fn = getattr(L, name, None)
            if fn is None:          # reported by missing_symbols(); calling it raises
                continue
            fn.argtypes = args
            fn.restype = RESTYPES.get(name, _i)
        _bound = L
    return _bound


def missing_symbols() -> list:
    L = lib()
    return [n for n in SIGNATURES if getattr(L, n, None) is None]


def call(name: str, *args) -> None:
    rc = getattr(lib(), name)(*args)
    if rc != 0:
        raise RuntimeError(f"{name} failed (code {rc}): {_lib.last_error()}")
