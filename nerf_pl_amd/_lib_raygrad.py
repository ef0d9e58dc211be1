"""ctypes binding of the ray-gradient entry points (include/nerf_pl_amd_raygrad.h).

They live in the same ``libnerf_pl_amd.so`` as the render path but are declared
in their own header and bound by their own table, so ``_lib.SIGNATURES`` stays
the image of ``nerf_pl_amd.h``.  As there, nothing falls back: a missing symbol
or a failed call raises.
"""
from __future__ import annotations

import ctypes

from . import _lib

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_u64 = ctypes.c_uint64
_f = ctypes.c_float

# name -> argtypes; every entry returns int (0 = ok)
SIGNATURES = {
    "nr_raygrad_mlp": [_p, _p, _p, _p, _i64, _i, _i64, _i, _i, _p, _p, _p, _p],
    "nr_raygrad_reduce": [_p, _p, _i64, _i, _p, _p],
    "nr_composite_raygrad": [_p, _i, _i, _p, _p, _p, _f, _u64, _i, _i64, _i, _i,
                             _p, _p, _p, _p, _p, _p, _p, _p, _p],
    "nr_merge_raygrad": [_p, _p, _p, _i64, _i, _i, _p, _p],
    "nr_coarse_z_raygrad": [_p, _p, _i64, _i, _i, _f, _p, _u64, _p, _p, _p],
}
RESTYPES = {}

_bound = None


def lib():
    """The handle of ``_lib.lib()`` with the ray-gradient entry points typed."""
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
