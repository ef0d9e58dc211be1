"""ctypes binding of the camera-pose gradient (include/nerf_pl_amd_posegrad.h).

The entry point lives in the same ``libnerf_pl_amd.so`` as the render path but
is declared in its own header and bound by its own table, so the other tables
stay the images of their headers.  As there, nothing falls back: a missing
symbol or a failed call raises.
"""
from __future__ import annotations

import ctypes

from . import _lib

_p = ctypes.c_void_p
_i = ctypes.c_int
_i64 = ctypes.c_int64
_f = ctypes.c_float

# name -> argtypes; every entry returns int (0 = ok)
SIGNATURES = {
    "nr_gen_rays_posegrad": [_p, _i64, _i, _i, _f, _f, _f, _i, _f, _f, _f, _f, _p, _i64,
                             _p, _p, _p, _p],
}
RESTYPES = {}

_bound = None


def lib():
    """The handle of ``_lib.lib()`` with the pose-gradient entry point typed."""
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
