"""CPU-side checks of the camera-pose gradient's entry point
(include/nerf_pl_amd_posegrad.h, nerf_pl_amd/_lib_posegrad.py): the header, the
ctypes table and the library agree symbol by symbol and argument by argument,
the new name collides with none of the four existing tables, and the entry
point validates sizes, pointers and alignment before it touches the device
(NR_EINVAL with its own name in the message)."""
import ctypes
import os
import re

import pytest

from conftest import REPO

NR_EINVAL = 10001
N = None          # null pointer
P = 0x10000       # a non-null, 16-byte aligned (never dereferenced) device address
ODD = 0x10004     # ... and one that is 4- but not 16-byte aligned
NAME = "nr_gen_rays_posegrad"

_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double}


def _header_prototypes():
    """name -> (return ctype, [argument ctypes]); any pointer is a c_void_p"""
    txt = open(os.path.join(REPO, "include", "nerf_pl_amd_posegrad.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)

    def ctype(decl):
        if "*" in decl:
            return ctypes.c_void_p
        return _CTYPES[[w for w in decl.split() if w != "const"][0]]

    protos = {}
    for ret, name, args in re.findall(r"\b(\w+[\s\*]+)(nr_\w+)\s*\(([^)]*)\)\s*;", txt):
        assert name not in protos, name
        protos[name] = (ctype(ret), [ctype(a) for a in args.split(",")])
    return protos


def test_header_table_and_library_agree():
    from nerf_pl_amd import _lib, _lib_mesh, _lib_mesh_normals, _lib_posegrad, _lib_raygrad
    protos = _header_prototypes()
    assert set(protos) == {NAME}
    assert set(protos) == set(_lib_posegrad.SIGNATURES)
    bad = {n: (ret, args) for n, (ret, args) in protos.items()
           if args != list(_lib_posegrad.SIGNATURES[n])
           or ret != _lib_posegrad.RESTYPES.get(n, ctypes.c_int)}
    assert not bad, bad
    assert _lib_posegrad.missing_symbols() == []
    # the other four tables are the images of their own headers and stay so
    others = (set(_lib.SIGNATURES) | set(_lib_mesh.SIGNATURES)
              | set(_lib_mesh_normals.SIGNATURES) | set(_lib_raygrad.SIGNATURES))
    assert not set(protos) & others
    assert len(_lib.SIGNATURES) == 90 and len(_lib_mesh.SIGNATURES) == 6 \
        and len(_lib_raygrad.SIGNATURES) == 5


def _args(**k):
    # nr_gen_rays_posegrad(c2w, n_poses, H, W, w_half, h_half, focal, ndc, ndc_near, ndc_cw,
    #                      ndc_ch, ndc_2near, sel, n, g_rays, g_c2w, g_focal_pose, stream)
    H, W, f = k.get("H", 5), k.get("W", 7), k.get("focal", 6.5)
    return [k.get("c2w", P), k.get("n_poses", 3), H, W, W / 2, H / 2, f, k.get("ndc", 0), 1.0,
            -2 * f / max(W, 1), -2 * f / max(H, 1), 2.0, k.get("sel", P), k.get("n", 48),
            k.get("g_rays", P), k.get("g_c2w", P), k.get("g_focal", N), N]


_CASES = [
    ("n negative", _args(n=-1)),
    ("n overflowing", _args(n=2 ** 62)),
    ("n at 2^31", _args(n=2 ** 31)),
    ("n_poses zero", _args(n_poses=0)),
    ("n_poses negative", _args(n_poses=-3)),
    ("n_poses * H * W overflowing", _args(n_poses=2 ** 31 - 1, H=2 ** 31 - 1, W=2 ** 31 - 1)),
    ("H zero", _args(H=0)),
    ("H negative", _args(H=-5)),
    ("W zero", _args(W=0)),
    ("W negative", _args(W=-7)),
    ("c2w null", _args(c2w=N)),
    ("g_rays null", _args(g_rays=N)),
    ("g_c2w null", _args(g_c2w=N)),
    ("g_rays misaligned", _args(g_rays=ODD)),
    ("focal zero", _args(focal=0.0)),
    ("sel null, n above the pixel count", _args(sel=N, n=3 * 5 * 7 + 1)),
    ("sel null, n above the pixel count, ndc", _args(sel=N, n=3 * 5 * 7 + 1, ndc=1)),
    ("bad n wins over the empty problem's pointers", _args(n=-1, c2w=N, g_rays=N, g_c2w=N)),
]


@pytest.mark.parametrize("k", range(len(_CASES)), ids=[c[0].replace(" ", "_") for c in _CASES])
def test_entry_point_checks_arguments_before_the_device(k):
    """No case reaches a launch or a memset: each is rejected before the device
    is touched, so this runs without a GPU."""
    from nerf_pl_amd import _lib, _lib_posegrad
    _, args = _CASES[k]
    rc = getattr(_lib_posegrad.lib(), NAME)(*args)
    assert rc == NR_EINVAL, (rc, _lib.last_error())
    assert NAME in _lib.last_error()


def test_call_raises_with_the_message():
    from nerf_pl_amd import _lib_posegrad
    with pytest.raises(RuntimeError, match=NAME + ".*focal"):
        _lib_posegrad.call(NAME, *_args(focal=0.0))
