"""CPU-side checks of the mesh-extraction entry points
(include/nerf_pl_amd_mesh.h, nerf_pl_amd/_lib_mesh.py): the header, the ctypes
table and the library agree symbol by symbol and argument by argument, and
every entry point validates sizes and pointers before it touches the device
(NR_EINVAL with its own name in the message; an empty problem is a no-op)."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import REPO

NR_EINVAL = 10001
N = None          # null pointer
P = 0x10000       # a non-null, 8-byte aligned (never dereferenced) device address
ODD = 0x10004     # ... and one that is 4- but not 8-byte aligned

_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double}


def _header_prototypes():
    """name -> (return ctype, [argument ctypes]); any pointer is a c_void_p"""
    txt = open(os.path.join(REPO, "include", "nerf_pl_amd_mesh.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)

    def ctype(decl):
        if "*" in decl:
            return ctypes.c_void_p
        # the type is the first word: a parameter's name follows it
        return _CTYPES[[w for w in decl.split() if w != "const"][0]]

    protos = {}
    for ret, name, args in re.findall(r"\b(\w+[\s\*]+)(nr_\w+)\s*\(([^)]*)\)\s*;", txt):
        assert name not in protos, name
        protos[name] = (ctype(ret), [ctype(a) for a in args.split(",")])
    return protos


def test_header_table_and_library_agree():
    from nerf_pl_amd import _lib, _lib_mesh
    protos = _header_prototypes()
    assert len(protos) == 6
    assert set(protos) == set(_lib_mesh.SIGNATURES), set(protos) ^ set(_lib_mesh.SIGNATURES)
    bad = {n: (ret, args) for n, (ret, args) in protos.items()
           if args != list(_lib_mesh.SIGNATURES[n])
           or ret != _lib_mesh.RESTYPES.get(n, ctypes.c_int)}
    assert not bad, bad
    assert set(_lib_mesh.RESTYPES) <= set(protos)
    assert _lib_mesh.missing_symbols() == []
    L = _lib_mesh.lib()
    assert all(getattr(L, n, None) is not None for n in protos)
    # the render path's table is the image of its own header and stays so
    assert not set(protos) & set(_lib.SIGNATURES)


def _w2c():
    return np.eye(4)[:3].copy()


def _cases():
    big = 2 ** 62
    G = [P, 4, 5, 6, 0.5]                      # sigma, d0, d1, d2, threshold
    c = []
    for name, tail in (("nr_mc_point_edges", [P, P, N]),
                       ("nr_mc_vertices", [P, P, 7, P, N]),
                       ("nr_mc_cell_tris", [P, P, N]),
                       ("nr_mc_triangles", [P, P, P, P, 7, 9, P, N])):
        for dims in ([1, 5, 6], [4, 1, 6], [4, 5, 1], [0, 5, 6], [-4, 5, 6], [4, 5, -6],
                     [2048, 1024, 1024]):           # 2^31 points
            c.append((name, [P] + dims + [0.5] + tail, NR_EINVAL))
        c.append((name, [N] + G[1:] + tail, NR_EINVAL))                     # null sigma
        for k, a in enumerate(tail[:-1]):
            if a == P:                                                      # each pointer in turn
                c.append((name, G + tail[:k] + [N] + tail[k + 1:], NR_EINVAL))
    c += [
        ("nr_mc_vertices", G + [P, P, -1, P, N], NR_EINVAL),
        ("nr_mc_vertices", G + [P, P, big, P, N], NR_EINVAL),
        ("nr_mc_vertices", G + [P, P, 3 * 120 + 1, P, N], NR_EINVAL),
        ("nr_mc_vertices", G + [N, N, 0, N, N], 0),
        ("nr_mc_vertices", G + [P, ODD, 7, P, N], NR_EINVAL),
        ("nr_mc_triangles", G + [P, P, P, P, -1, 9, P, N], NR_EINVAL),
        ("nr_mc_triangles", G + [P, P, P, P, 7, -1, P, N], NR_EINVAL),
        ("nr_mc_triangles", G + [P, P, P, P, 7, big, P, N], NR_EINVAL),
        ("nr_mc_triangles", G + [P, P, P, P, 7, 5 * 60 + 1, P, N], NR_EINVAL),
        ("nr_mc_triangles", G + [P, P, P, P, 0, 9, P, N], NR_EINVAL),
        ("nr_mc_triangles", G + [N, N, N, N, 0, 0, N, N], 0),
        ("nr_mc_triangles", G + [P, P, ODD, P, 7, 9, P, N], NR_EINVAL),
        ("nr_mc_triangles", G + [P, P, P, ODD, 7, 9, P, N], NR_EINVAL),
    ]
    rays = lambda **k: [k.get("v", P), k.get("n", 5), k.get("w2c", "w2c"), 20.0, k.get("W", 16),  # noqa: E731
                        k.get("H", 12), 2.0, 0.0, 0.0, 4.0, k.get("image", P), k.get("depth", P),
                        k.get("pix", P), k.get("colour", P), k.get("rays", P), N]
    c += [("nr_mesh_view_rays", rays(n=-1), NR_EINVAL),
          ("nr_mesh_view_rays", rays(n=2 ** 31), NR_EINVAL),
          ("nr_mesh_view_rays", rays(n=big), NR_EINVAL),
          ("nr_mesh_view_rays", rays(W=0), NR_EINVAL),
          ("nr_mesh_view_rays", rays(H=0), NR_EINVAL),
          ("nr_mesh_view_rays", rays(W=-3), NR_EINVAL),
          ("nr_mesh_view_rays", rays(W=2 ** 20, H=2 ** 20), NR_EINVAL),
          ("nr_mesh_view_rays", rays(n=0, v=N, w2c=N, image=N, depth=N, pix=N, colour=N, rays=N), 0),
          ("nr_mesh_view_rays", rays(depth=ODD), NR_EINVAL)]
    c += [("nr_mesh_view_rays", rays(**{k: N}), NR_EINVAL)
          for k in ("v", "w2c", "image", "depth", "pix", "colour", "rays")]
    fuse = lambda **k: [k.get("depth", P), k.get("colour", P), k.get("opacity", P), k.get("n", 5),  # noqa: E731
                        0.2, k.get("csum", P), k.get("wsum", P), N]
    c += [("nr_mesh_view_fuse", fuse(n=-1), NR_EINVAL),
          ("nr_mesh_view_fuse", fuse(n=big), NR_EINVAL),
          ("nr_mesh_view_fuse", fuse(n=0, depth=N, colour=N, opacity=N, csum=N, wsum=N), 0),
          ("nr_mesh_view_fuse", fuse(csum=ODD), NR_EINVAL),
          ("nr_mesh_view_fuse", fuse(wsum=ODD), NR_EINVAL),
          ("nr_mesh_view_fuse", fuse(depth=ODD), NR_EINVAL)]
    c += [("nr_mesh_view_fuse", fuse(**{k: N}), NR_EINVAL)
          for k in ("depth", "colour", "opacity", "csum", "wsum")]
    return c


_CASES = _cases()


@pytest.mark.parametrize("k", range(len(_CASES)), ids=[f"{i}-{c[0]}" for i, c in enumerate(_CASES)])
def test_entry_point_checks_arguments_before_the_device(k):
    """No case reaches a launch: each is rejected, or empty, before the device
    is touched, so this runs without a GPU.  (nr_mc_point_edges and
    nr_mc_cell_tris have no empty problem: every Di >= 2.)"""
    from nerf_pl_amd import _lib, _lib_mesh
    name, args, want = _CASES[k]
    w2c = _w2c()
    args = [w2c.ctypes.data if isinstance(a, str) else a for a in args]
    rc = getattr(_lib_mesh.lib(), name)(*args)
    assert rc == want, (name, rc, _lib.last_error())
    if want:
        assert name in _lib.last_error()


def test_call_raises_with_the_message():
    from nerf_pl_amd import _lib_mesh
    with pytest.raises(RuntimeError, match="nr_mc_point_edges.*>= 2"):
        _lib_mesh.call("nr_mc_point_edges", P, 1, 2, 2, 0.0, P, P, None)
