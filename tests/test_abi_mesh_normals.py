"""CPU-side checks of the vertex-normal entry points
(include/nerf_pl_amd_mesh_normals.h, nerf_pl_amd/_lib_mesh_normals.py): the
header, the ctypes table and the library agree symbol by symbol and argument
by argument, and every entry point validates sizes, pointers and alignment
before it touches the device (NR_EINVAL with its own name in the message; an
empty problem is a no-op)."""
import ctypes
import os
import re

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
    txt = open(os.path.join(REPO, "include", "nerf_pl_amd_mesh_normals.h")).read()
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
    from nerf_pl_amd import _lib, _lib_mesh, _lib_mesh_normals, _lib_raygrad
    protos = _header_prototypes()
    assert len(protos) == 2
    assert set(protos) == set(_lib_mesh_normals.SIGNATURES), \
        set(protos) ^ set(_lib_mesh_normals.SIGNATURES)
    bad = {n: (ret, args) for n, (ret, args) in protos.items()
           if args != list(_lib_mesh_normals.SIGNATURES[n])
           or ret != _lib_mesh_normals.RESTYPES.get(n, ctypes.c_int)}
    assert not bad, bad
    assert set(_lib_mesh_normals.RESTYPES) <= set(protos)
    assert _lib_mesh_normals.missing_symbols() == []
    L = _lib_mesh_normals.lib()
    assert all(getattr(L, n, None) is not None for n in protos)
    # the three other tables are the images of their own headers and stay so
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib_mesh.SIGNATURES)
                              | set(_lib_raygrad.SIGNATURES))
    assert len(_lib_mesh.SIGNATURES) == 6 and len(_lib_raygrad.SIGNATURES) == 5


def _cases():
    big = 2 ** 62
    # nr_mesh_vertex_normals(vertices, triangles, inc_offsets, inc_tris, n_vertices,
    #                        n_triangles, normals, stream)
    vn = lambda **k: [k.get("v", P), k.get("tris", P), k.get("off", P), k.get("inc", P),  # noqa: E731
                      k.get("nv", 7), k.get("nt", 9), k.get("out", P), N]
    c = [("nr_mesh_vertex_normals", vn(nv=-1), NR_EINVAL),
         ("nr_mesh_vertex_normals", vn(nt=-1), NR_EINVAL),
         ("nr_mesh_vertex_normals", vn(nv=2 ** 31), NR_EINVAL),
         ("nr_mesh_vertex_normals", vn(nv=big), NR_EINVAL),
         ("nr_mesh_vertex_normals", vn(nt=(2 ** 31 + 2) // 3), NR_EINVAL),    # 3 T >= 2^31
         ("nr_mesh_vertex_normals", vn(nt=2 ** 31), NR_EINVAL),
         ("nr_mesh_vertex_normals", vn(nt=big), NR_EINVAL),                   # 3 T overflows int64
         ("nr_mesh_vertex_normals", vn(nv=0, nt=big), NR_EINVAL),
         ("nr_mesh_vertex_normals", vn(off=ODD), NR_EINVAL),
         ("nr_mesh_vertex_normals", vn(out=ODD), NR_EINVAL),
         ("nr_mesh_vertex_normals", vn(nv=0, nt=0, v=N, tris=N, off=N, inc=N, out=N), 0),
         ("nr_mesh_vertex_normals", vn(nv=0, v=N, tris=N, off=N, inc=N, out=N), 0)]
    c += [("nr_mesh_vertex_normals", vn(**{k: N}), NR_EINVAL)
          for k in ("v", "tris", "off", "inc", "out")]
    # without triangles only triangles and inc_tris may be null
    c += [("nr_mesh_vertex_normals", vn(nt=0, tris=N, inc=N, **{k: N}), NR_EINVAL)
          for k in ("v", "off", "out")]
    # nr_mesh_normal_rays(vertices, normals, n, near, far, near_t, inward, rays, stream)
    nr = lambda **k: [k.get("v", P), k.get("normals", P), k.get("n", 5), 2.0, 6.0, 1.0, 1,  # noqa: E731
                      k.get("rays", P), N]
    c += [("nr_mesh_normal_rays", nr(n=-1), NR_EINVAL),
          ("nr_mesh_normal_rays", nr(n=2 ** 31), NR_EINVAL),
          ("nr_mesh_normal_rays", nr(n=big), NR_EINVAL),
          ("nr_mesh_normal_rays", nr(normals=ODD), NR_EINVAL),
          ("nr_mesh_normal_rays", nr(n=0, v=N, normals=N, rays=N), 0)]
    c += [("nr_mesh_normal_rays", nr(**{k: N}), NR_EINVAL) for k in ("v", "normals", "rays")]
    return c


_CASES = _cases()


@pytest.mark.parametrize("k", range(len(_CASES)), ids=[f"{i}-{c[0]}" for i, c in enumerate(_CASES)])
def test_entry_point_checks_arguments_before_the_device(k):
    """No case reaches a launch: each is rejected, or empty, before the device
    is touched, so this runs without a GPU."""
    from nerf_pl_amd import _lib, _lib_mesh_normals
    name, args, want = _CASES[k]
    rc = getattr(_lib_mesh_normals.lib(), name)(*args)
    assert rc == want, (name, rc, _lib.last_error())
    if want:
        assert name in _lib.last_error()


def test_call_raises_with_the_message():
    from nerf_pl_amd import _lib_mesh_normals
    with pytest.raises(RuntimeError, match="nr_mesh_vertex_normals.*n_triangles"):
        _lib_mesh_normals.call("nr_mesh_vertex_normals", P, P, P, P, 7, -2, P, None)
