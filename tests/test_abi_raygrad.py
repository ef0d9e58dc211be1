"""CPU-side checks of the ray-gradient entry points
(include/nerf_pl_amd_raygrad.h, nerf_pl_amd/_lib_raygrad.py): the header, the
ctypes table and the library agree symbol by symbol and argument by argument,
and every entry point validates sizes, pointers and alignment before it
touches the device (NR_EINVAL with its own name in the message; an empty
problem is a no-op)."""
import ctypes
import os
import re

import pytest

from conftest import REPO

NR_EINVAL = 10001
N = None          # null pointer
P = 0x10000       # a non-null, 16-byte aligned (never dereferenced) device address
ODD = 0x10004     # ... and one that is 4- but not 16-byte aligned

_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double}


def _header_prototypes():
    """name -> (return ctype, [argument ctypes]); any pointer is a c_void_p"""
    txt = open(os.path.join(REPO, "include", "nerf_pl_amd_raygrad.h")).read()
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
    from nerf_pl_amd import _lib, _lib_mesh, _lib_raygrad
    protos = _header_prototypes()
    assert len(protos) == 5
    assert set(protos) == set(_lib_raygrad.SIGNATURES), set(protos) ^ set(_lib_raygrad.SIGNATURES)
    bad = {n: (ret, args) for n, (ret, args) in protos.items()
           if args != list(_lib_raygrad.SIGNATURES[n])
           or ret != _lib_raygrad.RESTYPES.get(n, ctypes.c_int)}
    assert not bad, bad
    assert _lib_raygrad.missing_symbols() == []
    # the other tables are the images of their own headers and stay so
    assert not set(protos) & (set(_lib.SIGNATURES) | set(_lib_mesh.SIGNATURES))


def _cases():
    big = 2 ** 62
    c = []
    # nr_raygrad_mlp(params, grad_ws, rays, z, n, spr, n_rays, layout, sigma_only, samples,
    #                count, g_samples, stream)
    mlp = lambda **k: [k.get("params", P), k.get("grad_ws", P), k.get("rays", P), k.get("z", P),  # noqa: E731
                       k.get("n", 33), k.get("spr", 11), k.get("n_rays", 3), k.get("layout", 0), 0,
                       k.get("samples", N), k.get("count", N), k.get("out", P), N]
    c += [("nr_raygrad_mlp", mlp(n=-1), NR_EINVAL),
          ("nr_raygrad_mlp", mlp(n=2 ** 31, spr=1, n_rays=2 ** 31), NR_EINVAL),
          ("nr_raygrad_mlp", mlp(n=big), NR_EINVAL),
          ("nr_raygrad_mlp", mlp(n=34), NR_EINVAL),            # not n_rays * samples_per_ray
          ("nr_raygrad_mlp", mlp(spr=0), NR_EINVAL),
          ("nr_raygrad_mlp", mlp(spr=-11, n_rays=-3), NR_EINVAL),
          ("nr_raygrad_mlp", mlp(layout=3), NR_EINVAL),
          ("nr_raygrad_mlp", mlp(layout=-1), NR_EINVAL),
          ("nr_raygrad_mlp", mlp(samples=P), NR_EINVAL),       # a list without its count
          ("nr_raygrad_mlp", mlp(count=P), NR_EINVAL),
          ("nr_raygrad_mlp", mlp(grad_ws=ODD), NR_EINVAL),
          ("nr_raygrad_mlp", mlp(out=ODD), NR_EINVAL),
          ("nr_raygrad_mlp", mlp(n=0, n_rays=0, params=N, grad_ws=N, rays=N, z=N, out=N), 0)]
    c += [("nr_raygrad_mlp", mlp(**{k: N}), NR_EINVAL)
          for k in ("params", "grad_ws", "rays", "z", "out")]
    red = lambda **k: [k.get("gs", P), k.get("z", P), k.get("n_rays", 3), k.get("spr", 11),  # noqa: E731
                       k.get("out", P), N]
    c += [("nr_raygrad_reduce", red(n_rays=-1), NR_EINVAL),
          ("nr_raygrad_reduce", red(spr=0), NR_EINVAL),
          ("nr_raygrad_reduce", red(n_rays=2 ** 31), NR_EINVAL),
          ("nr_raygrad_reduce", red(n_rays=big), NR_EINVAL),
          ("nr_raygrad_reduce", red(gs=ODD), NR_EINVAL),
          ("nr_raygrad_reduce", red(out=ODD), NR_EINVAL),
          ("nr_raygrad_reduce", red(n_rays=0, gs=N, z=N, out=N), 0)]
    c += [("nr_raygrad_reduce", red(**{k: N}), NR_EINVAL) for k in ("gs", "z", "out")]
    comp = lambda **k: [k.get("raw", P), k.get("stride", 4), k.get("col", 3), k.get("z", P),  # noqa: E731
                        k.get("rays", P), N, 0.0, 0, 1, k.get("n_rays", 3), k.get("S", 11), 0,
                        P, P, P, k.get("g_disp", N), k.get("depth", N), k.get("opacity", N),
                        k.get("g_z", P), k.get("g_rays", P), N]
    c += [("nr_composite_raygrad", comp(n_rays=-1), NR_EINVAL),
          ("nr_composite_raygrad", comp(S=0), NR_EINVAL),
          ("nr_composite_raygrad", comp(n_rays=2 ** 31), NR_EINVAL),
          ("nr_composite_raygrad", comp(stride=3, col=2), NR_EINVAL),
          ("nr_composite_raygrad", comp(stride=4, col=0), NR_EINVAL),
          ("nr_composite_raygrad", comp(g_disp=P), NR_EINVAL),          # without depth, opacity
          ("nr_composite_raygrad", comp(g_disp=P, depth=P), NR_EINVAL),
          ("nr_composite_raygrad", comp(g_rays=ODD), NR_EINVAL),
          ("nr_composite_raygrad", comp(n_rays=0, raw=N, z=N, rays=N, g_z=N, g_rays=N), 0)]
    c += [("nr_composite_raygrad", comp(**{k: N}), NR_EINVAL)
          for k in ("raw", "z", "rays", "g_z", "g_rays")]
    mrg = lambda **k: [k.get("zc", P), k.get("zf", P), k.get("g", P), k.get("n_rays", 3),  # noqa: E731
                       k.get("S", 11), k.get("I", 5), k.get("out", P), N]
    c += [("nr_merge_raygrad", mrg(n_rays=-1), NR_EINVAL),
          ("nr_merge_raygrad", mrg(S=0), NR_EINVAL),
          ("nr_merge_raygrad", mrg(I=-1), NR_EINVAL),
          ("nr_merge_raygrad", mrg(n_rays=2 ** 31), NR_EINVAL),
          ("nr_merge_raygrad", mrg(n_rays=0, zc=N, zf=N, g=N, out=N), 0)]
    c += [("nr_merge_raygrad", mrg(**{k: N}), NR_EINVAL) for k in ("zc", "zf", "g", "out")]
    cz = lambda **k: [k.get("rays", P), k.get("tlin", P), k.get("n_rays", 3), k.get("S", 11), 0,  # noqa: E731
                      1.0, N, 0, k.get("g_z", P), k.get("out", P), N]
    c += [("nr_coarse_z_raygrad", cz(n_rays=-1), NR_EINVAL),
          ("nr_coarse_z_raygrad", cz(S=0), NR_EINVAL),
          ("nr_coarse_z_raygrad", cz(n_rays=2 ** 31), NR_EINVAL),
          ("nr_coarse_z_raygrad", cz(out=ODD), NR_EINVAL),
          ("nr_coarse_z_raygrad", cz(n_rays=0, rays=N, tlin=N, g_z=N, out=N), 0)]
    c += [("nr_coarse_z_raygrad", cz(**{k: N}), NR_EINVAL) for k in ("rays", "tlin", "g_z", "out")]
    return c


_CASES = _cases()


@pytest.mark.parametrize("k", range(len(_CASES)), ids=[f"{i}-{c[0]}" for i, c in enumerate(_CASES)])
def test_entry_point_checks_arguments_before_the_device(k):
    """No case reaches a launch: each is rejected, or empty, before the device
    is touched, so this runs without a GPU."""
    from nerf_pl_amd import _lib, _lib_raygrad
    name, args, want = _CASES[k]
    rc = getattr(_lib_raygrad.lib(), name)(*args)
    assert rc == want, (name, rc, _lib.last_error())
    if want:
        assert name in _lib.last_error()


def test_call_raises_with_the_message():
    from nerf_pl_amd import _lib_raygrad
    with pytest.raises(RuntimeError, match="nr_raygrad_mlp.*layout"):
        _lib_raygrad.call("nr_raygrad_mlp", P, P, P, P, 33, 11, 3, 7, 0, None, None, P, None)


def test_parameter_offsets_are_the_packing_s():
    """csrc/raygrad.hip reads W1, W5 and W_dir from the flat fp32 parameters at
    offsets it computes from the layer shapes: the same walk over
    packing.param_shapes() gives them"""
    from nerf_pl_amd import packing
    off, offs = 0, {}
    for name, shp in packing.param_shapes().items():
        offs[name] = off
        k = 1
        for d in shp:
            k *= d
        off += k
    lay = lambda fan: 256 * fan + 256     # noqa: E731
    assert offs["xyz_encoding_1.0.weight"] == 0
    assert offs["xyz_encoding_5.0.weight"] == lay(63) + 3 * lay(256)
    w_final = lay(63) + 3 * lay(256) + lay(319) + 3 * lay(256)
    assert offs["xyz_encoding_final.weight"] == w_final
    assert offs["dir_encoding.0.weight"] == w_final + lay(256)
