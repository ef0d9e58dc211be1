"""CPU-side checks of the fused SGD / RAdam / Ranger entry points
(include/nerf_pl_amd_optim.h, nerf_pl_amd/_lib_optim.py): the header, the
ctypes table and the library agree symbol by symbol and argument by argument,
the new names collide with none of the five existing tables, and the entry
points validate before they touch the device (NR_EINVAL with their own name in
the message)."""
import ctypes
import os
import re

import pytest

from conftest import REPO

NR_EINVAL = 10001
N = None          # null pointer
CAP = 48

_CTYPES = {"int": ctypes.c_int, "int64_t": ctypes.c_int64, "uint64_t": ctypes.c_uint64,
           "float": ctypes.c_float, "double": ctypes.c_double}


def _header_prototypes():
    """name -> (return ctype, [argument ctypes]); any pointer is a c_void_p"""
    txt = open(os.path.join(REPO, "include", "nerf_pl_amd_optim.h")).read()
    txt = re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)
    txt = re.sub(r"//[^\n]*", " ", txt)

    def ctype(decl):
        if "*" in decl:
            return ctypes.c_void_p
        return _CTYPES[[w for w in decl.split() if w != "const"][0]]

    protos = {}
    for ret, name, args in re.findall(r"\b(\w+[\s\*]+)(nr_\w+)\s*\(([^)]*)\)\s*;", txt):
        assert name not in protos, name
        args = args.strip()
        protos[name] = (ctype(ret), [] if args in ("", "void") else
                        [ctype(a) for a in args.split(",")])
    return protos


def test_header_table_and_library_agree():
    from nerf_pl_amd import (_lib, _lib_mesh, _lib_mesh_normals, _lib_optim, _lib_posegrad,
                             _lib_raygrad)
    protos = _header_prototypes()
    assert set(protos) == {"nr_optim_max_tensors", "nr_sgd_step", "nr_radam_step"}
    assert set(protos) == set(_lib_optim.SIGNATURES)
    bad = {n: (ret, args) for n, (ret, args) in protos.items()
           if args != list(_lib_optim.SIGNATURES[n])
           or ret != _lib_optim.RESTYPES.get(n, ctypes.c_int)}
    assert not bad, bad
    assert _lib_optim.missing_symbols() == []
    # the other five tables are the images of their own headers and stay so
    others = (set(_lib.SIGNATURES) | set(_lib_mesh.SIGNATURES)
              | set(_lib_mesh_normals.SIGNATURES) | set(_lib_raygrad.SIGNATURES)
              | set(_lib_posegrad.SIGNATURES))
    assert not set(protos) & others
    assert len(_lib.SIGNATURES) == 90 and len(_lib_mesh.SIGNATURES) == 6 \
        and len(_lib_raygrad.SIGNATURES) == 5 and len(_lib_posegrad.SIGNATURES) == 1


def test_the_cap_is_adams():
    from nerf_pl_amd import _lib, _lib_optim
    assert _lib_optim.lib().nr_optim_max_tensors() == CAP == _lib.lib().nr_adam_max_tensors()


def _table(k, value=0x10000):
    """a host table of k (never dereferenced) 16-byte aligned device addresses"""
    return (ctypes.c_void_p * max(k, 1))(*[value + 64 * i for i in range(max(k, 1))])


def _numel(k, value=8):
    return (ctypes.c_int64 * max(k, 1))(*([value] * max(k, 1)))


def _sgd(**k):
    # nr_sgd_step(params, grads, momentum_buf, numel, count, lr, momentum, weight_decay,
    #             first, stream)
    c = k.get("count", 2)
    return [k.get("params", _table(c)), k.get("grads", _table(c)), k.get("buf", _table(c)),
            k.get("numel", _numel(c)), c, 5e-4, k.get("momentum", 0.9), 0.0, k.get("first", 0), N]


def _radam(**k):
    # nr_radam_step(params, grads, exp_avg, exp_avg_sq, slow, numel, count, lr, beta1, beta2,
    #               eps, weight_decay, step, mode, lookahead_alpha, lookahead_sync, stream)
    c = k.get("count", 2)
    return [k.get("params", _table(c)), k.get("grads", _table(c)), k.get("exp_avg", _table(c)),
            k.get("exp_avg_sq", _table(c)), k.get("slow", _table(c)), k.get("numel", _numel(c)),
            c, 5e-4, k.get("beta1", 0.9), k.get("beta2", 0.999), 1e-8, 0.0, k.get("step", 7),
            k.get("mode", 0), k.get("alpha", 0.5), k.get("sync", 0), N]


_CASES = [
    ("sgd", "count negative", _sgd(count=-1)),
    ("sgd", "count above the cap", _sgd(count=CAP + 1)),
    ("sgd", "params null", _sgd(params=N)),
    ("sgd", "grads null", _sgd(grads=N)),
    ("sgd", "numel null", _sgd(numel=N)),
    ("sgd", "momentum with a null buffer table", _sgd(buf=N)),
    ("sgd", "numel negative", _sgd(numel=_numel(2, -1))),
    ("sgd", "first neither 0 nor 1", _sgd(first=2)),
    ("sgd", "a null pointer in the table", _sgd(params=_table(2, 0))),
    ("radam", "count negative", _radam(count=-1)),
    ("radam", "count above the cap", _radam(count=CAP + 1)),
    ("radam", "params null", _radam(params=N)),
    ("radam", "grads null", _radam(grads=N)),
    ("radam", "exp_avg null", _radam(exp_avg=N)),
    ("radam", "exp_avg_sq null", _radam(exp_avg_sq=N)),
    ("radam", "numel null", _radam(numel=N)),
    ("radam", "step zero", _radam(step=0)),
    ("radam", "step negative", _radam(step=-3)),
    ("radam", "step zero wins over the empty problem", _radam(step=0, count=0)),
    ("radam", "mode unknown", _radam(mode=3)),
    ("radam", "mode negative", _radam(mode=-1)),
    ("radam", "alpha above 1", _radam(alpha=1.5)),
    ("radam", "alpha negative", _radam(alpha=-0.1)),
    ("radam", "alpha nan", _radam(alpha=float("nan"))),
    ("radam", "lookahead_sync with a null slow", _radam(sync=1, slow=N)),
    ("radam", "lookahead_sync neither 0 nor 1", _radam(sync=2)),
    ("radam", "numel negative", _radam(numel=_numel(2, -1))),
    ("radam", "beta2 of 1", _radam(beta2=1.0)),
    ("radam", "rectified below the threshold", _radam(step=3, mode=0)),
    ("radam", "a null pointer in the table", _radam(exp_avg=_table(2, 0))),
]


@pytest.mark.parametrize("k", range(len(_CASES)),
                         ids=[(c[0] + " " + c[1]).replace(" ", "_") for c in _CASES])
def test_entry_points_check_arguments_before_the_device(k):
    """No case reaches a launch: each is rejected before the device is touched,
    so this runs without a GPU."""
    from nerf_pl_amd import _lib, _lib_optim
    which, _, args = _CASES[k]
    name = f"nr_{which}_step"
    rc = getattr(_lib_optim.lib(), name)(*args)
    assert rc == NR_EINVAL, (rc, _lib.last_error())
    assert name in _lib.last_error()


def test_empty_problems_return_zero_without_a_launch():
    from nerf_pl_amd import _lib_optim
    L = _lib_optim.lib()
    assert L.nr_sgd_step(*_sgd(count=0, params=N, grads=N, buf=N, numel=N)) == 0
    assert L.nr_radam_step(*_radam(count=0, params=N, grads=N, exp_avg=N, exp_avg_sq=N, slow=N,
                                   numel=N)) == 0
    # tensors without elements: nothing to launch either, and their pointers may be null
    assert L.nr_sgd_step(*_sgd(numel=_numel(2, 0), params=_table(2, 0))) == 0
    assert L.nr_radam_step(*_radam(numel=_numel(2, 0), sync=1, slow=_table(2, 0))) == 0


def test_call_raises_with_the_message():
    from nerf_pl_amd import _lib_optim
    with pytest.raises(RuntimeError, match="nr_radam_step.*mode"):
        _lib_optim.call("nr_radam_step", *_radam(mode=9))
    with pytest.raises(RuntimeError, match="nr_sgd_step.*count"):
        _lib_optim.call("nr_sgd_step", *_sgd(count=CAP + 1))
