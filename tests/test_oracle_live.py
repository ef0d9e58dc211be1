"""The oracle against the REFERENCE on cases of their own (make_golden.LIVE_CASES).

Every host checks the oracle against the fixtures the reference wrote for these
cases (tests/golden/live/, ``make_golden.py --live``: torchsearchsorted shim,
recorded random draws), as tests/test_oracle_golden.py does for its cases: with
the reference's recorded MLP outputs substituted the importance depths are
bit-identical and every output within a few ulp (the row sums' order is the
host's SIMD width), and end to end the outputs agree to GEMM-order tolerance.

Where a checkout of the reference exists ($NERF_REFERENCE) it is also run live,
through the fixture generator into a temporary fixture, and the oracle replays
the same draws: on one host both use the same PyTorch-CPU kernels, so every
output, intermediate and the MLP's raw outputs must be bit-identical."""
import os
import sys

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_golden_path

sys.path.insert(0, GOLDEN)
import make_golden as mg  # noqa: E402

HAVE_REFERENCE = os.path.isdir(os.path.join(mg.REF, "models"))


@pytest.fixture(scope="module")
def ref():
    return mg.import_reference()


def _stored(fx):
    """the checks that hold on any host (test_oracle_golden.py's, same bounds)"""
    import test_oracle_golden as T
    keys = [k for k in fx if k.startswith("out_")]
    assert keys
    _, res, cap = T._run_oracle(fx, substitute_raw=True)
    for k in keys:
        b = fx[k]
        tol = 4 * np.spacing(np.maximum(np.abs(b), 1.0).astype(np.float32))
        np.testing.assert_array_less(np.abs(res[k[4:]].detach().numpy() - b), tol + 1e-30,
                                     err_msg=k)
    if "z_pdf" in fx:
        np.testing.assert_array_equal(cap["z_pdf"].numpy(), fx["z_pdf"])
    _, res, cap = T._run_oracle(fx)
    for k in keys:
        a, b = res[k[4:]].detach().numpy().astype(np.float64), fx[k].astype(np.float64)
        tol = 1e-5 * (np.maximum(np.abs(b), 1.0) if "depth" in k else 1.0)
        bad = np.abs(a - b) > tol
        bad_rays = np.unique(np.nonzero(bad)[0]) if bad.ndim else np.array([])
        assert len(bad_rays) <= 1, (k, bad_rays, np.abs(a - b).max())
    np.testing.assert_allclose(cap["raw_coarse"].numpy(), fx["raw_coarse"], rtol=1e-5, atol=2e-6)


def _bit_exact(fx):
    import test_oracle_golden as T
    _, res, cap = T._run_oracle(fx)
    for k in [k for k in fx if k.startswith("out_")]:
        np.testing.assert_array_equal(res[k[4:]].detach().numpy(), fx[k], err_msg=k)
    np.testing.assert_array_equal(cap["raw_coarse"].numpy(), fx["raw_coarse"])
    if "raw_fine" in fx:
        np.testing.assert_array_equal(cap["raw_fine"].numpy(), fx["raw_fine"])
        np.testing.assert_array_equal(cap["z_pdf"].numpy(), fx["z_pdf"])


@pytest.mark.parametrize("case", mg.LIVE_CASES, ids=lambda c: c["name"])
def test_oracle_bit_exact_vs_live_reference(case, tmp_path, request):
    _stored(load_golden_path(os.path.join(mg.LIVE, case["name"] + ".npz")))
    if HAVE_REFERENCE:
        mg.run_live_case(request.getfixturevalue("ref"), case, str(tmp_path))
        _bit_exact(load_golden_path(os.path.join(str(tmp_path), case["name"] + ".npz")))
