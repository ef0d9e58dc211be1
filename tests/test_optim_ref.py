"""The optimizer fixtures (tests/golden/optim/optim_*.npz: the reference's own
RAdam and Ranger, fp32 on the CPU) against the float64 restatement of the
rules (tests/optim_ref.py), and the restatement's own landmarks.

Bound: every stored checkpoint within 4 ulp * max(1, |p|) + 1% of lr of float64.
Measured when the fixtures were made, the reference's fp32 run goes at most
0.19% of lr beyond the 4 ulp term over these 14 steps (radam_wd; 0.02% for
ranger_wd, nothing for the cases without decay), and at most 0.41% of lr from
float64 with no ulp term at all (radam_wd; the other cases at most 0.23%); the
GPU test allows the fused kernels 2%."""
import os

import numpy as np
import pytest

import optim_ref as R
from conftest import GOLDEN, load_golden_path

ULP = 2.0 ** -23


def _fx(name):
    return load_golden_path(os.path.join(GOLDEN, "optim", name + ".npz"))


@pytest.fixture(scope="module")
def inputs():
    return R.inputs_of(_fx("optim_inputs"))


def test_inputs_are_the_documented_ones(inputs):
    params, grads = inputs
    assert [p.shape for p in params] == R.SHAPES and len(grads) == R.STEPS == 14
    assert all(p.dtype == np.float32 for p in params)
    for s, gs in enumerate(grads, start=1):
        for k, g in enumerate(gs):
            if k == R.LATE and s < R.LATE_FROM:
                assert g is None
            else:
                assert g.shape == R.SHAPES[k] and g.dtype == np.float32
        assert not gs[0][:, :3].any() and gs[0][:, 3:].all()     # v = 0 meets eps there


@pytest.mark.parametrize("case", list(R.CASES))
def test_fixture_matches_float64_restatement(case, inputs):
    params, grads = inputs
    fx = _fx("optim_" + case)
    at, states = R.run(case, params, grads)
    assert set(at) == set(R.CHECKPOINTS) and set(states) == set(R.STATE_AT)
    worst = 0.0
    for step, ps in at.items():
        for k, p in enumerate(ps):
            got = fx[f"p{step}_{k}"]
            assert got.dtype == np.float32 and got.shape == p.shape
            d = np.abs(got.astype(np.float64) - p) - 4 * ULP * np.maximum(1.0, np.abs(p))
            worst = max(worst, float(d.max()))
    print(f"{case}: worst excess over 4 ulp, in units of lr: {worst / R.LR:.4f}")
    assert worst <= 0.01 * R.LR
    cls = R.CASES[case][0]
    for step, sts in states.items():
        for k, st in enumerate(sts):
            assert int(fx[f"s{step}_{k}_step"]) == st["step"] == step - (3 if k == R.LATE else 0)
            for key in R.STATE_KEYS[cls]:
                a, b = fx[f"s{step}_{k}_{key}"].astype(np.float64), st[key]
                tol = 1e-5 * np.abs(b).max()
                if key == "slow_buffer":       # a parameter: the parameters' bound
                    tol = 4 * ULP * max(1.0, np.abs(b).max()) + 0.01 * R.LR
                assert np.abs(a - b).max() <= tol, (step, k, key)


def test_radam_without_sgd_leaves_parameters_alone_below_the_threshold(inputs):
    params, grads = inputs
    fx = _fx("optim_radam_nosgd")
    moved = _fx("optim_radam")
    for k, p in enumerate(params):
        assert np.array_equal(fx[f"p5_{k}"], p)            # bit for bit
        assert k == R.LATE or not np.array_equal(fx[f"p6_{k}"], p)
        assert not np.array_equal(moved[f"p5_{k}"], p)
    # the late tensor (own step 3 at step 6) is still below it
    assert np.array_equal(fx[f"p6_{R.LATE}"], params[R.LATE])
    assert not np.array_equal(fx[f"p12_{R.LATE}"], params[R.LATE])


def test_mode_switches_at_step_six_under_both_rules():
    assert R.n_sma(0.999, 5) == pytest.approx(4.996, abs=1e-3)
    assert R.n_sma(0.999, 6) == pytest.approx(5.994, abs=1e-3)
    for step in range(1, 15):
        want = R.RECTIFIED if step >= 6 else R.SGD_LIKE
        assert R.radam_mode(0.999, step) == want                       # N_sma >= 5
        assert R.ranger_mode(0.999, step, 5) == want                   # N_sma > 5
        assert R.radam_mode(0.999, step, degenerated_to_sgd=False) == \
            (R.RECTIFIED if step >= 6 else R.SKIP)
    # the package's own N_sma, which picks the kernel's mode, is the same number
    from nerf_pl_amd.optim import n_sma
    for b2 in (0.999, 0.99):
        for step in (1, 5, 6, 7, 100):
            assert n_sma(b2, step) == pytest.approx(R.n_sma(b2, step), rel=1e-14)


def test_step_size_landmarks():
    # sgd-like: only the bias correction; rectified: tends to 1 / (1 - b1^t) from below
    assert R.step_size(0.9, 0.999, 1, R.SGD_LIKE) == pytest.approx(10.0)
    assert R.step_size(0.9, 0.999, 3, R.SKIP) == 0.0
    r6 = R.step_size(0.9, 0.999, 6, R.RECTIFIED) * (1 - 0.9 ** 6)
    assert 0.0 < r6 < 0.1            # the rectification starts small ...
    r = [R.step_size(0.9, 0.999, t, R.RECTIFIED) * (1 - 0.9 ** t) for t in (6, 60, 600, 60000)]
    assert r == sorted(r) and r[-1] == pytest.approx(1.0, abs=1e-2)    # ... and grows to 1


def test_lookahead_in_the_restatement():
    """at every k-th step the parameter becomes slow + alpha (p - slow)"""
    p0 = np.array([1.0, -2.0])
    g = np.array([0.5, 0.25])
    a = R.Ranger([p0], 1e-2, alpha=0.5, k=3)
    b = R.RAdam([p0], 1e-2, betas=(0.95, 0.999), eps=1e-5)
    for _ in range(3):
        a.step([g])
        b.step([g])
    assert np.allclose(a.params[0], p0 + 0.5 * (b.params[0] - p0), rtol=0, atol=1e-15)
    assert np.array_equal(a.state[0]["slow_buffer"], a.params[0])
