"""CPU self-test of tests/shadow64.py, the float64 reference and case builder
behind tests/test_gpu_shadow_kernels.py:

* ``reference(case, float32)`` is bitwise ``SO._sm_batched(...) + out_eps`` at
  the default options, on the committed fixtures' inputs;
* its float64 gradients agree with central differences in float64 (1e-6 of the
  tensor's max), on each run's min and max ray, a tie pair and random rays, and
  on hit, shared and unread texels;
* every ``make_case`` condition holds for every case (the shares are printed);
* the oracle's option branches (sigmoid, epsilon, delta) are pinned to the
  reference's own ``run_shadow_mapping`` (tests/golden/shadow_options, made by
  tests/golden/make_golden_shadow.py).
"""
import os

import numpy as np
import pytest
import torch

import shadow64 as S
from conftest import GOLDEN
from oracle import shadow_oracle as SO
from test_shadow_golden import CASES as FIXTURES, load_shadow, shadow_cfg

T = torch.from_numpy
FD_CASES = [c for c in S.CASES if not c.startswith("nonfinite")]


@pytest.mark.parametrize("fixture", [c for c in FIXTURES if not c.startswith("cfg5_128")])
def test_reference_fp32_is_the_batched_oracle_bitwise(fixture):
    fx = load_shadow(fixture)
    cfg = shadow_cfg(fx)
    wh = cfg["wh"]
    lw = SO.get_normed_w(T(fx["light_camera"]), torch.cat(
        [T(fx["light_pixels"]), T(fx["light_depth_coarse"]).view(-1, 1)], 1))[:, 3]
    case = dict(pixels=T(fx["pixels"]), depth=T(fx["out_depth_coarse"]), eye=T(fx["eye_pos"]),
                cams=T(fx["camera"]), light_eye=T(fx["light_eye"]), light_cam=T(fx["light_camera"]),
                lw=lw, res=(wh, wh), mode=cfg["method"], delta=1e-2, epsilon=0.0, sigmoid=False,
                out_eps=SO.EPSILON)
    want = SO._sm_batched((wh, wh), {"eye_pos": case["eye"], "camera": case["cams"]},
                          case["light_eye"], case["light_cam"],
                          torch.cat([case["pixels"], case["depth"].view(-1, 1)], 1), lw,
                          cfg["method"]) + SO.EPSILON
    got = S.reference(case, torch.float32, backward=False).out
    assert got.dtype == np.float32 and np.array_equal(got, want.numpy())


@pytest.mark.parametrize("name", list(S.CASES))
def test_case_conditions_hold(name):
    case = S.make_case(name)
    s = S.shares(case)
    print(f"{name}: seed {case['seed']}, " +
          ", ".join(f"{k} {v:.4g}" if isinstance(v, float) else f"{k} {v}" for k, v in s.items()))
    assert S.check_shares(case, s) is None
    assert case["depth"].shape[0] == sum(S.GEOMETRIES[S.CASES[name][0]]["lens"]) + \
        (3 if "tie_rows" in case else 0)
    assert all(case[k].dtype == torch.float32 for k in ("pixels", "depth", "eye", "cams", "lw",
                                                        "g_out", "light_eye", "light_cam"))
    g = case["g_out"].abs()
    assert g.min() >= 2.0 ** -10 and g.max() <= 1.0
    if case["mode"] == "shadow_method_1":
        assert s["kink_ok"]
    else:
        assert s["min_gap"] >= S.GAP
    if s["n"] >= 1000:
        assert s["clamped"] >= 0.10 and s["max_hits"] >= 20 and s["single_hits"] >= 1
        if case["mode"] == "shadow_method_1":
            assert s["interior"] >= 0.50 and s["below"] >= 0.10 and s["above"] >= 0.10
    # builder and reference agree on the texels: fp32 and float64 index alike
    assert np.array_equal(S.texel_keys(case), S.texel_keys(case, torch.float32))


def test_run_geometry_is_the_designed_one():
    case = S.make_case("runs_m2")
    starts = [s for s, _ in S.runs_of(case)]
    assert starts == [0, 1, 2, 64, 128, 129, 192, 257, 385, 388, 1088, 1090, 1281, 1282]
    assert case["depth"].shape[0] == 2531
    assert [len(S.runs_of(S.make_case(n))) for n in ("n1025_m2", "n1024_m1")] == [5, 5]


def test_special_cases_are_what_they_claim():
    ties = S.make_case("ties_m2")
    d = S.diffs(ties)
    (s0, e0), (s2, e2) = S.runs_of(ties)[0], S.runs_of(ties)[-1]
    assert sorted(np.nonzero(d[s0:e0] == d[s0:e0].min())[0] + s0) == sorted(ties["tie_rows"]["min"])
    assert sorted(np.nonzero(d[s0:e0] == d[s0:e0].max())[0] + s0) == sorted(ties["tie_rows"]["max"])
    assert e2 - s2 == 30 and np.unique(d[s2:e2]).size == 1
    assert S.runs_of(ties)[1][1] - S.runs_of(ties)[1][0] == 1
    for name in ("nonfinite_m1", "nonfinite_m2"):
        nf = S.make_case(name)
        key = S.texel_keys(nf)
        dirty = [bool(np.isin(key[s:e], nf["nonfinite_texels"]).any()) for s, e in S.runs_of(nf)]
        assert dirty == [False, True, False, True, False]
        assert torch.isnan(nf["lw"]).sum() == 1 and torch.isinf(nf["lw"]).sum() == 1
    single = S.make_case("single300_m1")
    assert single["eye"].shape == (3,) and single["cams"].shape == (3, 3)
    w, h = S.make_case("nonsquare_m1")["res"]
    assert (w, h) == (24, 16)
    u = S.project(S.make_case("nonsquare_m1"))[0].numpy()
    assert (np.clip(u, 0, w - 1) < h).all()
    lw = S.make_case("nonsquare_m2")["lw"].view(w, h)[:h]
    assert not torch.equal(lw, lw.T)


def _slice(case, s, e):
    sub = dict(case)
    for k in ("pixels", "depth", "g_out"):
        sub[k] = case[k][s:e]
    if case["eye"].dim() == 2:
        sub["eye"], sub["cams"] = case["eye"][s:e], case["cams"][s:e]
    sub.pop("_runs", None)
    return sub


def _fd_rays(case, rng):
    """each run's min and max ray where it is unique or a pair, the tie pair,
    then random rays: 32 in all (fewer where the case is smaller)"""
    d = S.diffs(case)
    rays, many = [], []
    for s, e in S.runs_of(case):
        for ext in (d[s:e].min(), d[s:e].max()):
            at = np.nonzero(d[s:e] == ext)[0] + s
            # three or more tied rays: the mean of the one-sided slopes is not
            # torch's even split, so central differences say nothing there
            (rays if at.size <= 2 else many).extend(at.tolist())
    rays = [i for i in dict.fromkeys(rays) if i not in many][:24]
    rest = [i for i in rng.permutation(d.shape[0]).tolist() if i not in rays + many]
    return rays + rest[:32 - len(rays)]


@pytest.mark.parametrize("name", FD_CASES)
def test_float64_gradients_match_central_differences(name):
    """L = sum(out * g_out).  The step is small against every margin the
    builder keeps (kinks, texel edges, gaps between a run's extremes); a tie
    PAIR is differentiable on neither side, and the central difference is the
    mean of the two one-sided slopes -- which is torch's even split over two."""
    case = S.make_case(name)
    ref = S.reference(case)
    rng = np.random.default_rng(5)
    g64 = case["g_out"].double().numpy()
    runs = S.runs_of(case)
    h = 2.0 ** -24
    worst = 0.0
    for i in _fd_rays(case, rng):
        s, e = next((s, e) for s, e in runs if s <= i < e)
        sub = _slice(case, s, e)
        outs = []
        for sign in (1.0, -1.0):
            dep = sub["depth"].double().clone()
            dep[i - s] += sign * h
            outs.append(S.reference(sub, backward=False, depth=dep).out)
        fd = ((outs[0] - outs[1]) * g64[s:e]).sum() / (2 * h)
        worst = max(worst, abs(fd - ref.g_depth[i]))
    scale = np.abs(ref.g_depth).max()
    print(f"{name}: d/d depth FD deviation {worst:.3g}, max |g| {scale:.3g}")
    assert worst <= 1e-6 * scale

    key = S.texel_keys(case)
    hits = np.bincount(key, minlength=case["lw"].shape[0])
    hit = np.nonzero(hits)[0]
    texels = [int(hits.argmax()), int(np.nonzero(hits == 1)[0][0])]
    if (hits == 0).any():
        texels.append(int(np.nonzero(hits == 0)[0][0]))
    texels += [int(k) for k in rng.permutation(hit) if k not in texels][:16 - len(texels)]
    h = 2.0 ** -26
    worst = 0.0
    for k in texels:
        outs = []
        for sign in (1.0, -1.0):
            lw = case["lw"].double().clone()
            lw[k] += sign * h
            outs.append(S.reference(case, backward=False, lw=lw).out)
        fd = ((outs[0] - outs[1]) * g64).sum() / (2 * h)
        worst = max(worst, abs(fd - ref.g_lw[k]))
    scale = np.abs(ref.g_lw).max()
    print(f"{name}: d/d light map FD deviation {worst:.3g}, max |g| {scale:.3g}")
    assert worst <= 1e-6 * scale
    assert (ref.g_lw[hits == 0] == 0).all()


def test_oracle_option_branches_match_reference():
    """sigmoid=True under method 2, (epsilon, delta) = (0.25, 0.5) and
    delta = 0.05 under method 1: the oracle against the reference's own
    run_shadow_mapping, at test_shadow_golden.py's 1e-5 relative bound."""
    with np.load(os.path.join(GOLDEN, "shadow_options", "options.npz"), allow_pickle=False) as z:
        fx = {k: z[k] for k in z.files}
    res = tuple(int(v) for v in fx["res"])
    mesh = torch.cat([T(fx["pixels"]), T(fx["depth"]).view(-1, 1)], 1)
    runs = {"m2_sigmoid": dict(mode="shadow_method_2", sigmoid=True),
            "m1_eps025_delta05": dict(mode="shadow_method_1", epsilon=0.25, delta=0.5),
            "m1_delta005": dict(mode="shadow_method_1", delta=0.05)}
    assert sorted("out_" + k for k in runs) == sorted(k for k in fx if k.startswith("out_"))
    for name, kw in runs.items():
        got = SO.run_shadow_mapping(res, T(fx["eye_pos"]), T(fx["camera"]), T(fx["light_eye"]),
                                    T(fx["light_camera"]), mesh, T(fx["light_w"]), **kw).numpy()
        want = fx["out_" + name]
        inside = ((want > 0) & (want < 1)).mean()
        print(f"{name}: {inside:.2f} strictly inside (0, 1), max dev {np.abs(got - want).max():.3g}")
        np.testing.assert_allclose(got, want, rtol=1e-5, atol=1e-6, err_msg=name)
    # the branches are told apart: the fixture's outputs differ from the defaults'
    base = SO.run_shadow_mapping(res, T(fx["eye_pos"]), T(fx["camera"]), T(fx["light_eye"]),
                                 T(fx["light_camera"]), mesh, T(fx["light_w"]),
                                 mode="shadow_method_2").numpy()
    assert np.abs(base - fx["out_m2_sigmoid"]).max() > 0.1
