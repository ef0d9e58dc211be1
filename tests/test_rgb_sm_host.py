"""The joint RGB + shadow-map render path (nerf_pl_amd.rendering_rgb_sm) on the
CPU: its host path against the fixtures produced by running the reference's
models/rendering_rgb_sm.py (tests/golden/make_golden_rgb_sm.py), replaying the
reference's draws.

* result keys equal the reference's; rgb / depth / opacity within parity.TOL
  (1e-4 absolute); ``disp_map_*`` within 1e-4 relative to max(1, |x|), the rule
  of the shadow tests (test_gpu_shadow._check_rows(rel=True)); sample_pdf bin
  flips screened and explained against the reference's own CDF;
* ``juntos_nan``: ``disp_map_fine`` NaN on every ray, ``disp_map_coarse`` finite;
* ``juntos_disp_loss``: the gradient through the disparity line, at
  test_host_path.py's gradient bound;
* ``test_time``: ``opacity_coarse`` without ``disp_map_coarse``;
* ``efficient_sm``'s key contract, the shadow kernels stubbed;
* the C ABI of the two new entry points validates before it launches."""
import os

import numpy as np
import pytest
import torch

import parity
from conftest import GOLDEN
from oracle import nerf_oracle as O
from screening import pdf_flips
from test_gpu_shadow import _check_rows
from test_shadow_golden import shadow_cfg

RGB_SM = os.path.join(GOLDEN, "rgb_sm")
CASES = ("juntos_sm2", "juntos_gol_sm1", "juntos_disp_loss", "juntos_nan")
FINITE = CASES[:3]
LEVELS = ("coarse", "fine")


def load_rgb_sm(name):
    with np.load(os.path.join(RGB_SM, name + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def rgb_sm_cfg(fx):
    cfg = shadow_cfg(fx)
    cfg.update(kind=str(fx["kind"]), sigma_bias=(cfg["sigma_bias"], float(fx["sigma_bias_fine"])),
               rgb_weight=float(fx["rgb_weight"]), sm_weight=float(fx["sm_weight"]))
    return cfg


def draws_of(fx):
    return [fx[f"draw{i}"] for i in range(int(fx["n_draws"]))]


def build_models(cfg, dev=None):
    from nerf_pl_amd import NeRF
    out = []
    for m in range(2):
        net = NeRF()
        net.load_state_dict(O.make_params(cfg["seeds"][m], sigma_bias=cfg["sigma_bias"][m]))
        out.append(net if dev is None else net.to(dev))
    return out


def render_keys(fx, prefix="out_"):
    """the reference render's result keys (efficient_sm adds sm_* afterwards)"""
    skip = ("light_rays", "light_pixels", "light_eye", "light_camera", "light_z_pdf",
            "light_wpdf")
    return sorted(k[len(prefix):] for k in fx
                  if k.startswith(prefix) and k not in skip and not k.startswith("out_sm_"))


def u_index(cfg, light):
    """position of a render's importance draw u in the recorded draws"""
    per = 1 if cfg["perturb"] > 0 else 0
    return (per + 4 if light else 0) + per + 1


def screen(fx, cfg, cap, light=False):
    """rays whose fine depths moved by a sample_pdf bin flip, each explained by
    a u within 1e-5 of a knot of the reference's own CDF"""
    pre = "light_" if light else ""
    ref = {"z_pdf": torch.from_numpy(fx[pre + "z_pdf"]), "weights_coarse": fx[pre + "wpdf"]}
    moved, explained = pdf_flips(cap["z_fine"], ref, draws_of(fx)[u_index(cfg, light)])
    assert not (moved & ~explained).any(), np.nonzero(moved & ~explained)[0]
    return moved


def check_render(label, res, fx, prefix, bad):
    """a render's result dict against the reference's: rgb / depth / opacity
    at parity.TOL absolute, disp_map at 1e-4 relative to max(1, |x|)"""
    assert sorted(res) == render_keys(fx, prefix), (sorted(res), render_keys(fx, prefix))
    none = np.zeros_like(bad)
    for k in sorted(res):
        got, ref = res[k].detach().cpu().numpy(), fx[prefix + k]
        assert got.shape == ref.shape, (k, got.shape, ref.shape)
        rows = bad if k.endswith("fine") else none
        if np.isnan(ref).any():
            assert np.isnan(ref).all() and np.isnan(got).all(), f"{label}/{k}: NaN placement"
            continue
        assert np.isfinite(got).all(), f"{label}/{k}: not finite"
        _check_rows(f"{label}/{k}", got, ref, 1e-4 if k.startswith("disp") else parity.TOL,
                    k.startswith("disp"), rows)


def run_renders(fx, cfg, models, rays_of, render_kw=None):
    """the camera render and (joint cases) the light render of a fixture through
    rendering_rgb_sm.render_rays, replaying its draws"""
    from nerf_pl_amd import Embedding, ReplayRNG
    from nerf_pl_amd import rendering_rgb_sm as RGS
    emb = [Embedding(3, 10), Embedding(3, 4)]
    rng = ReplayRNG(draws_of(fx))
    ccap, lcap, light = {}, {}, None
    with torch.set_grad_enabled(cfg["kind"] != "nan"):
        cam = RGS.render_rays(models, emb, rays_of("rays"), cfg["N_samples"], False,
                              cfg["perturb"], cfg["noise_std"], cfg["N_importance"], 32768, False,
                              rng=rng, _capture=ccap)
    if cfg["kind"] == "juntos":
        with torch.set_grad_enabled(cfg["grad_on_light"]):     # train_rgb_sm_juntos.py:156-164
            light = RGS.render_rays(models, emb, rays_of("light_rays"), cfg["N_samples"], False,
                                    cfg["perturb"], cfg["noise_std"], cfg["light_importance"],
                                    32768, False, rng=rng, _capture=lcap,
                                    **(render_kw or {}))
    assert rng.exhausted()
    return cam, light, ccap, lcap


@pytest.mark.parametrize("case", CASES)
def test_host_render_matches_reference(case):
    torch.set_num_threads(8)
    fx = load_rgb_sm(case)
    cfg = rgb_sm_cfg(fx)
    with torch.no_grad():
        cam, light, ccap, lcap = run_renders(fx, cfg, build_models(cfg),
                                             lambda k: torch.from_numpy(fx[k]))
    bad = screen(fx, cfg, ccap)
    assert bad.mean() <= 0.05
    check_render(case, cam, fx, "out_", bad)
    if case == "juntos_nan":
        assert np.isnan(cam["disp_map_fine"].numpy()).all()
        assert not cam["opacity_fine"].any()
        assert np.isfinite(cam["disp_map_coarse"].numpy()).all()
    if light is not None:
        lbad = screen(fx, cfg, lcap, True) if cfg["light_importance"] > 0 else \
            np.zeros(fx["light_rays"].shape[0], bool)
        assert lbad.mean() <= 0.05
        check_render(case + "/light", light, fx, "light_", lbad)


def test_host_disparity_gradients_match_reference():
    """juntos_disp_loss: MSE(rgb_*) + the squared distance of both disparity
    maps from a target -- the reference's autograd through
    1 / max(1e-10, depth / sum(weights))"""
    torch.set_num_threads(8)
    fx = load_rgb_sm("juntos_disp_loss")
    cfg = rgb_sm_cfg(fx)
    models = build_models(cfg)
    cam, _, ccap, _ = run_renders(fx, cfg, models, lambda k: torch.from_numpy(fx[k]))
    assert not screen(fx, cfg, ccap).any()
    tgt, td = torch.from_numpy(fx["target"]), torch.from_numpy(fx["target_disp"])
    loss = 0
    for lvl in LEVELS:
        loss = loss + torch.mean((cam["rgb_" + lvl] - tgt) ** 2)
    loss = loss + torch.mean((cam["disp_map_fine"] - td) ** 2) + \
        torch.mean((cam["disp_map_coarse"] - td) ** 2)
    np.testing.assert_allclose(loss.item(), float(fx["loss"]), rtol=1e-5)
    loss.backward()
    n = 0
    for m, net in enumerate(models):
        for name, p in net.named_parameters():
            key = f"grad{m}_{name}"
            g = p.grad.numpy()
            gmax = np.abs(fx.get(key + "_full", fx.get(key + "_val"))).max()
            got, ref = (g, fx[key + "_full"]) if key + "_full" in fx else \
                (g.reshape(-1)[fx[key + "_idx"]], fx[key + "_val"])
            np.testing.assert_allclose(got, ref, rtol=1e-3, atol=1e-4 * gmax + 1e-12, err_msg=key)
            n += 1
    assert n == 48


def test_host_shared_keys_are_rendering_render_rays():
    """the keys the joint renderer shares with rendering.render_rays carry the
    same bits under the same draws (one function, a disparity switch)"""
    from nerf_pl_amd import Embedding, ReplayRNG, render_rays
    from nerf_pl_amd import rendering_rgb_sm as RGS
    fx = load_rgb_sm("juntos_disp_loss")
    cfg = rgb_sm_cfg(fx)
    models = build_models(cfg)
    args = (models, [Embedding(3, 10), Embedding(3, 4)], torch.from_numpy(fx["rays"]), 16, False,
            1.0, 1.0, 16, 32768, False)
    with torch.no_grad():
        a = RGS.render_rays(*args, rng=ReplayRNG(draws_of(fx)))
        b = render_rays(*args, rng=ReplayRNG(draws_of(fx)))
    assert sorted(a) == sorted(list(b) + ["disp_map_coarse", "disp_map_fine"])
    for k in b:
        assert torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("n_importance", [0, 8])
def test_test_time_has_no_coarse_disparity(n_importance):
    from nerf_pl_amd import Embedding, NeRF
    from nerf_pl_amd import rendering_rgb_sm as RGS
    torch.manual_seed(3)
    rays = torch.cat([torch.randn(6, 6), torch.full((6, 1), 2.0), torch.full((6, 1), 6.0)], 1)
    with torch.no_grad():
        res = RGS.render_rays([NeRF(), NeRF()], [Embedding(3, 10), Embedding(3, 4)], rays, 8,
                              False, 0, 0, n_importance, 32768, False, True)
    want = ["opacity_coarse"]
    if n_importance > 0:
        want += ["rgb_fine", "depth_fine", "opacity_fine", "disp_map_fine"]
    assert sorted(res) == sorted(want)
    with pytest.raises(NotImplementedError):
        RGS.render_rays([NeRF()], [Embedding(3, 10), Embedding(3, 4)], rays, 8, depth_only=True)


@pytest.mark.parametrize("light_fine", [False, True])
def test_efficient_sm_key_contract(monkeypatch, light_fine):
    """sm_* written, every other entry the same object as before, and the fine
    level reading the coarse light map when Light_N_importance is false"""
    from nerf_pl_amd import efficient_shadow_mapping as ESM
    from nerf_pl_amd import rendering_rgb_sm as RGS
    n, wh = 5, 4
    normed, maps = [], []

    def normed_depth(cam, pixels, depth):
        normed.append(depth)
        return depth + 0

    def shadow_map(depth, pixels, eye, cams, leye, lcam, light_w, res, mode, out_eps=0.0):
        maps.append((depth, light_w, mode, out_eps))
        return torch.full((depth.shape[0], 3), float(len(maps)))

    monkeypatch.setattr(ESM, "normed_depth", normed_depth)
    monkeypatch.setattr(ESM, "shadow_map", shadow_map)
    cam = {f"{q}_{lvl}": torch.rand(n, 3) if q == "rgb" else torch.rand(n)
           for lvl in LEVELS for q in ("rgb", "depth", "opacity", "disp_map")}
    before = dict(cam)
    light = {f"depth_{lvl}": torch.rand(wh * wh) for lvl in LEVELS}
    ppc = {"eye_pos": torch.rand(n, 3), "camera": torch.rand(n, 3, 3)}
    light_ppc = {"eye_pos": torch.rand(3), "camera": torch.rand(3, 3)}
    out = RGS.efficient_sm(torch.rand(n, 3), torch.rand(wh * wh, 3), cam, light, ppc, light_ppc,
                           (wh, wh), True, light_fine, "shadow_method_1")
    assert out is cam
    assert sorted(out) == sorted(list(before) + ["sm_coarse", "sm_fine"])
    for k, v in before.items():
        assert out[k] is v, k
    assert torch.equal(out["sm_coarse"], torch.full((n, 3), 1.0))
    assert torch.equal(out["sm_fine"], torch.full((n, 3), 2.0))
    assert maps[0][0] is before["depth_coarse"] and maps[1][0] is before["depth_fine"]
    assert all(m[2] == "shadow_method_1" and m[3] == ESM.EPSILON for m in maps)
    if light_fine:
        assert len(normed) == 2 and normed[1] is light["depth_fine"]
        assert maps[1][1] is not maps[0][1]
    else:
        assert len(normed) == 1 and normed[0] is light["depth_coarse"]
        assert maps[1][1] is maps[0][1]
    # coarse only: no fine level is touched
    cam2 = {k: v for k, v in before.items() if k.endswith("coarse")}
    out2 = RGS.efficient_sm(torch.rand(n, 3), torch.rand(wh * wh, 3), cam2, light, ppc, light_ppc,
                            (wh, wh), False, light_fine, "shadow_method_2")
    assert sorted(out2) == sorted([k for k in before if k.endswith("coarse")] + ["sm_coarse"])


def test_fixtures_are_not_degenerate():
    for case in FINITE:
        fx = load_rgb_sm(case)
        outs = [k for k in fx if k.startswith("out_")]
        assert len(outs) >= 8
        for k in outs:
            assert np.isfinite(fx[k]).all(), (case, k)
            assert fx[k].std() > 0, (case, k, "constant")
        assert os.path.getsize(os.path.join(RGB_SM, case + ".npz")) <= 578 * 1024
    fx = load_rgb_sm("juntos_nan")
    assert np.isnan(fx["out_disp_map_fine"]).all()
    assert np.isfinite(fx["out_disp_map_coarse"]).all()


def test_disp_entry_points_validate_before_launch():
    """sizes and pointers are checked before anything is launched; an empty
    batch is a no-op; g_disp needs the forward's depth and opacity"""
    from nerf_pl_amd import _lib
    L = _lib.lib()
    N, P, EINVAL = None, 0x10000, 10001
    fwd = [N, 4, 3, N, N, N, 1.0, 0, 1, 4, 64, 0, 0, N, N, N, N, N, N]
    bwd = [N, 4, 3, N, N, N, 1.0, 0, 1, 4, 64, 0, N, N, N, N, N, N, N, N]

    def with_(args, **kw):
        a = list(args)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return a
    cases = [("nr_composite_disp_fwd", fwd, EINVAL),
             ("nr_composite_disp_fwd", with_(fwd, _9=-1), EINVAL),
             ("nr_composite_disp_fwd", with_(fwd, _9=0), 0),
             ("nr_composite_disp_fwd", with_(fwd, _10=0), EINVAL),
             # every pointer but disp
             ("nr_composite_disp_fwd", with_(fwd, _0=P, _3=P, _4=P, _13=P, _14=P, _15=P, _17=P),
              EINVAL),
             ("nr_composite_disp_bwd", bwd, EINVAL),
             ("nr_composite_disp_bwd", with_(bwd, _9=-1), EINVAL),
             ("nr_composite_disp_bwd", with_(bwd, _9=0), 0),
             # g_disp without depth / opacity
             ("nr_composite_disp_bwd", with_(bwd, _0=P, _3=P, _4=P, _15=P, _18=P), EINVAL)]
    for entry, args, rc in cases:
        got = getattr(L, entry)(*args)
        assert got == rc, f"{entry}{tuple(args)} returned {got}: {_lib.last_error()}"
        if rc == EINVAL:
            assert entry in _lib.last_error(), _lib.last_error()
