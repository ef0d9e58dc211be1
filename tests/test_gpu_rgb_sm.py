"""The joint RGB + shadow-map render path on the GPU: the disparity compositing
kernels (csrc/render.hip, nr_composite_disp_fwd / nr_composite_disp_bwd) called
directly, the reference fixtures end to end (tests/golden/rgb_sm, produced by
running the reference's models/rendering_rgb_sm.py), and the consistency of
nerf_pl_amd.rendering_rgb_sm with nerf_pl_amd.rendering.

Kernels (inputs of tests/composite64.make_case, the shapes and regimes of
tests/test_gpu_composite.py):

* forward: rgb, depth, opacity, weights carry ops.composite_forward's bits;
  disp is NaN exactly where opacity == 0 and elsewhere within 2^-22 |disp| of
  1 / max(1e-10, D / O) evaluated in float64 from the kernel's own fp32 D and O
  (two fp32 operations of one ulp, 2^-23, each);
* backward without g_disp: ops.composite_backward's bits;
* backward with g_disp: against composite64.Composite64.backward with the
  disparity's gradient folded into g_depth and g_opacity in longdouble, at
  test_gpu_composite.py's bound 2^-22 |ref| + 1e-12 M_i + 2^-126 (exact zeros
  where the reference is zero); rays of NaN disparity left out.

Fixtures: the CPU test's tolerances (tests/test_rgb_sm_host.py); sm_* at the
shadow tests' tolerances and screening (tests/test_gpu_shadow.py) with the 5%
cap; loss at rtol 1e-5 when nothing is screened; parameter gradients normwise
within max(1e-4, sqrt(2) x the reference's fp32-vs-float64 distance) per tensor.
"""
import numpy as np
import pytest
import torch

import composite64 as C64
import parity
from oracle import nerf_oracle as O
from oracle import shadow_oracle as SO
from test_gpu_composite import (NAMES, RAYS, SEED, STREAM, SUBSETS, case, group, ratio_to_bound,
                                same_bits)
from test_gpu_shadow import _check_rows, levels, light_map, shadow_diffs, texel_keys
from test_rgb_sm_host import (LEVELS, build_models, check_render, draws_of, load_rgb_sm,
                              rgb_sm_cfg, run_renders, screen)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
T = torch.from_numpy
SAMPLES = (1, 2, 3, 63, 64, 65, 129, 193)
SHAPES = [(S, n) for S in SAMPLES for n in RAYS]
F32 = np.float32


def g_disp_of(S, n):
    return np.random.default_rng([5, S, n]).standard_normal(n).astype(F32)


def dev(a):
    return None if a is None else T(np.ascontiguousarray(a)).to(DEV)


def disp_forward(k, raw, white_back):
    from nerf_pl_amd import ops
    return ops.composite_disp_forward(*k.fwd_args(raw), white_back)


def disp_backward(k, raw, white_back, g, g_disp=None, depth=None, opacity=None):
    from nerf_pl_amd import ops
    return ops.composite_disp_backward(*k.fwd_args(raw), white_back, g["g_rgb"], g["g_depth"],
                                       g["g_opacity"], g_disp, depth, opacity)


@pytest.mark.parametrize("regime", C64.REGIMES)
def test_disp_forward(regime):
    """Measured on the MI355X, worst |disp - ref| / |disp| per regime: typical
    7.7e-8, opaque 6.9e-8, last 7.9e-8, noise 6.0e-8, ndc 7.8e-8 (bound 2^-22 =
    2.4e-7); closed is all NaN.  NaN rays of 43 at S = 2 / 3: typical 16 / 7,
    opaque 3 / 0, last 0 / 0, noise 14 / 5, ndc 12 / 5."""
    from nerf_pl_amd import ops
    worst, mixed = 0.0, {2: [0, 0], 3: [0, 0]}
    for S, n in SHAPES:
        k = case(regime, S, n)
        for raw in (k.raw4, k.raw1):
            what = f"{regime} S={S} n={n} stride {raw.shape[-1]}"
            outs = {}
            for wb in (False, True):
                rgb, depth, opac, disp, w = outs[wb] = disp_forward(k, raw, wb)
                base = ops.composite_forward(*k.fwd_args(raw), wb)
                assert (rgb is None) == (raw is k.raw1) and (base[0] is None) == (rgb is None)
                for got, exp, q in zip((rgb, depth, opac, w), base, ("rgb", "depth", "opacity", "w")):
                    assert got is None or same_bits(got, exp), f"{what} white_back={wb}: {q}"
                assert disp.shape == (n,)
            # white_back does not enter (rendering_rgb_sm.py:197-200)
            assert np.array_equal(outs[False][3].cpu().numpy(), outs[True][3].cpu().numpy(),
                                  equal_nan=True), what
            _, depth, opac, disp, _ = outs[False]
            D, Op, got = depth.cpu().numpy(), opac.cpu().numpy(), disp.cpu().numpy()
            nan = Op == 0
            assert np.array_equal(np.isnan(got), nan), f"{what}: NaN placement"
            with np.errstate(all="ignore"):
                q = D.astype(np.float64) / Op.astype(np.float64)
                ref = 1.0 / np.maximum(1e-10, q)
            err = np.abs(got[~nan] - ref[~nan]) / np.abs(got[~nan])
            worst = max(worst, float(err.max(initial=0)))
            assert (err <= 2.0 ** -22).all(), f"{what}: disp {err.max():.3g} relative"
            if S == 1 or regime == "closed":
                assert nan.all(), what
            elif S >= 63:
                assert not nan.any() and q.min() > 1e-10, f"{what}: min q {q.min():.3g}"
            elif raw is k.raw4:
                mixed[S][0] += int(nan.sum())
                mixed[S][1] += n
    if regime == "typical":     # S = 2, 3: NaN and finite disparities in one launch
        for S, (a, b) in mixed.items():
            assert 0 < a < b, (S, a, b)
    print(f"disp forward {regime}: worst |disp - ref| / |disp| {worst:.3g} (bound {2.0 ** -22:.3g}); "
          f"NaN rays at S=2, 3: {mixed}")


def clamp_case(S):
    """make_case('typical', S, 5) with ray 2 remade: z_0 = 0, sample 0 opaque,
    every later sigma < 0 -- depth exactly 0, opacity 1, q = 0: the clamp"""
    cs = {k: (None if v is None else np.array(v)) for k, v in C64.make_case("typical", S, 5).items()}
    raw = cs["raw"].reshape(5, S, 4)
    cs["z"][2, 0] = 0.0
    raw[2, 0, 3] = 1e4
    raw[2, 1:, 3] = -1.0
    return cs


@pytest.mark.parametrize("S", [3, 65])
def test_clamped_ray(S):
    from nerf_pl_amd import ops
    cs = clamp_case(S)
    raw, z, rays = dev(cs["raw"]), dev(cs["z"]), dev(cs["rays"])
    args = (raw, z, rays, None, 0.0, SEED, STREAM, False)
    rgb, depth, opac, disp, w = ops.composite_disp_forward(*args)
    assert depth[2].item() == 0.0 and opac[2].item() == 1.0
    assert disp.cpu().numpy()[2] == F32(1e10)
    others = [0, 1, 3, 4]
    g = {x: dev(cs[x]) for x in NAMES}
    gq = dev(g_disp_of(S, 5))
    alone = ops.composite_disp_backward(*args, None, None, None, gq, depth, opac).view(5, S, 4)
    assert not alone[2].any(), "g_disp reached a clamped ray"
    assert alone[others].any()
    both = ops.composite_disp_backward(*args, g["g_rgb"], g["g_depth"], g["g_opacity"], gq,
                                       depth, opac).view(5, S, 4)
    plain = ops.composite_backward(*args, g["g_rgb"], g["g_depth"], g["g_opacity"]).view(5, S, 4)
    assert same_bits(both[2], plain[2])
    assert not same_bits(both[others], plain[others])


@pytest.mark.parametrize("regime", C64.REGIMES)
def test_backward_without_g_disp_is_composite_backward(regime):
    from nerf_pl_amd import ops
    for S, n in SHAPES:
        k = case(regime, S, n)
        for wb in (False, True):
            _, depth, opac, _, _ = disp_forward(k, k.raw4, wb)
            for names in [()] + SUBSETS:
                g = {x: (k.g[x] if x in names else None) for x in NAMES}
                for raw in (k.raw4, k.raw1):
                    if raw is k.raw1 and "g_rgb" in names:
                        continue
                    exp = ops.composite_backward(*k.fwd_args(raw), wb, g["g_rgb"], g["g_depth"],
                                                 g["g_opacity"])
                    what = (regime, S, n, wb, names, raw.shape[-1])
                    assert same_bits(disp_backward(k, raw, wb, g), exp), what
                    # the forward's outputs handed over, still no g_disp
                    assert same_bits(disp_backward(k, raw, wb, g, None, depth, opac), exp), what


def folded_reference(monkeypatch, regime, S, white_back, names):
    """(d sigma, d c, M, kept rays) of the (regime, S) group: Composite64.backward
    with g_disp folded into g_depth and g_opacity in longdouble from the
    kernel's own fp32 D and O -- where q = D / O > 1e-10 (the kernel's fp32
    quotient), g_depth += g_disp (-O / D^2) and g_opacity += g_disp / D"""
    grp = group(regime, S)
    D, Op = [], []
    for n in RAYS:
        k = case(regime, S, n)
        _, depth, opac, _, _ = disp_forward(k, k.raw4, False)
        D.append(depth.cpu().numpy())
        Op.append(opac.cpu().numpy())
    D, Op = np.concatenate(D), np.concatenate(Op)
    gq = np.concatenate([g_disp_of(S, n) for n in RAYS])
    W = C64.WIDE
    with np.errstate(all="ignore"):
        q = D / Op
        assert q.dtype == F32
        on = q > F32(1e-10)
        Dw, Ow, gw = D.astype(W), Op.astype(W), gq.astype(W)
        gd = np.where(on, gw * (-Ow / (Dw * Dw)), W(0))
        go = np.where(on, gw / Dw, W(0))
    if "g_depth" in names:
        gd = gd + grp.g["g_depth"].astype(W)
    if "g_opacity" in names:
        go = go + grp.g["g_opacity"].astype(W)
    f32 = C64._f32
    # the folded gradients are no fp32 values: let them through as they are
    monkeypatch.setattr(C64, "_f32", lambda t: t if isinstance(t, np.ndarray) and t.dtype == W
                        and W is not F32 else f32(t))
    dsig, dc, M = grp.fw.backward(white_back, grp.g["g_rgb"] if "g_rgb" in names else None, gd, go)
    monkeypatch.setattr(C64, "_f32", f32)
    return dsig, dc, M, ~np.isnan(q)


@pytest.mark.parametrize("white_back", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("names", [(), NAMES], ids=["alone", "with-all"])
@pytest.mark.parametrize("regime", C64.REGIMES)
def test_backward_with_g_disp_matches_composite64(monkeypatch, regime, names, white_back):
    """The kernel adds g_disp (D - O z_i) / D^2 to dw_i as one difference: the two
    folded terms cancel on a ray whose weight sits on one sample (D = O z_i),
    where the reference's gradient is exactly 0 (csrc/render.hip
    composite_bwd_kernel).  Measured on the MI355X, worst ratio to the bound
    over every shape and background, d sigma / d c: g_disp alone 0.249 / 0
    (noise), with all four gradients 0.248 / 0.474 (typical, ndc); closed 0 / 0
    (every ray's disparity is NaN)."""
    worst = [0.0, 0.0, None]
    for S in SAMPLES:
        dsig, dc, M, keep = folded_reference(monkeypatch, regime, S, white_back, names)
        if S >= 63 and regime != "closed":
            assert keep.all(), f"{regime} S={S}: rays of NaN disparity left out"
        for i, n in enumerate(RAYS):
            k = case(regime, S, n)
            rows = k.rows
            kp = keep[rows]
            g = {x: (k.g[x] if x in names else None) for x in NAMES}
            _, depth, opac, _, _ = disp_forward(k, k.raw4, white_back)
            gq = dev(g_disp_of(S, n))
            got = disp_backward(k, k.raw4, white_back, g, gq, depth, opac)
            got = got.cpu().numpy().reshape(n, S, 4)
            what = f"{regime} S={S} n={n} {'+'.join(names) or 'g_disp alone'} white_back={white_back}"
            assert np.isfinite(got).all(), what
            rs = ratio_to_bound(got[kp][..., 3], dsig[rows][kp], 1e-12 * M[rows][kp],
                                what + " d sigma")
            rc = ratio_to_bound(got[kp][..., :3], dc[rows][kp], 0, what + " d c")
            if rs > worst[0] or rc > worst[1]:
                worst = [max(rs, worst[0]), max(rc, worst[1]), what]
            assert rs <= 1 and rc <= 1, f"{what}: d sigma {rs:.3g}, d c {rc:.3g} of the bound"
            # a ray of NaN disparity gets nr_composite_bwd's gradient
            plain = disp_backward(k, k.raw4, white_back, g).cpu().numpy().reshape(n, S, 4)
            assert np.array_equal(got[~kp].view(np.int32), plain[~kp].view(np.int32)), what
            if not names:
                # sigma-only rows: the stride-4 call's sigma column, bit for bit
                got1 = disp_backward(k, k.raw1, white_back, g, gq, depth, opac)
                assert got1.shape == (n * S, 1)
                assert same_bits(got1[:, 0], T(got[..., 3].reshape(-1))), what + " stride 1"
    print(f"disp backward {regime} {'+'.join(names) or 'g_disp alone'} white_back={white_back}: "
          f"worst ratio to the bound d sigma {worst[0]:.3g}, d c {worst[1]:.3g} ({worst[2]})")


def test_autograd_is_the_direct_call():
    """functions.composite_disp_apply: a loss on disp reaches the kernel as
    g_disp with the forward's saved depth and opacity; a loss that leaves disp
    out is _Composite's backward, bit for bit (no gradient is materialised)"""
    from nerf_pl_amd import functions
    for regime, S, n in (("typical", 65, 37), ("noise", 129, 5), ("opaque", 3, 37)):
        k = case(regime, S, n)
        for raw0 in (k.raw4, k.raw1):
            raw = raw0.clone().requires_grad_(True)
            rgb, depth, opac, disp, w = functions.composite_disp_apply(*k.fwd_args(raw), True)
            assert not w.requires_grad
            gq = dev(g_disp_of(S, n))
            keep = ~torch.isnan(disp)
            (disp[keep] * gq[keep]).sum().backward()
            none = {x: None for x in NAMES}
            direct = disp_backward(k, raw0, True, none, torch.where(keep, gq, torch.zeros_like(gq)),
                                   depth.detach(), opac.detach())
            assert same_bits(raw.grad, direct), (regime, S, n, raw0.shape[-1])
            raw_a = raw0.clone().requires_grad_(True)
            raw_b = raw0.clone().requires_grad_(True)
            a = functions.composite_disp_apply(*k.fwd_args(raw_a), True)
            b = functions.composite_apply(*k.fwd_args(raw_b), True)
            ((a[1] * k.g["g_depth"]).sum() + (a[2] * k.g["g_opacity"]).sum()).backward()
            ((b[1] * k.g["g_depth"]).sum() + (b[2] * k.g["g_opacity"]).sum()).backward()
            assert same_bits(raw_a.grad, raw_b.grad), (regime, S, n, raw0.shape[-1])


# ---------------------------------------------------------------------------
# fixtures end to end
# ---------------------------------------------------------------------------
def joint_loss(out, fx, cfg, screened=None):
    """rgb_weight * MSE(rgb_*) + sm_weight * SMMSE(sm_*) (train_rgb_sm_juntos.py:
    181-184); ``screened`` rays' targets are their own outputs"""
    d = out["rgb_coarse"]
    keep = None if screened is None else torch.as_tensor(~screened, device=d.device)[:, None]
    loss = 0
    for key, tkey, wt in (("rgb", "target", cfg["rgb_weight"]), ("sm", "target_sm", cfg["sm_weight"])):
        for lvl in LEVELS:
            v = out[f"{key}_{lvl}"]
            t = T(fx[tkey]).to(v.device, v.dtype)
            if keep is not None:
                t = torch.where(keep, t, v.detach())
            loss = loss + wt * torch.mean((v - t) ** 2)
    return loss


def oracle_step(fx, cfg, screened):
    """the joint step by the fp32 oracle (the reference's arithmetic) on the
    loss without the screened rays; returns the parameters with their gradients"""
    params = [{k: v.requires_grad_(True)
               for k, v in O.make_params(cfg["seeds"][m], sigma_bias=cfg["sigma_bias"][m]).items()}
              for m in range(2)]
    rng = O.ReplayRNG(draws_of(fx))
    a = (cfg["N_samples"], False, cfg["perturb"], cfg["noise_std"])
    cam = O.render_rays(params, T(fx["rays"]), *a, cfg["N_importance"], rng=rng)
    with torch.set_grad_enabled(cfg["grad_on_light"]):
        light = O.render_rays(params, T(fx["light_rays"]), *a, cfg["light_importance"], rng=rng)
    assert rng.exhausted()
    wh = cfg["wh"]
    sm = SO.efficient_sm(T(fx["pixels"]), T(fx["light_pixels"]), cam, light,
                         {"eye_pos": T(fx["eye_pos"]), "camera": T(fx["camera"])},
                         T(fx["light_eye"]), T(fx["light_camera"]), (wh, wh), True,
                         cfg["light_importance"] > 0, cfg["method"])
    out = dict(cam, sm_coarse=sm["rgb_coarse"], sm_fine=sm["rgb_fine"])
    joint_loss(out, fx, cfg, screened).backward()
    return params


def check_gradients(case_name, fx, models, ref_params=None):
    """normwise <= max(1e-4, sqrt(2) bound64) per tensor against the fixture's
    gradients (or, after screening, the oracle's on the masked loss)"""
    for m, net in enumerate(models):
        for name, p in net.named_parameters():
            key = f"grad{m}_{name}"
            g = p.grad.detach().cpu().numpy().astype(np.float64).reshape(-1)
            if ref_params is not None:
                ref, got = ref_params[m][name].grad.double().reshape(-1).numpy(), g
                b64 = float(fx.get(key + "_bound64"))
            elif key + "_full" in fx:
                ref, got = fx[key + "_full"].astype(np.float64).reshape(-1), g
                b64 = float(fx[key + "_bound64"])
            else:
                ref, got = fx[key + "_val"].astype(np.float64), g[fx[key + "_idx"]]
                b64 = float(fx[key + "_pbound64"])
            bound = max(1e-4, np.sqrt(2.0) * b64)
            d = np.linalg.norm(got - ref) / (np.linalg.norm(ref) + 1e-30)
            print(f"{key}: normwise {d:.3g} (bound {bound:.3g})")
            assert d <= bound, f"{case_name} {key}: normwise deviation {d:.3g} > {bound:.3g}"


def render_and_check(case_name):
    fx = load_rgb_sm(case_name)
    cfg = rgb_sm_cfg(fx)
    models = build_models(cfg, DEV)
    cam, light, ccap, lcap = run_renders(fx, cfg, models, lambda k: T(fx[k]).to(DEV))
    cam_flip = screen(fx, cfg, ccap)
    check_render(case_name, cam, fx, "out_", cam_flip)
    n_light = fx["light_rays"].shape[0] if light is not None else 0
    light_flip = np.zeros(n_light, bool)
    if light is not None:
        if cfg["light_importance"] > 0:
            light_flip = screen(fx, cfg, lcap, True)
        check_render(case_name + "/light", light, fx, "light_", light_flip)
    print(f"{case_name}: sample_pdf knot flips: {int(cam_flip.sum())} camera, "
          f"{int(light_flip.sum())} light rays")
    return fx, cfg, models, cam, light, cam_flip, light_flip


@pytest.mark.parametrize("case_name", ["juntos_sm2", "juntos_gol_sm1"])
def test_joint_training_step_matches_reference(case_name):
    """train_rgb_sm_juntos.py:137-199 through the drop-in API, replaying the
    reference's draws: full-MLP camera render, full-MLP light render (under
    autograd for --grad_on_light), efficient_sm, the weighted loss, backward.
    Measured on the MI355X: no ray screened in either case; sm_* within 1.2e-7
    (juntos_sm2) and 6.0e-6 (juntos_gol_sm1); loss 0.31010583 against 0.3101058
    and 0.48389155 against 0.48389164; largest normwise gradient deviation
    6.8e-7 (juntos_sm2) and 9.94e-5 of the 1e-4 bound (juntos_gol_sm1, the fine
    model's sigma.weight, the same figure in two runs: shadow_method_1 divides
    the depth difference by delta = 1e-2)."""
    from nerf_pl_amd import rendering_rgb_sm as RGS
    fx, cfg, models, cam, light, cam_flip, light_flip = render_and_check(case_name)
    wh, method = cfg["wh"], cfg["method"]
    n_cam = fx["rays"].shape[0]
    before = dict(cam)
    ppc = {"eye_pos": T(fx["eye_pos"]).to(DEV), "camera": T(fx["camera"]).to(DEV)}
    light_ppc = {"eye_pos": T(fx["light_eye"]), "camera": T(fx["light_camera"])}
    out = RGS.efficient_sm(T(fx["pixels"]), T(fx["light_pixels"]), cam, light, ppc, light_ppc,
                           (wh, wh), True, cfg["light_importance"] > 0, method)
    assert sorted(out) == sorted(k[4:] for k in fx if k.startswith("out_"))
    assert all(out[k] is v for k, v in before.items())
    # screening of test_gpu_shadow.check_training_step, per shadow level
    runs = SO.shadow_runs(T(fx["eye_pos"]))
    screened = np.zeros(n_cam, bool)
    tol_sm = 1e-4 if method == "shadow_method_1" else 2e-5
    for lvl, dkey, lkey in levels(fx, cfg):
        own = cam_flip if lvl == "fine" else np.zeros(n_cam, bool)
        k_ref, _ = texel_keys(fx, fx[dkey], wh)
        k_our, m_our = texel_keys(fx, cam[dkey[4:]].detach().cpu().numpy(), wh)
        lflip = light_flip if lkey == "light_depth_fine" else np.zeros_like(light_flip)
        bad = own | (k_ref != k_our) | (m_our < 1e-4) | lflip[k_ref] | lflip[k_our]
        if method == "shadow_method_2" and bad.any():
            d_ref = shadow_diffs(fx, fx[dkey], light_map(fx, lkey).numpy(), wh)
            lw_our = light_map(fx, None, T(light[lkey[6:]].detach().cpu().numpy())).numpy()
            d_our = shadow_diffs(fx, cam[dkey[4:]].detach().cpu().numpy(), lw_our, wh)
            for s, e in runs:
                if not bad[s:e].any():
                    continue
                ext_r = np.array([d_ref[s:e].min(), d_ref[s:e].max()])
                ext_o = np.array([d_our[s:e].min(), d_our[s:e].max()])
                if (np.abs(ext_o - ext_r) > 1e-5 * np.maximum(1.0, np.abs(ext_r))).any():
                    bad[s:e] = True
        screened |= bad
        _check_rows(f"{case_name}/sm_{lvl}", out[f"sm_{lvl}"].detach().cpu().numpy(),
                    fx[f"out_sm_{lvl}"], tol_sm, False, bad)
    assert screened.mean() <= 0.05, f"{int(screened.sum())} screened camera rays"

    loss = joint_loss(out, fx, cfg)
    clean = not screened.any()
    print(f"{case_name}: loss {loss.item():.8g} (reference {float(fx['loss']):.8g}), "
          f"{int(screened.sum())} camera rays screened")
    np.testing.assert_allclose(loss.item(), float(fx["loss"]), rtol=1e-5 if clean else 2e-3)
    if clean:
        loss.backward()
        check_gradients(case_name, fx, models)
    else:
        joint_loss(out, fx, cfg, screened).backward()
        check_gradients(case_name, fx, models, oracle_step(fx, cfg, screened))


def test_disparity_loss_gradients_match_reference():
    """juntos_disp_loss: the reference's autograd through 1 / max(1e-10, depth /
    sum(weights)) against nr_composite_disp_bwd under the drop-in render"""
    fx, cfg, models, cam, _, cam_flip, _ = render_and_check("juntos_disp_loss")
    assert not cam_flip.any()
    tgt, td = T(fx["target"]).to(DEV), T(fx["target_disp"]).to(DEV)
    loss = 0
    for lvl in LEVELS:
        loss = loss + torch.mean((cam["rgb_" + lvl] - tgt) ** 2)
    loss = loss + torch.mean((cam["disp_map_fine"] - td) ** 2) + \
        torch.mean((cam["disp_map_coarse"] - td) ** 2)
    np.testing.assert_allclose(loss.item(), float(fx["loss"]), rtol=1e-5)
    loss.backward()
    check_gradients("juntos_disp_loss", fx, models)


def test_nan_disparity_fixture():
    fx, cfg, models, cam, _, _, _ = render_and_check("juntos_nan")
    assert torch.isnan(cam["disp_map_fine"]).all() and not cam["opacity_fine"].any()
    assert torch.isfinite(cam["disp_map_coarse"]).all()


# ---------------------------------------------------------------------------
# consistency
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("test_time", [False, True], ids=["train", "test_time"])
def test_shared_keys_are_rendering_render_rays(test_time):
    from nerf_pl_amd import Embedding, ReplayRNG, render_rays
    from nerf_pl_amd import rendering_rgb_sm as RGS
    fx = load_rgb_sm("juntos_sm2")
    cfg = rgb_sm_cfg(fx)
    models = build_models(cfg, DEV)
    draws = draws_of(fx)[:5]
    args = (models, [Embedding(3, 10), Embedding(3, 4)], T(fx["rays"]).to(DEV), 16, False, 1.0,
            1.0, 16, 32768, False, test_time)
    with torch.set_grad_enabled(not test_time):
        a = RGS.render_rays(*args, rng=ReplayRNG(draws))
        b = render_rays(*args, rng=ReplayRNG(draws))
    extra = ["disp_map_fine"] + ([] if test_time else ["disp_map_coarse"])
    assert sorted(a) == sorted(list(b) + extra)
    assert ("rgb_coarse" in b) == (not test_time)
    for k in b:
        assert same_bits(a[k], b[k]), k
    for lvl in LEVELS[1 if test_time else 0:]:
        d, o = a["depth_" + lvl].double(), a["opacity_" + lvl].double()
        np.testing.assert_allclose(a["disp_map_" + lvl].detach().cpu().numpy(),
                                   (1 / torch.clamp_min(d / o, 1e-10)).detach().cpu().numpy(),
                                   rtol=2.0 ** -22)


def test_depth_only_light_render():
    """depth_only=True: the same models' sigma-only graph -- depth / opacity
    within parity.TOL of the full render, no rgb_*, and after a backward
    through sm_* nothing reaches the rgb head"""
    from nerf_pl_amd import rendering_rgb_sm as RGS
    from nerf_pl_amd.functions import _SIGMA_ONLY_UNUSED
    fx = load_rgb_sm("juntos_gol_sm1")
    cfg = rgb_sm_cfg(fx)
    wh = cfg["wh"]
    rays_of = lambda k: T(fx[k]).to(DEV)   # noqa: E731
    full_models = build_models(cfg, DEV)
    _, full_light, _, _ = run_renders(fx, cfg, full_models, rays_of)
    ppc = {"eye_pos": rays_of("eye_pos"), "camera": rays_of("camera")}
    light_ppc = {"eye_pos": T(fx["light_eye"]), "camera": T(fx["light_camera"])}
    for cam_depth_only in (False, True):
        models = build_models(cfg, DEV)
        if cam_depth_only:
            from nerf_pl_amd import Embedding, ReplayRNG
            rng = ReplayRNG(draws_of(fx))
            emb = [Embedding(3, 10), Embedding(3, 4)]
            a = (cfg["N_samples"], False, cfg["perturb"], cfg["noise_std"])
            cam = RGS.render_rays(models, emb, rays_of("rays"), *a, cfg["N_importance"],
                                  rng=rng, depth_only=True)
            light = RGS.render_rays(models, emb, rays_of("light_rays"), *a,
                                    cfg["light_importance"], rng=rng, depth_only=True)
            assert rng.exhausted()
            assert sorted(cam) == sorted(f"{q}_{lvl}" for lvl in LEVELS
                                         for q in ("depth", "opacity", "disp_map"))
        else:
            cam, light, _, _ = run_renders(fx, cfg, models, rays_of, {"depth_only": True})
        assert sorted(light) == ["depth_coarse", "disp_map_coarse", "opacity_coarse"]
        assert light["depth_coarse"].requires_grad        # --grad_on_light
        for k in ("depth_coarse", "opacity_coarse"):
            err = (light[k] - full_light[k]).abs().max().item()
            print(f"depth_only light {k}: max |sigma-only - full| {err:.3g}")
            assert err <= parity.TOL, (k, err)
        out = RGS.efficient_sm(T(fx["pixels"]), T(fx["light_pixels"]), cam, light, ppc, light_ppc,
                               (wh, wh), True, False, cfg["method"])
        tsm = rays_of("target_sm")
        (torch.mean((out["sm_coarse"] - tsm) ** 2) + torch.mean((out["sm_fine"] - tsm) ** 2)).backward()
        for m, net in enumerate(models):
            for name, p in net.named_parameters():
                if name in _SIGMA_ONLY_UNUSED:
                    if cam_depth_only:
                        assert p.grad is None, (m, name)
                    else:
                        assert p.grad is None or not p.grad.any(), (m, name)
                else:
                    assert p.grad is not None and p.grad.any(), (m, name)
