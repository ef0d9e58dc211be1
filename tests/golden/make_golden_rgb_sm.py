"""Golden fixtures for the joint RGB + shadow-map path, made by running the
REFERENCE (``models/rendering_rgb_sm.py``, ``losses.py``,
``models/efficient_shadow_mapping.py``, ``models/camera.py``) here, in the build
container:

    python tests/golden/make_golden_rgb_sm.py [case ...]   # default: all

Scene, per-pose camera runs (pose A, pose B, pose A again) and the recording
of every random draw are those of make_golden_shadow.py; 16x16 light image, 48
camera rays, 16 + 16 samples.  Output: ``tests/golden/rgb_sm/<case>.npz`` (plain
arrays, no pickle).

* ``juntos_sm2`` -- one step of train_rgb_sm_juntos.py:137-199: the full-MLP
  render of the camera batch, the full-MLP render of the light image under
  ``no_grad`` with ``Light_N_importance`` > 0, ``efficient_sm``
  (shadow_method_2) and ``rgb_weight * MSE(rgb_*) + sm_weight * SMMSE(sm_*)``
  with weights 1.0 / 0.5 (unequal, so that swapped weights show), backward.
* ``juntos_gol_sm1`` -- the same with ``--grad_on_light`` (:156-159),
  shadow_method_1, light coarse only.
* ``juntos_disp_loss`` -- the render alone with the loss MSE(rgb_*) +
  mean((disp_map_fine - t)^2) + mean((disp_map_coarse - t)^2): the reference's
  autograd through its disparity line (rendering_rgb_sm.py:197).
* ``juntos_nan`` -- forward only, the fine model's sigma bias -5: every fine
  sigma is <= 0, ``opacity_fine`` == 0 and ``disp_map_fine`` is NaN on every
  ray (0 / 0 through torch.max) while ``disp_map_coarse`` stays finite.

Recorded: draws (``draw<i>``, camera render first), inputs, ``out_*`` (the
camera result dict after ``efficient_sm``), ``light_*``, the reference's
importance depths and the coarse weights they were drawn from (``z_pdf`` /
``wpdf``, ``light_z_pdf`` / ``light_wpdf``: sample_pdf's discontinuity is
screened against them), targets, loss, and per parameter tensor the gradient's
sum, norm, values (whole when small, else probes) and its distance from the
same step in float64 (``*_bound64`` / ``*_pbound64``, by the oracle).

Asserted here, on the reference's data alone: in the first three cases every
output is finite and not constant; at most one camera ray has an importance
draw within tests/screening.py's window of a CDF knot.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, REPO)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(REPO, "tests"))

from make_golden import RecordingTorch, import_reference  # noqa: E402
from make_golden_shadow import scene  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402
from oracle import shadow_oracle as SO  # noqa: E402
from oracle.nerf_oracle import make_params  # noqa: E402
from screening import _cdf  # noqa: E402

OUT = os.path.join(HERE, "rgb_sm")
WH, N_SAMPLES, N_IMPORTANCE = 16, 16, 16
RUNS = [(0, 20), (1, 16), (0, 12)]
SEEDS = (31, 32)
N_PROBE = 2048
KNOT_WINDOW = 1e-5          # screening.pdf_flips' thr
MAX_BYTES = 578 * 1024      # the largest shadow fixture


def disparity(depth, opacity):
    """rendering_rgb_sm.py:197 on a result dict's depth and opacity"""
    return 1. / torch.max(1e-10 * torch.ones_like(depth), depth / opacity)


def step_loss(kind, out, tgt, tgt_sm, tgt_disp, rgb_weight, sm_weight):
    """the case's loss of a result dict (losses.py:4-26 written out)"""
    def both(key, t):
        v = torch.mean((out[key + "_coarse"] - t) ** 2)
        if key + "_fine" in out:
            v = v + torch.mean((out[key + "_fine"] - t) ** 2)
        return v
    if kind == "disp_loss":
        return both("rgb", tgt) + torch.mean((out["disp_map_fine"] - tgt_disp) ** 2) + \
            torch.mean((out["disp_map_coarse"] - tgt_disp) ** 2)
    return rgb_weight * both("rgb", tgt) + sm_weight * both("sm", tgt_sm)


def near_knot_rays(wpdf, u):
    """rays with an importance draw within KNOT_WINDOW of a knot of the CDF of
    the (padded) coarse weights ``wpdf``"""
    cdf = _cdf(wpdf).double().numpy()
    d = np.abs(cdf[:, None, :] - np.asarray(u, np.float64)[:, :, None]).min(-1)
    return (d < KNOT_WINDOW).any(1)


def oracle_step64(c, fx, rays, light_rays, pix, pixels, ppc, light, draws):
    """the case's step in float64 by the oracle: the full render is
    oracle.nerf_oracle.render_rays (rendering.py's, whose outputs the joint
    renderer shares) with the disparity line added, the shadow stage
    oracle.shadow_oracle.efficient_sm with its rgb_* outputs renamed sm_*"""
    dt = torch.float64
    params = [{k: v.to(dt).requires_grad_(True)
               for k, v in make_params(s, c["sigma_bias"][m]).items()}
              for m, s in enumerate(SEEDS)]
    rng = O.ReplayRNG([d for _, d in draws])
    rng._queue = [q.to(dt) for q in rng._queue]
    cam = O.render_rays(params, rays.to(dt), N_SAMPLES, False, c["perturb"], c["noise_std"],
                        N_IMPORTANCE, rng=rng)
    for lvl in ("coarse", "fine"):
        cam["disp_map_" + lvl] = disparity(cam["depth_" + lvl], cam["opacity_" + lvl])
    if c["kind"] == "juntos":
        with torch.set_grad_enabled(c["grad_on_light"]):
            lres = O.render_rays(params, light_rays.to(dt), N_SAMPLES, False, c["perturb"],
                                 c["noise_std"], c["light_importance"], rng=rng)
        ppc64 = {k: v.to(dt) for k, v in ppc.items()}
        sm = SO.efficient_sm(pix.to(dt), pixels.to(dt), cam, lres, ppc64, light.eye_pos.to(dt),
                             light.camera.to(dt), (WH, WH), True, c["light_importance"] > 0,
                             c["method"])
        cam["sm_coarse"], cam["sm_fine"] = sm["rgb_coarse"], sm["rgb_fine"]
    assert rng.exhausted()

    def t(k):
        return torch.from_numpy(fx[k]).to(dt)
    step_loss(c["kind"], cam, t("target"), t("target_sm"), t("target_disp"), c["rgb_weight"],
              c["sm_weight"]).backward()
    return params


def run_case(ref, name, c):
    ref_nerf, rs, camera_mod, ref_losses = ref
    seed = c["seed"]
    torch.manual_seed(seed)
    light, light_rays, pixels, cams = scene(WH, camera_mod.Camera)
    g = torch.Generator().manual_seed(seed)
    rays, pix, eyes, mats = [], [], [], []
    for pose, count in RUNS:
        cam, crays = cams[pose]
        idx = torch.randperm(crays.shape[0], generator=g)[:count]
        rays.append(crays[idx]); pix.append(pixels[idx])
        eyes.append(cam.eye_pos.expand(count, 3)); mats.append(cam.camera.expand(count, 3, 3))
    rays, pix = torch.cat(rays).contiguous(), torch.cat(pix).contiguous()
    ppc = {"eye_pos": torch.cat(eyes).contiguous(), "camera": torch.cat(mats).contiguous()}
    n = rays.shape[0]
    target = torch.rand(n, 3, generator=g)
    target_sm = torch.rand(n, 3, generator=g)
    target_disp = 0.2 * torch.rand(n, generator=g)

    models = []
    for m, s in enumerate(SEEDS):
        net = ref_nerf.NeRF()
        net.load_state_dict(make_params(s, sigma_bias=c["sigma_bias"][m]))
        models.append(net)
    emb = [ref_nerf.Embedding(3, 10), ref_nerf.Embedding(3, 4)]
    juntos, train = c["kind"] == "juntos", c["kind"] != "nan"

    pdf_log = []
    orig_pdf = rs.sample_pdf

    def sample_pdf_rec(rays_, weights, *a, **k):
        z = orig_pdf(rays_, weights, *a, **k)
        pdf_log.append((z.detach().clone(),
                        torch.nn.functional.pad(weights.detach().clone(), (1, 1))))
        return z

    torch.manual_seed(seed)
    rec = RecordingTorch()
    saved = rs.torch
    rs.torch, rs.sample_pdf = rec, sample_pdf_rec
    light_res = {}
    try:
        with torch.set_grad_enabled(train):
            cam_res = rs.render_rays(models, emb, rays, N_SAMPLES, False, c["perturb"],
                                     c["noise_std"], N_IMPORTANCE, 32768, False)
        if juntos:
            with torch.set_grad_enabled(c["grad_on_light"]):   # train_rgb_sm_juntos.py:156-164
                light_res = rs.render_rays(models, emb, light_rays, N_SAMPLES, False,
                                           c["perturb"], c["noise_std"], c["light_importance"],
                                           32768, False)
    finally:
        rs.torch, rs.sample_pdf = saved, orig_pdf
    cam_out = cam_res
    if juntos:
        cam_out = rs.efficient_sm(pix, pixels, cam_res, light_res, ppc, light,
                                  image_shape=(WH, WH), fine_sampling=True,
                                  Light_N_importance=c["light_importance"] > 0,
                                  shadow_method=c["method"])
    out = {
        # the layout of the shadow fixtures' cfg (test_shadow_golden.shadow_cfg)
        "cfg": np.array([WH, N_SAMPLES, N_IMPORTANCE, c["light_importance"],
                         1 if c["method"] == "shadow_method_1" else 2, c["sigma_bias"][0],
                         c["perturb"], c["noise_std"], SEEDS[0], SEEDS[1],
                         1 if c["grad_on_light"] else 0], dtype=np.float64),
        "kind": np.array(c["kind"]), "sigma_bias_fine": np.array(c["sigma_bias"][1]),
        "rgb_weight": np.array(c["rgb_weight"]), "sm_weight": np.array(c["sm_weight"]),
        "rays": rays.numpy(), "pixels": pix.numpy(), "eye_pos": ppc["eye_pos"].numpy(),
        "camera": ppc["camera"].numpy(), "target": target.numpy(),
        "target_sm": target_sm.numpy(), "target_disp": target_disp.numpy(),
        "n_draws": np.array(len(rec.draws)),
        "z_pdf": pdf_log[0][0].numpy(), "wpdf": pdf_log[0][1].numpy(),
    }
    if juntos:
        out.update({"light_rays": light_rays.numpy(), "light_pixels": pixels.numpy(),
                    "light_eye": light.eye_pos.numpy(), "light_camera": light.camera.numpy()})
        if c["light_importance"] > 0:
            out["light_z_pdf"], out["light_wpdf"] = pdf_log[1][0].numpy(), pdf_log[1][1].numpy()
    for i, (kind, t) in enumerate(rec.draws):
        out[f"draw{i}"] = t.numpy()
        out[f"draw{i}_kind"] = np.array(kind)
    for k, v in cam_out.items():
        out[f"out_{k}"] = v.detach().numpy()
    for k, v in light_res.items():
        out[f"light_{k}"] = v.detach().numpy()

    # conditions on the reference's data alone
    per = 1 if c["perturb"] > 0 else 0
    knots = near_knot_rays(out["wpdf"], rec.draws[per + 1][1].numpy())
    assert knots.sum() <= 1, f"{name}: {int(knots.sum())} camera rays draw next to a CDF knot"
    if train:
        for k, v in out.items():
            if k.startswith(("out_", "light_depth", "light_disp", "light_opacity", "light_rgb")):
                assert np.isfinite(v).all(), f"{name}: {k} is not finite"
                assert v.std() > 0, f"{name}: {k} is constant"
    else:
        assert np.isnan(out["out_disp_map_fine"]).all() and not out["out_opacity_fine"].any()
        assert np.isfinite(out["out_disp_map_coarse"]).all()

    if train:
        if juntos:       # train_rgb_sm_juntos.py:181-184, the reference's loss modules
            loss = c["rgb_weight"] * ref_losses.loss_dict["mse"]()(cam_out, target) + \
                c["sm_weight"] * ref_losses.loss_dict["sm"]()(cam_out, target_sm)
        else:
            loss = step_loss(c["kind"], cam_out, target, target_sm, target_disp, 1.0, 0.0)
        loss.backward()
        out["loss"] = np.array(loss.item(), dtype=np.float64)
        pg = np.random.Generator(np.random.PCG64(5))
        ref_grads, probes = {}, {}
        for m, net in enumerate(models):
            for pname, p in net.named_parameters():
                assert p.grad is not None, (name, pname)
                gr = p.grad.detach().numpy().astype(np.float32)
                key = f"grad{m}_{pname}"
                ref_grads[key] = gr
                out[key + "_sum"] = np.array(gr.astype(np.float64).sum())
                out[key + "_l2"] = np.array(np.sqrt((gr.astype(np.float64) ** 2).sum()))
                flat = gr.reshape(-1)
                if flat.size <= 1024:
                    out[key + "_full"] = gr
                else:
                    idx = np.sort(pg.choice(flat.size, N_PROBE, replace=False))
                    out[key + "_idx"] = idx.astype(np.int64)
                    out[key + "_val"] = flat[idx]
                    probes[key] = idx
        params64 = oracle_step64(c, out, rays, light_rays, pix, pixels, ppc, light, rec.draws)
        for m, p in enumerate(params64):
            for pname, w in p.items():
                key = f"grad{m}_{pname}"
                g32 = ref_grads[key].astype(np.float64).reshape(-1)
                g64 = w.grad.reshape(-1).numpy()
                out[key + "_bound64"] = np.array(np.linalg.norm(g32 - g64) /
                                                 (np.linalg.norm(g32) + 1e-300))
                if key in probes:
                    i = probes[key]
                    out[key + "_pbound64"] = np.array(np.linalg.norm(g32[i] - g64[i]) /
                                                      (np.linalg.norm(g32[i]) + 1e-300))
    os.makedirs(OUT, exist_ok=True)
    path = os.path.join(OUT, f"{name}.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= MAX_BYTES, f"{name}: {size} bytes"
    worst = max([float(out[k]) for k in out if k.endswith("bound64")], default=0.0)
    print(f"{name}: {len(rec.draws)} draws, loss {float(out.get('loss', np.nan)):.6f}, "
          f"{int(knots.sum())} rays next to a knot, worst bound64 {worst:.3g}, "
          f"{size / 1024:.1f} KiB")


def case(kind, seed, method="shadow_method_2", light_importance=0, grad_on_light=False,
         sigma_bias=(0.5, 0.5), rgb_weight=1.0, sm_weight=0.5):
    return dict(kind=kind, seed=seed, method=method, light_importance=light_importance,
                grad_on_light=grad_on_light, sigma_bias=sigma_bias, perturb=1.0, noise_std=1.0,
                rgb_weight=rgb_weight, sm_weight=sm_weight)


CASES = {
    "juntos_sm2": case("juntos", 77, light_importance=16),
    "juntos_gol_sm1": case("juntos", 79, method="shadow_method_1", grad_on_light=True),
    "juntos_disp_loss": case("disp_loss", 80),
    "juntos_nan": case("nan", 81, sigma_bias=(0.5, -5.0)),
}


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ref_nerf, _ = import_reference()
    import losses as ref_losses                    # noqa: E402
    import models.camera as camera_mod             # noqa: E402
    import models.rendering_rgb_sm as rs           # noqa: E402
    ref = (ref_nerf, rs, camera_mod, ref_losses)
    for name in sys.argv[1:] or list(CASES):
        run_case(ref, name, CASES[name])


if __name__ == "__main__":
    main()
