"""The joint RGB + shadow-map training step (train_rgb_sm_juntos.py:137-199
through nerf_pl_amd.rendering_rgb_sm) timed at cfg5's shape: a 128x128 light
image re-rendered every step, 512 camera rays, 64 + 64 samples, light 64 + 64,
noise_std 0, shadow_method_2, rgb_weight 1 / sm_weight 0.5, FusedAdam.

    python dev/joint_step.py [--steps 20] [--warmup 5] [--rounds 3] [--grad-on-light]
    python dev/joint_step.py --modes full,plain --rounds 1          # under a kernel trace

Alternates the modes in one process, ``--rounds`` times, each window ``--steps``
steps after ``--warmup`` between device synchronisations; prints one JSON line
(camera rays/s per mode, mean and every round).  Modes: ``depth_only`` -- the
light render with ``depth_only=True`` (sigma-only graph); ``full`` -- without it
(the reference's full MLP); ``plain`` -- the same step on
``nerf_pl_amd.rendering.render_rays`` (no disparity maps), so that a kernel trace
holds the plain compositing kernels (``composite_*_kernel<false>``) beside the
disparity ones (``<true>``) on the same launch shapes.  The scene is bench.py's
cfg5 scene (synthetic poses, random targets, default-init NeRF pair).
"""
import argparse
import json
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--img", type=int, default=128)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--samples", type=int, default=64)
    ap.add_argument("--importance", type=int, default=64)
    ap.add_argument("--grad-on-light", action="store_true")
    ap.add_argument("--modes", default="depth_only,full")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("dev/joint_step.py measures on the GPU: no HIP device found")

    import bench
    from nerf_pl_amd import render_rays as plain_render
    from nerf_pl_amd import rendering_rgb_sm as RGS
    from nerf_pl_amd.optim import FusedAdam
    from nerf_pl_amd.rays import generate_rays
    dev = torch.device("cuda", 0)
    wh, S, I, B = a.img, a.samples, a.importance, a.batch
    scene = bench.shadow_scene(wh, 4, dev)
    models, emb = bench._models(dev)
    opt = FusedAdam([p for m in models for p in m.parameters()], lr=5e-4, eps=1e-8)
    hw = wh * wh
    total = 4 * hw
    torch.manual_seed(4321)
    tgt_rgb = torch.rand(total, 3, device=dev)
    tgt_sm = torch.rand(total, 3, device=dev)
    light_ppc = {"eye_pos": scene["light_eye"], "camera": scene["light_cam"]}
    pos = [0]

    def step(mode):
        sel = torch.arange(pos[0], pos[0] + B, device=dev)
        pos[0] = (pos[0] + B) % total
        rays = generate_rays(scene["c2ws"], wh, wh, scene["focal"], 1.0, 200.0, sel)
        pose = sel // hw
        ppc = {"eye_pos": scene["eyes"][pose], "camera": scene["mats"][pose]}
        render = plain_render if mode == "plain" else RGS.render_rays
        kw = {"depth_only": True} if mode == "depth_only" else {}
        cam = render(models, emb, rays, S, False, 1.0, 0.0, I)
        with torch.set_grad_enabled(a.grad_on_light):
            light = render(models, emb, scene["light_rays"], S, False, 1.0, 0.0, I, **kw)
        out = RGS.efficient_sm(scene["pixels"][sel % hw], scene["light_pixels"], cam, light, ppc,
                               light_ppc, (wh, wh), True, True, "shadow_method_2")
        loss = 0
        for key, tgt, wt in (("rgb", tgt_rgb[sel], 1.0), ("sm", tgt_sm[sel], 0.5)):
            for lvl in ("coarse", "fine"):
                loss = loss + wt * torch.mean((out[f"{key}_{lvl}"] - tgt) ** 2)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
        return loss

    modes = a.modes.split(",")
    assert set(modes) <= {"depth_only", "full", "plain"}, modes
    rates = {m: [] for m in modes}
    for _ in range(a.rounds):
        for m in modes:
            for _ in range(a.warmup):
                step(m)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss = step(m)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if not torch.isfinite(loss):
                raise SystemExit(f"loss {loss.item()} after the timed window")
            rates[m].append(a.steps * B / dt)
    name = {"depth_only": "light_depth_only", "full": "light_full_mlp", "plain": "plain_render"}
    print(json.dumps({
        "workload": f"joint rgb+sm step, {wh}^2 light image ({S}+{I}"
                    f"{', autograd' if a.grad_on_light else ', no_grad'}), {B} camera rays "
                    f"({S}+{I}), noise_std 0, shadow_method_2, FusedAdam",
        "steps": a.steps, "warmup": a.warmup,
        **{name[m] + "_rays_per_s": round(sum(v) / len(v), 1) for m, v in rates.items()},
        **{name[m] + "_rounds": [round(x, 1) for x in v] for m, v in rates.items()},
        **{name[m] + "_ms_per_step": round(1e3 * B * len(v) / sum(v), 3) for m, v in rates.items()},
    }))


if __name__ == "__main__":
    main()
