"""Generate tests/golden/raygrad/raygrad_cfg.npz by running the REFERENCE
implementation: ``rays.grad`` of the reference's own ``render_rays`` (plain
PyTorch, differentiable in the (N, 8) ray tensor), with recorded draws, for
N_importance 0 and > 0.  tests/test_raygrad_ref.py pins the oracle's ray
gradient to it.

    python tests/golden/make_golden_raygrad.py

Needs a checkout of the reference (``NERF_REFERENCE``, see make_golden.py),
imported only here.  The loss is the reference's MSE (losses.py:4-14) plus the
mean of every depth map, so that near, far and the depths carry gradient
beside the colours.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

from make_golden import RecordingTorch, import_reference, pick  # noqa: E402
from oracle.nerf_oracle import make_params  # noqa: E402
from nerf_pl_amd.rays import blender_rays  # noqa: E402

N_RAYS, N_SAMPLES, N_IMPORTANCE, SEEDS, SIGMA_BIAS = 16, 16, 12, (31, 32), 0.5


def main():
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    ref_nerf, ref_rendering = import_reference()
    rays0 = pick(blender_rays(64, 2, near=2.0, far=6.0), N_RAYS, 41)
    g = torch.Generator().manual_seed(42)
    target = torch.rand(N_RAYS, 3, generator=g)
    out = {"rays": rays0.numpy(), "target": target.numpy(),
           "cfg": np.array([N_SAMPLES, N_IMPORTANCE, SEEDS[0], SEEDS[1], SIGMA_BIAS], np.float64)}
    emb = [ref_nerf.Embedding(3, 10), ref_nerf.Embedding(3, 4)]
    for level, n_imp in (("coarse", 0), ("fine", N_IMPORTANCE)):
        models = []
        for s in SEEDS[:2 if n_imp else 1]:
            net = ref_nerf.NeRF()
            net.load_state_dict(make_params(s, sigma_bias=SIGMA_BIAS))
            models.append(net)
        torch.manual_seed(7)
        rays = rays0.clone().requires_grad_(True)
        rec = RecordingTorch()
        saved = ref_rendering.torch
        ref_rendering.torch = rec
        try:
            res = ref_rendering.render_rays(models, emb, rays, N_SAMPLES, False, 1.0, 1.0, n_imp,
                                            32768, False, False)
        finally:
            ref_rendering.torch = saved
        loss = torch.mean((res["rgb_coarse"] - target) ** 2)
        if "rgb_fine" in res:
            loss = loss + torch.mean((res["rgb_fine"] - target) ** 2)
        loss = loss + sum(res[k].mean() for k in res if k.startswith("depth_"))
        loss.backward()
        for i, (_, t) in enumerate(rec.draws):
            out[f"{level}_draw{i}"] = t.numpy()
        out[f"{level}_loss"] = np.array(loss.item(), np.float64)
        out[f"{level}_rays_grad"] = rays.grad.numpy()
    os.makedirs(os.path.join(HERE, "raygrad"), exist_ok=True)
    path = os.path.join(HERE, "raygrad", "raygrad_cfg.npz")
    np.savez_compressed(path, **out)
    print(f"{path}: {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
