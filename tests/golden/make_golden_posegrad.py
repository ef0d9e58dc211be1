"""Pose-gradient fixtures from the REFERENCE's own ``get_rays`` and
``get_ndc_rays`` (datasets/ray_utils.py:27-50, :53-93): ``c2w.grad`` by the
reference's fp32 autograd for a seeded upstream gradient on the rays.

    python tests/golden/make_golden_posegrad.py

Needs a checkout of the reference (``NERF_REFERENCE``); the two function
bodies are taken and vetted by ``make_golden_rays.reference_functions()`` and
run with ``c2w.requires_grad_()``.  Cases: 3 poses at 5 x 7, Blender and NDC.
Before writing, the script checks that the reference's fp32 gradient is within
1e-4 of the largest entry of the float64 restatement (tests/posegrad64.py),
the bound tests/test_posegrad_ref.py then asserts.  Output:
``tests/golden/posegrad/posegrad.npz`` (plain arrays, a few KB).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, REPO)

import make_golden_rays as MGR  # noqa: E402
import posegrad64 as P64  # noqa: E402
from oracle import rays_oracle as RO  # noqa: E402

H, W = 5, 7
CASES = [(6.5, False), (7.25, True)]      # (focal, ndc)


def three_poses(ndc):
    return torch.cat([MGR.poses(0, ndc), MGR.poses(1, ndc)[:1]]).contiguous()


def main():
    get_rays, get_ndc_rays = MGR.reference_functions()
    arrs = {}
    for k, (f, ndc) in enumerate(CASES):
        c2w = three_poses(ndc).requires_grad_(True)
        dirs = RO.get_ray_directions(H, W, f)
        os_, ds_ = [], []
        for m in c2w:
            o, d = get_rays(dirs, m)
            if ndc:
                o, d = get_ndc_rays(H, W, f, 1.0, o, d)
            os_.append(o)
            ds_.append(d)
        g = torch.Generator().manual_seed(100 + k)
        g_rays = torch.randn(3 * H * W, 8, generator=g)
        ((torch.cat(os_) * g_rays[:, 0:3]).sum() + (torch.cat(ds_) * g_rays[:, 3:6]).sum()).backward()
        ref64, _ = P64.pose_grad(c2w.detach().numpy(), H, W, f, g_rays.numpy(), ndc=ndc)
        err = np.abs(c2w.grad.numpy() - ref64).max() / np.abs(ref64).max()
        print(f"case {k} (ndc {ndc}): the reference's fp32 autograd is {err:.3g} of the largest "
              "entry from float64")
        assert err <= 1e-4, err
        arrs[f"c{k}_poses"] = c2w.detach().numpy()
        arrs[f"c{k}_cfg"] = np.array([H, W, f, float(ndc)], np.float64)
        arrs[f"c{k}_g_rays"] = g_rays.numpy()
        arrs[f"c{k}_c2w_grad"] = c2w.grad.numpy()
    arrs["n_cases"] = np.array(len(CASES))
    os.makedirs(os.path.join(HERE, "posegrad"), exist_ok=True)
    out = os.path.join(HERE, "posegrad", "posegrad.npz")
    np.savez_compressed(out, **arrs)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
