"""The float64 restatement of the camera-pose gradient (tests/posegrad64.py)
against float64 torch autograd of a float64 copy of
``oracle.rays_oracle.ray_buffer``, and against the reference's own autograd
(tests/golden/posegrad/, made by tests/golden/make_golden_posegrad.py)."""
import os

import numpy as np
import pytest
import torch

import posegrad64 as P64
from conftest import GOLDEN, load_golden_path
from oracle import rays_oracle as RO

FIXTURE = os.path.join(GOLDEN, "posegrad", "posegrad.npz")


def _close(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err, scale = np.abs(got - ref).max(), np.abs(ref).max()
    print(f"{what}: err {err:.3g}, scale {scale:.3g}")
    assert scale > 0 and err <= tol * scale, f"{what}: err {err:.3g}, scale {scale:.3g}"


def test_float64_copy_is_the_oracle():
    """the copy with focal as a tensor, run in fp32, is ray_buffer bit for bit"""
    for ndc in (False, True):
        P = P64.poses(2, ndc, 1)
        ref = RO.ray_buffer(P, 6, 9, 8.5, 2.0, 6.0, ndc)
        assert torch.equal(P64.ray_buffer(P, 6, 9, 8.5, 2.0, 6.0, ndc), ref)
        assert torch.equal(P64.ray_buffer(P, 6, 9, torch.tensor(8.5), 2.0, 6.0, ndc), ref)


@pytest.mark.parametrize("mode", ["all", "sel"])
@pytest.mark.parametrize("ndc", [False, True], ids=["blender", "ndc"])
def test_restatement_matches_float64_autograd(ndc, mode):
    H, W, f, n_poses = 5, 7, 6.75, 3
    P = P64.poses(n_poses, ndc, 3)
    g = torch.Generator().manual_seed(5)
    sel = None
    if mode == "sel":       # repeats, pose 1 never selected, out-of-range entries in between
        pool = torch.cat([torch.arange(0, H * W), torch.arange(2 * H * W, 3 * H * W)])
        sel = pool[torch.randint(0, pool.shape[0], (60,), generator=g)]
        sel[::7] = -1
        sel[3::11] = n_poses * H * W
    n = n_poses * H * W if sel is None else sel.shape[0]
    g_rays = torch.randn(n, 8, generator=g)
    ref_c2w, ref_f = P64.autograd_pose_grad(P, H, W, f, g_rays, sel, ndc)
    got_c2w, got_f = P64.pose_grad(P.numpy(), H, W, f, g_rays.numpy(),
                                   None if sel is None else sel.numpy(), ndc)
    _close(got_c2w, ref_c2w, 1e-10, "g_c2w")
    _close(got_f.sum(), ref_f, 1e-10, "g_focal")
    if sel is not None:
        assert (got_c2w[1] == 0).all() and got_f[1] == 0 and (ref_c2w[1] == 0).all()
    if ndc:     # analytically the shifted origin's z is -near: o2 and d2 do not move with the pose
        gz = torch.zeros(n, 8)
        gz[:, 2], gz[:, 5] = g_rays[:, 2], g_rays[:, 5]
        z_c2w, z_f = P64.pose_grad(P.numpy(), H, W, f, gz.numpy(),
                                   None if sel is None else sel.numpy(), ndc)
        assert np.abs(z_c2w).max() <= 1e-12 * np.abs(ref_c2w).max() and abs(z_f.sum()) <= 1e-12


def test_partial_range_without_sel():
    """sel null and n below the pixel count: the first n pixels"""
    H, W, f = 4, 5, 5.5
    P = P64.poses(3, False, 7)
    g_rays = torch.randn(27, 8, generator=torch.Generator().manual_seed(2))
    ref_c2w, ref_f = P64.autograd_pose_grad(P, H, W, f, g_rays)
    got_c2w, got_f = P64.pose_grad(P.numpy(), H, W, f, g_rays.numpy())
    _close(got_c2w, ref_c2w, 1e-10, "g_c2w")
    _close(got_f.sum(), ref_f, 1e-10, "g_focal")
    assert (got_c2w[2] == 0).all()


@pytest.mark.parametrize("case", [0, 1], ids=["blender", "ndc"])
def test_restatement_matches_the_references_autograd(case):
    """c2w.grad of the reference's own get_rays / get_ndc_rays (fp32 autograd,
    3 poses at 5 x 7, a seeded upstream gradient): 1e-4 of the largest entry,
    the figure test_raygrad_ref.py uses for the same kind of pin"""
    fx = load_golden_path(FIXTURE)
    assert int(fx["n_cases"]) == 2
    H, W, f, ndc = fx[f"c{case}_cfg"]
    assert (int(H), int(W), bool(ndc)) == (5, 7, bool(case)) and fx[f"c{case}_poses"].shape == (3, 3, 4)
    got, _ = P64.pose_grad(fx[f"c{case}_poses"], int(H), int(W), float(f), fx[f"c{case}_g_rays"],
                           ndc=bool(ndc))
    _close(got, fx[f"c{case}_c2w_grad"], 1e-4, "g_c2w")
