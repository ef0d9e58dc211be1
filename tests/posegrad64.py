"""Float64 restatement of the camera-pose gradient (csrc/posegrad.hip, DESIGN.md
20): per ray the transpose of get_rays / get_ndc_rays written out by hand, per
pose the sum over its rays.  Plain numpy; the same case split as the kernel
(ndc on / off, sel / null, out-of-range entries).  Also the float64 (or fp32)
torch copy of ``oracle.rays_oracle.ray_buffer`` with focal as a tensor, which
autograd differentiates: the reference of tests/test_posegrad_ref.py and
tests/test_gpu_posegrad.py.
"""
import math

import numpy as np
import torch

from nerf_pl_amd.rays import pose_spherical


def poses(n, ndc, seed):
    """n poses: forward-facing (small rotations about every axis, so that all
    twelve entries matter and d_z stays near -1) or on a sphere"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(n):
        if ndc:
            a, b, c = (0.15 * (2 * torch.rand(3, generator=g) - 1)).tolist()
            rz = torch.tensor([[math.cos(a), -math.sin(a), 0], [math.sin(a), math.cos(a), 0], [0, 0, 1.]])
            ry = torch.tensor([[math.cos(b), 0, math.sin(b)], [0, 1., 0], [-math.sin(b), 0, math.cos(b)]])
            rx = torch.tensor([[1., 0, 0], [0, math.cos(c), -math.sin(c)], [0, math.sin(c), math.cos(c)]])
            t = 0.1 * (2 * torch.rand(3, 1, generator=g) - 1)
            out.append(torch.cat([rz @ ry @ rx, t], 1))
        else:
            th, ph = (360 * torch.rand(1, generator=g) - 180).item(), (-60 * torch.rand(1, generator=g)).item()
            out.append(pose_spherical(th, ph, 3.5 + torch.rand(1, generator=g).item()))
    return torch.stack(out).float()


def pose_grad(poses, H, W, focal, g_rays, sel=None, ndc=False, ndc_near=1.0):
    """(g_c2w (n_poses, 3, 4), g_focal_pose (n_poses)) in float64 from the
    upstream gradient g_rays (n, 8); ray k is global pixel sel[k] (or k)."""
    m = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    g = np.asarray(g_rays, np.float64)
    n_poses, hw = m.shape[0], H * W
    pix = np.arange(g.shape[0], dtype=np.int64) if sel is None else np.asarray(sel, np.int64)
    assert pix.shape[0] == g.shape[0]
    ok = (pix >= 0) & (pix < n_poses * hw)          # out of range: the ray contributes nothing
    pix, g = pix[ok], g[ok]
    p, rem = pix // hw, pix % hw
    i, j = (rem % W).astype(np.float64), (rem // W).astype(np.float64)
    f = float(focal)
    dc = np.stack([(i - W / 2) / f, -(j - H / 2) / f, -np.ones_like(i)], -1)
    R, o = m[p, :, :3], m[p, :, 3]
    du = np.einsum("krc,kc->kr", R, dc)
    nrm = np.linalg.norm(du, axis=1, keepdims=True)
    d = du / nrm
    go, gd = g[:, 0:3].copy(), g[:, 3:6].copy()
    gf = np.zeros(g.shape[0])
    if ndc:
        cw, ch = -1. / (W / (2. * f)), -1. / (H / (2. * f))
        t = -(ndc_near + o[:, 2]) / d[:, 2]
        s = o + t[:, None] * d
        ox, oy = s[:, 0] / s[:, 2], s[:, 1] / s[:, 2]
        q0, q1 = d[:, 0] / d[:, 2], d[:, 1] / d[:, 2]
        g_o2 = go[:, 2] - gd[:, 2]
        g_ox, g_oy = cw * (go[:, 0] - gd[:, 0]), ch * (go[:, 1] - gd[:, 1])
        g_q0, g_q1 = cw * gd[:, 0], ch * gd[:, 1]
        gf = (ox * go[:, 0] + (q0 - ox) * gd[:, 0]) * cw / f \
            + (oy * go[:, 1] + (q1 - oy) * gd[:, 1]) * ch / f
        gs = np.stack([g_ox / s[:, 2], g_oy / s[:, 2],
                       -(g_ox * ox + g_oy * oy) / s[:, 2] - g_o2 * 2. * ndc_near / s[:, 2] ** 2], -1)
        g_t = (gs * d).sum(1)
        go = gs.copy()
        go[:, 2] -= g_t / d[:, 2]
        gd = t[:, None] * gs
        gd[:, 0] += g_q0 / d[:, 2]
        gd[:, 1] += g_q1 / d[:, 2]
        gd[:, 2] += -(g_q0 * q0 + g_q1 * q1) / d[:, 2] - g_t * t / d[:, 2]
    gu = (gd - d * (d * gd).sum(1, keepdims=True)) / nrm
    per_ray = np.concatenate([gu[:, :, None] * dc[:, None, :], go[:, :, None]], 2)   # (k, 3, 4)
    gdc = np.einsum("krc,kr->kc", R, gu)
    gf = gf - (gdc[:, 0] * dc[:, 0] + gdc[:, 1] * dc[:, 1]) / f
    g_c2w = np.zeros((n_poses, 3, 4))
    g_focal = np.zeros(n_poses)
    np.add.at(g_c2w, p, per_ray)
    np.add.at(g_focal, p, gf)
    return g_c2w, g_focal


def ray_buffer(poses, H, W, focal, near, far, ndc=False, ndc_near=1.0):
    """``oracle.rays_oracle.ray_buffer`` in the dtype of ``poses`` with focal a
    tensor (or a float): (n_poses*H*W, 8), differentiable in both."""
    dt = poses.dtype
    j, i = torch.meshgrid(torch.arange(H, dtype=dt), torch.arange(W, dtype=dt), indexing="ij")
    dirs = torch.stack([(i - W / 2) / focal, -(j - H / 2) / focal, -torch.ones_like(i)], -1)
    out = []
    for c2w in poses.reshape(-1, 3, 4):
        d = dirs @ c2w[:, :3].T
        d = (d / torch.norm(d, dim=-1, keepdim=True)).reshape(-1, 3)
        o = c2w[:, 3].expand(d.shape)
        if ndc:
            t = -(ndc_near + o[..., 2]) / d[..., 2]
            o = o + t[..., None] * d
            ox_oz = o[..., 0] / o[..., 2]
            oy_oz = o[..., 1] / o[..., 2]
            o0 = -1. / (W / (2. * focal)) * ox_oz
            o1 = -1. / (H / (2. * focal)) * oy_oz
            o2 = 1. + 2. * ndc_near / o[..., 2]
            d0 = -1. / (W / (2. * focal)) * (d[..., 0] / d[..., 2] - ox_oz)
            d1 = -1. / (H / (2. * focal)) * (d[..., 1] / d[..., 2] - oy_oz)
            o, d = torch.stack([o0, o1, o2], -1), torch.stack([d0, d1, 1 - o2], -1)
            near, far = 0.0, 1.0
        out.append(torch.cat([o, d, near * torch.ones_like(o[:, :1]),
                              far * torch.ones_like(o[:, :1])], 1))
    return torch.cat(out, 0)


def autograd_pose_grad(poses, H, W, focal, g_rays, sel=None, ndc=False, ndc_near=1.0,
                       dtype=torch.float64):
    """(c2w.grad, focal.grad) of sum(rays * g_rays) by torch autograd of
    ``ray_buffer`` in ``dtype``; rays of out-of-range ``sel`` entries are left out."""
    c2w = torch.as_tensor(poses).to(dtype).clone().requires_grad_(True)
    f = torch.tensor(float(focal), dtype=dtype, requires_grad=True)
    buf = ray_buffer(c2w, H, W, f, 2.0, 6.0, ndc, ndc_near)
    g = torch.as_tensor(g_rays).to(dtype)
    if sel is not None:
        sel = torch.as_tensor(sel, dtype=torch.int64)
        ok = (sel >= 0) & (sel < buf.shape[0])
        buf, g = buf[sel[ok]], g[ok]
    else:
        buf = buf[:g.shape[0]]
    (buf[:, :6] * g[:, :6]).sum().backward()
    return c2w.grad.numpy().astype(np.float64), float(f.grad)
