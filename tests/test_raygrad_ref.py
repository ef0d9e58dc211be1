"""The float64 restatement of the ray gradient (tests/raygrad64.py) against
float64 torch autograd of the oracle, stage by stage and end to end, and the
oracle's ray gradient against the reference's own (tests/golden/raygrad/)."""
import os

import numpy as np
import pytest
import torch

import raygrad64 as R64
from composite64 import make_case
from conftest import GOLDEN, load_golden_path
from oracle import nerf_oracle as O

F64 = torch.float64


def _rays(n, g, near=2.0, far=6.0):
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True) * (0.5 + torch.rand(n, 1, generator=g))
    return torch.cat([torch.randn(n, 3, generator=g) * 0.3, d,
                      torch.full((n, 1), near) + 0.1 * torch.rand(n, 1, generator=g),
                      torch.full((n, 1), far) + 0.1 * torch.rand(n, 1, generator=g)], 1)


def _close(got, ref, tol, what):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    err = np.abs(got - ref).max()
    scale = np.abs(ref).max()
    assert err <= tol * scale + 1e-300, f"{what}: err {err:.3g}, scale {scale:.3g}"


@pytest.mark.parametrize("sigma_only", [False, True])
def test_mlp_input_gradient_formula(sigma_only):
    g = torch.Generator().manual_seed(11)
    n, S = 5, 7
    p = {k: v.to(F64) for k, v in O.make_params(7, sigma_bias=0.4).items()}
    rays = _rays(n, g).to(F64).requires_grad_(True)
    z = (2 + 4 * torch.rand(n, S, generator=g)).to(F64).requires_grad_(True)
    xyz = (rays[:, None, 0:3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    xe = O.embed(xyz, 10)
    de = O.embed(rays[:, 3:6], 4).repeat_interleave(S, 0)
    out, taps = R64.mlp_taps(p, xe, de, sigma_only)
    ref = O.nerf_forward(p, xe if sigma_only else torch.cat([xe, de], 1), sigma_only=sigma_only)
    assert torch.equal(out, ref)
    gout = torch.randn(out.shape, generator=g).to(F64)
    (out * gout).sum().backward()
    g_rays, g_z = R64.mlp_input_grad(p, rays, z, taps[1].grad, taps[5].grad,
                                     None if sigma_only else taps["dir"].grad)
    _close(g_rays, rays.grad, 1e-12, "g_rays")
    _close(g_z, z.grad, 1e-12, "g_z")
    assert (rays.grad[:, 6:] == 0).all()


@pytest.mark.parametrize("regime", ["typical", "noise", "ndc"])
@pytest.mark.parametrize("white_back", [False, True])
@pytest.mark.parametrize("disp", [False, True])
def test_composite_formula(regime, white_back, disp):
    c = make_case(regime, 13, 6, seed=3)
    n, S = c["z"].shape
    raw = torch.from_numpy(c["raw"]).to(F64).view(n, S, 4)
    z = torch.from_numpy(c["z"]).to(F64).requires_grad_(True)
    rays = torch.from_numpy(c["rays"]).to(F64).requires_grad_(True)
    noise = [c["noise"] if c["noise"] is not None else np.zeros((n, S), np.float32)]
    rgb, depth, w = O.composite(raw[..., 3], raw[..., :3], z, rays[:, 3:6], c["noise_std"],
                                white_back, O.ReplayRNG(noise))
    opac = w.sum(1)
    g_disp = np.random.default_rng(5).standard_normal(n).astype(np.float32)
    loss = (rgb * torch.from_numpy(c["g_rgb"])).sum() + (depth * torch.from_numpy(c["g_depth"])).sum() \
        + (opac * torch.from_numpy(c["g_opacity"])).sum()
    if disp:
        loss = loss + (R64.disp_map(depth, opac) * torch.from_numpy(g_disp)).sum()
    loss.backward()
    g_z, g_d = R64.composite_raygrad(
        c["raw"], c["z"], c["rays"], c["noise"], c["noise_std"], white_back, c["g_rgb"],
        c["g_depth"], c["g_opacity"], g_disp if disp else None,
        depth.detach().float().numpy(), opac.detach().float().numpy())
    # the restatement takes what the kernel reads: the disparity's D, O rounded
    # to fp32, and sigma + noise as the forward rounds it (one fp32 add)
    tol = 1e-5 if disp else (1e-6 if c["noise"] is not None else 1e-9)
    _close(g_z, z.grad, tol, "g_z")
    _close(g_d, rays.grad[:, 3:6], tol, "g_d")


def test_merge_formula():
    g = torch.Generator().manual_seed(2)
    zc = torch.sort(torch.rand(4, 9, generator=g), 1)[0].to(F64).requires_grad_(True)
    zp = torch.rand(4, 6, generator=g).to(F64)
    zf, _ = torch.sort(torch.cat([zc, zp], 1), 1)
    gz = torch.randn(4, 15, generator=g).to(F64)
    (zf * gz).sum().backward()
    got = R64.merge_raygrad(zc.detach().numpy(), zf.detach().numpy(), gz.numpy())
    assert np.array_equal(got, zc.grad.numpy())


@pytest.mark.parametrize("use_disp", [False, True])
@pytest.mark.parametrize("perturb", [0.0, 1.0, 0.6])
@pytest.mark.parametrize("S", [1, 2, 9])
def test_coarse_z_formula(use_disp, perturb, S):
    g = torch.Generator().manual_seed(4)
    rays = _rays(5, g).to(F64).requires_grad_(True)
    u = torch.rand(5, S, generator=g)
    z = O.coarse_z(rays, S, use_disp, perturb, O.ReplayRNG([u]))
    gz = torch.randn(5, S, generator=g).to(F64)
    (z * gz).sum().backward()
    gn, gf = R64.coarse_z_raygrad(rays.detach().numpy(), S, use_disp, perturb, u.numpy(), gz.numpy())
    # t = linspace in fp32 widened on both sides; the oracle multiplies perturb * u in fp32
    _close(gn, rays.grad[:, 6], 1e-6, "g_near")
    _close(gf, rays.grad[:, 7], 1e-6, "g_far")
    assert (rays.grad[:, :6] == 0).all()


def _draws(n, S, I, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.rand(n, S, generator=g), torch.randn(n, S, generator=g),
            torch.rand(n, I, generator=g), torch.rand(n, I, generator=g),
            torch.randn(n, S + I, generator=g)]


@pytest.mark.parametrize("use_disp,white_back", [(False, False), (True, True)])
def test_render64_is_the_oracle(use_disp, white_back):
    """render64 without pinned depths is oracle.render_rays: same outputs and,
    in float64 autograd, the same ray gradient"""
    n, S, I = 6, 8, 5
    g = torch.Generator().manual_seed(1)
    models = [{k: v.to(F64) for k, v in O.make_params(s, sigma_bias=0.5).items()} for s in (1, 2)]
    draws = _draws(n, S, I, 3)
    tgt = torch.rand(n, 3, generator=g).to(F64)
    grads = []
    for fn in ("oracle", "render64"):
        rays = _rays(n, torch.Generator().manual_seed(9)).to(F64).requires_grad_(True)
        if fn == "oracle":
            res = O.render_rays(models, rays, S, use_disp, 1.0, 1.0, I, 1 << 20, white_back,
                                rng=O.ReplayRNG(draws))
        else:
            res = R64.render64(models, rays, S, use_disp, 1.0, 1.0, I, white_back, draws)
        loss = O.mse_loss(res, tgt) + res["depth_fine"].mean() + res["depth_coarse"].mean()
        loss.backward()
        grads.append((rays.grad.clone(), {k: v.detach() for k, v in res.items()}))
    for k, v in grads[0][1].items():
        assert torch.equal(v, grads[1][1][k]), k
    _close(grads[1][0], grads[0][0], 1e-12, "rays.grad")
    assert grads[0][0][:, 6:].abs().max() > 0 and grads[0][0][:, :6].abs().max() > 0


def test_staged_chain_is_the_oracle():
    """stages 1-4 composed by hand (coarse pass, replayed draws) reproduce the
    float64 autograd ray gradient of oracle.render_rays"""
    n, S = 5, 9
    g = torch.Generator().manual_seed(6)
    p = {k: v.to(F64) for k, v in O.make_params(3, sigma_bias=0.5).items()}
    draws = _draws(n, S, 4, 8)[:2]
    rays = _rays(n, g).to(F64).requires_grad_(True)
    cap = {}
    res = O.render_rays([p], rays, S, True, 1.0, 1.0, 0, 1 << 20, True, rng=O.ReplayRNG(draws),
                        capture=cap)
    g_rgb = torch.randn(n, 3, generator=g).to(F64)
    g_dep = torch.randn(n, generator=g).to(F64)
    ((res["rgb_coarse"] * g_rgb).sum() + (res["depth_coarse"] * g_dep).sum()).backward()
    # by hand, at the oracle's own float64 depths
    z = cap["z_coarse"].detach()
    xyz = (rays.detach()[:, None, 0:3] + rays.detach()[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
    xe = O.embed(xyz, 10).requires_grad_(True)      # so that the taps join a graph
    de = O.embed(rays.detach()[:, 3:6], 4).repeat_interleave(S, 0)
    out, taps = R64.mlp_taps(p, xe, de)
    raw = out.detach().clone().requires_grad_(True)
    zz = z.clone().requires_grad_(True)
    dd = rays.detach()[:, 3:6].clone().requires_grad_(True)
    r4 = raw.view(n, S, 4)
    rgb, depth, _ = O.composite(r4[..., 3], r4[..., :3], zz, dd, 1.0, True, O.ReplayRNG(draws[1:]))
    ((rgb * g_rgb).sum() + (depth * g_dep).sum()).backward()
    out.backward(raw.grad)
    g1, gz1 = R64.mlp_input_grad(p, rays.detach(), z, taps[1].grad, taps[5].grad, taps["dir"].grad)
    g_z = gz1 + zz.grad.numpy()
    gn, gf = R64.coarse_z_raygrad(rays.detach().numpy(), S, True, 1.0, draws[0].numpy(), g_z)
    total = g1.copy()
    total[:, 3:6] += dd.grad.numpy()
    total[:, 6], total[:, 7] = gn, gf
    _close(total, rays.grad, 1e-6, "rays.grad")


FIXTURE = os.path.join(GOLDEN, "raygrad", "raygrad_cfg.npz")


@pytest.mark.parametrize("level", ["coarse", "fine"])
def test_oracle_ray_gradient_is_the_references(level):
    """rays.grad of the reference's own render_rays (fp32 autograd, replayed
    draws; tests/golden/make_golden_raygrad.py) against the oracle's, N_importance
    0 and > 0.  Both are fp32 autograd of the same sequence of torch ops, so
    they agree to the order of the BLAS's summation: 1e-4 of the largest entry
    (the gradient carries the 2^9 cos(2^9 x) terms)."""
    fx = load_golden_path(FIXTURE)
    S, I = int(fx["cfg"][0]), (int(fx["cfg"][1]) if level == "fine" else 0)
    draws = [fx[f"{level}_draw{i}"] for i in range(5 if I else 2)]
    params = [O.make_params(int(fx["cfg"][2]), sigma_bias=float(fx["cfg"][4])),
              O.make_params(int(fx["cfg"][3]), sigma_bias=float(fx["cfg"][4]))]
    rays = torch.from_numpy(fx["rays"]).clone().requires_grad_(True)
    res = O.render_rays(params, rays, S, False, 1.0, 1.0, I, 32768, False,
                        rng=O.ReplayRNG(draws))
    loss = O.mse_loss(res, torch.from_numpy(fx["target"])) + \
        sum(res[k].mean() for k in res if k.startswith("depth_"))
    np.testing.assert_allclose(loss.item(), float(fx[f"{level}_loss"]), rtol=1e-5)
    loss.backward()
    ref = fx[f"{level}_rays_grad"]
    err = np.abs(rays.grad.numpy() - ref).max(0)
    scale = np.abs(ref).max(0)
    assert (err <= 1e-4 * scale.max()).all(), (err, scale)
