"""Gradients with respect to the rays on the device (csrc/raygrad.hip,
DESIGN.md 18): every new kernel against the float64 restatement
(tests/raygrad64.py), the MLP's input gradient against CPU autograd of the
oracle MLP, and ``rays.grad`` of the three ``render_rays`` end to end against
the float64 oracle at the depths and fp32 positions the kernels chose.

Bounds.  Per tensor, max |ours - ref| <= max(2e-4, 2 floor) max |ref|, where
``floor`` is the fp32 CPU evaluation's own distance from float64 on the same
inputs (the reference algorithm's arithmetic); end to end the rule of
tests/grad64.py (normwise, max(1e-4, 2 floor), floor over ten evaluation
points).  Every figure is printed before it is asserted.
"""
import numpy as np
import pytest
import torch

import grad64
import raygrad64 as R64
from composite64 import REGIMES, make_case
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
F64 = torch.float64
SIZES = [(3, 11), (23, 37)]       # 33 samples: one block and one sample; the ragged small case


def _dev(a):
    return None if a is None else torch.as_tensor(a).to(DEV)


def _bound(got, ref64, ref32, what, tol=2e-4):
    """max-abs error within max(tol, 2 floor) of the largest reference entry"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    scale = np.abs(ref64).max()
    if scale == 0:          # a gradient that is exactly zero (e.g. no open sample) stays so
        assert (got == 0).all(), f"{what}: nonzero where the reference is exactly 0"
        return
    floor = 0.0 if ref32 is None else np.abs(np.asarray(ref32, np.float64) - ref64).max() / scale
    err = np.abs(got - ref64).max() / scale
    print(f"{what}: err {err:.3g} of max |ref| {scale:.3g}, fp32 floor {floor:.3g}, "
          f"bound {max(tol, 2 * floor):.3g}")
    assert err <= max(tol, 2 * floor), f"{what}: {err:.3g} > {max(tol, 2 * floor):.3g}"


# ---------------------------------------------------------------------------
# the MLP's input gradient alone
# ---------------------------------------------------------------------------
def _mlp_case(size, sigma_only, seed=3):
    """rays, z, the output gradient (kink samples zeroed) and the CPU
    references: float64 autograd at the fp32 positions, and fp32 autograd"""
    p = O.make_params(7, sigma_bias=0.4)
    g = torch.Generator().manual_seed(seed)
    n_rays, spr = size
    rays = torch.cat([torch.randn(n_rays, 3, generator=g) * 0.3,
                      torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1)
                      * (0.7 + 0.6 * torch.rand(n_rays, 1, generator=g)),
                      torch.full((n_rays, 1), 2.0), torch.full((n_rays, 1), 6.0)], 1)
    z = 2 + 4 * torch.rand(n_rays, spr, generator=g)
    gout = torch.randn(n_rays * spr, 1 if sigma_only else 4, generator=g)
    gout *= torch.exp2(-20 * torch.rand(n_rays, 1, generator=g)).repeat_interleave(spr, 0)
    xyz = rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]
    x = torch.cat([O.embed(xyz.reshape(-1, 3), 10),
                   O.embed(rays[:, 3:6], 4).repeat_interleave(spr, 0)], 1)
    # screen ReLU-kink samples, as test_mlp_backward_matches_autograd does
    with torch.no_grad():
        xe, de = x[:, :63], x[:, 63:]
        h, kink = xe, torch.zeros(x.shape[0], dtype=torch.bool)
        for i in range(8):
            if i == 4:
                h = torch.cat([xe, h], -1)
            pre = torch.nn.functional.linear(h, p[f"xyz_encoding_{i+1}.0.weight"],
                                             p[f"xyz_encoding_{i+1}.0.bias"])
            kink |= (pre.abs() < 2e-6).any(1)
            h = torch.relu(pre)
        if not sigma_only:
            feat = torch.nn.functional.linear(h, p["xyz_encoding_final.weight"],
                                              p["xyz_encoding_final.bias"])
            pre = torch.nn.functional.linear(torch.cat([feat, de], -1),
                                             p["dir_encoding.0.weight"], p["dir_encoding.0.bias"])
            kink |= (pre.abs() < 2e-6).any(1)
    assert kink.float().mean() < 0.1, kink.sum()
    gout[kink] = 0
    refs = {}
    for dt in (torch.float32, F64):
        r = rays.clone().to(dt).requires_grad_(True)
        zz = z.clone().to(dt).requires_grad_(True)
        pos = r[:, None, :3] + r[:, None, 3:6] * zz[..., None]
        if dt == F64:      # at the fp32 positions the kernels (and the fp32 reference) form
            pos = pos + (xyz.to(F64) - pos).detach()
        xe = O.embed(pos.reshape(-1, 3), 10)
        xin = xe if sigma_only else torch.cat([xe, O.embed(r[:, 3:6], 4).repeat_interleave(spr, 0)], 1)
        out = O.nerf_forward({k: v.to(dt) for k, v in p.items()}, xin, sigma_only=sigma_only)
        (out * gout.to(dt)).sum().backward()
        refs[dt] = (r.grad.numpy(), zz.grad.numpy(), out.detach())
    return p, rays, z, gout, refs


def _ours_mlp(p, rays, z, gout, sigma_only):
    from nerf_pl_amd import NeRF
    from nerf_pl_amd.functions import mlp_apply
    net = NeRF()
    net.load_state_dict(p)
    net = net.to(DEV)
    r = rays.to(DEV).requires_grad_(True)
    zz = z.to(DEV).requires_grad_(True)
    out = mlp_apply(net, rays=r, z=zz, spr=z.shape[1], sigma_only=sigma_only)
    (out * gout.to(DEV)).sum().backward()
    return net, out.detach().cpu(), r.grad, zz.grad


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("sigma_only", [False, True], ids=["full", "sigma"])
@pytest.mark.parametrize("math", ["fp32", "f16x3", "bf16x6"])
def test_mlp_input_gradient_matches_autograd(math, sigma_only, size, monkeypatch):
    from nerf_pl_amd import ops
    monkeypatch.setattr(ops, "MATH", math)
    p, rays, z, gout, refs = _mlp_case(size, sigma_only)
    net, out, g_rays, g_z = _ours_mlp(p, rays, z, gout, sigma_only)
    assert (out - refs[torch.float32][2]).abs().max() < 2e-5
    assert g_rays is not None and g_z is not None, "no gradient with respect to the rays"
    g_rays, g_z = g_rays.cpu().numpy(), g_z.cpu().numpy()
    assert (g_rays[:, 6:] == 0).all()
    (r64, z64, _), (r32, z32, _) = refs[F64], refs[torch.float32]
    _bound(g_rays[:, 0:3], r64[:, 0:3], r32[:, 0:3], f"{math} g_o")
    _bound(g_rays[:, 3:6], r64[:, 3:6], r32[:, 3:6], f"{math} g_d")
    _bound(g_z, z64, z32, f"{math} g_z")
    unused = ("dir_encoding", "rgb", "xyz_encoding_final") if sigma_only else ()
    assert all(q.grad is not None for name, q in net.named_parameters()
               if not name.startswith(unused))


@pytest.mark.parametrize("sigma_only", [False, True], ids=["full", "sigma"])
@pytest.mark.parametrize("math", ["fp32", "f16x3", "bf16x6"])
def test_backward_modes_give_identical_ray_gradients(math, sigma_only, monkeypatch):
    """every-sample, _active and _listed backward: unlisted samples contribute
    exact zeros, so rays.grad and z.grad agree bit for bit; the output gradient
    zeroes whole rays and whole 32-sample blocks"""
    from nerf_pl_amd import functions, ops
    monkeypatch.setattr(ops, "MATH", math)
    p, rays, z, gout, _ = _mlp_case((23, 37), sigma_only)
    gout = gout.view(23, 37, -1).clone()
    gout[3] = 0
    gout[10:12] = 0
    gout = gout.view(23 * 37, -1)
    gout[64:96] = 0
    gout[320:384] = 0
    got = {}
    for mode, (active, defer) in {"": (False, "none"), "_active": (True, "none"),
                                  "_listed": (True, "all")}.items():
        monkeypatch.setattr(functions, "ACTIVE_SAMPLES", active)
        monkeypatch.setattr(functions, "DEFER_SAVE", defer)
        net, _, g_rays, g_z = _ours_mlp(p, rays, z, gout, sigma_only)
        assert net.__dict__["_nr_defer_last"] == (mode == "_listed")
        got[mode] = (g_rays, g_z)
    assert got[""][0].abs().max() > 0
    for mode in ("_active", "_listed"):
        assert torch.equal(got[mode][0], got[""][0]), f"{mode}: rays.grad differs"
        assert torch.equal(got[mode][1], got[""][1]), f"{mode}: z.grad differs"
    zero = (gout == 0).all(1).view(23, 37)
    assert (got[""][1][zero.to(DEV)] == 0).all()


# ---------------------------------------------------------------------------
# compositing, merge, stratified depths: each kernel against the restatement
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("size", SIZES + [(2, 130)])          # 130: three 64-sample chunks
@pytest.mark.parametrize("disp", [False, True], ids=["", "disp"])
@pytest.mark.parametrize("white_back", [False, True], ids=["", "white"])
@pytest.mark.parametrize("regime", REGIMES)
def test_composite_ray_gradient(regime, white_back, disp, size):
    from nerf_pl_amd import ops
    n_rays, S = size
    c = make_case(regime, S, n_rays, seed=1)
    g_disp = np.random.default_rng(7).standard_normal(n_rays).astype(np.float32) if disp else None
    dv = {k: _dev(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    args = (dv["raw"], dv["z"], dv["rays"], dv.get("noise"), c["noise_std"], 0, 1, white_back)
    depth = opac = None
    if disp:
        _, depth, opac, _, _ = ops.composite_forward(*args, disp=True)
    g_z, g_rays = ops.composite_ray_gradient(*args, dv["g_rgb"], dv["g_depth"], dv["g_opacity"],
                                             _dev(g_disp), depth, opac, disp=disp)
    ref_z, ref_d = R64.composite_raygrad(
        c["raw"], c["z"], c["rays"], c["noise"], c["noise_std"], white_back, c["g_rgb"],
        c["g_depth"], c["g_opacity"], g_disp, None if depth is None else depth.cpu().numpy(),
        None if opac is None else opac.cpu().numpy())
    g_rays = g_rays.cpu().numpy()
    assert (g_rays[:, [0, 1, 2, 6, 7]] == 0).all()
    _bound(g_z.cpu().numpy(), ref_z, None, f"{regime} g_z")
    if np.abs(ref_d).max() > 0:
        _bound(g_rays[:, 3:6], ref_d, None, f"{regime} g_d")
    else:
        assert (g_rays[:, 3:6] == 0).all()


def test_composite_ray_gradient_philox_noise():
    """the in-kernel draws of (seed, stream) against the same draws replayed"""
    from nerf_pl_amd import ops
    c = make_case("typical", 37, 23, seed=2)
    dv = {k: _dev(v) for k, v in c.items() if isinstance(v, np.ndarray)}
    _, nrm = ops.probe_rand(5, 4, 23 * 37, device=DEV)
    g = [dv["g_rgb"], dv["g_depth"], dv["g_opacity"]]
    a = ops.composite_ray_gradient(dv["raw"], dv["z"], dv["rays"], None, 0.7, 5, 4, False, *g)
    b = ops.composite_ray_gradient(dv["raw"], dv["z"], dv["rays"], nrm.view(23, 37), 0.7, 5, 4,
                                   False, *g)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("size", SIZES + [(5, 64)])
def test_merge_ray_gradient(size):
    from nerf_pl_amd import ops
    n_rays, S = size
    I = 5 if S < 64 else 128
    g = torch.Generator().manual_seed(S)
    rays = torch.cat([torch.randn(n_rays, 6, generator=g), torch.full((n_rays, 1), 2.0),
                      torch.full((n_rays, 1), 6.0)], 1).to(DEV)
    z_c = ops.coarse_z(rays, S, False, 1.0, u=torch.rand(n_rays, S, generator=g).to(DEV))
    w = torch.rand(n_rays, S, generator=g).to(DEV)
    _, z_f = ops.sample_pdf(w, rays, I, u=torch.rand(n_rays, I, generator=g).to(DEV),
                            jitter=torch.rand(n_rays, I, generator=g).to(DEV), z_coarse=z_c,
                            merge=True)
    g_zf = torch.randn(n_rays, S + I, generator=g).to(DEV)
    got = ops.merge_ray_gradient(z_c, z_f, g_zf).cpu().numpy()
    ref = R64.merge_raygrad(z_c.cpu().numpy(), z_f.cpu().numpy(), g_zf.cpu().numpy())
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("size", SIZES + [(2, 130), (4, 1)])
@pytest.mark.parametrize("perturb", [0.0, 1.0], ids=["", "perturb"])
@pytest.mark.parametrize("use_disp", [False, True], ids=["", "disp"])
def test_coarse_z_ray_gradient(use_disp, perturb, size):
    from nerf_pl_amd import ops
    n_rays, S = size
    g = torch.Generator().manual_seed(S + 1)
    rays = torch.cat([torch.randn(n_rays, 6, generator=g),
                      2.0 + torch.rand(n_rays, 1, generator=g),
                      6.0 + torch.rand(n_rays, 1, generator=g)], 1)
    u = torch.rand(n_rays, S, generator=g)
    g_z = torch.randn(n_rays, S, generator=g)
    got = ops.coarse_z_ray_gradient(rays.to(DEV), S, use_disp, perturb,
                                    u.to(DEV) if perturb > 0 else None, 0, g_z.to(DEV)).cpu().numpy()
    gn, gf = R64.coarse_z_raygrad(rays.numpy(), S, use_disp, perturb, u.numpy(), g_z.numpy())
    assert (got[:, :6] == 0).all()
    _bound(got[:, 6], gn, None, "g_near")
    _bound(got[:, 7], gf, None, "g_far")


def test_no_listed_sample_gives_zero_gradients():
    """an output gradient of zeros lists no sample (device-side count 0):
    nothing of grad_ws is read and every ray gradient is an exact zero"""
    p, rays, z, gout, _ = _mlp_case((3, 11), False)
    _, _, g_rays, g_z = _ours_mlp(p, rays, z, torch.zeros_like(gout), False)
    assert (g_rays == 0).all() and (g_z == 0).all()


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
N, S, I = 48, 8, 5
SIGMA_BIAS = 0.5


def _e2e_inputs(seed):
    from nerf_pl_amd.rays import blender_rays
    g = torch.Generator().manual_seed(seed)
    rays = blender_rays(16, 1, near=2.0, far=6.0)
    rays = rays[torch.randperm(rays.shape[0], generator=g)[:N]].contiguous()
    draws = [torch.rand(N, S, generator=g), torch.randn(N, S, generator=g),
             torch.rand(N, I, generator=g), torch.rand(N, I, generator=g),
             torch.randn(N, S + I, generator=g)]
    return rays, draws


def _models(seed, n_models, trainable=True):
    from nerf_pl_amd import NeRF
    ms = []
    for m in range(n_models):
        net = NeRF()
        net.load_state_dict(O.make_params(seed + m, sigma_bias=SIGMA_BIAS))
        ms.append(net.to(DEV).requires_grad_(trainable))
    return ms


def _render(kind, models, rays, draws, n_imp, use_disp=False, white_back=False, cap=None):
    """one of the three render_rays, replayed draws"""
    from nerf_pl_amd import Embedding, ReplayRNG, render_rays, rendering_rgb_sm, rendering_shadows
    emb = [Embedding(3, 10), Embedding(3, 4)]
    d = draws if n_imp else draws[:2]
    args = (models, emb, rays, S, use_disp, 1.0, 1.0, n_imp, 32768, white_back)
    if kind == "render":
        return render_rays(*args, rng=ReplayRNG(d), _capture=cap)
    if kind == "shadows":
        return rendering_shadows.render_rays(*args, rng=ReplayRNG(d), _capture=cap)
    return rendering_rgb_sm.render_rays(*args, rng=ReplayRNG(d), depth_only=kind == "depth_only",
                                        _capture=cap)


def _functional(out, keep, seed, prefix=""):
    g = torch.Generator().manual_seed(seed)
    tot = 0
    for k in sorted(out):
        coef = torch.randn(out[k].shape, generator=g) * keep.view(-1, *[1] * (out[k].dim() - 1))
        if k.startswith(prefix):
            tot = tot + (out[k] * coef.to(out[k].device, out[k].dtype)).sum()
    return tot


def _cols(g):
    g = g.detach().cpu().double()
    return {f"rays[:, {j}]": g[:, j] for j in range(8)}


E2E = [("render", 0, False, False, "f16x3"), ("render", I, False, False, "f16x3"),
       ("render", I, False, False, "fp32"), ("render", I, True, True, "bf16x6"),
       ("rgb_sm", I, True, True, "f16x3"), ("shadows", I, False, False, "f16x3"),
       ("depth_only", I, False, False, "f16x3")]


@pytest.mark.parametrize("kind,n_imp,use_disp,white_back,math", E2E)
def test_ray_gradient_matches_float64_oracle(kind, n_imp, use_disp, white_back, math, monkeypatch):
    """rays.grad, all 8 columns, within max(1e-4, 2 x the fp32 oracle's own
    distance from float64) of the float64 oracle at the depths and fp32
    positions our kernels formed (tests/grad64.py's rule and screening).
    shadows / depth_only: a loss on depth_* alone."""
    from nerf_pl_amd import functions, ops
    monkeypatch.setattr(ops, "MATH", math)
    depth_only = kind in ("shadows", "depth_only")
    disp = kind != "render"
    prefix = "depth_" if depth_only else ""
    n_models = 2 if n_imp else 1
    rays, draws = _e2e_inputs(5)
    models = _models(21, n_models)
    r = rays.to(DEV).requires_grad_(True)
    cap = {}
    res = _render(kind, models, r, draws, n_imp, use_disp, white_back, cap)
    zc = cap["z_coarse"].detach().cpu()
    zf = cap["z_fine"].detach().cpu() if n_imp else None

    def oracle(dt, ulp):
        ps = []
        for m in range(n_models):
            p = O.make_params(21 + m, sigma_bias=SIGMA_BIAS)
            ps.append({k: v.to(dt) for k, v in p.items()} if ulp is None
                      else grad64.ulp_perturbed(p, ulp + m, dt))
        rr = rays.clone().to(dt).requires_grad_(True)
        c = {}
        out = R64.render64(ps, rr, S, use_disp, 1.0, 1.0, n_imp, white_back,
                           draws if n_imp else draws[:2], zc, zf, depth_only=depth_only,
                           disp=disp, dtype=dt, capture=c)
        return ps, rr, out, c

    pts = {u: (oracle(torch.float32, u), oracle(F64, u)) for u in grad64.FLOOR_POINTS}
    p64s, _, out64, cap64 = pts[None][1]
    assert sorted(out64) == sorted(res), (sorted(out64), sorted(res))
    for k in res:       # the forward: the north star's 1e-4 absolute
        assert (res[k].detach().cpu().double() - out64[k].detach()).abs().max() < 1e-4, k
    # screening, as tests/test_gpu_random.py: compositing ReLU kinks between our
    # sigma and float64's, and MLP ReLUs our forward switched against float64
    passes = [(0, zc, "coarse", draws[1])] + ([(1, zf, "fine", draws[4])] if n_imp else [])
    ones = torch.ones(N, dtype=torch.bool)
    gm = torch.autograd.grad(_functional(out64, ones, 9, prefix),
                             [cap64["raw_" + lv] for _, _, lv, _ in passes], retain_graph=True)
    bad = np.zeros(N, bool)
    monkeypatch.setattr(functions, "_DEBUG", {})
    monkeypatch.setattr(functions, "DEFER_SAVE", "none")
    for (mi, z, lv, noise), g in zip(passes, gm):
        spr = z.shape[1]
        with torch.no_grad():
            sig = functions.mlp_apply(models[mi], rays=rays.to(DEV), z=z.to(DEV), spr=spr,
                                      sigma_only=depth_only)[:, -1].view(-1, spr)
        k, e = grad64.relu_kinks(sig, cap64["raw_" + lv][..., -1].reshape(-1, spr), noise)
        assert e.all(), "a compositing ReLU switched away from its kink"
        bad |= k
        # the masks of the full-graph training forward at the same depths (layers
        # 1-8 run the same instructions in the sigma-only graph)
        functions._DEBUG.pop("fwd_saves", None)
        functions.mlp_apply(models[mi], rays=rays.to(DEV), z=z.to(DEV), spr=spr)
        save, n, _ = functions._DEBUG["fwd_saves"][0]
        xyz = (rays[:, None, :3] + rays[:, None, 3:6] * z[:, :, None]).reshape(-1, 3)
        x64 = torch.cat([O.embed(xyz.double(), 10),
                         O.embed(rays[:, 3:6].double(), 4).repeat_interleave(spr, 0)], 1)
        flip, expl, _ = grad64.mlp_flips(save, n, x64, p64s[mi], gmag=g.abs().amax(1))
        assert expl.all(), "an MLP ReLU switched away from its kink"
        bad |= flip.reshape(-1, spr).any(1)
    monkeypatch.setattr(functions, "_DEBUG", None)
    print(f"{kind} {math}: {int(bad.sum())} of {N} rays screened")
    assert bad.sum() <= max(1, 0.1 * N), f"{bad.sum()} rays screened"
    keep = torch.from_numpy(~bad)
    _functional(res, keep, 9, prefix).backward()
    assert r.grad is not None, "no gradient with respect to the rays"
    g32s, g64s = [], []
    for (_, r32, o32, _), (_, r64, o64, _) in pts.values():
        _functional(o32, keep, 9, prefix).backward()
        _functional(o64, keep, 9, prefix).backward()
        g32s.append(_cols(r32.grad))
        g64s.append(_cols(r64.grad))
    floor = grad64.fp32_floor(g32s, g64s)
    print("fp32 floors:", {k: f"{v:.3g}" for k, v in floor.items()})
    worst, where = grad64.check(_cols(r.grad), g64s[0], floor, label=f"{kind} {math}")
    print(f"{kind} {math}: worst {worst:.2f} of its bound ({where})")


def _step(models, rays_req_grad, kind="render"):
    rays, draws = _e2e_inputs(6)
    r = rays.to(DEV).requires_grad_(rays_req_grad)
    for m in models:
        m.zero_grad(set_to_none=True)
    res = _render(kind, models, r, draws, I)
    _functional(res, torch.ones(N, dtype=torch.bool), 4).backward()
    return res, r.grad


def test_frozen_networks_same_ray_gradient():
    """pose inversion: frozen networks give the rays.grad of trainable ones,
    bit for bit, and no parameter gets a gradient"""
    _, g_train = _step(_models(21, 2), True)
    frozen = _models(21, 2, trainable=False)
    _, g_frozen = _step(frozen, True)
    assert g_frozen is not None and g_train is not None
    assert g_train.abs().max() > 0 and torch.isfinite(g_train).all()
    assert torch.equal(g_frozen, g_train)
    assert all(p.grad is None for m in frozen for p in m.parameters())


@pytest.mark.parametrize("kind", ["render", "rgb_sm", "shadows"])
def test_nothing_moves_for_the_parameters(kind):
    """with and without rays.requires_grad: the same result dict and the same
    parameter gradients, bit for bit"""
    models = _models(21, 2)
    res_a, g = _step(models, False, kind)
    assert g is None
    grads_a = [p.grad.clone() for m in models for p in m.parameters() if p.grad is not None]
    res_b, g = _step(models, True, kind)
    assert g is not None
    grads_b = [p.grad for m in models for p in m.parameters() if p.grad is not None]
    for k in res_a:
        assert torch.equal(res_a[k], res_b[k]), k
    assert len(grads_a) == len(grads_b) > 0
    for a, b in zip(grads_a, grads_b):
        assert torch.equal(a, b)


def test_no_silent_path():
    """every path that cannot produce the ray gradient says so"""
    from nerf_pl_amd import Embedding, NeRF, render_rays, rendering_shadows
    rays, _ = _e2e_inputs(7)
    r = rays.to(DEV).requires_grad_(True)
    models = _models(21, 1)
    with pytest.raises(NotImplementedError, match="composable"):
        render_rays(models, [Embedding(3, 6), Embedding(3, 4)], r, S, False, 0, 0, 0)
    with pytest.raises(NotImplementedError, match="sharded"):
        rendering_shadows.render_rays_sharded(models, [Embedding(3, 10), Embedding(3, 4)], r, S)
    x = torch.randn(7, 90, device=DEV, requires_grad=True)
    with pytest.raises(NotImplementedError, match="embedded"):
        NeRF().to(DEV)(x)


def test_bf16_arithmetic_reads_its_own_rows(monkeypatch):
    """NERF_PL_AMD_MATH=bf16 keeps its gradient rows as bf16 in N16 slots at
    half the block stride (x3.h NR_BF1): the input-gradient kernel reads that
    layout (2).  The arithmetic is not fp32-accurate, so the reference is the
    same arithmetic emulated in float64 (tests/test_gpu_bf16.py _LinBF16 /
    _FinalDirBF16): dz1, dz5, dz_dir of the emulated backward rounded to bf16
    as the kernels store them, then stage 1 of the restatement with the fp32
    weights.  Bound: test_bf16_backward_is_the_documented_arithmetic's, 1e-2
    of each gradient's L2 norm (the kernels and the emulation differ in fp32
    accumulation order, whose ulps occasionally flip a bf16 rounding of an
    intermediate gradient).  bf16's own distance from float64 is printed."""
    from nerf_pl_amd import ops
    from test_gpu_bf16 import _FinalDirBF16, _LinBF16, rb
    monkeypatch.setattr(ops, "MATH", "bf16")
    p, rays, z, gout, refs = _mlp_case((23, 37), False)
    _, _, g_rays, g_z = _ours_mlp(p, rays, z, gout, False)
    spr = z.shape[1]
    xyz = (rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)   # fp32 positions
    P = {k: v.double() for k, v in p.items()}
    xe = O.embed(xyz, 10).double().requires_grad_(True)
    xd = O.embed(rays[:, 3:6], 4).repeat_interleave(spr, 0).double()
    lin = lambda h, name, r=True: _LinBF16.apply(h, P[name + ".weight"], P[name + ".bias"], r, r)  # noqa: E731
    h, taps = xe, {}
    for i in range(8):
        if i == 4:
            h = torch.cat([xe, h], -1)
        taps[i] = lin(h, f"xyz_encoding_{i + 1}.0")
        taps[i].retain_grad()
        h = torch.relu(taps[i])
    sigma = lin(h, "sigma", False)
    pre = _FinalDirBF16.apply(h, xd, P["xyz_encoding_final.weight"], P["xyz_encoding_final.bias"],
                              P["dir_encoding.0.weight"], P["dir_encoding.0.bias"])
    pre.retain_grad()
    out = torch.cat([torch.sigmoid(lin(torch.relu(pre), "rgb.0", False)), sigma], -1)
    (out * gout.double()).sum().backward()
    emu_rays, emu_z = R64.mlp_input_grad(p, rays, z, rb(taps[0].grad), rb(taps[4].grad),
                                         rb(pre.grad), xyz=xyz)
    r64, z64, _ = refs[F64]
    for what, got, emu, ref in (("g_o", g_rays[:, 0:3], emu_rays[:, 0:3], r64[:, 0:3]),
                                ("g_d", g_rays[:, 3:6], emu_rays[:, 3:6], r64[:, 3:6]),
                                ("g_z", g_z, emu_z, z64)):
        got = got.cpu().double().numpy()
        err = np.linalg.norm(got - emu) / np.linalg.norm(ref)
        own = np.linalg.norm(emu - ref) / np.linalg.norm(ref)
        print(f"bf16 {what}: {err:.3g} of its norm from the bf16 emulation (the emulation: "
              f"{own:.3g} from float64)")
        assert err <= 1e-2, f"{what}: {err:.3g}"
