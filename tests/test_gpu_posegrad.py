"""Camera-pose gradients on the device (csrc/posegrad.hip):
``nr_gen_rays_posegrad`` through ``generate_rays``'s autograd route against
the float64 restatement (tests/posegrad64.py) and float64 torch autograd of
the ray buffer, its determinism, the unchanged forward, and the wiring from
``loss.backward()`` of a render down to ``c2w.grad``.

Bounds.  test_gpu_raygrad._bound's rule, restated: per tensor
max |ours - ref64| <= max(2e-4, 2 floor) max |ref64|, where ``floor`` is the
distance of the fp32 CPU autograd from float64 on the same inputs.  Every
figure is printed before it is asserted.  No ray is screened out anywhere.
"""
import numpy as np
import pytest
import torch

import posegrad64 as P64
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NEAR, FAR = 2.0, 6.0


def _bound(got, ref64, ref32, what, tol=2e-4):
    """max-abs error within max(tol, 2 floor) of the largest reference entry"""
    got, ref64 = np.asarray(got, np.float64), np.asarray(ref64, np.float64)
    scale = np.abs(ref64).max()
    assert scale > 0, f"{what}: the reference gradient is zero"
    floor = np.abs(np.asarray(ref32, np.float64) - ref64).max() / scale
    err = np.abs(got - ref64).max() / scale
    print(f"{what}: err {err:.3g} of max |ref| {scale:.3g}, fp32 floor {floor:.3g}, "
          f"bound {max(tol, 2 * floor):.3g}")
    assert err <= max(tol, 2 * floor), f"{what}: {err:.3g} > {max(tol, 2 * floor):.3g}"


# name -> (n_poses, H, W, focal, how the rays are chosen)
SHAPES = {
    "3x5x7-all": (3, 5, 7, 6.5, None),
    "3x5x7-sel": (3, 5, 7, 6.5, "gaps"),       # repeats, pose 1 never, out-of-range entries
    "n1": (2, 5, 7, 6.5, 1),
    "n255": (2, 5, 7, 6.5, 255),
    "n257": (2, 5, 7, 6.5, 257),
    "n1000": (2, 5, 7, 6.5, 1000),             # more than 256 rays on one pose: every wave, the strided walk
    "2x40x40-all": (2, 40, 40, 44.0, None),    # 1,600 rays per pose
}
_CACHE = {}


def _case(shape, ndc):
    """inputs and the CPU references of one case, computed once and shared:
    float64 autograd, the float64 restatement and fp32 autograd"""
    key = (shape, ndc)
    if key in _CACHE:
        return _CACHE[key]
    n_poses, H, W, f, how = SHAPES[shape]
    g = torch.Generator().manual_seed(list(SHAPES).index(shape) + 17 * ndc)
    P = P64.poses(n_poses, ndc, 11 + n_poses)
    hw, sel = H * W, None
    if how == "gaps":
        pool = torch.cat([torch.arange(0, hw), torch.arange(2 * hw, 3 * hw)])
        sel = pool[torch.randint(0, pool.shape[0], (90,), generator=g)]
        sel[::7] = -1
        sel[3::11] = n_poses * hw
        assert not ((sel >= hw) & (sel < 2 * hw)).any() and (sel == -1).any() \
            and (sel == n_poses * hw).any() and sel.unique().numel() < sel.numel()
    elif how is not None:
        sel = torch.randint(0, n_poses * hw, (how,), generator=g)
    n = n_poses * hw if sel is None else sel.shape[0]
    g_rays = torch.randn(n, 8, generator=g)
    ref64 = P64.autograd_pose_grad(P, H, W, f, g_rays, sel, ndc)
    ref32 = P64.autograd_pose_grad(P, H, W, f, g_rays, sel, ndc, dtype=torch.float32)
    re64 = P64.pose_grad(P.numpy(), H, W, f, g_rays.numpy(), None if sel is None else sel.numpy(), ndc)
    # the restatement is the float64 autograd (test_posegrad_ref.py: 1e-10)
    assert np.abs(re64[0] - ref64[0]).max() <= 1e-10 * np.abs(ref64[0]).max()
    _CACHE[key] = dict(P=P, H=H, W=W, f=f, sel=sel, g_rays=g_rays, ref64=ref64, ref32=ref32,
                       re64=re64, n_poses=n_poses)
    return _CACHE[key]


def _ours(c, ndc, focal_mode):
    """c2w.grad and focal.grad through generate_rays and rays.backward"""
    from nerf_pl_amd.rays import generate_rays
    c2w = c["P"].to(DEV).requires_grad_(focal_mode != "alone")
    focal = c["f"] if focal_mode == "off" else torch.tensor(c["f"], requires_grad=True)
    sel = None if c["sel"] is None else c["sel"].to(DEV)
    rays = generate_rays(c2w, c["H"], c["W"], focal, NEAR, FAR, sel, ndc=ndc)
    assert rays.requires_grad and rays.grad_fn is not None, "the rays do not reach the poses"
    rays.backward(c["g_rays"].to(DEV))
    torch.cuda.synchronize()
    return rays.detach(), c2w.grad, (None if focal_mode == "off" else focal.grad)


@pytest.mark.parametrize("focal_mode", ["off", "on", "alone"])
@pytest.mark.parametrize("ndc", [False, True], ids=["blender", "ndc"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_pose_gradient_matches_float64(shape, ndc, focal_mode):
    from nerf_pl_amd.rays import generate_rays
    c = _case(shape, ndc)
    if ndc:     # no quotient of the NDC transform is ill-conditioned
        world = generate_rays(c["P"].to(DEV), c["H"], c["W"], c["f"], NEAR, FAR)
        assert world[:, 5].abs().min() > 0.5
    rays, g_c2w, g_f = _ours(c, ndc, focal_mode)
    what = f"{shape} {'ndc' if ndc else 'blender'} focal {focal_mode}"
    if c["sel"] is not None:
        bad = ((c["sel"] < 0) | (c["sel"] >= c["n_poses"] * c["H"] * c["W"])).to(DEV)
        assert torch.isnan(rays[bad]).all() and torch.isfinite(rays[~bad]).all()
    if focal_mode == "alone":
        assert g_c2w is None
    else:
        assert g_c2w.shape == c["P"].shape and g_c2w.dtype == torch.float32 and g_c2w.device == DEV
        assert torch.isfinite(g_c2w).all()
        _bound(g_c2w.cpu().numpy(), c["ref64"][0], c["ref32"][0], what + ": g_c2w")
        _bound(g_c2w.cpu().numpy(), c["re64"][0], c["ref32"][0], what + ": g_c2w (restatement)")
        used = np.zeros(c["n_poses"], bool)
        pix = np.arange(rays.shape[0]) if c["sel"] is None else c["sel"].numpy()
        ok = (pix >= 0) & (pix < c["n_poses"] * c["H"] * c["W"])
        used[pix[ok] // (c["H"] * c["W"])] = True
        for p in np.flatnonzero(~used):     # a pose that no ray selects: exactly zero
            assert (g_c2w[p] == 0).all()
        if shape == "3x5x7-sel":
            assert not used[1]
    if focal_mode == "off":
        assert g_f is None
    else:
        assert g_f.shape == () and g_f.dtype == torch.float32 and g_f.device.type == "cpu"
        _bound(g_f.item(), c["ref64"][1], c["ref32"][1], what + ": g_focal")
        _bound(g_f.item(), c["re64"][1].sum(), c["ref32"][1], what + ": g_focal (restatement)")


@pytest.mark.parametrize("ndc", [False, True], ids=["blender", "ndc"])
def test_two_runs_give_identical_buffers(ndc):
    from nerf_pl_amd.rays import pose_gradient
    c = _case("n1000", ndc)
    args = (c["P"].to(DEV), c["H"], c["W"], c["f"], c["g_rays"].to(DEV), c["sel"].to(DEV), ndc)
    a = pose_gradient(*args, with_focal=True)
    b = pose_gradient(*args, with_focal=True)
    assert a[0].abs().max() > 0 and a[1].dtype == torch.float64 and a[1].abs().max() > 0
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # ... and the focal partials do not disturb the pose's
    assert torch.equal(pose_gradient(*args)[0], a[0])


def test_single_pose_and_partial_range():
    """c2w of shape (3, 4) gets a (3, 4) gradient; with sel null and fewer rays
    than pixels the launch covers the first n pixels and later poses get zeros"""
    from nerf_pl_amd._lib import ptr, stream_of
    from nerf_pl_amd._lib_posegrad import call
    from nerf_pl_amd.rays import generate_rays
    c = _case("3x5x7-all", False)
    c2w = c["P"][0].to(DEV).requires_grad_(True)
    generate_rays(c2w, 5, 7, 6.5, NEAR, FAR).backward(c["g_rays"][:35].to(DEV))
    assert c2w.grad.shape == (3, 4)
    ref = P64.pose_grad(c["P"][:1].numpy(), 5, 7, 6.5, c["g_rays"][:35].numpy())[0]
    _bound(c2w.grad.cpu().numpy(), ref[0], ref[0], "single pose: g_c2w")
    n = 50                                              # pose 0, 15 pixels of pose 1, nothing of pose 2
    P, g = c["P"].to(DEV), c["g_rays"][:n].contiguous().to(DEV)
    out = torch.full((3, 3, 4), 7.0, device=DEV)
    call("nr_gen_rays_posegrad", ptr(P), 3, 5, 7, 3.5, 2.5, 6.5, 0, 1.0, -13 / 7, -13 / 5, 2.0, None,
         n, ptr(g), ptr(out), None, stream_of(DEV))
    ref = P64.pose_grad(c["P"].numpy(), 5, 7, 6.5, c["g_rays"][:n].numpy())[0]
    _bound(out.cpu().numpy(), ref, ref, "first 50 pixels: g_c2w")
    assert (out[2] == 0).all()


def test_empty_batch_gives_zeros():
    """n == 0 is not a no-op: the outputs are gradients, and are cleared"""
    from nerf_pl_amd._lib import ptr, stream_of
    from nerf_pl_amd._lib_posegrad import call
    P = _case("3x5x7-all", False)["P"].to(DEV)
    g = torch.zeros(4, 8, device=DEV)
    out = torch.full((3, 3, 4), 7.0, device=DEV)
    out_f = torch.full((3,), 7.0, dtype=torch.float64, device=DEV)
    sel = torch.zeros(4, dtype=torch.int64, device=DEV)
    call("nr_gen_rays_posegrad", ptr(P), 3, 5, 7, 3.5, 2.5, 6.5, 0, 1.0, -13 / 7, -13 / 5, 2.0,
         ptr(sel), 0, ptr(g), ptr(out), ptr(out_f), stream_of(DEV))
    assert (out == 0).all() and (out_f == 0).all()
    # ... and through autograd: an empty selection leaves a zero gradient, not none
    from nerf_pl_amd.rays import generate_rays
    c2w = P.clone().requires_grad_(True)
    rays = generate_rays(c2w, 5, 7, 6.5, NEAR, FAR, sel[:0])
    assert rays.shape == (0, 8) and rays.grad_fn is not None
    rays.sum().backward()
    assert c2w.grad.shape == (3, 3, 4) and (c2w.grad == 0).all()


@pytest.mark.parametrize("ndc", [False, True], ids=["blender", "ndc"])
def test_forward_unchanged(ndc):
    """the autograd route returns the plain launch's rays, bit for bit, and the
    colours, which carry no gradient"""
    from nerf_pl_amd.rays import generate_rays
    c = _case("3x5x7-sel", ndc)
    pool = torch.rand(3 * 5 * 7, 3, generator=torch.Generator().manual_seed(1)).to(DEV)
    sel = c["sel"].to(DEV)
    c2w = torch.nn.Parameter(c["P"].to(DEV))
    rays, rgb = generate_rays(c2w, 5, 7, 6.5, NEAR, FAR, sel, ndc=ndc, rgb_pool=pool)
    rays0, rgb0 = generate_rays(c2w.detach(), 5, 7, 6.5, NEAR, FAR, sel, ndc=ndc, rgb_pool=pool)
    assert rays.grad_fn is not None and rays0.grad_fn is None
    bits = lambda t: t.detach().view(torch.int32)      # NaN rows (out-of-range entries) compare too  # noqa: E731
    assert torch.equal(bits(rays), bits(rays0))
    assert rgb is not None and not rgb.requires_grad and torch.equal(bits(rgb), bits(rgb0))
    # without colours one tensor comes back, as on the plain path
    only = generate_rays(c2w, 5, 7, 6.5, NEAR, FAR, sel, ndc=ndc)
    assert isinstance(only, torch.Tensor) and only.grad_fn is not None
    assert torch.equal(bits(only), bits(rays0))


def test_nothing_moves_without_a_pose_that_requires_grad():
    from nerf_pl_amd.rays import generate_rays
    c = _case("3x5x7-all", False)
    rays = generate_rays(c["P"].to(DEV), 5, 7, 6.5, NEAR, FAR)
    assert rays.grad_fn is None and not rays.requires_grad
    rays = generate_rays(c["P"].to(DEV), 5, 7, torch.tensor(6.5), NEAR, FAR)     # a focal tensor, no grad
    assert rays.grad_fn is None and not rays.requires_grad
    with torch.no_grad():
        rays = generate_rays(torch.nn.Parameter(c["P"].to(DEV)), 5, 7, 6.5, NEAR, FAR)
    assert rays.grad_fn is None and not rays.requires_grad


# ---------------------------------------------------------------------------
# composition: loss.backward() of a render reaches c2w.grad
# ---------------------------------------------------------------------------
N, S, I = 48, 8, 5
IMG = 16


def _models(seed):
    from nerf_pl_amd import NeRF
    ms = []
    for m in range(2):
        net = NeRF()
        net.load_state_dict(O.make_params(seed + m, sigma_bias=0.5))
        ms.append(net.to(DEV))
    return ms


@pytest.mark.parametrize("kind", ["render", "shadows"])
def test_render_backward_reaches_the_poses(kind):
    """three poses as a Parameter, RaySampler.next(48), render_rays at 8 + 5
    samples, loss.backward(): c2w.grad is, bit for bit, the new op applied to
    the rays.grad the existing path gives when the same rays are a detached
    leaf with the same draws.  The render's own ray gradient is tested in
    test_gpu_raygrad.py; this pins the wiring."""
    from nerf_pl_amd import Embedding, ReplayRNG, render_rays, rendering_shadows
    from nerf_pl_amd.rays import RaySampler, blender_focal, pose_gradient, pose_spherical
    focal = blender_focal(IMG)
    poses = torch.stack([pose_spherical(-150.0 + 110.0 * k, -30.0, 4.0) for k in range(3)])
    g = torch.Generator().manual_seed(8)
    draws = [torch.rand(N, S, generator=g), torch.randn(N, S, generator=g),
             torch.rand(N, I, generator=g), torch.rand(N, I, generator=g),
             torch.randn(N, S + I, generator=g)]
    pool = torch.rand(3 * IMG * IMG, 3, generator=g).to(DEV)
    emb = [Embedding(3, 10), Embedding(3, 4)]
    fn = render_rays if kind == "render" else rendering_shadows.render_rays

    def loss_of(rays, rgbs):
        res = fn(_models(21), emb, rays, S, False, 1.0, 1.0, I, 32768, False, rng=ReplayRNG(draws))
        if kind == "shadows":
            return (res["depth_fine"] * rgbs[:, 0]).sum()
        return ((res["rgb_coarse"] - rgbs) ** 2).mean() + ((res["rgb_fine"] - rgbs) ** 2).mean()

    c2w = torch.nn.Parameter(poses.to(DEV))
    sampler = RaySampler(c2w, IMG, IMG, focal, NEAR, FAR, rgb_pool=pool, seed=5)
    assert sampler.c2w is c2w
    rays, rgbs = sampler.next(N)
    assert rays.requires_grad and not rgbs.requires_grad
    loss_of(rays, rgbs).backward()
    assert c2w.grad is not None and c2w.grad.shape == (3, 3, 4)

    twin = RaySampler(poses.to(DEV), IMG, IMG, focal, NEAR, FAR, rgb_pool=pool, seed=5)
    sel = RaySampler(poses.to(DEV), IMG, IMG, focal, NEAR, FAR, seed=5).next_indices(N)
    leaf, rgbs2 = twin.next(N)
    assert leaf.grad_fn is None and torch.equal(leaf, rays.detach()) and torch.equal(rgbs2, rgbs)
    leaf.requires_grad_(True)
    loss_of(leaf, rgbs2).backward()
    assert leaf.grad is not None and leaf.grad[:, :6].abs().max() > 0
    want, _ = pose_gradient(poses.to(DEV), IMG, IMG, focal, leaf.grad, sel)
    assert want.abs().max() > 0 and torch.isfinite(want).all()
    assert torch.equal(c2w.grad, want)
