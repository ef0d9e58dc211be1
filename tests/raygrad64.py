"""Float64 restatement of the ray gradient, stage by stage (test infrastructure,
like composite64.py and grad64.py).

The reference's ``render_rays`` is plain PyTorch, differentiable in its (N, 8)
ray tensor.  The device path carries that gradient through four stages, each a
closed form restated here in float64 with plain loops:

  1. the MLP's input gradient from dz1, dz5, dz_dir  (``mlp_input_grad``)
  2. compositing in the depths and |d|               (``composite_raygrad``)
  3. the merge of coarse and importance depths       (``merge_raygrad``)
  4. the stratified depths in near and far           (``coarse_z_raygrad``)

tests/test_raygrad_ref.py checks every one against float64 torch autograd of
``oracle.nerf_oracle``; tests/test_gpu_raygrad.py checks the kernels against
these.  ``render64`` is the oracle's ``render_rays`` sequence from the oracle's
own pieces, in float64 autograd, evaluated AT the fp32 depths and positions the
kernels form (straight-through: value fp32, derivative float64).  The oracle's
``fp32_positions`` hook forms them by casting, which sends the gradient through
fp32 arithmetic; the float64 gradient is needed here, so the positions are
formed in this module and the oracle stays as it is.
"""
import numpy as np
import torch

from oracle import nerf_oracle as O

F64 = torch.float64


# ---------------------------------------------------------------------------
# stage 1
# ---------------------------------------------------------------------------
def mlp_taps(p, xe, de, sigma_only=False):
    """nerf_forward (nerf.py:83-124) keeping the pre-activations of layers 1
    and 5 and of the dir layer as graph nodes with retained gradients:
    (out, {1: z1, 5: z5, "dir": z_dir})"""
    lin = torch.nn.functional.linear
    taps, h = {}, xe
    for i in range(8):
        if i == 4:
            h = torch.cat([xe, h], -1)
        pre = lin(h, p[f"xyz_encoding_{i + 1}.0.weight"], p[f"xyz_encoding_{i + 1}.0.bias"])
        if i in (0, 4):
            pre.retain_grad()
            taps[i + 1] = pre
        h = torch.relu(pre)
    sigma = lin(h, p["sigma.weight"], p["sigma.bias"])
    if sigma_only:
        return sigma, taps
    feat = lin(h, p["xyz_encoding_final.weight"], p["xyz_encoding_final.bias"])
    pre = lin(torch.cat([feat, de], -1), p["dir_encoding.0.weight"], p["dir_encoding.0.bias"])
    pre.retain_grad()
    taps["dir"] = pre
    rgb = torch.sigmoid(lin(torch.relu(pre), p["rgb.0.weight"], p["rgb.0.bias"]))
    return torch.cat([rgb, sigma], -1), taps


def encoding_chain(g_e, x, n_freqs):
    """g_x (n, 3) from the channel gradients g_e (n, 3 (2 F + 1)) of
    [x, sin 2^0 x, cos 2^0 x, ...] (nerf.py:33-38) at x (n, 3)"""
    g_x = g_e[:, 0:3].copy()
    for k in range(n_freqs):
        f = 2.0 ** k
        g_x = g_x + f * (np.cos(f * x) * g_e[:, 3 + 6 * k:6 + 6 * k]
                         - np.sin(f * x) * g_e[:, 6 + 6 * k:9 + 6 * k])
    return g_x


def mlp_input_grad(p, rays, z, dz1, dz5, dzdir=None, xyz=None):
    """(g_rays (R, 8), g_z (R, S)) of stage 1: numpy float64 throughout.
    rays (R, 8), z (R, S); dz* (R S, width) the gradients of the layers'
    pre-activations; ``xyz`` (R S, 3): the positions to evaluate the encoding
    at (default o + d z in float64)."""
    f = lambda t: np.asarray(t.detach() if hasattr(t, "detach") else t, np.float64)  # noqa: E731
    rays, z, dz1, dz5 = f(rays), f(z), f(dz1), f(dz5)
    R, S = z.shape
    o, d = rays[:, 0:3], rays[:, 3:6]
    if xyz is None:
        xyz = (o[:, None, :] + d[:, None, :] * z[:, :, None]).reshape(-1, 3)
    g_e = dz1 @ f(p["xyz_encoding_1.0.weight"]) + dz5 @ f(p["xyz_encoding_5.0.weight"])[:, 0:63]
    g_x = encoding_chain(g_e, f(xyz), 10).reshape(R, S, 3)
    g = np.zeros((R, 8))
    g[:, 0:3] = g_x.sum(1)
    g[:, 3:6] = (z[:, :, None] * g_x).sum(1)
    if dzdir is not None:
        g_de = (f(dzdir) @ f(p["dir_encoding.0.weight"])[:, 256:283]).reshape(R, S, 27).sum(1)
        g[:, 3:6] += encoding_chain(g_de, d, 4)
    g_z = (d[:, None, :] * g_x).sum(-1)
    return g, g_z


# ---------------------------------------------------------------------------
# stage 2
# ---------------------------------------------------------------------------
def composite_raygrad(raw, z, rays, noise=None, noise_std=0.0, white_back=False, g_rgb=None,
                      g_depth=None, g_opacity=None, g_disp=None, depth=None, opacity=None):
    """(g_z (n, S), g_d (n, 3)) of the compositing (rendering.py:169-198) from
    the fp32 inputs the kernel gets, in float64 (composite64's forward):
        g_delta_i = T_i (dw_i - R_i) e_i relu(s_i)
        g_z[i]    = w_i (g_depth - gq O) + |d| (g_delta_{i-1} - [i < S-1] g_delta_i)
        g_|d|     = sum_{i<S-1} g_delta_i (z_{i+1} - z_i) + 1e10 g_delta_{S-1}
    ``g_disp`` with the forward's fp32 ``depth`` / ``opacity`` (D, O): disp =
    O / D where D / O > 1e-10 adds gq (D - O z_i) to dw_i, gq = g_disp / D^2."""
    from composite64 import Composite64, _f32
    dt = np.float64
    fw = Composite64(raw, z, rays, noise, noise_std, dtype=dt)
    n, S = fw.n, fw.S
    g_rgb, g_depth, g_opacity, g_disp = _f32(g_rgb), _f32(g_depth), _f32(g_opacity), _f32(g_disp)
    gc = np.zeros((n, 3), dt) if g_rgb is None else g_rgb.astype(dt)
    gd = np.zeros(n, dt) if g_depth is None else g_depth.astype(dt)
    go = np.zeros(n, dt) if g_opacity is None else g_opacity.astype(dt)
    if white_back:
        go = go - (gc[:, 0] + gc[:, 1] + gc[:, 2])
    dw = (fw.c * gc[:, None, :]).sum(-1) + gd[:, None] * fw.z + go[:, None]
    gdz = gd.copy()
    if g_disp is not None:
        D32, O32 = _f32(depth), _f32(opacity)
        with np.errstate(divide="ignore", invalid="ignore"):
            on = (D32 / O32) > np.float32(1e-10)
        D, Oq = D32.astype(dt), O32.astype(dt)
        gq = np.where(on, g_disp.astype(dt) / np.where(on, D * D, 1.0), 0.0)
        dw = dw + np.where(on, gq, 0.0)[:, None] * (np.where(on, D, 0.0)[:, None]
                                                     - np.where(on, Oq, 0.0)[:, None] * fw.z)
        gdz = gdz - gq * np.where(on, Oq, 0.0)
    R = np.zeros((n, S), dt)
    run = np.zeros(n, dt)
    for i in range(S - 1, -1, -1):
        R[:, i] = run
        run = fw.f[:, i] * run + dw[:, i] * fw.alpha[:, i]
    r = np.maximum(fw.s32, 0).astype(dt)
    g_delta = fw.T * (dw - R) * fw.e * r
    d = _f32(rays)[:, 3:6].astype(dt)
    dn = np.sqrt((d * d).sum(1))
    g_z = fw.w * gdz[:, None]
    g_z[:, 1:] += dn[:, None] * g_delta[:, :-1]
    g_z[:, :-1] -= dn[:, None] * g_delta[:, :-1]
    g_dn = (g_delta[:, :-1] * (fw.z[:, 1:] - fw.z[:, :-1])).sum(1)
    if S > 1:
        g_dn = g_dn + 1e10 * g_delta[:, -1]
    return g_z, g_dn[:, None] * d / dn[:, None]


# ---------------------------------------------------------------------------
# stage 3
# ---------------------------------------------------------------------------
def merge_raygrad(z_coarse, z_fine, g_zfine):
    """g_zcoarse (n, S): walk the sorted coarse row and the sorted merged row
    together, matching equal bit patterns in order (a coarse depth takes the
    first of equal merged entries not yet taken)."""
    zc, zf, g = (np.asarray(t) for t in (z_coarse, z_fine, g_zfine))
    out = np.zeros(zc.shape, g.dtype)
    for r in range(zc.shape[0]):
        j = 0
        for i in range(zc.shape[1]):
            while zf[r, j] != zc[r, i]:
                j += 1
            out[r, i] = g[r, j]
            j += 1
    return out


# ---------------------------------------------------------------------------
# stage 4
# ---------------------------------------------------------------------------
def coarse_z_raygrad(rays, n_samples, use_disp, perturb, u, g_z):
    """(g_near, g_far) (n,) of the stratified depths (rendering.py:216-232);
    ``u`` the fp32 draws (n, S) or None; perturb * u formed in fp32 as the
    forward forms it"""
    rays = np.asarray(rays, np.float64)
    g_z = np.asarray(g_z, np.float64)
    n, S = g_z.shape
    near, far = rays[:, 6:7], rays[:, 7:8]
    t = torch.linspace(0, 1, n_samples).numpy().astype(np.float64)[None, :]
    if perturb > 0:
        pu = (np.float32(perturb) * np.asarray(u, np.float32)).astype(np.float64)
        gl, gu = g_z * (1 - pu), g_z * pu
        g_zb = np.zeros((n, S))
        # lower_k = zb_0 | mid_{k-1};  upper_k = mid_k | zb_{S-1};  mid_k = (zb_k + zb_{k+1}) / 2
        g_zb[:, 0] += gl[:, 0]
        g_zb[:, -1] += gu[:, -1]
        for k in range(1, S):
            g_zb[:, k - 1] += 0.5 * gl[:, k]
            g_zb[:, k] += 0.5 * gl[:, k]
        for k in range(S - 1):
            g_zb[:, k] += 0.5 * gu[:, k]
            g_zb[:, k + 1] += 0.5 * gu[:, k]
    else:
        g_zb = g_z
    if not use_disp:
        return (g_zb * (1 - t)).sum(1), (g_zb * t).sum(1)
    zb = 1 / ((1 - t) / near + t / far)
    return (g_zb * zb * zb * (1 - t) / near ** 2).sum(1), (g_zb * zb * zb * t / far ** 2).sum(1)


# ---------------------------------------------------------------------------
# the whole render, float64 autograd at the kernels' fp32 depths and positions
# ---------------------------------------------------------------------------
def _through(x64, x32):
    """value x32 (widened), derivative that of x64"""
    return x64 + (x32.to(x64.dtype) - x64).detach()


def disp_map(depth, opacity):
    """rendering_rgb_sm.py:197"""
    return 1 / torch.max(torch.tensor(1e-10, dtype=depth.dtype), depth / opacity)


def render64(models, rays, N_samples, use_disp, perturb, noise_std, N_importance, white_back,
             draws, z_coarse32=None, z_fine32=None, depth_only=False, disp=False, dtype=F64,
             capture=None):
    """oracle.render_rays (training branch) rebuilt from the oracle's pieces so
    that the depths and positions can be pinned: ``rays`` (N, 8) in ``dtype``
    (a leaf that requires grad), ``models`` parameter dicts in ``dtype``;
    ``z_coarse32`` / ``z_fine32``: the fp32 depths the kernels formed -- each
    pass then runs AT those depths and at fp32(o + d z), with float64
    derivatives (None: the oracle's own, in ``dtype``).  The merged fine depths
    take the derivative of the coarse depths at their places (importance
    depths detached, rendering.py:253-255).  ``depth_only``: the sigma-only
    graph (rendering_shadows.py:164-198); ``disp``: also disp_map_*."""
    rng = O.ReplayRNG(draws)
    cap = capture if capture is not None else {}
    n = rays.shape[0]
    r32 = rays.detach().float()
    o, d = rays[:, 0:3], rays[:, 3:6]
    demb = None if depth_only else O.embed(d, 4)

    def one_pass(level, p, z, z32):
        S = z.shape[1]
        xyz = o[:, None, :] + d[:, None, :] * z[:, :, None]
        if z32 is not None:
            z = _through(z, z32)
            xyz = _through(xyz, r32[:, None, 0:3] + r32[:, None, 3:6] * z32[:, :, None])
        raw = O.run_mlp(p, xyz, demb, 1 << 30, sigma_only=depth_only)
        cap["raw_" + level] = raw
        raw = raw.view(n, S, -1)
        rgbs = torch.zeros(n, S, 3, dtype=raw.dtype) if depth_only else raw[..., :3]
        rgb, depth, w = O.composite(raw[..., -1], rgbs, z, d, noise_std, white_back, rng)
        res = {} if depth_only else {"rgb_" + level: rgb}
        res["depth_" + level] = depth
        res["opacity_" + level] = w.sum(1)
        if disp:
            res["disp_map_" + level] = disp_map(depth, w.sum(1))
        return res, w, z

    z_c = O.coarse_z(rays, N_samples, use_disp, perturb, rng)
    result, w_c, z_c_used = one_pass("coarse", models[0], z_c,
                                     None if z_coarse32 is None else z_coarse32.float())
    if N_importance > 0:
        z_pdf = O.sample_pdf(rays.detach(), w_c[:, 1:-1].detach(), N_importance, rng).detach()
        if z_fine32 is None:
            z_f, _ = torch.sort(torch.cat([z_c, z_pdf], -1), -1)
            z_f32 = None
        else:
            # the kernels' merged row: each coarse depth's place found by value
            z_f32 = z_fine32.float()
            zc32 = (z_c_used.detach().float() if z_coarse32 is None else z_coarse32.float())
            pos = torch.from_numpy(_places(zc32.numpy(), z_f32.numpy()))
            z_f = z_f32.to(dtype).clone()
            z_f = z_f.scatter(1, pos, z_c)            # coarse entries: functions of the rays
        fine, _, _ = one_pass("fine", models[1], z_f, z_f32)
        result.update(fine)
    return result


def _places(zc, zf):
    pos = np.zeros(zc.shape, np.int64)
    for r in range(zc.shape[0]):
        j = 0
        for i in range(zc.shape[1]):
            while zf[r, j] != zc[r, i]:
                j += 1
            pos[r, i] = j
            j += 1
    return pos
