"""High-precision reference of the volume compositing and its backward (test
infrastructure, like parity.py and grad64.py).

The compositing backward kernel (csrc/render.hip composite_bwd_kernel)
evaluates, in double from the fp32 inputs,

    delta_i = (z_{i+1} - z_i) |d|,  the last 1e10 |d|  (0 with one sample)
    s_i     = fp32(sigma_i + fp32(noise_i * noise_std))
    e_i     = exp(-delta_i relu(s_i)),  a_i = 1 - e_i,  f_i = e_i + 1e-10
    T_i     = prod_{j<i} f_j,           w_i = a_i T_i
    dw_i    = <g_rgb, c_i> + g_depth z_i + g_opacity (- sum g_rgb if white_back)
    R_i     = sum_{k>i} dw_k a_k prod_{i<j<k} f_j
    dsig_i  = T_i (dw_i - R_i) e_i delta_i [s_i > 0],   dc_i = w_i g_rgb

and rounds each gradient to fp32 once.  This module evaluates the same closed
form in ``numpy.longdouble`` (80-bit on x86; float64 where longdouble is no
wider) with plain sequential loops over the samples and ``expm1`` for a_i.

Why not float64 autograd of ``oracle.composite``: the reference's
``1 - alphas + 1e-10`` forms f_i as 1 - (1 - e_i) + 1e-10, which loses e_i's
low bits once the transmittance saturates (f_i ~ 1e-10); its float64 gradient
is then off by up to ~2e-6 of the natural scale of d sigma,

    M_i = T_i e_i delta_i (|dw_i| + sum_{k>i} |dw_k| a_k prod_{i<j<k} f_j),

far above what an fp32-rounded double kernel must meet.  The closed form above
in float64 stays within ~1e-13 M_i of its longdouble evaluation
(tests/test_composite64.py measures it), which is the headroom the GPU bound
of tests/test_gpu_composite.py rests on.
"""
import numpy as np

WIDE = np.longdouble if np.finfo(np.longdouble).eps < np.finfo(np.float64).eps else np.float64

REGIMES = ("typical", "opaque", "closed", "last", "noise", "ndc")


def _f32(t):
    if t is None:
        return None
    if hasattr(t, "detach"):
        t = t.detach().cpu().numpy()
    t = np.asarray(t)
    assert t.dtype == np.float32, t.dtype
    return t


class Composite64:
    """Forward quantities of one batch, in ``dtype``; ``backward`` per set of
    incoming gradients.  Arrays are (n_rays, S), the sample axis last."""

    def __init__(self, raw, z, rays, noise=None, noise_std=0.0, dtype=WIDE):
        dt = self.dt = dtype
        z32 = _f32(z)
        n, S = z32.shape
        raw32 = _f32(raw).reshape(n, S, -1)
        stride = raw32.shape[-1]
        assert stride in (1, 4), stride
        sig = raw32[..., stride - 1]
        if noise is not None:
            # fp32 product, then fp32 sum (render.hip sample_noise, alpha_of)
            s32 = sig + _f32(noise).reshape(n, S) * np.float32(noise_std)
        else:
            assert noise_std == 0, ("the in-kernel Philox draw has no reference here: "
                                    "tests/test_gpu_philox.py proves it equal to replayed noise")
            s32 = sig.copy()
        assert s32.dtype == np.float32
        self.n, self.S, self.s32 = n, S, s32
        self.open = s32 > 0
        self.c = (raw32[..., :3] if stride == 4 else np.zeros((n, S, 3), np.float32)).astype(dt)
        self.z = z32.astype(dt)
        d = _f32(rays)[:, 3:6].astype(dt)
        dn = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
        delta = np.zeros((n, S), dt)
        delta[:, :-1] = (self.z[:, 1:] - self.z[:, :-1]) * dn[:, None]
        delta[:, -1] = dt(1e10) * dn if S > 1 else 0
        self.delta = delta
        self._forward(np.maximum(s32, 0).astype(dt))

    def _forward(self, r):
        """e, alpha, f, T, w from relu(s) = r (kept apart so a finite
        difference can re-evaluate the forward at a moved r)"""
        dt = self.dt
        x = self.delta * r
        self.e = np.exp(-x)
        self.alpha = -np.expm1(-x)
        self.f = self.e + dt(1e-10)
        T = np.ones((self.n, self.S), dt)
        run = np.ones(self.n, dt)
        for i in range(self.S):
            T[:, i] = run
            run = run * self.f[:, i]
        self.T = T
        self.w = self.alpha * T

    def outputs(self, white_back, w=None, const=True):
        """rgb (n, 3), depth, opacity of the weights ``w`` (default: ours);
        ``const=False`` leaves out white_back's constant 1 (the outputs are
        then linear in w)"""
        w = self.w if w is None else w
        dt = self.dt
        rgb = np.zeros((self.n, 3), dt)
        depth = np.zeros(self.n, dt)
        opac = np.zeros(self.n, dt)
        for i in range(self.S):
            rgb = rgb + w[:, i, None] * self.c[:, i]
            depth = depth + w[:, i] * self.z[:, i]
            opac = opac + w[:, i]
        if white_back:
            rgb = rgb - opac[:, None] + (1 if const else 0)
        return rgb, depth, opac

    def backward(self, white_back, g_rgb=None, g_depth=None, g_opacity=None):
        """d sigma (n, S), d c (n, S, 3) and the scale M (n, S)"""
        dt, n, S = self.dt, self.n, self.S
        g_rgb, g_depth, g_opacity = _f32(g_rgb), _f32(g_depth), _f32(g_opacity)
        gc = np.zeros((n, 3), dt) if g_rgb is None else g_rgb.astype(dt)
        gd = np.zeros(n, dt) if g_depth is None else g_depth.astype(dt)
        go = np.zeros(n, dt) if g_opacity is None else g_opacity.astype(dt)
        if white_back:
            go = go - (gc[:, 0] + gc[:, 1] + gc[:, 2])
        dw = (self.c * gc[:, None, :]).sum(-1) + gd[:, None] * self.z + go[:, None]
        R = np.zeros((n, S), dt)
        Rabs = np.zeros((n, S), dt)
        run = np.zeros(n, dt)
        run_abs = np.zeros(n, dt)
        for i in range(S - 1, -1, -1):
            R[:, i] = run
            Rabs[:, i] = run_abs
            run = self.f[:, i] * run + dw[:, i] * self.alpha[:, i]
            run_abs = self.f[:, i] * run_abs + np.abs(dw[:, i]) * self.alpha[:, i]
        ted = self.T * self.e * self.delta
        dsig = np.where(self.open, ted * (dw - R), dt(0))
        M = ted * (np.abs(dw) + Rabs)
        dc = self.w[:, :, None] * gc[:, None, :]
        return dsig, dc, M


def composite64(raw, z, rays, noise=None, noise_std=0.0, white_back=False, g_rgb=None,
                g_depth=None, g_opacity=None, dtype=WIDE):
    """(d sigma, d c, w, M) of the fp32 inputs the kernel gets"""
    fw = Composite64(raw, z, rays, noise, noise_std, dtype)
    dsig, dc, M = fw.backward(white_back, g_rgb, g_depth, g_opacity)
    return dsig, dc, fw.w, M


def make_case(regime, S, n_rays, seed=0):
    """Seeded fp32 inputs of one regime: dict of numpy arrays raw (n*S, 4),
    z (n, S), rays (n, 8), noise (n, S) or None, noise_std, g_rgb, g_depth,
    g_opacity.  Directions are not unit (|d| in [0.3, 3]); depths are sorted
    uniform in [1, 200] ([0, 1] for ``ndc``)."""
    assert regime in REGIMES, regime
    g = np.random.default_rng([seed, REGIMES.index(regime), S, n_rays])
    f32 = np.float32
    lo, hi = (0.0, 1.0) if regime == "ndc" else (1.0, 200.0)
    z = np.sort(g.uniform(lo, hi, (n_rays, S)).astype(f32), axis=1)
    d = g.standard_normal((n_rays, 3))
    d *= (g.uniform(0.3, 3.0, (n_rays, 1)) / np.linalg.norm(d, axis=1, keepdims=True))
    rays = np.concatenate([g.standard_normal((n_rays, 3)), d,
                           np.full((n_rays, 1), lo), np.full((n_rays, 1), hi)], 1).astype(f32)
    nrm = g.standard_normal((n_rays, S))
    if regime in ("typical", "noise", "ndc"):
        sig = 0.05 * nrm
    elif regime == "opaque":
        sig = 5.0 * nrm + 3.0
    else:                                   # closed, last: sigma <= 0, some exactly 0
        sig = -np.abs(0.05 * nrm)
        sig[:, ::7] = 0.0
        if regime == "last":                # delta sigma of order 1 at the 1e10 |d| delta
            sig[:, -1] = 3e-10 * g.uniform(0.01, 0.99, n_rays)
    raw = np.concatenate([g.uniform(0, 1, (n_rays, S, 3)), sig[..., None]], -1).astype(f32)
    noise = g.standard_normal((n_rays, S)).astype(f32) if regime == "noise" else None
    return dict(raw=raw.reshape(n_rays * S, 4), z=z, rays=rays, noise=noise,
                noise_std=1.0 if regime == "noise" else 0.0,
                g_rgb=g.standard_normal((n_rays, 3)).astype(f32),
                g_depth=(g.standard_normal(n_rays) / hi).astype(f32),
                g_opacity=g.standard_normal(n_rays).astype(f32))
