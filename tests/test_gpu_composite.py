"""The two compositing kernels (csrc/render.hip composite_fwd_kernel,
composite_bwd_kernel) and the stratified depths, called directly, at the
sample counts around the 64-sample chunk, ray counts that do not fill the
4-waves-per-block launch, both raw layouts and every set of incoming gradients.

Backward: against tests/composite64.py (the kernel's closed form in
longdouble; why not float64 autograd of the reference formula: its docstring),

    |d sigma - ref| <= 2^-22 |ref| + 1e-12 M_i + 2^-126
    |d c     - ref| <= 2^-22 |ref| + 2^-126

2^-22: a double result rounded once to fp32 (d c: twice), with margin; 1e-12
M_i: ~10x the float64 evaluation's own distance from longdouble
(test_composite64.py, 9.7e-14); 2^-126: fp32 underflow.  Exact zeros where
the reference is exactly zero (closed ReLU, one sample per ray, e underflowed).

Forward: against the fp32 CPU oracle (the reference's own arithmetic), with
the bounds of test_gpu_kernels.test_composite_forward: 2e-6 absolute on
weights, rgb and opacity, 2e-6 on depth relative to max(|depth|, 1).
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import composite64 as C64
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SAMPLES = (1, 2, 3, 63, 64, 65, 128, 129, 192, 193)
RAYS = (1, 5, 37)            # 5 and 37: no multiple of the 4 waves per block
SHAPES = [(S, n) for S in SAMPLES for n in RAYS]
NAMES = ("g_rgb", "g_depth", "g_opacity")
SUBSETS = [c for k in (1, 2, 3) for c in itertools.combinations(NAMES, k)]
SEED, STREAM = 0, 1


class Group:
    """The ray counts of one (regime, S) share one evaluation of the reference
    (its sequential loops over the samples cost the same for 1 ray as for 43)."""

    def __init__(self, regime, S):
        self.cases = [C64.make_case(regime, S, n) for n in RAYS]
        first = self.cases[0]

        def cat(k):
            return None if first[k] is None else np.concatenate([c[k] for c in self.cases])
        self.fw = C64.Composite64(cat("raw"), cat("z"), cat("rays"), cat("noise"),
                                  first["noise_std"])
        self.g = {k: cat(k) for k in NAMES}
        self.done = {}

    def backward(self, white_back, names):
        key = (white_back, names)
        if key not in self.done:
            self.done[key] = self.fw.backward(
                white_back, **{x: (self.g[x] if x in names else None) for x in NAMES})
        return self.done[key]


@functools.lru_cache(maxsize=None)
def group(regime, S):
    return Group(regime, S)


class Case:
    def __init__(self, regime, S, n):
        self.grp = group(regime, S)
        i = RAYS.index(n)
        cs = self.cs = self.grp.cases[i]
        self.rows = slice(sum(RAYS[:i]), sum(RAYS[:i]) + n)
        self.S, self.n = S, n
        dev = lambda a: None if a is None else torch.from_numpy(a).to(DEV)   # noqa: E731
        self.raw4 = dev(cs["raw"])
        self.raw1 = self.raw4[:, 3:].contiguous()
        self.z, self.rays, self.noise = dev(cs["z"]), dev(cs["rays"]), dev(cs["noise"])
        self.noise_std = cs["noise_std"]
        self.g = {k: dev(cs[k]) for k in NAMES}

    def ref_backward(self, white_back, names):
        """(d sigma, d c, M) of composite64 for this case's rays"""
        return tuple(a[self.rows] for a in self.grp.backward(white_back, names))

    def fwd_args(self, raw):
        return raw, self.z, self.rays, self.noise, self.noise_std, SEED, STREAM


@functools.lru_cache(maxsize=None)
def case(regime, S, n):
    return Case(regime, S, n)


def bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def backward(k, raw, white_back, g):
    from nerf_pl_amd import ops
    return ops.composite_backward(*k.fwd_args(raw), white_back, g["g_rgb"], g["g_depth"],
                                  g["g_opacity"])


def ratio_to_bound(got, ref, extra, what):
    """worst |got - ref| / (2^-22 |ref| + extra + 2^-126); exact zeros where
    the reference is exactly zero"""
    got = got.astype(C64.WIDE)
    bound = 2.0 ** -22 * np.abs(ref) + extra + 2.0 ** -126
    r = np.abs(got - ref) / bound
    assert np.all(np.isfinite(got)), what
    assert not got[ref == 0].any(), f"{what}: nonzero where the reference is exactly 0"
    return float(r.max(initial=0))


@pytest.mark.parametrize("white_back", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("names", SUBSETS, ids="+".join)
@pytest.mark.parametrize("regime", C64.REGIMES)
def test_backward_matches_composite64(regime, names, white_back):
    """Measured on the MI355X, worst ratio to the bound over every shape, set of
    gradients and background, d sigma / d c: typical 0.249 / 0.463, opaque
    0.249 / 0.442, closed 0 / 0 (all exact zeros), last 0.246 / 0.384, noise
    0.248 / 0.467, ndc 0.249 / 0.474.  0.25 = 2^-24 / 2^-22 is one fp32
    rounding of an otherwise exact value, 0.5 two of them (d c = fp32(w) *
    g_rgb)."""
    worst = [0.0, 0.0, None]
    for S, n in SHAPES:
        k = case(regime, S, n)
        g = {x: (k.g[x] if x in names else None) for x in NAMES}
        dsig, dc, M = k.ref_backward(white_back, names)
        got = backward(k, k.raw4, white_back, g).cpu().numpy().reshape(n, S, 4)
        what = f"{regime} S={S} n={n} {'+'.join(names)} white_back={white_back}"
        rs = ratio_to_bound(got[..., 3], dsig, 1e-12 * M, what + " d sigma")
        rc = ratio_to_bound(got[..., :3], dc, 0, what + " d c")
        if rs > worst[0] or rc > worst[1]:
            worst = [max(rs, worst[0]), max(rc, worst[1]), what]
        assert rs <= 1 and rc <= 1, f"{what}: d sigma {rs:.3g}, d c {rc:.3g} of the bound"
        if "g_rgb" in names:
            continue
        # sigma-only rows: the stride-4 call with a zero colour gradient, bit for bit
        got1 = backward(k, k.raw1, white_back, g)
        assert got1.shape == (n * S, 1)
        zero_c = dict(g, g_rgb=torch.zeros(n, 3, device=DEV))
        got4 = backward(k, k.raw4, white_back, zero_c)
        assert same_bits(got1[:, 0], got4[:, 3]), what + " stride 1 vs stride 4"
        assert same_bits(got1[:, 0], torch.from_numpy(got[..., 3].reshape(-1))), what
        assert not got4[:, :3].any()
        if white_back:
            # no colour gradient: white_back must not shift the opacity gradient
            black = backward(k, k.raw1, False, g)
            assert same_bits(got1, black), what + " white_back shifted go without g_rgb"
    print(f"composite backward {regime} {'+'.join(names)} white_back={white_back}: worst ratio "
          f"to the bound d sigma {worst[0]:.3g}, d c {worst[1]:.3g} ({worst[2]})")


@pytest.mark.parametrize("white_back", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("regime", C64.REGIMES)
def test_autograd_is_the_direct_call(regime, white_back):
    """functions.composite_apply + autograd with a loss on one output at a time
    is the direct kernel call with the other incoming gradients zero, bit for
    bit (the _Composite.backward wiring: argument order, has_noise, None for
    the unused outputs)."""
    from nerf_pl_amd import functions
    for S, n in SHAPES:
        k = case(regime, S, n)
        for raw0, outs in ((k.raw4, (0, 1, 2)), (k.raw1, (1, 2))):
            for o in outs:
                raw = raw0.clone().requires_grad_(True)
                res = functions.composite_apply(*k.fwd_args(raw), white_back)
                gin = k.g[NAMES[o]]
                (res[o] * gin).sum().backward()
                zeros = {"g_rgb": None if raw0 is k.raw1 else torch.zeros(n, 3, device=DEV),
                         "g_depth": torch.zeros(n, device=DEV),
                         "g_opacity": torch.zeros(n, device=DEV)}
                direct = backward(k, raw0, white_back, dict(zeros, **{NAMES[o]: gin}))
                assert same_bits(raw.grad, direct), (regime, S, n, raw0.shape[-1], NAMES[o])
                alone = backward(k, raw0, white_back,
                                 {x: (gin if x == NAMES[o] else None) for x in NAMES})
                assert same_bits(direct, alone), (regime, S, n, raw0.shape[-1], NAMES[o], "None")


def oracle32(k, white_back):
    cs = k.cs
    n, S = k.n, k.S
    raw = torch.from_numpy(cs["raw"]).view(n, S, 4)
    noise = torch.zeros(n, S) if cs["noise"] is None else torch.from_numpy(cs["noise"])
    return O.composite(raw[..., 3], raw[..., :3], torch.from_numpy(cs["z"]),
                       torch.from_numpy(cs["rays"][:, 3:6]), cs["noise_std"], white_back,
                       O.ReplayRNG([noise]))


@pytest.mark.parametrize("white_back", [False, True], ids=["black", "white"])
@pytest.mark.parametrize("regime", C64.REGIMES)
def test_forward_matches_oracle(regime, white_back):
    from nerf_pl_amd import ops
    worst = dict(w=0.0, rgb=0.0, opacity=0.0, depth=0.0)
    for S, n in SHAPES:
        k = case(regime, S, n)
        rgb, depth, opac, w = ops.composite_forward(*k.fwd_args(k.raw4), white_back)
        assert rgb.shape == (n, 3) and depth.shape == (n,) and opac.shape == (n,)
        assert w.shape == (n, S)
        if S == 1:
            # the reference composites nothing (weights (N, 0)): every output 0
            assert not w.any() and not depth.any() and not opac.any()
            assert torch.equal(rgb, torch.full_like(rgb, 1.0 if white_back else 0.0))
        else:
            ref_rgb, ref_depth, ref_w = oracle32(k, white_back)
            err = dict(w=(w.cpu() - ref_w).abs().max().item(),
                       rgb=(rgb.cpu() - ref_rgb).abs().max().item(),
                       opacity=(opac.cpu() - ref_w.sum(1)).abs().max().item(),
                       depth=((depth.cpu() - ref_depth).abs()
                              / ref_depth.abs().clamp_min(1.0)).max().item())
            for q, e in err.items():
                worst[q] = max(worst[q], e)
                assert e < 2e-6, f"{regime} S={S} n={n}: {q} {e:.3g} from the fp32 oracle"
        # the entry points of the eval path and of the sigma-only render
        _, _, opac_w, w_w = ops.composite_forward(*k.fwd_args(k.raw4), white_back,
                                                  weights_only=True)
        assert same_bits(w_w, w) and same_bits(opac_w, opac)
        rgb1, depth1, opac1, w1 = ops.composite_forward(*k.fwd_args(k.raw1), white_back)
        assert rgb1 is None
        assert same_bits(w1, w) and same_bits(depth1, depth) and same_bits(opac1, opac)
        _, _, opac1w, w1w = ops.composite_forward(*k.fwd_args(k.raw1), white_back,
                                                  weights_only=True)
        assert same_bits(w1w, w) and same_bits(opac1w, opac)
        if white_back:
            plain = ops.composite_forward(*k.fwd_args(k.raw4), False)
            assert same_bits(plain[3], w) and same_bits(plain[1], depth)
            assert same_bits(rgb, plain[0] + (1.0 - plain[2])[:, None])
    print(f"composite forward {regime} white_back={white_back}: worst from the fp32 oracle "
          + ", ".join(f"{q} {e:.2g}" for q, e in worst.items()))


def test_in_kernel_noise_is_deterministic():
    """noise=None with noise_std > 0 draws Philox normals in the kernel: the
    same (seed, stream) gives the same bits in two calls, forward and backward,
    and another seed differs.  That the backward re-draws what the forward
    drew, and what those draws are, is tests/test_gpu_philox.py's: there the
    in-kernel draw has a reference (both kernels against replay of the draws)"""
    from nerf_pl_amd import ops
    for S, n in ((65, 37), (193, 5)):
        k = case("typical", S, n)
        a = (k.raw4, k.z, k.rays, None, 1.0)
        f1 = ops.composite_forward(*a, 7, STREAM, False)
        f2 = ops.composite_forward(*a, 7, STREAM, False)
        assert all(same_bits(x, y) for x, y in zip(f1, f2))
        f3 = ops.composite_forward(*a, 8, STREAM, False)
        assert not same_bits(f1[3], f3[3])
        g = (k.g["g_rgb"], k.g["g_depth"], k.g["g_opacity"])
        b1 = ops.composite_backward(*a, 7, STREAM, False, *g)
        b2 = ops.composite_backward(*a, 7, STREAM, False, *g)
        assert same_bits(b1, b2)
        assert not same_bits(b1, ops.composite_backward(*a, 8, STREAM, False, *g))


@pytest.mark.parametrize("use_disp", [False, True], ids=["depth", "disp"])
@pytest.mark.parametrize("perturb", [0.0, 0.5, 1.0])
@pytest.mark.parametrize("S", [1, 2, 65])
def test_coarse_z_bit_exact(S, perturb, use_disp):
    from nerf_pl_amd import ops
    n = 37
    g = torch.Generator().manual_seed(S)
    near = torch.rand(n, 1, generator=g) * 2 + 0.5
    far = near + torch.rand(n, 1, generator=g) * 100 + 1
    rays = torch.cat([torch.randn(n, 6, generator=g), near, far], 1)
    u = torch.rand(n, S, generator=g)
    ref = O.coarse_z(rays, S, use_disp, perturb, O.ReplayRNG([u]))
    z = ops.coarse_z(rays.to(DEV), S, use_disp, perturb, u=u.to(DEV) if perturb > 0 else None)
    assert z.shape == (n, S)
    np.testing.assert_array_equal(z.cpu().numpy(), ref.numpy())
