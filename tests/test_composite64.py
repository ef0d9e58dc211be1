"""Self-test of tests/composite64.py, the high-precision compositing reference
(CPU only).  The accuracy claim rests on the central-difference witness and on
the float64-vs-longdouble headroom; the comparison with float64 autograd of
``oracle.composite`` is a sanity witness only (that formula cancels once the
transmittance saturates, see composite64's docstring)."""
import numpy as np
import pytest
import torch

import composite64 as C64
from oracle import nerf_oracle as O

SHAPES = (2, 3, 5, 64, 65, 193)
N_RAYS = 37
# float64 underflow: where e_i = exp(-delta s) drops below the float64 range
# (delta s > 708) a float64 evaluation holds 0 or a subnormal and the
# longdouble one a value of that size; such a gradient is far below fp32's
# range too (the GPU bound's 2^-126 covers it)
TINY64 = float(np.finfo(np.float64).tiny)
SUBSETS = (("g_rgb",), ("g_depth",), ("g_opacity",), ("g_rgb", "g_depth", "g_opacity"))


def cases():
    for regime in C64.REGIMES:
        for S in SHAPES:
            yield regime, S, C64.make_case(regime, S, N_RAYS)


def grads(cs, names):
    return {k: (cs[k] if k in names else None) for k in ("g_rgb", "g_depth", "g_opacity")}


def oracle64(fw, cs, white_back):
    """float64 oracle.composite on the fp32 s = sigma + noise the kernel sees"""
    n, S = fw.n, fw.S
    s = torch.from_numpy(fw.s32).double().requires_grad_(True)
    rgbs = torch.from_numpy(cs["raw"]).view(n, S, 4)[..., :3].double()
    z = torch.from_numpy(cs["z"]).double()
    d = torch.from_numpy(cs["rays"][:, 3:6]).double()
    rgb, depth, w = O.composite(s, rgbs, z, d, 0.0, white_back,
                                O.ReplayRNG([torch.zeros(n, S)]))
    return s, rgb, depth, w


def test_one_sample_is_all_zero():
    for regime in C64.REGIMES:
        cs = C64.make_case(regime, 1, 5)
        fw = C64.Composite64(cs["raw"], cs["z"], cs["rays"], cs["noise"], cs["noise_std"])
        for wb in (False, True):
            dsig, dc, M = fw.backward(wb, cs["g_rgb"], cs["g_depth"], cs["g_opacity"])
            rgb, depth, opac = fw.outputs(wb, const=False)
            for a in (dsig, dc, M, fw.w, rgb, depth, opac):
                assert not a.any()


def test_forward_matches_float64_oracle():
    """w, rgb, depth agree with oracle.composite in float64 to 1e-12 of the
    ray's largest value, outside the opaque regime (the oracle cancels there).
    The oracle's alpha = 1 - exp(-x) also carries exp's absolute rounding near
    1, 2^-53, whatever the size of alpha (a ray of thin NDC slabs whose last
    sample is closed has every weight below 1e-4): that absolute error, times
    the S terms of a sum and the largest |z|, is allowed on top."""
    worst = 0.0
    for regime, S, cs in cases():
        if regime == "opaque":
            continue
        fw = C64.Composite64(cs["raw"], cs["z"], cs["rays"], cs["noise"], cs["noise_std"])
        for wb in (False, True):
            _, rgb_o, depth_o, w_o = oracle64(fw, cs, wb)
            rgb, depth, _ = fw.outputs(wb)
            for got, ref in ((fw.w, w_o), (rgb, rgb_o), (depth, depth_o)):
                ref = ref.detach().numpy().reshape(fw.n, -1)
                err = np.abs(got.reshape(fw.n, -1) - ref)
                scale = np.broadcast_to(np.abs(ref).max(1, keepdims=True), err.shape)
                absr = 2.0 ** -53 * S * max(1.0, float(np.abs(cs["z"]).max()))
                assert np.all(err <= 1e-12 * scale + absr), (regime, S, wb)
                worst = max(worst, float((err[scale > 0] / scale[scale > 0]).max(initial=0)))
    print(f"composite64 forward vs float64 oracle: worst {worst:.3g} of the ray's max")


def test_dsigma_near_float64_autograd():
    """sanity witness: within 1e-5 M_i of float64 autograd of oracle.composite
    (about 5x that formula's own measured deficit), every regime"""
    worst = {}
    for regime, S, cs in cases():
        fw = C64.Composite64(cs["raw"], cs["z"], cs["rays"], cs["noise"], cs["noise_std"])
        for wb in (False, True):
            for names in SUBSETS:
                g = grads(cs, names)
                s, rgb, depth, w = oracle64(fw, cs, wb)
                loss = 0
                if g["g_rgb"] is not None:
                    loss = loss + (rgb * torch.from_numpy(g["g_rgb"]).double()).sum()
                if g["g_depth"] is not None:
                    loss = loss + (depth * torch.from_numpy(g["g_depth"]).double()).sum()
                if g["g_opacity"] is not None:
                    loss = loss + (w.sum(1) * torch.from_numpy(g["g_opacity"]).double()).sum()
                ref = torch.autograd.grad(loss, s)[0].numpy()
                dsig, _, M = fw.backward(wb, **g)
                err = np.abs(dsig - ref)
                assert np.all(err <= 1e-5 * M + TINY64), (regime, S, wb, names)
                big = 1e-12 * M > TINY64
                worst[regime] = max(worst.get(regime, 0.0),
                                    float((err[big] / M[big]).max(initial=0)))
    print("composite64 d sigma vs float64 autograd, worst |diff| / M: "
          + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))


@pytest.mark.skipif(np.finfo(np.longdouble).eps > 1e-18,
                    reason="numpy.longdouble is no wider than float64 on this host: central "
                           "differences cannot resolve 1e-9 of the gradient's scale")
def test_dsigma_matches_central_differences():
    """The independent witness: central differences of the forward functional
    <g_rgb, rgb> + <g_depth, depth> + <g_opacity, opacity> in longdouble agree
    with the closed-form d sigma within 1e-9 M_i on a dozen entries per regime.

    Step: 1e-6 |s_i|, and no smaller than 1e-6 / delta_i (1e-6 in the exponent
    delta s): the difference quotient's rounding noise is eps / (e_i * step in
    the exponent) of M_i and its truncation (step in the exponent)^2 / 6, so a
    step relative to a small s alone would drown in noise.  The difference
    F(s+h) - F(s-h) is taken weight by weight (the outputs are linear in the
    weights, and the weights before sample i do not move), so the noise scales
    with T_i like M_i does.  Entries are open (s > 0; a closed one has d sigma
    exactly 0, checked apart) with delta s <= 8: past that e_i < 3e-4 and the
    quotient's noise eps / (e_i * 1e-6) nears the 1e-9 asked for."""
    ld = np.longdouble
    worst = {}
    for regime in C64.REGIMES:
        picked = 0
        for S in SHAPES:
            cs = C64.make_case(regime, S, N_RAYS)
            fw = C64.Composite64(cs["raw"], cs["z"], cs["rays"], cs["noise"], cs["noise_std"], ld)
            r0 = np.maximum(fw.s32, 0).astype(ld)
            x = fw.delta * r0
            rr, ii = np.nonzero(fw.open & (x <= 8) & (fw.delta > 0))
            if regime == "closed":
                assert rr.size == 0
                continue
            take = np.linspace(0, rr.size - 1, min(3, rr.size)).astype(int) if rr.size else []
            for wb, names in ((False, SUBSETS[3]), (True, SUBSETS[3]), (True, SUBSETS[0])):
                g = grads(cs, names)
                dsig, _, M = fw.backward(wb, **g)
                for t in take:
                    r_, i_ = rr[t], ii[t]
                    h = ld(1e-6) * max(r0[r_, i_], 1 / fw.delta[r_, i_])
                    ws = []
                    for sgn in (1, -1):
                        mv = C64.Composite64(cs["raw"], cs["z"], cs["rays"], cs["noise"],
                                             cs["noise_std"], ld)
                        r = r0.copy()
                        r[r_, i_] += sgn * h
                        assert r[r_, i_] > 0
                        mv._forward(r)
                        ws.append(mv.w)
                    rgb, depth, opac = fw.outputs(wb, w=ws[0] - ws[1], const=False)
                    dF = ld(0)
                    if g["g_rgb"] is not None:
                        dF = dF + (rgb[r_] * g["g_rgb"][r_].astype(ld)).sum()
                    if g["g_depth"] is not None:
                        dF = dF + depth[r_] * ld(g["g_depth"][r_])
                    if g["g_opacity"] is not None:
                        dF = dF + opac[r_] * ld(g["g_opacity"][r_])
                    fd = dF / (2 * h)
                    ratio = float(abs(fd - dsig[r_, i_]) / M[r_, i_])
                    worst[regime] = max(worst.get(regime, 0.0), ratio)
                    assert ratio <= 1e-9, (regime, S, wb, names, r_, i_, ratio)
                    picked += 1
        if regime != "closed":
            assert picked >= 12, (regime, picked)
    print("composite64 d sigma vs central differences, worst |diff| / M: "
          + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))


def test_closed_samples_have_zero_gradient():
    for regime, S, cs in cases():
        fw = C64.Composite64(cs["raw"], cs["z"], cs["rays"], cs["noise"], cs["noise_std"])
        dsig, _, _ = fw.backward(True, cs["g_rgb"], cs["g_depth"], cs["g_opacity"])
        assert not dsig[~fw.open].any()
        if regime == "closed":
            assert not dsig.any() and not fw.w.any()


def test_float64_headroom():
    """the same closed form in float64 stays within 1e-12 M_i of longdouble:
    the headroom the GPU bound (1e-12 M_i next to the fp32 rounding) rests on"""
    worst = {}
    for regime, S, cs in cases():
        a = (cs["raw"], cs["z"], cs["rays"], cs["noise"], cs["noise_std"])
        wide, dbl = C64.Composite64(*a), C64.Composite64(*a, dtype=np.float64)
        for wb in (False, True):
            for names in SUBSETS:
                g = grads(cs, names)
                ds_w, dc_w, M = wide.backward(wb, **g)
                ds_d, dc_d, _ = dbl.backward(wb, **g)
                err = np.abs(ds_d - ds_w)
                assert np.all(err <= 1e-12 * M + TINY64), (regime, S, wb, names)
                big = 1e-12 * M > TINY64
                worst[regime] = max(worst.get(regime, 0.0),
                                    float((err[big] / M[big]).max(initial=0)))
                assert np.all(np.abs(dc_d - dc_w) <= 1e-12 * np.abs(dc_w) + TINY64)
    print("composite64 float64 vs longdouble, worst |diff| / M: "
          + ", ".join(f"{k} {v:.2g}" for k, v in worst.items()))
