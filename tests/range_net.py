"""Networks that fill the f16x3 range contract (test infrastructure, host only;
DESIGN.md 3 "Exactness contract": |w| < 255, activations < 65504, max-norm
growth of every W^T in the data-gradient chain < 2^9, per-product error
<= 3 * 2^-22 relative plus 2^-25 absolute per operand element).

``build(regime)`` rescales the nn.Linear-default network of
``make_params(7, sigma_bias=0.4)`` so that weights, activations or the
data gradient's layer-to-layer growth come near one clause of that envelope
(or, for the ``over_*`` regimes, just past exactly one of them);
``certificate`` measures in float64 where a network sits.  ``evaluate``
gives output and every parameter gradient in float64 -- for the f16x3 legs
at ``params64``: ``repr_h3`` of the matrix-core weights, the value the packed hi + lo
pieces hold, so that the comparison is of the kernels' products, scales and
sums and not of the packing's 2^-22 rounding.  ``floors`` is the CPU fp32
oracle's own distance from float64 (tests/grad64.py), the unit of the bound

    |ours - g64| / |g64|  <=  C * max(floor32, 2^-23)     per tensor,

C = 16: the contract's per-product error 3 * 2^-22 is 12 fp32 unit roundoffs,
rounded up to a power of two; 2^-23 is one fp32 ulp, the least an fp32
evaluation can be asked for.  No absolute floor: grad64.ABS_FLOOR (1e-4) would
hide a dropped lo piece.

Samples whose gradient is discontinuous at the evaluation point get a zero
output gradient: any unit of a ReLU layer with
|pre| <= 2^-18 (sum_k |w_k x_k| + |b|) in float64 -- four times the contract's
worst-case per-product bound summed over the terms, a band that scales with
the weights (the absolute 2e-6 of test_mlp_backward_matches_autograd does
not)."""
import functools
import math

import numpy as np
import torch

from grad64 import FLOOR_POINTS, fp32_floor, ulp_perturbed
from oracle import nerf_oracle as O

C = 16.0
ULP32 = 2.0 ** -23
KINK_BAND = 2.0 ** -18      # screened: |pre| <= KINK_BAND * (sum |w x| + |b|)
FLIP_BAND = 2.0 ** -16      # a mask differing from float64 is explained within this band
SEED, SIGMA_BIAS = 7, 0.4

IN_CONTRACT = ("init", "grown", "swing", "spiky", "hot", "tiny")
OUT_OF_CONTRACT = ("over_w", "over_act", "over_growth")
REGIMES = IN_CONTRACT + OUT_OF_CONTRACT

# the contract's caps
W_CAP, ACT_CAP, GROWTH_CAP = 255.0, 65504.0, 512.0

# the weights that reach the matrix cores as packed hi / lo pieces (the sigma
# and rgb heads are fp32 FMAs on the fp32 head block; biases are fp32)
SPLIT_WEIGHTS = tuple(f"xyz_encoding_{i}.0.weight" for i in range(1, 9)) + \
    ("xyz_encoding_final.weight", "dir_encoding.0.weight")

# parameters the sigma-only graph does not reach
SIGMA_ONLY_UNUSED = ("xyz_encoding_final.weight", "xyz_encoding_final.bias", "dir_encoding.0.weight",
                     "dir_encoding.0.bias", "rgb.0.weight", "rgb.0.bias")

XYZ_CH, W = 63, 256


def _hid(i):
    return f"xyz_encoding_{i}.0"


def _hcols(i):
    """the h-columns (last 256 input columns) of hidden layer i's weight"""
    return slice(XYZ_CH, None) if i == 5 else slice(None)


def _scaled(p, factors, h_only=()):
    """hidden layer i's weight times factors[i - 1] (h-columns only for the
    layers in h_only), its bias times the cumulative product"""
    cum = 1.0
    for i, f in enumerate(factors, start=1):
        cum *= f
        w = p[_hid(i) + ".weight"]
        if i in h_only:
            w[:, _hcols(i)] *= f
        else:
            w *= f
        p[_hid(i) + ".bias"] *= cum
    return p


def _spikes(p, first=254.0):
    """hidden layers 3 and 6: 16 entries at distinct rows and distinct columns
    (numpy PCG64 seed 11; per layer: rows, columns, magnitudes, signs) set to
    +-U(100, 254), each layer's first to exactly 254 -- layer 3's to ``first``;
    the h-columns of the next layer that read those rows times 2^-8"""
    g = np.random.Generator(np.random.PCG64(11))
    for i in (3, 6):
        rows = g.choice(W, 16, replace=False)
        cols = g.choice(W, 16, replace=False)
        vals = g.uniform(100.0, 254.0, 16) * g.choice([-1.0, 1.0], 16)
        vals[0] = first if i == 3 else 254.0
        w = p[_hid(i) + ".weight"]
        w[torch.from_numpy(rows), torch.from_numpy(cols)] = torch.from_numpy(vals.astype(np.float32))
        nxt = p[_hid(i + 1) + ".weight"]
        nxt[:, torch.from_numpy(rows)] *= 2.0 ** -8
    return p


SWING = (32, 1 / 32, 16, 1 / 16, 56, 1 / 56, 8, 1 / 8)
HOT = (250, 50, 5, 1 / 40, 1 / 40, 1 / 40, 1, 1)


def build(regime):
    """the parameter dict (fp32 tensors) of a regime"""
    p = {k: v.clone() for k, v in O.make_params(SEED, sigma_bias=SIGMA_BIAS).items()}
    if regime == "init":
        return p
    if regime == "grown":
        for i in range(1, 9):
            p[_hid(i) + ".weight"] *= 5.0
            p[_hid(i) + ".bias"] *= 5.0
        return p
    if regime == "swing":
        return _scaled(p, SWING)
    if regime == "spiky":
        return _spikes(p)
    if regime == "hot":
        return _scaled(p, HOT, h_only=(5,))
    if regime == "tiny":
        p[_hid(4) + ".weight"] *= 2.0 ** -12
        p[_hid(4) + ".bias"] *= 2.0 ** -12
        return p
    if regime == "over_w":
        return _spikes(p, first=256.0)
    if regime == "over_act":
        return _scaled(p, (4 * HOT[0],) + HOT[1:], h_only=(5,))
    if regime == "over_growth":
        return _scaled(p, (1, 1, 1, 1, 2000.0, 1 / 2000.0, 1, 1), h_only=(5,))
    raise ValueError(regime)


@functools.lru_cache(maxsize=None)
def inputs(n_rays, spr):
    """rays, depths and output gradient of test_mlp_backward_matches_autograd
    (seed 3, per-ray magnitude spread 2^-20 .. 1), the embedded input in fp32
    (the oracle's) and in float64 at the fp32 sample positions.  Shared:
    callers must not modify the tensors."""
    g = torch.Generator().manual_seed(3)
    rays = torch.cat([torch.randn(n_rays, 3, generator=g) * 0.3,
                      torch.nn.functional.normalize(torch.randn(n_rays, 3, generator=g), dim=-1),
                      torch.full((n_rays, 1), 2.0), torch.full((n_rays, 1), 6.0)], 1)
    z = 2 + 4 * torch.rand(n_rays, spr, generator=g)
    gout = torch.randn(n_rays * spr, 4, generator=g)
    gout *= torch.exp2(-20 * torch.rand(n_rays, 1, generator=g)).repeat_interleave(spr, 0)
    xyz = (rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)     # fp32, as the kernels
    d = rays[:, 3:6]
    x32 = torch.cat([O.embed(xyz, 10), O.embed(d, 4).repeat_interleave(spr, 0)], 1)
    x64 = torch.cat([O.embed(xyz.double(), 10), O.embed(d.double(), 4).repeat_interleave(spr, 0)], 1)
    return dict(rays=rays, z=z, gout=gout, x32=x32, x64=x64, n=n_rays * spr, spr=spr)


def to64(p):
    return {k: v.double() for k, v in p.items()}


def layers64(p64, x64, grad=False):
    """float64 forward keeping every ReLU layer's input, pre-activation and
    name: (out, [(name, input, pre)], feat)"""
    xe, de = x64[:, :XYZ_CH], x64[:, XYZ_CH:]
    h, recs = xe, []
    for i in range(1, 9):
        if i == 5:
            h = torch.cat([xe, h], -1)
        pre = torch.nn.functional.linear(h, p64[_hid(i) + ".weight"], p64[_hid(i) + ".bias"])
        if grad:
            pre.retain_grad()
        recs.append((f"h{i}", h, pre))
        h = torch.relu(pre)
    sigma = torch.nn.functional.linear(h, p64["sigma.weight"], p64["sigma.bias"])
    feat = torch.nn.functional.linear(h, p64["xyz_encoding_final.weight"], p64["xyz_encoding_final.bias"])
    hin = torch.cat([feat, de], -1)
    pre = torch.nn.functional.linear(hin, p64["dir_encoding.0.weight"], p64["dir_encoding.0.bias"])
    if grad:
        pre.retain_grad()
    recs.append(("hdir", hin, pre))
    rgb = torch.sigmoid(torch.nn.functional.linear(torch.relu(pre), p64["rgb.0.weight"], p64["rgb.0.bias"]))
    return torch.cat([rgb, sigma], -1), recs, feat


def _band(p64, name, hin, pre, band):
    """per sample: some unit of the layer within ``band`` of its magnitude sum"""
    key = (_hid(int(name[1:])) if name != "hdir" else "dir_encoding.0")
    mag = hin.abs() @ p64[key + ".weight"].abs().T + p64[key + ".bias"].abs()
    return pre.abs() <= band * mag


def certificate(params, x):
    """float64: max |w|; max activation per layer (h1 .. h8, feat, hdir) and
    sigma; max over inputs of sum_out |W| for every transposed layer the data
    gradient streams (the h-columns of hidden layers 2-8, xyz_encoding_final,
    dir_encoding.0[:, :256]); the kink band (bool per sample)."""
    p64 = to64(params)
    with torch.no_grad():
        out, recs, feat = layers64(p64, x.double())
        acts = {name: torch.relu(pre).max().item() for name, _, pre in recs}
        acts["feat"] = feat.abs().max().item()
        kink = torch.zeros(x.shape[0], dtype=torch.bool)
        for name, hin, pre in recs:
            kink |= _band(p64, name, hin, pre, KINK_BAND).any(1)
        growth = {_hid(i): p64[_hid(i) + ".weight"][:, _hcols(i)].abs().sum(0).max().item()
                  for i in range(2, 9)}
        growth["xyz_encoding_final"] = p64["xyz_encoding_final.weight"].abs().sum(0).max().item()
        growth["dir_encoding.0"] = p64["dir_encoding.0.weight"][:, :W].abs().sum(0).max().item()
    return dict(max_w=max(v.abs().max().item() for k, v in p64.items() if k.endswith("weight")),
                acts=acts, max_act=max(acts.values()), sigma=out[:, 3].abs().max().item(),
                growth=growth, max_growth=max(growth.values()), kink=kink)


def clauses(cert):
    """which clauses of the contract a certificate breaks"""
    return {"w": not cert["max_w"] < W_CAP, "act": not cert["max_act"] < ACT_CAP,
            "growth": not cert["max_growth"] < GROWTH_CAP}


def repr_h3(w):
    """(f16(256 w) + f16(256 w - f16(256 w))) / 256 in float64: the weight the
    f16x3 kernels multiply by (x3.h split2h on the fp32 product 256 w, which
    is exact; the residual 256 w - hi is exact in fp32 too)"""
    w = torch.as_tensor(w, dtype=torch.float32)
    s = w * 256.0
    hi = s.to(torch.float16).float()
    lo = (s - hi).to(torch.float16).float()
    return (hi.double() + lo.double()) / 256.0


def params64(params, math):
    """the float64 parameters a leg's reference is evaluated at: f16x3 at
    repr_h3 of the matrix-core weights, fp32 and bf16x6 at the weights as
    they are"""
    p64 = to64(params)
    if math == "f16x3":
        for k in SPLIT_WEIGHTS:
            p64[k] = repr_h3(params[k])
    return p64


def evaluate(p, x, gout, dt, sigma_only=False, keep=False):
    """output and every parameter gradient of sum(out * gout) in dtype dt
    (torch CPU autograd of the oracle MLP); with keep also the float64
    records of layers64 (inputs, pre-activations and their gradients)"""
    pr = {k: v.detach().to(dt).clone().requires_grad_(True) for k, v in p.items()}
    x = x.to(dt)
    if keep:
        out, recs, _ = layers64(pr, x, grad=True)
    else:
        out, recs = O.nerf_forward(pr, x), None
    g = gout.to(dt)
    ((out[:, 3:] * g[:, 3:]).sum() if sigma_only else (out * g).sum()).backward()
    grads = {k: v.grad.detach() for k, v in pr.items()
             if v.grad is not None and not (sigma_only and k in SIGMA_ONLY_UNUSED)}
    return out.detach(), grads, recs


def floors(params, x32, x64, gout, points=FLOOR_POINTS, sigma_only=False, entry=None):
    """the CPU fp32 oracle's distance from float64 over the floor points
    (grad64.fp32_floor): per tensor normwise, and per output column.  Every
    point compares the fp32 evaluation with the float64 evaluation at the
    same (perturbed) weights.  ``entry`` (optional dict) receives, per tensor,
    the entrywise max over the points of |g32 - g64|."""
    g32s, g64s = [], []
    fo = np.zeros(4)
    for seed in points:
        p32 = params if seed is None else ulp_perturbed(params, seed, torch.float32)
        p64 = to64(params) if seed is None else ulp_perturbed(params, seed, torch.float64)
        o32, g32, _ = evaluate(p32, x32, gout, torch.float32, sigma_only)
        o64, g64, _ = evaluate(p64, x64, gout, torch.float64, sigma_only)
        g32s.append(g32)
        g64s.append(g64)
        d = (o32.double() - o64).norm(dim=0) / o64.norm(dim=0)
        fo = np.maximum(fo, d.numpy())
        if entry is not None:
            for k in g64:
                e = (g32[k].double() - g64[k]).abs()
                entry[k] = torch.maximum(entry[k], e) if k in entry else e
    return fp32_floor(g32s, g64s), fo


def bound(floor):
    return C * max(floor, ULP32)


def deviations(ours, g64, floor):
    """[(deviation / bound, name, deviation, bound)] per tensor, worst first"""
    rows = []
    for k, e64 in g64.items():
        got = ours[k].double()
        dev = ((got - e64).norm() / e64.norm()).item()
        rows.append((dev / bound(floor[k]), k, dev, bound(floor[k])))
    rows.sort(key=lambda r: -r[0] if r[0] == r[0] else -math.inf)
    return rows


def flips(masks, p64, x64, screened):
    """(unexplained, dropped): ``masks`` maps h1 .. h8 / hdir to the bool mask
    (n, width) the kernels' forward chose; on unscreened samples it must equal
    the float64 mask.  A sample that differs is dropped (bool per sample) when
    every differing unit's float64 pre-activation lies within FLIP_BAND of its
    magnitude sum, and unexplained otherwise."""
    n = x64.shape[0]
    bad = torch.zeros(n, dtype=torch.bool)
    drop = torch.zeros(n, dtype=torch.bool)
    with torch.no_grad():
        _, recs, _ = layers64(p64, x64)
        for name, hin, pre in recs:
            if name not in masks:
                continue
            f = (masks[name] != (pre > 0)) & ~screened[:, None]
            near = _band(p64, name, hin, pre, FLIP_BAND)
            bad |= (f & ~near).any(1)
            drop |= f.any(1)
    return bad, drop & ~bad
