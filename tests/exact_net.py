"""Integer-valued NeRF networks on which the fused MLP kernels must be exact
(test infrastructure, no GPU use; DESIGN.md 3 "Exactness contract").

The split arithmetics are exact operations plus a bounded truncation: every
range scaling is a power of two (x3.h, mlp_bwd3.hip gscale_from,
wgrad_common.h task_scale), f16x3 keeps hi*hi + hi*lo + lo*hi of an 11+11-bit
split, bf16x6 the six products of piece-index sum <= 2 of an 8+8+8-bit split,
and fp32 MFMA products are exact.  On operands that are small dyadic numbers
every product is therefore exact and every fp32 partial sum is a multiple of
one quantum below 2^24 quanta, so the result does not depend on the summation
order: the float64 evaluation below IS the answer, and the GPU tests compare
with ``==``.

This module builds such networks (``build_net``), inputs (``embedded_input``,
``ray_input``) and output gradients (``make_gout``), evaluates forward and
backward in float64 (``reference``: every value is a dyadic number far inside
float64's 53 bits, so float64 is exact integer arithmetic in quanta), and
states when an input is admissible for an arithmetic (``certify``).
"""
from __future__ import annotations

import numpy as np
import torch

from nerf_pl_amd import packing

W, WD, XYZ_CH, DIR_CH = packing.W, packing.WD, packing.XYZ_CH, packing.DIR_CH
F64 = torch.float64
LAYER = [f"xyz_encoding_{i}.0" for i in range(1, 9)]
ARITHS = ("fp32", "bf16x6", "f16x3", "bf16")
# parameters a sigma-only graph does not reach
SIGMA_ONLY_UNUSED = ("xyz_encoding_final.weight", "xyz_encoding_final.bias",
                     "dir_encoding.0.weight", "dir_encoding.0.bias",
                     "rgb.0.weight", "rgb.0.bias")
ZERO_KINDS = ("dense", "scattered", "blocks", "runs", "one", "none")


# -- networks ------------------------------------------------------------------
def _allowed(fan, trig):
    """input columns a sparse row may read: with ``trig`` false only the raw
    coordinates of an embedding (its first three channels) and the hidden
    units -- every weight that multiplies a sin / cos channel stays zero"""
    if trig:
        return np.arange(fan)
    if fan == XYZ_CH:
        return np.arange(3)
    if fan == W + XYZ_CH:
        return np.concatenate([np.arange(3), np.arange(XYZ_CH, fan)])
    if fan == W + DIR_CH:
        return np.concatenate([np.arange(W), np.arange(W, W + 3)])
    return np.arange(fan)


WIDE_BITS, WIDE_SHIFT = (11, 12), 11


def _values(g, k, two, wide=False):
    v = g.choice([-1.0, 1.0], size=k)
    if wide:      # +-m 2^-11, m odd with 12 significant bits: 1 <= |w| < 2, a nonzero lo piece
        m = g.integers(2 ** WIDE_BITS[0], 2 ** WIDE_BITS[1], size=k) | 1
        return v * m.astype(np.float64) * 2.0 ** -WIDE_SHIFT
    if two:
        v = v * g.choice([1.0, 2.0], size=k)
    return v


def _bias(g, rows, bmax):
    return torch.from_numpy(g.integers(-bmax, bmax + 1, size=rows).astype(np.float64))


def build_net(kind="general", seed=0, k=3, two=False, trig=True, bmax=1, rgb_nnz=8,
              wide=None):
    """{name: float64 tensor} in packing.param_shapes() order.

    Every weight row has ``k`` nonzero entries from {-1, +1} (``two``: from
    {+-1, +-2}); biases are integers in [-bmax, bmax].

    "general": independent sparse rows in every layer, a dense +-1 sigma
    head (d h8 is dense), a sparse rgb head of ``rgb_nnz`` entries per row.

    "twin": every hidden layer (1-8, final, dir) is split by a random
    permutation into unit sets A and B of equal size; B's rows copy A's rows,
    reading B's units of the previous layer where A reads A's (the PE / dir
    channels and the layer-5 skip are shared, cross weights are zero), so a
    twin pair has equal activations.  The sigma head reads both halves with
    independent +-1 weights; rgb.0.weight[c, a] = s and [c, twin(a)] = -s with
    a zero bias, so every rgb pre-activation is exactly 0, rgb = 0.5, and the
    sigmoid's backward is g / 4.  The rgb gradient flows down A and B with
    opposite signs and never cancels (the halves share no hidden unit).

    ``trig`` false (the ray input): every weight column that multiplies a
    sin / cos channel is zero.  ``wide`` (a layer name such as
    "xyz_encoding_8.0"): the "wide weights" family -- that layer's nonzero
    weights are +-m 2^-11, m odd, with 12 significant bits."""
    g = np.random.Generator(np.random.PCG64(seed))
    shapes = packing.param_shapes()
    p = {}
    twin = kind == "twin"
    if kind not in ("general", "twin"):
        raise ValueError(kind)
    prev = None                 # (A, B) unit sets of the previous hidden layer
    hidden = LAYER + ["xyz_encoding_final", "dir_encoding.0"]
    for name in hidden:
        rows, fan = shapes[name + ".weight"]
        w = np.zeros((rows, fan))
        # columns that hold the previous layer's hidden units start at h0
        h0 = {XYZ_CH: None, W: 0, W + XYZ_CH: XYZ_CH, W + DIR_CH: 0}[fan]
        ok = _allowed(fan, trig)
        if not twin:
            for r in range(rows):
                kk = min(k, len(ok))
                w[r, g.choice(ok, size=kk, replace=False)] = _values(g, kk, two, name == wide)
            b = _bias(g, rows, bmax)
        else:
            perm = g.permutation(rows)
            A, B = perm[:rows // 2], perm[rows // 2:]
            hid = np.zeros(fan, dtype=bool)
            if h0 is not None:
                hid[h0:h0 + W] = True
            shared = ok[~hid[ok]]
            # an A row reads shared inputs and the previous layer's A units
            pool = shared if prev is None else np.concatenate([shared, h0 + prev[0]])
            tw = None if prev is None else dict(zip((h0 + prev[0]).tolist(),
                                                    (h0 + prev[1]).tolist()))
            ba = g.integers(-bmax, bmax + 1, size=rows // 2).astype(np.float64)
            b = np.zeros(rows)
            for a_, b_, bb in zip(A, B, ba):
                kk = min(k, len(pool))
                cols = g.choice(pool, size=kk, replace=False)
                vals = _values(g, kk, two, name == wide)
                w[a_, cols] = vals
                w[b_, [c if (tw is None or c not in tw) else tw[c] for c in cols.tolist()]] = vals
                b[a_] = b[b_] = bb
            b = torch.from_numpy(b)
            prev = (A, B)
        p[name + ".weight"] = torch.from_numpy(w)
        p[name + ".bias"] = b
        if name == "xyz_encoding_8.0":
            p["sigma.weight"] = torch.from_numpy(g.choice([-1.0, 1.0], size=(1, W)))
            p["sigma.bias"] = _bias(g, 1, bmax)
            # xyz_encoding_final reads h8: prev stays (A, B) of layer 8
    wr = np.zeros((3, WD))
    if twin:
        A, B = prev
        for c in range(3):
            pick = g.choice(len(A), size=min(rgb_nnz, len(A)), replace=False)
            s = g.choice([-1.0, 1.0], size=len(pick))
            wr[c, A[pick]] = s
            wr[c, B[pick]] = -s
        br = torch.zeros(3, dtype=F64)
    else:
        for c in range(3):
            wr[c, g.choice(WD, size=rgb_nnz, replace=False)] = _values(g, rgb_nnz, two)
        br = _bias(g, 3, bmax)
    p["rgb.0.weight"] = torch.from_numpy(wr)
    p["rgb.0.bias"] = br
    return {k_: p[k_].to(F64).reshape(shapes[k_]) for k_ in shapes}


# -- inputs --------------------------------------------------------------------
def embedded_input(n, q=0, seed=0):
    """x (n, 90) float64 with entries k 2^-q, |x| <= 1 (q = 0: -1, 0, 1)"""
    g = np.random.Generator(np.random.PCG64(seed))
    s = 2 ** q
    return torch.from_numpy(g.integers(-s, s + 1, size=(n, XYZ_CH + DIR_CH)).astype(np.float64) / s)


def ray_input(n_rays, spr, qz=0, seed=0):
    """(rays (n_rays, 8), z (n_rays, spr), x (n, 90)) float64: integer origins
    and directions, depths k 2^-qz in [0, 3), so xyz = o + d z is exact in
    fp32; x is the embedding of those positions and directions in float64
    (only its raw-xyz and raw-direction channels are exact; the networks used
    with it have zero weights on every sin / cos channel)"""
    g = np.random.Generator(np.random.PCG64(seed))
    o = g.integers(-1, 2, size=(n_rays, 3)).astype(np.float64)
    d = g.integers(-1, 2, size=(n_rays, 3)).astype(np.float64)
    s = 2 ** qz
    z = np.sort(g.integers(0, 3 * s, size=(n_rays, spr)).astype(np.float64) / s, axis=1)
    rays = torch.from_numpy(np.concatenate([o, d, np.zeros((n_rays, 1)),
                                            np.full((n_rays, 1), 3.0)], 1))
    z = torch.from_numpy(z)
    xyz = (rays[:, None, :3] + rays[:, None, 3:6] * z[..., None]).reshape(-1, 3)
    x = torch.cat([embed64(xyz, 10), embed64(rays[:, 3:6], 4).repeat_interleave(spr, 0)], 1)
    return rays, z, x


def embed64(x, n_freqs):
    """the positional encoding (oracle.nerf_oracle.embed) in float64"""
    parts = [x]
    for f in range(n_freqs):
        parts += [torch.sin(2.0 ** f * x), torch.cos(2.0 ** f * x)]
    return torch.cat(parts, -1)


def raw_only(x):
    """x with every sin / cos channel zeroed: what the certificate (and the
    exact part of the reference) sees of a ray input, whose trig channels meet
    zero weights only"""
    x = x.clone()
    x[:, 3:XYZ_CH] = 0
    x[:, XYZ_CH + 3:] = 0
    return x


def trig_columns(name):
    """columns of a first-layer / skip / dir weight that multiply a sin / cos
    channel (inexact gradients in the ray input), as a bool mask, or None"""
    fan = packing.param_shapes()[name][-1] if name.endswith(".weight") else None
    m = None
    if name in ("xyz_encoding_1.0.weight", "xyz_encoding_5.0.weight"):
        m = np.zeros(fan, dtype=bool)
        m[3:XYZ_CH] = True
    elif name == "dir_encoding.0.weight":
        m = np.zeros(fan, dtype=bool)
        m[W + 3:] = True
    return m


def make_gout(n, kind="dense", mode="mixed", q=0, gmax=2, seed=0):
    """(n, 4) float64 output gradient with entries k 2^-q, |k| <= gmax; the rgb
    columns are multiples of 4 quanta (the sigmoid's backward at rgb = 0.5 is
    g / 4).  ``mode``: "mixed", "rgb" (zero sigma column), "sigma" (zero rgb
    columns).  ``kind`` zeroes rows like test_gpu_active._zeroed: "dense",
    "scattered", "blocks", "runs", "one" (a sample of the partial last
    block), "none"."""
    g = np.random.Generator(np.random.PCG64(seed))
    x = g.integers(-gmax, gmax + 1, size=(n, 4)).astype(np.float64)
    x[:, :3] *= 4
    if mode == "rgb":
        x[:, 3] = 0
    elif mode == "sigma":
        x[:, :3] = 0
    elif mode != "mixed":
        raise ValueError(mode)
    idx = np.arange(n)
    if kind == "scattered":
        x[g.random(n) < 0.5] = 0
    elif kind == "blocks":
        x[(idx // 32) % 7 != 3] = 0
        if n <= 3 * 32:             # too few blocks for the pattern: keep block 0
            x[:] = 0
            x[:min(n, 32)] = make_gout(min(n, 32), "dense", mode, 0, gmax, seed + 1).numpy()
    elif kind == "runs":
        x[(idx % 64 < 20) | (idx % 64 > 40) | (g.random(n) < 0.3)] = 0
    elif kind == "one":
        keep = n - 1 - ((n - 1) % 32) // 2      # inside the last (partial) block
        row = x[keep].copy()
        if not row.any():
            row = np.array([4.0, -4.0, 4.0, 1.0]) * (x[0] * 0 + 1)
            if mode == "rgb":
                row[3] = 0
            elif mode == "sigma":
                row[:3] = 0
        x[:] = 0
        x[keep] = row
    elif kind == "none":
        x[:] = 0
    elif kind != "dense":
        raise ValueError(kind)
    return torch.from_numpy(x * 2.0 ** -q)


# -- exact reference -----------------------------------------------------------
def reference(p, x, g_out=None, sigma_only=False):
    """Forward and (with ``g_out`` (n, 4), or (n, 1) for sigma_only) full
    backward of nerf.py:83-124 in float64.  Returns a dict: ``acts`` (h1..h8,
    feat, hdir), ``pre_rgb``, ``out`` ((n, 4) [rgb, sigma] or (n, 1)), ``dz``
    (the gradient at every layer's pre-activation: h1..h8, feat, hdir, rgb,
    sigma) and ``grads`` (24 parameter gradients; 18 for sigma_only).  A
    pre-activation of exactly 0 is "off"."""
    lin = torch.nn.functional.linear
    xe, xd = x[:, :XYZ_CH], x[:, XYZ_CH:]
    acts, ins = {}, {}
    h = xe
    for i, name in enumerate(LAYER):
        if i == 4:
            h = torch.cat([xe, h], -1)
        ins[name] = h
        h = torch.relu(lin(h, p[name + ".weight"], p[name + ".bias"]))
        acts[f"h{i + 1}"] = h
    h8 = h
    sigma = lin(h8, p["sigma.weight"], p["sigma.bias"])
    res = {"acts": acts, "ins": ins}
    if sigma_only:
        res["out"] = sigma
    else:
        feat = lin(h8, p["xyz_encoding_final.weight"], p["xyz_encoding_final.bias"])
        ins["dir_encoding.0"] = torch.cat([feat, xd], -1)
        hdir = torch.relu(lin(ins["dir_encoding.0"], p["dir_encoding.0.weight"],
                              p["dir_encoding.0.bias"]))
        pre_rgb = lin(hdir, p["rgb.0.weight"], p["rgb.0.bias"])
        rgb = torch.sigmoid(pre_rgb)
        acts["feat"], acts["hdir"] = feat, hdir
        res["pre_rgb"] = pre_rgb
        res["out"] = torch.cat([rgb, sigma], -1)
    if g_out is None:
        return res
    dz, gr = {}, {}
    dsig = g_out[:, -1:]
    dz["sigma"] = dsig
    gr["sigma.weight"] = dsig.T @ h8
    gr["sigma.bias"] = dsig.sum(0)
    dh = dsig @ p["sigma.weight"]
    if not sigma_only:
        dz["rgb"] = g_out[:, :3] * (1 - rgb) * rgb
        gr["rgb.0.weight"] = dz["rgb"].T @ hdir
        gr["rgb.0.bias"] = dz["rgb"].sum(0)
        dz["hdir"] = (dz["rgb"] @ p["rgb.0.weight"]) * (hdir > 0)
        gr["dir_encoding.0.weight"] = dz["hdir"].T @ ins["dir_encoding.0"]
        gr["dir_encoding.0.bias"] = dz["hdir"].sum(0)
        dz["feat"] = (dz["hdir"] @ p["dir_encoding.0.weight"])[:, :W]
        gr["xyz_encoding_final.weight"] = dz["feat"].T @ h8
        gr["xyz_encoding_final.bias"] = dz["feat"].sum(0)
        dh = dh + dz["feat"] @ p["xyz_encoding_final.weight"]
    for i in range(7, -1, -1):
        name = LAYER[i]
        d = dh * (acts[f"h{i + 1}"] > 0)
        dz[f"h{i + 1}"] = d
        gr[name + ".weight"] = d.T @ ins[name]
        gr[name + ".bias"] = d.sum(0)
        if i:
            dh = d @ p[name + ".weight"]
            if i == 4:
                dh = dh[:, XYZ_CH:]
    res["dz"] = dz
    res["grads"] = {k: gr[k].reshape(p[k].shape) for k in p if k in gr}
    return res


# -- certificate ---------------------------------------------------------------
def _t(v):
    return v.detach() if isinstance(v, torch.Tensor) else torch.as_tensor(np.asarray(v), dtype=F64)


def _bits(v):
    """(width, lowest set bit) over a float64 array: width = significant bits
    of the widest entry with trailing zeros removed (an odd integer m 2^e has
    width bit_length(m); 0 for an all-zero array); lowest set bit = the
    smallest value of any entry's last set bit (inf for an all-zero array)"""
    v = _t(v).reshape(-1)
    v = v[v != 0]
    if v.numel() == 0:
        return 0, float("inf")
    m, e = torch.frexp(v)
    mi = (m.abs() * 2.0 ** 53).to(torch.int64)
    tz = torch.log2((mi & -mi).to(F64)).to(torch.int64)      # trailing zeros of the 53-bit mantissa
    return int(53 - tz.min()), float(2.0 ** float((e.to(torch.int64) - 53 + tz).min()))


def width(v):
    return _bits(v)[0]


def lowbit(v):
    return _bits(v)[1]


def _width_ok(arith, wa, wb):
    if arith == "fp32":
        return True
    if arith == "f16x3":
        return wa <= 22 and wb <= 22 and min(wa, wb) <= 11
    if arith == "bf16x6":
        return (wa <= 8 and wb <= 24) or (wa <= 16 and wb <= 16) or (wa <= 24 and wb <= 8)
    if arith == "bf16":
        return wa <= 8 and wb <= 8
    raise ValueError(arith)


class Certificate:
    """``failures``: the violated conditions (empty: the input is admissible);
    ``stats``: per GEMM (width a, width b, log2 of the largest sum of |term|
    in quanta), and ``stats["worst"]``"""

    def __init__(self):
        self.failures, self.stats = [], {}

    @property
    def ok(self):
        return not self.failures

    def __bool__(self):
        return self.ok

    def __repr__(self):
        return f"Certificate(ok={self.ok}, failures={self.failures[:6]})"


def _profile(p, x, g_out, sigma_only, ref):
    """the arithmetic-independent facts of certify(): per GEMM the operand
    widths and the largest sum of |term| in quanta, the ranges, and the f16x3
    scaled lowest bits -- computed once per reference"""
    gemms, ranges, f16 = [], [], []
    bits = {}

    def B(v):      # operands recur (an activation feeds forward and weight gradient)
        key = (v.data_ptr(), tuple(v.shape), tuple(v.stride()))
        if key not in bits:
            bits[key] = (_bits(v), v)
        return bits[key][0]

    def gemm(label, a, b, bias=None, split=True):
        """every dot product of a (m, k) with b (k, n) [+ bias]"""
        a, b = _t(a), _t(b)
        (wa, la), (wb, lb) = B(a), B(b)
        if wa == 0 or wb == 0:
            gemms.append((label, wa, wb, 0.0, split))
            return
        quantum = la * lb
        s = a.abs() @ b.abs()
        if bias is not None and bool(_t(bias).any()):
            bb = _t(bias).abs()
            quantum = min(quantum, _bits(bb)[1])
            s = s + (bb[:, None] if bb.ndim == 1 else bb)
        gemms.append((label, wa, wb, float(s.max()) / quantum, split))

    acts, ins = ref["acts"], ref["ins"]
    hid = list(LAYER) if sigma_only else LAYER + ["xyz_encoding_final", "dir_encoding.0"]
    for name in hid + ["sigma"] + ([] if sigma_only else ["rgb.0"]):
        wmax = float(p[name + ".weight"].abs().max())
        if not wmax < 255:
            ranges.append(f"{name}: |w| reaches {wmax} (limit 255)")
    for k, v in list(acts.items()) + [("x", x)]:
        amax = float(v.abs().max())
        if not amax < 65504:
            ranges.append(f"{k}: activation reaches {amax} (limit 65504)")
    # forward: D[feature][sample] = W X + b
    for name in hid:
        src = acts["h8"] if name == "xyz_encoding_final" else ins[name]
        gemm(f"fwd {name}", p[name + ".weight"], src.T, p[name + ".bias"])
        f16.append((f"fwd {name}: scaled weight", B(p[name + ".weight"])[1] * 2.0 ** 8))
        f16.append((f"fwd {name}: activation", B(src.T)[1]))
    gemm("fwd sigma", p["sigma.weight"], acts["h8"].T, p["sigma.bias"], split=False)
    if not sigma_only:
        gemm("fwd rgb", p["rgb.0.weight"], acts["hdir"].T, p["rgb.0.bias"], split=False)
    if g_out is None:
        return gemms, ranges, f16
    dz = ref["dz"]
    # the largest gradient a sample carries anywhere in the chain bounds the
    # producer maximum its per-sample scale is renormalised from
    per_sample = torch.stack([v.abs().amax(1) for v in dz.values()]).amax(0)

    def dgrad_bits(label, d):
        """f16x3: B values = sigma * dz with the producer's max near 2^kGT = 2^6
        (mlp_bwd3.hip gscale_from); the weight gradient scales the segment's
        max into [2^14, 2^15) (wgrad_common.h task_scale)"""
        if not bool(d.any()):
            return
        rows = d.abs().amax(1) > 0
        lb = _bits(d)[1]
        ps = per_sample[rows].max()
        f16.append((f"{label}: per-sample-scaled gradient",
                    lb * 2.0 ** 6 / 2.0 ** (float(torch.floor(torch.log2(ps))) + 1)))
        f16.append((f"{label}: task-scaled gradient",
                    lb * 2.0 ** 14 / 2.0 ** float(torch.floor(torch.log2(d.abs().max())))))

    def growth(name, w):
        gmax = float(w.abs().sum(0).max())
        if not gmax < 2.0 ** 9:
            ranges.append(f"dgrad {name}: max-norm growth of W^T is {gmax} (limit 2^9)")

    # data gradient: d in[feature][sample] = W^T dz (+ the sigma head's injection)
    if not sigma_only:
        gemm("dgrad rgb", p["rgb.0.weight"].T, dz["rgb"].T, split=False)
        wd = p["dir_encoding.0.weight"][:, :W]
        gemm("dgrad dir", wd.T, dz["hdir"].T)
        growth("dir_encoding.0", wd)
        inj = p["sigma.weight"].abs().T @ dz["sigma"].abs().T
        gemm("dgrad final", p["xyz_encoding_final.weight"].T, dz["feat"].T, inj)
        growth("xyz_encoding_final", p["xyz_encoding_final.weight"])
        dgrad_bits("hdir", dz["hdir"])
        dgrad_bits("feat", dz["feat"])
    for i in range(7, 0, -1):
        w = p[LAYER[i] + ".weight"]
        w = w[:, XYZ_CH:] if i == 4 else w
        gemm(f"dgrad {LAYER[i]}", w.T, dz[f"h{i + 1}"].T)
        growth(LAYER[i], w)
    for i in range(8):
        dgrad_bits(f"h{i + 1}", dz[f"h{i + 1}"])
    # weight gradient: dW = sum over samples dz^T in; db = sum dz
    ones = torch.ones(x.shape[0], 1, dtype=F64)
    for i, name in enumerate(LAYER):
        gemm(f"wgrad {name}", dz[f"h{i + 1}"].T, ins[name])
        gemm(f"bgrad {name}", dz[f"h{i + 1}"].T, ones, split=False)
    gemm("wgrad sigma", dz["sigma"].T, acts["h8"])
    gemm("bgrad sigma", dz["sigma"].T, ones, split=False)
    if not sigma_only:
        gemm("wgrad rgb", dz["rgb"].T, acts["hdir"])
        gemm("bgrad rgb", dz["rgb"].T, ones, split=False)
        # dir_encoding: G = sum dz_dir h8^T and the dir-PE columns by the GEMM;
        # nr_wgrad_dir_feat: dW_dir[:, :256] = G W_final^T + db_dir b_final^T,
        # dW_final = W_dir[:, :256]^T G, db_final = W_dir[:, :256]^T db_dir (fp32 fma)
        gemm("wgrad dir G", dz["hdir"].T, acts["h8"])
        gemm("wgrad dir pe", dz["hdir"].T, x[:, XYZ_CH:])
        gemm("bgrad dir", dz["hdir"].T, ones, split=False)
        G = dz["hdir"].T @ acts["h8"]
        db = dz["hdir"].sum(0)
        wf, bf = p["xyz_encoding_final.weight"], p["xyz_encoding_final.bias"]
        gemm("dir_feat G W_final^T", G, wf.T, db.abs()[:, None] * bf.abs()[None, :], split=False)
        gemm("dir_feat W_dir^T G", wd.T, G, split=False)
        gemm("dir_feat W_dir^T db", wd.T, db[:, None], split=False)
    return gemms, ranges, f16


def certify(arith, p, x, g_out=None, sigma_only=False, ref=None):
    """The conditions under which the ``arith`` kernels are exact on network
    ``p``, input ``x`` (n, 90) and output gradient ``g_out``, evaluated on the
    float64 reference alone (``ref``: a precomputed reference(...) of the same
    arguments; the arithmetic-independent part is cached in it).

    For every GEMM of the forward, the data gradient, the weight gradient and
    nr_wgrad_dir_feat, with operands a and b (width = significant bits with
    trailing zeros removed):
      f16x3   both <= 22 and min(width a, width b) <= 11   (lo*lo is dropped)
      bf16x6  (wa, wb) within (8, 24), (16, 16) or (24, 8) (piece-index sum <= 2)
      bf16    both <= 8
      fp32    none
    and for every arithmetic and every dot product the sum of |term| over all
    n samples or all k (plus |bias|) is < 2^24 quanta (quantum = product of
    the operands' lowest set bits): sufficient for any summation order.
    Ranges: |w| < 255 (packed f16x3 weights carry 2^8 in fp16, x3.h kWScale),
    activations < 65504 (x3.h), max-norm growth of every W^T < 2^9
    (mlp_bwd3.hip kGT headroom), and the lowest set bit of every f16x3
    operand after its documented scale >= 2^-24 (fp16 subnormal spacing).
    The fp32 VALU heads and nr_wgrad_dir_feat carry the sum condition only."""
    if arith not in ARITHS:
        raise ValueError(arith)
    if ref is None:
        ref = reference(p, x, g_out, sigma_only)
    if "_profile" not in ref:
        ref["_profile"] = _profile(p, x, g_out, sigma_only, ref)
    gemms, ranges, f16 = ref["_profile"]
    c = Certificate()
    c.failures.extend(ranges)
    worst = {"sum_log2": 0.0, "wa": 0, "wb": 0}
    for label, wa, wb, tot, split in gemms:
        if split and not _width_ok(arith, wa, wb):
            c.failures.append(f"{label}: operand widths ({wa}, {wb}) outside the {arith} rule")
        if not tot < 2.0 ** 24:
            c.failures.append(f"{label}: sum of |term| reaches 2^{np.log2(tot):.1f} quanta "
                              "(limit 2^24)")
        lg = float(np.log2(tot)) if tot > 0 else 0.0
        c.stats[label] = (wa, wb, lg)
        worst["sum_log2"] = max(worst["sum_log2"], lg)
        if split:
            worst["wa"], worst["wb"] = max(worst["wa"], wa), max(worst["wb"], wb)
    if arith == "f16x3":
        for label, low in f16:
            if low < 2.0 ** -24:
                c.failures.append(f"{label}: lowest set bit 2^{np.log2(low):.0f} after its "
                                  "scale (limit 2^-24)")
    c.stats["worst"] = worst
    return c


# -- the cases the tests use ------------------------------------------------------
# sample counts: the smallest that cross a 32-sample block, a 128-sample
# workgroup, the padded block count, and several workgroups per weight-gradient
# task; as rays (n_rays, samples per ray).  The two large sizes are those of
# test_gpu_render.py::test_mlp_backward_matches_autograd.
SIZES = {1: (1, 1), 31: (1, 31), 32: (1, 32), 33: (1, 33), 127: (1, 127), 128: (2, 64),
         129: (3, 43), 851: (23, 37), 31049: (509, 61)}
SPLIT3 = ("fp32", "bf16x6", "f16x3")
# family -> (arithmetics, sizes).  "int": q = 0, every arithmetic (bf16 with
# |g| <= 1); "frac": inputs and output gradients k 2^-q, q per size so that
# the certificate holds (activations reach 12-14 bits: nonzero lo pieces);
# "wide8" / "wide5" / "widedir": one layer's weights 12 bits wide
FAMILIES = {
    "int": (ARITHS, tuple(SIZES)),
    "frac": (SPLIT3, (33, 127, 129, 851)),
    "wide8": (SPLIT3, (33, 129)),
    "wide5": (SPLIT3, (33, 129)),
    "widedir": (SPLIT3, (33, 129)),
}
FRAC_Q = {33: 8, 127: 8, 129: 8, 851: 7}
_WIDE = {"wide8": "xyz_encoding_8.0", "wide5": "xyz_encoding_5.0", "widedir": "dir_encoding.0"}
_CACHE = {}


def net(kind, trig=True, wide=None):
    """the (cached) network of a construction; twins get a dense rgb head (64
    pairs per channel) so that every tensor's gradient is well populated"""
    key = ("net", kind, trig, wide)
    if key not in _CACHE:
        _CACHE[key] = build_net(kind, seed=3, trig=trig, wide=wide,
                                rgb_nnz=64 if kind == "twin" else 8)
    return _CACHE[key]


def case(family, n, kind="twin", inp="emb", mode="mixed", zero="dense", sigma_only=False,
         backward=True):
    """One cached test case: dict with ``p``, ``x`` (n, 90), for inp = "rays"
    also ``rays`` / ``z`` / ``spr``, ``g`` (the output gradient, (n, 4), or
    (n, 1) for sigma_only), ``ref`` (reference on x) and ``cert_ref`` (the
    reference the certificate reads: for rays, on raw_only(x))."""
    key = (family, n, kind, inp, mode, zero, sigma_only, backward)
    if key in _CACHE:
        return _CACHE[key]
    q = FRAC_Q[n] if family == "frac" else 0
    if family.startswith("wide") and zero == "dense" and n > 33:
        zero = "scattered"          # dense exceeds 2^24 quanta at n = 129 (certify)
    c = {"p": net(kind, trig=inp == "emb", wide=_WIDE.get(family)), "q": q}
    if inp == "emb":
        c["x"] = embedded_input(n, q, seed=1)
        xc = c["x"]
    else:
        nr, spr = SIZES[n]
        c["rays"], c["z"], c["x"] = ray_input(nr, spr, min(q, 2), seed=2)
        c["spr"] = spr
        xc = raw_only(c["x"])
    g = None
    if backward:
        g = make_gout(n, zero, "sigma" if sigma_only else mode, q=q, gmax=1, seed=1000 + n)
        if sigma_only:
            g = g[:, 3:].contiguous()
    c["g"] = g
    c["ref"] = reference(c["p"], c["x"], g, sigma_only)
    c["xc"] = xc
    c["cert_ref"] = c["ref"] if xc is c["x"] else reference(c["p"], xc, g, sigma_only)
    c["sigma_only"] = sigma_only
    if n > 1000:
        # a large case keeps what the comparisons read (activations in fp32:
        # exact, every value is below 24 bits; outputs; parameter gradients)
        # and the certificate's facts, not its ~1.5 GB of float64 intermediates
        c["cert_ref"]["_profile"] = _profile(c["p"], xc, g, sigma_only, c["cert_ref"])
        for r in (c["ref"], c["cert_ref"]):
            r.pop("ins", None)
            r.pop("dz", None)
            if r is not c["ref"]:
                r.pop("acts", None)
        c["ref"]["acts"] = {k: v.float() for k, v in c["ref"]["acts"].items()}
    _CACHE[key] = c
    return c


def certify_case(arith, c):
    return certify(arith, c["p"], c["xc"], c["g"], c["sigma_only"], ref=c["cert_ref"])


def _spec(arith, family, n, kind="twin", inp="emb", mode="mixed", zero="dense",
          sigma_only=False, path="every", w4=1, so_kernels=True):
    return dict(arith=arith, family=family, n=n, kind=kind, inp=inp, mode=mode, zero=zero,
                sigma_only=sigma_only, path=path, w4=w4, so_kernels=so_kernels)


def spec_id(s):
    t = [s["arith"], s["family"], str(s["n"]), s["kind"], s["inp"]]
    if "path" in s:
        t += [s["mode"], s["zero"], s["path"]]
        if s["sigma_only"]:
            t.append("so1" if s["so_kernels"] else "so0")
        if s["arith"] == "f16x3" and not s["w4"]:
            t.append("w4=0")
    return "-".join(t)


def spec_case(s):
    return case(s["family"], s["n"], s["kind"], s["inp"], s.get("mode", "mixed"),
                s.get("zero", "dense"), s.get("sigma_only", False))


# the combinations that run at n = 31,049 (integer family, twin, mixed, dense):
# (arithmetic, input, path, NR_WGRAD_W4)
LARGE = (("f16x3", "emb", "active", 1), ("fp32", "emb", "every", 1), ("bf16", "emb", "every", 1),
         ("f16x3", "rays", "every", 1), ("f16x3", "rays", "active", 0),
         ("bf16x6", "rays", "deferred", 1))
_PATHS = {"emb": ("every", "active"), "rays": ("every", "active", "deferred")}


def backward_specs():
    """every backward case of tests/test_gpu_exact.py (the CPU suite certifies
    each): arithmetic x family x size x construction x input x gradient
    columns x zero rows x path (every sample / active list / deferred save)"""
    out = []
    small = [n for n in SIZES if n < 1000]
    for inp, paths in _PATHS.items():
        # 1. every size: twin, mixed gradient, no zero rows
        for n in small:
            for a in SPLIT3:
                out += [_spec(a, "int", n, inp=inp, path=p) for p in paths]
            out.append(_spec("bf16", "int", n, inp=inp))
        # 2. the gradient's columns: general with g_rgb = 0 (exact zeros for
        #    final, dir, rgb), twin with rgb only and sigma only
        for n in (33, 851):
            for a in SPLIT3:
                for kind, mode in (("general", "sigma"), ("twin", "rgb"), ("twin", "sigma")):
                    out += [_spec(a, "int", n, kind=kind, inp=inp, mode=mode, path=p)
                            for p in paths[-2:]]
        # 3. zero rows of every kind through the list paths
        for a in SPLIT3:
            for zero in ZERO_KINDS[1:]:
                out += [_spec(a, "int", 851, inp=inp, zero=zero, path=p) for p in paths[1:]]
        # 6. fractional family (lo pieces of activations), 7. wide weights (lo
        #    pieces of weights, wide downstream activations / upstream dz)
        for a in SPLIT3:
            for n in FAMILIES["frac"][1]:
                out += [_spec(a, "frac", n, inp=inp, path=p) for p in paths[-2:]]
    for a in SPLIT3:
        for fam in _WIDE:
            for n in FAMILIES[fam][1]:
                out += [_spec(a, fam, n, path=p) for p in _PATHS["emb"]]
    # 4. sigma-only graphs (ray input only), on the sigma-only kernels and on
    #    the full kernels with a zero rgb gradient
    for a in SPLIT3:
        for so in (True, False):
            for n in (33, 129, 851):
                out += [_spec(a, "int", n, inp="rays", sigma_only=True, path=p, so_kernels=so)
                        for p in _PATHS["rays"]]
            for zero in ZERO_KINDS[1:]:
                out.append(_spec(a, "int", 851, inp="rays", zero=zero, sigma_only=True,
                                 path="deferred" if so else "active", so_kernels=so))
    out.append(_spec("bf16", "int", 851, inp="rays", sigma_only=True))
    # 5. f16x3: the register-staged weight gradient (NR_WGRAD_W4=0) beside the
    #    LDS-DMA one (the default above)
    for fam, n in (("int", 129), ("int", 851), ("frac", 851), ("frac", 129)):
        out += [_spec("f16x3", fam, n, inp="emb", path=p, w4=0) for p in _PATHS["emb"]]
        out += [_spec("f16x3", fam, n, inp="rays", path=p, w4=0) for p in _PATHS["rays"]]
    out += [_spec("f16x3", "int", 851, inp="rays", zero=z, path="active", w4=0)
            for z in ZERO_KINDS[1:]]
    out += [_spec("f16x3", fam, 129, path="active", w4=0) for fam in _WIDE]
    # 8. the large size
    out += [_spec(a, "int", 31049, inp=inp, path=p, w4=w) for a, inp, p, w in LARGE]
    return out


def forward_specs():
    """every forward case of tests/test_gpu_exact.py: (arith, family, n, kind, inp)"""
    out = []
    for a in ARITHS:
        for inp in _PATHS:
            out += [dict(arith=a, family="int", n=n, kind="twin", inp=inp) for n in SIZES
                    if n < 1000 or (a, inp) in [(x[0], x[1]) for x in LARGE]]
            out += [dict(arith=a, family="int", n=n, kind="general", inp=inp, mode="sigma")
                    for n in (33, 129, 851)]
    for a in SPLIT3:
        for inp in _PATHS:
            out += [dict(arith=a, family="frac", n=n, kind="twin", inp=inp)
                    for n in FAMILIES["frac"][1]]
        for fam in _WIDE:
            out += [dict(arith=a, family=fam, n=n, kind="twin", inp="emb")
                    for n in FAMILIES[fam][1]]
    return out
