"""High-precision reference and case builder for the shadow-map kernels
(csrc/shadow.hip) -- test infrastructure, like composite64.py.

``reference(case, dtype)`` is oracle/shadow_oracle.py run per run of equal eye
position (``shadow_runs`` then ``run_shadow_mapping`` with the case's options,
``+ out_eps``), in ``torch.float64`` or ``torch.float32``; the depths and the
light map are leaves and ``backward(g_out)`` gives d/d depth and d/d light map
by autograd.  No arithmetic is restated here: the oracle is pinned to the
reference (tests/test_shadow_golden.py, tests/test_shadow64.py) and its float64
autograd is the plain high-precision form.

``make_case(name)`` builds deterministic fp32 inputs on which the fp32 kernel,
the fp32 oracle and the float64 oracle take the same discrete decisions, so the
GPU tests (tests/test_gpu_shadow_kernels.py) screen out no ray.  Every
condition is computed from the float64 reference; a draw that misses one is
redrawn with the next seed:

* texel margin: every (u, v) is at least ``TEXEL_MARGIN`` from a truncation
  edge, clamped coordinates at least that far outside [0, res - 1];
* shadow_method_1: the light map is designed from the rays -- the first ray to
  hit texel k sets lw[k] = wl - delta m with m drawn from (-0.5, 1.5) -- so
  that rays are spread over the clip's three pieces, and no m lies within
  ``KINK_MARGIN`` of a kink {0, epsilon, 1};
* shadow_method_2: in every run the two smallest (and the two largest)
  distinct differences are ``GAP`` (max - min) apart, so argmin and argmax are
  the same in fp32 and float64 (rays duplicated on purpose are bitwise ties in
  any precision);
* cases of 1000 rays or more ("full" cases) also hold the shares of
  ``check_shares``: clamped >= 10 % with every reachable border hit, a texel
  with >= 20 rays and one with exactly one, and under method 1 >= 50 %
  interior, >= 10 % clipped below, >= 10 % clipped above.  The small cases
  (n = 1, 64, 65, the tie and non-finite batches) are too few rays for shares
  and keep the margins only.
"""
import math

import numpy as np
import torch

from oracle import shadow_oracle as SO

GRID = 64                   # camera pixel grid (pixel centres i + 0.5)
TEXEL_MARGIN = 0.05
KINK_MARGIN = 1e-3
GAP = 1e-4
RUN_LENS = (1, 1, 62, 64, 1, 63, 65, 128, 3, 700, 2, 191, 1, 1249)      # n = 2531

_M1 = "shadow_method_1"
_M2 = "shadow_method_2"
OPTIONS = {
    "m1": dict(mode=_M1, delta=1e-2, epsilon=0.0, sigmoid=False),
    "m1_d05": dict(mode=_M1, delta=0.05, epsilon=0.0, sigmoid=False),
    "m1_eps": dict(mode=_M1, delta=0.5, epsilon=0.25, sigmoid=False),
    "m2": dict(mode=_M2, delta=1e-2, epsilon=0.0, sigmoid=False),
    "m2_sig": dict(mode=_M2, delta=1e-2, epsilon=0.0, sigmoid=True),
}
# lens: per-pose run lengths (poses cycle, so a pose comes back after another)
GEOMETRIES = {
    "runs": dict(lens=RUN_LENS),
    "n1025": dict(lens=(1, 300, 64, 500, 160)),
    "n1024": dict(lens=(1, 300, 64, 500, 159)),
    "n64": dict(lens=(64,)),
    "n65": dict(lens=(1, 64)),
    "n1": dict(lens=(1,)),
    "single300": dict(lens=(300,), single=True),        # eye (3,), camera (3,3)
    "nonsquare": dict(lens=(120, 1, 100, 79), res=(24, 16)),
    "ties": dict(lens=(40, 1, 30), ties=True),
    "nonfinite": dict(lens=(50, 70, 1, 90, 60), nonfinite=True),
    "tie1": dict(lens=(100, 150)),
}
CASES = {f"runs_{o}": ("runs", o) for o in OPTIONS}
CASES.update({f"{g}_{o}": (g, o) for g in ("n1025", "n1024", "n64", "n65", "n1", "single300",
                                            "nonsquare", "nonfinite") for o in ("m1", "m2")})
CASES["ties_m2"] = ("ties", "m2")
CASES["tie1_m1"] = ("tie1", "m1")


def _scene(res):
    """One light and three camera poses, as tests/test_gpu_shadow_random._scene."""
    from nerf_pl_amd.camera import Camera
    from nerf_pl_amd.rays import LEGO_CAMERA_ANGLE_X, pose_spherical
    hfov = LEGO_CAMERA_ANGLE_X * 180. / np.pi
    light = Camera(hfov, res)
    light.set_pose_using_blender_matrix(pose_spherical(35.0, -55.0, 4.0), False)
    cams = []
    for theta in (-20.0, 60.0, 140.0):
        cam = Camera(hfov, (GRID, GRID))
        cam.set_pose_using_blender_matrix(pose_spherical(theta, -30.0, 4.0), False)
        cams.append((cam.eye_pos.float(), cam.camera.float()))
    return light.eye_pos.float(), light.camera.float(), cams


def _per_ray(case):
    n = case["depth"].shape[0]
    eye, cams = case["eye"], case["cams"]
    if eye.dim() == 1:
        eye, cams = eye.expand(n, 3), cams.expand(n, 3, 3)
    return eye, cams


def runs_of(case):
    """SO.shadow_runs of the case's eye positions (kept with the case)."""
    if "_runs" not in case:
        case["_runs"] = SO.shadow_runs(_per_ray(case)[0]) if case["depth"].shape[0] else []
    return case["_runs"]


def project(case, dtype=torch.float64, depth=None):
    """(u, v, wl) per ray before clamping, by the oracle's functions."""
    eye, cams = _per_ray(case)
    px = case["pixels"].to(dtype)
    dep = (case["depth"] if depth is None else depth).to(dtype)
    le, lc = case["light_eye"].to(dtype), case["light_cam"].to(dtype)
    parts = []
    for s, e in runs_of(case):
        wc = SO.get_normed_w(cams[s].to(dtype), torch.cat([px[s:e], dep[s:e, None]], 1))
        R, Q = SO.transformation_to(eye[s].to(dtype), cams[s].to(dtype), le, lc)
        parts.append(SO.get_diff_projections(wc[:, :3], wc[:, 3], R, Q))
    return torch.cat(parts).unbind(1)


def texel_keys(case, dtype=torch.float64):
    """Texel index of every ray: w_light.view(w, h)[v, u] reads v * h + u."""
    w, h = case["res"]
    u, v, _ = project(case, dtype)
    return (v.clamp(0, h - 1).long() * h + u.clamp(0, w - 1).long()).numpy()


class Reference:
    """out (n,3), pre (out without out_eps), g_depth (n,), g_lw (w*h,) as numpy
    arrays of ``dtype``."""


def reference(case, dtype=torch.float64, backward=True, depth=None, lw=None):
    """The oracle per run with the case's options; ``backward``: also d/d depth
    and d/d light map of sum(out * g_out).  ``depth`` / ``lw`` replace the
    case's (the finite differences of tests/test_shadow64.py)."""
    eye, cams = _per_ray(case)
    px = case["pixels"].to(dtype)
    dep = (case["depth"] if depth is None else depth).to(dtype).clone().requires_grad_(backward)
    lwt = (case["lw"] if lw is None else lw).to(dtype).clone().requires_grad_(backward)
    le, lc = case["light_eye"].to(dtype), case["light_cam"].to(dtype)
    parts = []
    for s, e in runs_of(case):
        parts.append(SO.run_shadow_mapping(
            case["res"], eye[s].to(dtype), cams[s].to(dtype), le, lc,
            torch.cat([px[s:e], dep[s:e, None]], 1), lwt, case["mode"], case["delta"],
            case["epsilon"], sigmoid=case["sigmoid"]))
    pre = torch.cat(parts, 0)
    out = pre + case["out_eps"]
    r = Reference()
    r.out, r.pre = out.detach().numpy(), pre.detach().numpy()
    if backward:
        out.backward(case["g_out"].to(dtype))
        r.g_depth, r.g_lw = dep.grad.numpy(), lwt.grad.numpy()
    return r


def diffs(case, dtype=torch.float64):
    """wl - w_light_bounded per ray (efficient_shadow_mapping.py:114)."""
    _, _, wl = project(case, dtype)
    return (wl - case["lw"].to(dtype)[torch.from_numpy(texel_keys(case, dtype))]).numpy()


def _margin_ok(x, size):
    """at least TEXEL_MARGIN from a truncation edge; clamped values that far outside"""
    inside = (x >= 0) & (x <= size - 1)
    frac = np.abs(x - np.round(x))
    return np.where(inside, frac >= TEXEL_MARGIN,
                    (x <= -TEXEL_MARGIN) | (x >= size - 1 + TEXEL_MARGIN))


def _sample_run(rng, pose, light, res, count):
    """Rejection-sample ``count`` rays of one pose: random pixel centres, depth
    uniform in [2, 6], texel margin kept; half of the clamped candidates are
    dropped so that hit texels are not mostly border texels."""
    eye, cam = pose
    w, h = res
    pix_all, dep_all, have = [], [], 0
    while have < count:
        m = 4 * count + 64
        pix = np.concatenate([rng.integers(0, GRID, (m, 2)) + 0.5, np.ones((m, 1))], 1)
        dep = rng.uniform(2.0, 6.0, m)
        keep_clamped = rng.random(m) < 0.5
        c = dict(pixels=torch.from_numpy(pix.astype(np.float32)),
                 depth=torch.from_numpy(dep.astype(np.float32)), eye=eye, cams=cam,
                 light_eye=light[0], light_cam=light[1])
        u, v, _ = (t.numpy() for t in project(c))
        ok = _margin_ok(u, w) & _margin_ok(v, h)
        if w != h:
            ok &= u < h         # the range the reference's view(w, h)[v, u] accepts
        clamped = (u < 0) | (u > w - 1) | (v < 0) | (v > h - 1)
        ok &= ~clamped | keep_clamped
        pix_all.append(c["pixels"][ok]); dep_all.append(c["depth"][ok])
        have += int(ok.sum())
    pix, dep = torch.cat(pix_all)[:count].clone(), torch.cat(dep_all)[:count].clone()
    if count >= 100:
        _pile(pix, dep, pose, light, res)
    return pix, dep


PILE = 24


def _pile(pix, dep, pose, light, res):
    """Overwrite the last PILE rays with one unclamped ray's pixel at depths a
    few 2^-11 apart, all in that ray's texel: a texel that >= 20 rays read."""
    w, h = res
    step = torch.arange(1, PILE + 1, dtype=torch.float32) * 2.0 ** -11
    for i in range(dep.shape[0] - PILE):
        c = dict(pixels=pix[i].expand(PILE + 1, 3), eye=pose[0], cams=pose[1],
                 depth=torch.cat([dep[i:i + 1], dep[i] + step]),
                 light_eye=light[0], light_cam=light[1])
        u, v, _ = (t.numpy() for t in project(c))
        inside = (u > 0) & (u < min(w, h) - 1) & (v > 0) & (v < h - 1)
        same = (np.floor(u) == np.floor(u[0])) & (np.floor(v) == np.floor(v[0]))
        if (inside & same & _margin_ok(u, w) & _margin_ok(v, h)).all():
            pix[-PILE:], dep[-PILE:] = c["pixels"][1:], c["depth"][1:]
            return
    raise AssertionError("no ray to pile on")


def _draw_m(rng, k, epsilon, inner_only=False):
    """m in (-0.5, 1.5): 70 % inside the clip's linear piece, 15 % below, 15 % above"""
    lo = max(0.0, epsilon)
    piece = rng.random(k) * (0.7 if inner_only else 1.0)
    inner = rng.uniform(lo + 0.02, 0.98, k)
    below = rng.uniform(-0.5, min(0.0, epsilon) - 0.02, k)
    above = rng.uniform(1.02, 1.5, k)
    return np.where(piece < 0.70, inner, np.where(piece < 0.85, below, above))


def _near_kink(m, epsilon):
    return np.minimum.reduce([np.abs(m - k) for k in (0.0, epsilon, 1.0)]) < KINK_MARGIN


def _design_light_map(rng, case):
    """shadow_method_1: lw[k] = wl - delta m of the first ray to hit texel k.
    Texels whose later rays land near a kink get a new m (a few passes)."""
    w, h = case["res"]
    delta, eps = case["delta"], case["epsilon"]
    key = texel_keys(case)
    wl = project(case)[2].numpy()
    texels, first = np.unique(key, return_index=True)
    lw = np.full(w * h, 0.05, np.float32)           # background: mid-range wl
    todo = np.ones(texels.shape[0], bool)
    for _ in range(64):
        lw[texels[todo]] = (wl[first[todo]] - delta * _draw_m(rng, int(todo.sum()), eps, key.size < 4))
        m = (wl - lw[key].astype(np.float64)) / delta
        bad = np.unique(key[_near_kink(m, eps)])
        if bad.size == 0:
            break
        todo = np.isin(texels, bad)
    return torch.from_numpy(lw)


def m_values(case):
    """shadow_method_1's pre-clip value (wl - wlb) / delta per ray, float64"""
    return diffs(case) / case["delta"]


def run_gaps(case):
    """per run: (gap of the two smallest distinct differences, of the two
    largest) / (max - min); inf where a run has fewer than two distinct values
    or a non-finite one"""
    d = diffs(case)
    out = []
    for s, e in runs_of(case):
        v = np.unique(d[s:e])
        if v.size < 2 or not np.isfinite(v).all():
            out.append((math.inf, math.inf))
            continue
        rng_ = v[-1] - v[0]
        out.append(((v[1] - v[0]) / rng_, (v[-1] - v[-2]) / rng_))
    return out


def shares(case):
    """The builder's statistics, from the float64 reference."""
    w, h = case["res"]
    u, v, _ = (t.numpy() for t in project(case))
    key = texel_keys(case)
    hits = np.bincount(key, minlength=w * h)
    s = dict(n=int(u.shape[0]),
             clamped=float(((u < 0) | (u > w - 1) | (v < 0) | (v > h - 1)).mean()),
             borders=(int((u < 0).sum()), int((u > w - 1).sum()), int((v < 0).sum()),
                      int((v > h - 1).sum())),
             max_hits=int(hits.max()), single_hits=int((hits == 1).sum()),
             margin_ok=bool((_margin_ok(u, w) & _margin_ok(v, h)).all()))
    if case["mode"] == _M1:
        m, eps = m_values(case), case["epsilon"]
        m = m[np.isfinite(m)]
        s.update(interior=float(((m > max(0.0, eps) + KINK_MARGIN) & (m < 1 - KINK_MARGIN)).mean()),
                 below=float((m < eps - KINK_MARGIN).mean()),
                 above=float((m > 1 + KINK_MARGIN).mean()),
                 kink_ok=not _near_kink(m, eps).any())
    else:
        gaps = run_gaps(case)
        s.update(min_gap=float(min(min(g) for g in gaps)))
    return s


def check_shares(case, s):
    """Why a draw is unusable, or None."""
    if not s["margin_ok"]:
        return "texel margin"
    if case["mode"] == _M1 and not s["kink_ok"]:
        return "ray near a kink"
    if case["mode"] == _M2 and s["min_gap"] < GAP:
        return "extremes too close"
    if s["n"] < 1000:
        return None
    w, h = case["res"]
    # w > h: rays keep clamped u < h, so the u = w - 1 border is out of reach
    need = [0, 2, 3] if w != h else [0, 1, 2, 3]
    if s["clamped"] < 0.10 or any(s["borders"][b] == 0 for b in need):
        return "clamping not exercised"
    if s["max_hits"] < 20 or s["single_hits"] < 1:
        return "hit counts"
    if case["mode"] == _M1 and (s["interior"] < 0.50 or s["below"] < 0.10 or s["above"] < 0.10):
        return "method 1 shares"
    return None


def _add_ties(case):
    """Run 0 holds its min ray 3 times and its max ray twice (duplicated rows);
    the last run is one ray repeated (max = min, denominator 1e-5)."""
    (s0, e0), last = runs_of(case)[0], runs_of(case)[-1]
    d = diffs(case)[s0:e0]
    lo, hi = s0 + int(d.argmin()), s0 + int(d.argmax())
    rows = list(range(s0, e0)) + [lo, lo, hi] + list(range(e0, last[0])) + \
        [last[0]] * (last[1] - last[0])
    for k in ("pixels", "depth", "eye", "cams"):
        case[k] = case[k][rows].contiguous()
    del case["_runs"]
    case["tie_rows"] = dict(min=[lo, e0, e0 + 1], max=[hi, e0 + 2])


def _add_nonfinite(case):
    """One NaN texel read by rays of run 1 and one +inf texel read by rays of
    run 3; runs 0, 2 and 4 read neither."""
    runs = runs_of(case)
    key = texel_keys(case)
    clean = np.concatenate([key[s:e] for s, e in (runs[0], runs[2], runs[4])])
    picks = []
    for r in (1, 3):
        s, e = runs[r]
        own = [k for k in key[s:e] if k not in clean and k not in picks]
        if not own:
            return False
        picks.append(own[0])
    case["lw"][picks[0]] = float("nan")
    case["lw"][picks[1]] = float("inf")
    case["nonfinite_texels"] = picks
    return True


def _build(name, seed):
    geom_name, opt_name = CASES[name]
    geom = GEOMETRIES[geom_name]
    res = geom.get("res", (64, 64))
    rng = np.random.default_rng(seed)
    light_eye, light_cam, poses = _scene(res)
    pix, dep, eye, cams = [], [], [], []
    for k, count in enumerate(geom["lens"]):
        p, d = _sample_run(rng, poses[k % 3], (light_eye, light_cam), res, count)
        pix.append(p); dep.append(d)
        eye.append(poses[k % 3][0].expand(count, 3)); cams.append(poses[k % 3][1].expand(count, 3, 3))
    case = dict(name=name, seed=seed, res=res, out_eps=0.0, light_eye=light_eye,
                light_cam=light_cam, pixels=torch.cat(pix).contiguous(),
                depth=torch.cat(dep).contiguous(), eye=torch.cat(eye).contiguous(),
                cams=torch.cat(cams).contiguous(), **OPTIONS[opt_name])
    if geom.get("single"):
        case["eye"], case["cams"] = poses[0][0].clone(), poses[0][1].clone()
    if geom.get("nonfinite"):
        case["nonfinite"] = True
    # shadow_method_2 reads a random map over the range of wl
    case["lw"] = torch.from_numpy((0.02 + 0.06 * rng.random(res[0] * res[1])).astype(np.float32))
    if geom.get("ties"):
        _add_ties(case)
    if case["mode"] == _M1:
        case["lw"] = _design_light_map(rng, case)
    if geom.get("nonfinite") and not _add_nonfinite(case):
        return None, "no private texel for the non-finite values"
    n = case["depth"].shape[0]
    # upstream gradient: random per channel, magnitudes spread over 2^-10 .. 1
    case["g_out"] = torch.from_numpy(
        (rng.choice([-1.0, 1.0], (n, 3)) * 2.0 ** (-10.0 * rng.random((n, 3)))).astype(np.float32))
    why = check_shares(case, shares(case))
    return case, why


_CACHE = {}


def make_case(name):
    """Deterministic: the first seed (from a per-name start) whose draw holds
    every condition.  Tensors are fp32 CPU; treat them as read-only."""
    if name not in _CACHE:
        base = 1000 * (1 + sorted(CASES).index(name))
        for seed in range(base, base + 200):
            case, why = _build(name, seed)
            if why is None:
                _CACHE[name] = case
                break
        else:
            raise AssertionError(f"{name}: no usable draw in 200 seeds (last: {why})")
    return _CACHE[name]
