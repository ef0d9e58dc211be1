"""The production randomness: the Philox draws the kernels make in-register
when they get no replay tensor (``rng=None`` -> PhiloxRNG; csrc/common.h
nr_rand_uniform / nr_rand_normal), which every other parity test bypasses by
replaying recorded draws.

Three layers, each bit for bit unless stated:

* the draws themselves (ops.probe_rand, the library's test hook) against the
  numpy model tests/philox_ref.py, which tests/test_philox_ref.py ties to the
  published Philox4x32-10 vectors: uniforms equal, normals finite and within
  2^-20 (1 + radius) of the float64 Box-Muller value;
* each kernel with null draw pointers against the same kernel fed the probe's
  draws as replay tensors: coarse_z (stream 0), sample_pdf (2, 3), the
  compositing forward and backward pairs (1, 4).  The backward comparison is
  the forward/backward consistency check: the gradient is taken at the sigma +
  noise the forward composited;
* the public render paths with PhiloxRNG(seed) against ReplayRNG of the
  probe's draws in the reference's draw order: every result, the captured
  depths and weights, and the parameter gradients of a fixed linear functional.

So whatever the suite proves about replayed draws holds for the in-kernel
ones, and the stream ids (rng.STREAM_*), the per-element indexing and both
words of seed and index are pinned.
"""
import functools
import itertools

import numpy as np
import pytest
import torch

import philox_ref as P
from oracle import nerf_oracle as O
from test_gpu_composite import NAMES, case

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SEEDS = (0, 7, 2 ** 62 - 12345, 0x9E3779B97F4A7C15)   # plain, high word set, bit 63 set
IDX0 = (0, 2 ** 32 - 3, 2 ** 40 + 5)                  # across the low word's wrap; high word set
N_PROBE = 4099                                        # 17 blocks of 256, the last one partial
# model-searched counters (seed 7) where the normal's first word keeps 24 one
# bits (u1 = 1, radius 0) and 24 zero bits (u1 = 2^-24, the largest radius)
EDGE_SEED = 7
EDGES = {1: (19072461, 48431782), 4: (36384934, 22435996)}   # stream: (u1 = 1, u1 = 2^-24)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32),
                                              b.contiguous().view(torch.int32))


def probe(seed, stream, n, idx0=0):
    from nerf_pl_amd import ops
    return ops.probe_rand(seed, stream, n, idx0, device=DEV)


def replay_uniform(seed, stream, rows, cols):
    return probe(seed, stream, rows * cols)[0].view(rows, cols)


def replay_normal(seed, stream, rows, cols):
    return probe(seed, stream, rows * cols)[1].view(rows, cols)


def make_rays(n, seed):
    """(n, 8) rays with per-ray near / far and directions that are not unit"""
    g = torch.Generator().manual_seed(seed)
    near = torch.rand(n, 1, generator=g) * 2 + 0.5
    far = near + torch.rand(n, 1, generator=g) * 20 + 1
    return torch.cat([torch.randn(n, 6, generator=g), near, far], 1).to(DEV)


# ---------------------------------------------------------------------------
# the draws against the model
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_uniform_is_the_model(seed):
    for stream, idx0 in itertools.product(P.STREAMS, IDX0):
        u, _ = probe(seed, stream, N_PROBE, idx0)
        idx = np.uint64(idx0) + np.arange(N_PROBE, dtype=np.uint64)
        ref = P.uniform(seed, stream, idx)
        got = u.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), \
            f"seed {seed:#x} stream {stream} idx0 {idx0}: first at {np.flatnonzero(got != ref)[:4]}"


def normal_ratio(seed, stream, idx0, n):
    """worst |normal - normal64| / (2^-20 (1 + radius64)) of n draws from idx0"""
    _, g = probe(seed, stream, n, idx0)
    idx = np.uint64(idx0) + np.arange(n, dtype=np.uint64)
    got = g.cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), f"seed {seed:#x} stream {stream} idx0 {idx0}: non-finite normal"
    bound = 2.0 ** -20 * (1.0 + P.radius64(seed, stream, idx))
    return float((np.abs(got - P.normal64(seed, stream, idx)) / bound).max())


def test_normal_is_finite_and_accurate():
    """|n - normal64| <= 2^-20 (1 + radius64): the fp32 argument 2 pi u2 is off by
    <= 5.5e-7 (the constant's rounding plus one product rounding below 6.29),
    cosf adds ~2 ulp, the radius ~2^-23 relative -- about 7e-7 radius + 2e-7,
    1.5x inside the bound.  The model-searched edges are included: u1 = 1
    (radius 0, the bound is 2^-20) and u1 = 2^-24 (radius sqrt(48 ln 2)).

    Measured on the MI355X, worst ratio to the bound over every seed, stream
    and idx0 and the edges: 0.301."""
    worst = 0.0
    for seed, stream, idx0 in itertools.product(SEEDS, P.STREAMS, IDX0):
        worst = max(worst, normal_ratio(seed, stream, idx0, N_PROBE))
    for stream, (one, tiny) in EDGES.items():
        m = P.mantissa(P.words(EDGE_SEED, stream, [one, tiny], P.NORMAL)[0])
        assert m.tolist() == [0xFFFFFF, 0], "the edge counters are not the model's edges"
        assert P.radius64(EDGE_SEED, stream, [one])[0] == 0.0
        assert P.radius64(EDGE_SEED, stream, [tiny])[0] == P.RADIUS_MAX
        for at in (one, tiny):
            worst = max(worst, normal_ratio(EDGE_SEED, stream, at - 2, 5))
    print(f"in-kernel normal: worst ratio to 2^-20 (1 + radius) {worst:.3g}")
    assert worst <= 1.0, f"normal {worst:.3g} of the bound: device logf / cosf"


def test_probe_outputs_are_optional():
    from nerf_pl_amd import _lib, ops
    u, g = probe(7, 2, 300, 11)
    for keep_u, keep_g in ((True, False), (False, True)):
        a = torch.full((300,), -7.0, device=DEV)
        _lib.call("nr_probe_rand", 7, 2, 11, 300, _lib.ptr(a) if keep_u else None,
                  _lib.ptr(a) if keep_g else None, _lib.stream_of(DEV))
        assert same_bits(a, u if keep_u else g)
    assert ops.probe_rand(7, 2, 0, device=DEV)[0].shape == (0,)


# ---------------------------------------------------------------------------
# each kernel: null draw pointers against replay of the probe's draws
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_coarse_z_draws_stream_0(seed):
    from nerf_pl_amd import ops
    for (S, n), perturb, use_disp in itertools.product(
            ((1, 1), (2, 5), (64, 4), (65, 37)), (0.5, 1.0), (False, True)):
        rays = make_rays(n, S)
        u = replay_uniform(seed, 0, n, S)
        drawn = ops.coarse_z(rays, S, use_disp, perturb, u=None, seed=seed)
        fed = ops.coarse_z(rays, S, use_disp, perturb, u=u, seed=seed ^ 1)
        what = f"seed {seed:#x} S={S} n={n} perturb={perturb} use_disp={use_disp}"
        assert same_bits(drawn, fed), what
        if S > 1:
            still = ops.coarse_z(rays, S, use_disp, 0.0, u=None, seed=seed)
            assert not same_bits(drawn, still), what + ": nothing was perturbed"


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_sample_pdf_draws_streams_2_and_3(seed):
    from nerf_pl_amd import ops
    for (S, I), n in itertools.product(((3, 1), (8, 5), (64, 128), (65, 129)), (1, 37)):
        rays = make_rays(n, S + I)
        g = torch.Generator().manual_seed(S * 1000 + n)
        w = torch.rand(n, S, generator=g)
        w[n // 2] = 0.0                      # a ray of zero weights: the uniform pdf
        w = w.to(DEV)
        z_c = ops.coarse_z(rays, S, False, 0.0)
        u, jit = replay_uniform(seed, 2, n, I), replay_uniform(seed, 3, n, I)
        fed = ops.sample_pdf(w, rays, I, u=u, jitter=jit, seed=seed ^ 1, z_coarse=z_c, merge=True)
        assert fed[0].shape == (n, I) and fed[1].shape == (n, S + I)
        for name, kw in (("both drawn", {}), ("u fed", dict(u=u)), ("jitter fed", dict(jitter=jit))):
            got = ops.sample_pdf(w, rays, I, seed=seed, z_coarse=z_c, merge=True, **kw)
            what = f"seed {seed:#x} S={S} I={I} n={n}, {name}"
            assert same_bits(got[0], fed[0]), what + ": z_pdf"
            assert same_bits(got[1], fed[1]), what + ": z_fine"
        alone, _ = ops.sample_pdf(w, rays, I, seed=seed)              # no merge
        assert same_bits(alone, fed[0])


SAMPLES = (1, 2, 63, 64, 65, 129, 193)
RAYS = (1, 5, 37)
ALL_NAMES = NAMES + ("g_disp",)


def subsets(names):
    return [c for k in range(len(names) + 1) for c in itertools.combinations(names, k)]


@functools.lru_cache(maxsize=None)
def g_disp_of(S, n):
    return torch.from_numpy(
        np.random.default_rng([5, S, n]).standard_normal(n).astype(np.float32)).to(DEV)


@pytest.mark.parametrize("stream", [1, 4], ids=["coarse", "fine"])
@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_composite_draws_its_stream(seed, stream):
    """Forward and backward, both entry-point pairs, both raw layouts: noise=None
    is the call with noise = the probe's normals of (seed, stream).  Normals
    matched the probe bit for bit on the MI355X (no screening needed)."""
    from nerf_pl_amd import ops
    other = 5 - stream
    for S, n, noise_std in itertools.product(SAMPLES, RAYS, (1.0, 0.5)):
        k = case("typical", S, n)
        noise = replay_normal(seed, stream, n, S)
        g_all = dict(k.g, g_disp=g_disp_of(S, n))
        for raw in (k.raw4, k.raw1):
            what = f"seed {seed:#x} stream {stream} S={S} n={n} std={noise_std} " \
                   f"stride {raw.shape[-1]}"
            drawn = (raw, k.z, k.rays, None, noise_std, seed, stream)
            fed = (raw, k.z, k.rays, noise, noise_std, seed ^ 1, other)
            names = ALL_NAMES if raw is k.raw4 else ALL_NAMES[1:]     # no rgb, no g_rgb
            for wb in (False, True):
                f_d, f_f = ops.composite_forward(*drawn, wb), ops.composite_forward(*fed, wb)
                assert (f_d[0] is None) == (raw is k.raw1)
                for a, b, q in zip(f_d, f_f, ("rgb", "depth", "opacity", "weights")):
                    assert a is None or same_bits(a, b), f"{what} white_back={wb}: {q}"
                w_d = ops.composite_forward(*drawn, wb, weights_only=True)
                assert same_bits(w_d[2], f_f[2]) and same_bits(w_d[3], f_f[3]), \
                    f"{what} white_back={wb}: weights_only"
                d_d = ops.composite_disp_forward(*drawn, wb)
                d_f = ops.composite_disp_forward(*fed, wb)
                for a, b, q in zip(d_d, d_f, ("rgb", "depth", "opacity", "disp", "weights")):
                    assert a is None or same_bits(a, b), f"{what} white_back={wb}: disp pair {q}"
                depth, opac = d_f[1], d_f[2]
                for sub in subsets(names):
                    g = [g_all[x] if x in sub else None for x in ALL_NAMES]
                    lbl = f"{what} white_back={wb} {'+'.join(sub) or 'no gradient'}"
                    b_d = ops.composite_disp_backward(*drawn, wb, *g, depth, opac)
                    b_f = ops.composite_disp_backward(*fed, wb, *g, depth, opac)
                    assert same_bits(b_d, b_f), lbl + ": composite_disp_backward"
                    if "g_disp" not in sub:
                        b_d = ops.composite_backward(*drawn, wb, *g[:3])
                        b_f = ops.composite_backward(*fed, wb, *g[:3])
                        assert same_bits(b_d, b_f), lbl + ": composite_backward"
        if S >= 63:
            w_here = ops.composite_forward(k.raw4, k.z, k.rays, None, noise_std, seed, stream,
                                           False)[3]
            w_other = ops.composite_forward(k.raw4, k.z, k.rays, None, noise_std, seed, other,
                                            False)[3]
            assert not same_bits(w_here, w_other), f"S={S} n={n}: streams 1 and 4 draw alike"
            quiet = ops.composite_forward(k.raw4, k.z, k.rays, None, 0.0, seed, stream, False)[3]
            assert not same_bits(w_here, quiet), f"S={S} n={n}: no noise was drawn"


# ---------------------------------------------------------------------------
# the public paths: PhiloxRNG(seed) against ReplayRNG of the probe's draws
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def models():
    from nerf_pl_amd import NeRF
    out = []
    for s in (1, 2):
        m = NeRF()
        m.load_state_dict(O.make_params(s, sigma_bias=0.5))
        out.append(m.to(DEV))
    return out


def reference_order_draws(seed, n, S, I, perturb):
    """the five draws in the reference's order (nerf_pl_amd/rng.py), each a
    stream of its own indexed from 0"""
    d = [replay_uniform(seed, 0, n, S)] if perturb > 0 else []
    d.append(replay_normal(seed, 1, n, S))
    if I > 0:
        d += [replay_uniform(seed, 2, n, I), replay_uniform(seed, 3, n, I),
              replay_normal(seed, 4, n, S + I)]
    return d


@functools.lru_cache(maxsize=None)
def camera_rays(n):
    g = torch.Generator().manual_seed(n)
    o = torch.randn(n, 3, generator=g) * 0.5
    d = torch.randn(n, 3, generator=g)
    d = d / d.norm(dim=1, keepdim=True) * (0.5 + torch.rand(n, 1, generator=g))
    return torch.cat([o, d, torch.tensor([2.0, 6.0]).expand(n, 2)], 1).contiguous().to(DEV)


def run_render(render, rng, n, S, I, train, use_disp=False, perturb=1.0, noise_std=1.0,
               white_back=False, test_time=False, **extra):
    """every result, the captured depths and weights and (train) every parameter
    gradient of sum_k <c_k, result_k> with fixed random c_k"""
    from nerf_pl_amd import Embedding
    nets = models()
    for m in nets:
        m.zero_grad(set_to_none=True)
    cap = {}
    with torch.set_grad_enabled(train):
        res = render(nets, [Embedding(3, 10), Embedding(3, 4)], camera_rays(n), S, use_disp,
                     perturb, noise_std, I, 32768, white_back, test_time, rng=rng, _capture=cap,
                     **extra)
        out = {k: v.detach() for k, v in res.items()}
        out.update({"captured " + k: v.detach() for k, v in cap.items()})
        if train:
            g = torch.Generator().manual_seed(99)
            loss = 0.0
            for key in sorted(res):
                loss = loss + (res[key] * torch.randn(res[key].shape, generator=g).to(DEV)).sum()
            loss.backward()
            for i, m in enumerate(nets):
                for name, p in m.named_parameters():
                    out[f"d model {i} {name}"] = None if p.grad is None else p.grad.clone()
    torch.cuda.synchronize()
    return out


def assert_philox_is_replay(render, seed, n, S, I, train, want, **flags):
    from nerf_pl_amd import PhiloxRNG, ReplayRNG
    replay = ReplayRNG(reference_order_draws(seed, n, S, I, flags.get("perturb", 1.0)), seed ^ 1)
    fed = run_render(render, replay, n, S, I, train, **flags)
    assert replay.exhausted()
    drawn = run_render(render, PhiloxRNG(seed), n, S, I, train, **flags)
    assert set(drawn) == set(fed) and set(want) <= set(drawn), sorted(set(want) - set(drawn))
    if train:
        assert any(k.startswith("d model") and v is not None and v.any() for k, v in fed.items())
    for key in sorted(fed):
        a, b = drawn[key], fed[key]
        assert (a is None) == (b is None), key
        assert a is None or same_bits(a, b), \
            f"seed {seed:#x} n={n} S={S} I={I} {flags}: {key} differs, PhiloxRNG vs replay"


BOTH = ("coarse", "fine")
CAPTURED = ["captured " + k for k in ("z_coarse", "weights_coarse", "z_fine", "weights_fine")]
RENDER_CASES = {
    "training": ((37, 64, 128), True, dict(perturb=1.0, noise_std=1.0)),
    "tiny": ((5, 3, 1), True, dict(perturb=0.0, noise_std=1.0)),
    "coarse only": ((37, 32, 0), True, dict(perturb=1.0, noise_std=0.5)),
    "test_time": ((16, 64, 64), False, dict(test_time=True)),
    "disp white": ((23, 16, 24), True, dict(use_disp=True, white_back=True, perturb=0.5)),
}


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
@pytest.mark.parametrize("name", RENDER_CASES)
def test_render_rays(name, seed):
    from nerf_pl_amd import render_rays
    (n, S, I), train, flags = RENDER_CASES[name]
    levels = BOTH if I else BOTH[:1]
    want = [f"{q}_{lv}" for lv in levels for q in ("rgb", "depth", "opacity")]
    if flags.get("test_time"):
        want = ["opacity_coarse", "rgb_fine", "depth_fine", "opacity_fine"]
    want += CAPTURED if I else CAPTURED[:2]
    assert_philox_is_replay(render_rays, seed, n, S, I, train, want, **flags)


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
@pytest.mark.parametrize("depth_only", [False, True], ids=["full", "depth_only"])
def test_rgb_sm_render_rays(depth_only, seed):
    from nerf_pl_amd import rendering_rgb_sm
    want = [f"{q}_{lv}" for lv in BOTH for q in ("depth", "opacity", "disp_map")] + CAPTURED
    if not depth_only:
        want += ["rgb_coarse", "rgb_fine"]
    assert_philox_is_replay(rendering_rgb_sm.render_rays, seed, 23, 16, 24, True, want,
                            depth_only=depth_only)


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_shadow_render_rays(seed):
    from nerf_pl_amd import rendering_shadows
    want = [f"{q}_{lv}" for lv in BOTH for q in ("depth", "opacity", "disp_map")] + CAPTURED[:3]
    assert_philox_is_replay(rendering_shadows.render_rays, seed, 23, 16, 24, True, want)


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_public_sample_pdf(seed):
    import nerf_pl_amd
    n, bins, I = 37, 62, 128
    rays = camera_rays(n)
    w = torch.rand(n, bins, generator=torch.Generator().manual_seed(3)).to(DEV)
    replay = nerf_pl_amd.ReplayRNG([replay_uniform(seed, 2, n, I), replay_uniform(seed, 3, n, I)],
                                   seed ^ 1)
    fed = nerf_pl_amd.sample_pdf(rays, w, I, rng=replay)
    assert replay.exhausted() and fed.shape == (n, I)
    assert same_bits(nerf_pl_amd.sample_pdf(rays, w, I, rng=nerf_pl_amd.PhiloxRNG(seed)), fed)


def test_unseeded_philox_follows_the_torch_generator():
    from nerf_pl_amd import PhiloxRNG
    torch.manual_seed(5)
    first = (PhiloxRNG().seed, PhiloxRNG().seed)
    assert first[0] != first[1], "two render calls in a row would draw the same numbers"
    torch.manual_seed(5)
    assert (PhiloxRNG().seed, PhiloxRNG().seed) == first
    assert all(0 <= s < 2 ** 62 for s in first)
