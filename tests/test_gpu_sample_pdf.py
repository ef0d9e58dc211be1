"""nr_sample_pdf (csrc/render.hip sample_pdf_kernel) at its edges: one bin, the
bitonic sort's power-of-two padding just below, at and above a power of two,
degenerate weights, ties, the rank-sort fallback for coarse depths that do not
ascend, and the size limits.

Reference: oracle.sample_pdf on weights[:, 1:-1] and torch.sort of the
concatenation on the CPU.  The idiom of test_gpu_kernels.test_sample_pdf_and_merge:
importance depths are bit-exact, every mismatch is explained by a u within 1e-6
of a reference CDF knot, and mismatches stay below 1e-3 of the samples.  The
seeds are chosen so that the oracle alone puts no u within 1e-6 of a knot
(asserted), so here every importance depth must match.  One exception is by
construction: u = 0 sits exactly on the first knot, cdf[0] = 0, which is the
constant 0 in the reference and in the kernel alike -- no rounding moves it.
"""
import numpy as np
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
SHAPES = [(3, 1), (3, 2), (4, 63), (33, 64), (33, 65), (64, 127), (64, 129), (5, 300)]
KINDS = ("random", "zero", "spike", "span")
# (S, I, n_rays, kind, draws) -> seed, where seed 0 leaves a u within 1e-6 of a knot
SEEDS = {(33, 64, 37, "spike", "random"): 1, (33, 65, 37, "spike", "random"): 1,
         (64, 127, 37, "random", "random"): 4, (64, 127, 37, "zero", "random"): 10,
         (64, 127, 37, "spike", "random"): 4, (64, 127, 37, "random", "ties"): 4,
         (64, 129, 37, "random", "random"): 2, (64, 129, 37, "zero", "random"): 10,
         (64, 129, 37, "spike", "random"): 4, (1026, 1022, 1, "random", "random"): 320,
         (64, 1984, 2, "random", "random"): 5}


def make(S, I, n, kind, draws="random", nearfar="ordinary"):
    g = torch.Generator().manual_seed(SEEDS.get((S, I, n, kind, draws), 0))
    if kind == "random":
        w = torch.rand(n, S, generator=g)
    elif kind == "zero":                      # the uniform CDF of the 1e-5 floor
        w = torch.zeros(n, S)
    elif kind == "spike":                     # one weight of 1.0 among zeros
        w = torch.zeros(n, S)
        w[torch.arange(n), torch.randint(1, S - 1, (n,), generator=g)] = 1.0
    else:                                     # values spanning 1e-12 .. 1
        w = 10.0 ** (-12.0 * torch.rand(n, S, generator=g))
    near = torch.rand(n, 1, generator=g) * 3 + 0.5
    far = near + torch.rand(n, 1, generator=g) * 100 + 1
    if nearfar == "mixed":
        # every third ray descends (near > far); every third has near == far,
        # half of those at 0 (every depth exactly equal: fp32 near (1 - t) +
        # near t is near only to an ulp)
        i = torch.arange(n)[:, None]
        near, far = torch.where(i % 3 == 1, far, near), torch.where(i % 3 == 1, near, far)
        near = torch.where(i % 6 == 5, torch.zeros_like(near), near)
        far = torch.where(i % 3 == 2, near, far)
    rays = torch.cat([torch.randn(n, 6, generator=g), near, far], 1)
    u = torch.rand(n, I, generator=g)
    jit = torch.rand(n, I, generator=g)
    if draws == "ties":                       # duplicates, and ties with z_coarse[0] = near
        u[:, ::3] = 0.0
        jit[:, ::3] = 0.0
    z_coarse = O.coarse_z(rays, S, False, 0.0, None).contiguous()
    return w, rays, u, jit, z_coarse


def knot_distance(w, u):
    """smallest |u - knot| over the batch, the exact pair u = 0 / cdf[0] = 0 apart"""
    ww = w[:, 1:-1] + 1e-5
    cdf = torch.cat([torch.zeros(w.shape[0], 1), torch.cumsum(ww / ww.sum(-1, keepdim=True), -1)],
                    -1)
    d = (cdf[:, None, :] - u[:, :, None]).abs()
    d[:, :, 0] = torch.where(u == 0, torch.ones_like(u), d[:, :, 0])
    return d.min().item(), cdf


def run_and_check(S, I, n, kind, draws="random", nearfar="ordinary"):
    from nerf_pl_amd import ops
    w, rays, u, jit, z_coarse = make(S, I, n, kind, draws, nearfar)
    dist, cdf = knot_distance(w, u)
    assert dist >= 1e-6, f"seed leaves a u {dist:.3g} from a CDF knot: choose another"
    ref = O.sample_pdf(rays, w[:, 1:-1], I, O.ReplayRNG([u, jit]))
    z_pdf, z_fine = ops.sample_pdf(w.to(DEV), rays.to(DEV), I, u=u.to(DEV), jitter=jit.to(DEV),
                                   z_coarse=z_coarse.to(DEV), merge=True)
    assert z_pdf.shape == (n, I) and z_fine.shape == (n, S + I)
    z_pdf, z_fine = z_pdf.cpu(), z_fine.cpu()
    bad = (z_pdf != ref).numpy()
    for r, j in zip(*np.nonzero(bad)):
        assert (cdf[r] - u[r, j]).abs().min().item() < 1e-6, (S, I, n, kind, r, j)
    assert bad.mean() < 1e-3
    # a slot written twice or not at all shows here: the merged depths are the
    # sorted concatenation of the coarse depths and the kernel's own z_pdf
    exp = torch.sort(torch.cat([z_coarse, z_pdf], 1), 1)[0]
    np.testing.assert_array_equal(z_fine.numpy(), exp.numpy())
    # z_pdf alone (no merge) is the same
    only, none = ops.sample_pdf(w.to(DEV), rays.to(DEV), I, u=u.to(DEV), jitter=jit.to(DEV))
    assert none is None
    np.testing.assert_array_equal(only.cpu().numpy(), z_pdf.numpy())
    return z_pdf, z_fine, z_coarse


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("n", [1, 37])
@pytest.mark.parametrize("S,I", SHAPES)
def test_shapes_and_weights(S, I, n, kind):
    run_and_check(S, I, n, kind)


@pytest.mark.parametrize("S,I", SHAPES)
def test_ties(S, I):
    """u = 0 and jitter = 0 on every third sample: equal importance depths, and
    ties with the first coarse depth (both are the ray's near)"""
    z_pdf, z_fine, z_coarse = run_and_check(S, I, 37, "random", draws="ties")
    assert torch.equal(z_pdf[:, 0], z_coarse[:, 0])
    n_ties = (I + 2) // 3 + 1
    assert torch.equal(z_fine[:, :n_ties], z_coarse[:, :1].expand(-1, n_ties))


@pytest.mark.parametrize("S,I", [(3, 2), (33, 65), (64, 129), (5, 300)])
def test_rank_sort_fallback(S, I):
    """Coarse depths that do not ascend (near > far) leave the bitonic sort +
    merge for the rank sort; rays with near == far (every depth equal) and
    ordinary rays share the batch."""
    z_pdf, z_fine, z_coarse = run_and_check(S, I, 37, "random", draws="ties", nearfar="mixed")
    assert (z_coarse[1][:-1] > z_coarse[1][1:]).all()       # ray 1 descends
    assert not z_coarse[5].any() and not z_pdf[5].any() and not z_fine[5].any()


def test_size_limits():
    from nerf_pl_amd import ops
    run_and_check(1026, 5, 3, "random")          # kPdfMaxBins = 1024 bins
    run_and_check(1026, 1022, 1, "random")       # kMergeMax = 2048 merged depths
    run_and_check(64, 1984, 2, "random")         # the same with P = 2048
    for S, I, merge in ((1027, 5, True), (1027, 5, False), (1026, 1023, True), (64, 1985, True)):
        w = torch.rand(2, S, device=DEV)
        rays = torch.rand(2, 8, device=DEV)
        z = torch.rand(2, S, device=DEV)
        with pytest.raises(RuntimeError, match="nr_sample_pdf"):
            ops.sample_pdf(w, rays, I, u=torch.rand(2, I, device=DEV),
                           jitter=torch.rand(2, I, device=DEV), z_coarse=z, merge=merge)
    torch.cuda.synchronize()


def test_empty_calls_return_without_a_launch():
    from nerf_pl_amd import ops
    w, rays, u, jit, z_coarse = make(33, 64, 0, "random")
    z_pdf, z_fine = ops.sample_pdf(w.to(DEV), rays.to(DEV), 64, u=u.to(DEV), jitter=jit.to(DEV),
                                   z_coarse=z_coarse.to(DEV), merge=True)
    assert z_pdf.shape == (0, 64) and z_fine.shape == (0, 97)
    w, rays, u, jit, z_coarse = make(33, 0, 5, "random")
    z_pdf, z_fine = ops.sample_pdf(w.to(DEV), rays.to(DEV), 0, u=u.to(DEV), jitter=jit.to(DEV),
                                   z_coarse=z_coarse.to(DEV), merge=True)
    # nothing is written then (render_rays asks for importance depths only
    # when N_importance > 0): the shapes are all there is to check
    assert z_pdf.shape == (5, 0) and z_fine.shape == (5, 33)
    torch.cuda.synchronize()
