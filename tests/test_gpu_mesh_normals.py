"""The vertex-normal kernels (csrc/mesh_normals.hip) and the
``--use_vertex_normal`` path of nerf_pl_amd.extract on the device, against the
restatements of tests/mesh_normals_ref.py.

Bounds (none taken from the kernels' output):
  * a unit normal is within 1e-12 absolute per component of the float64
    restatement (the same float64 operations in the same order; 1e-12 is the
    project's bound for float64 sums) wherever the restatement's
    ``|m_v| >= 1e-6 * sum_t |n_t|`` -- a well-conditioned vertex; a vertex
    below that is only required to be a unit vector or (0, 0, 1).  The sphere
    and the torus have no such vertex (tests/test_mesh_normals_ref.py confirms
    it on the CPU), a random field may have 1%;
  * the rays equal the float32 restatement bit for bit;
  * the colours equal a hand-written chunk loop of ``render_rays`` bit for bit.
"""
import numpy as np
import pytest
import torch

import mesh_normals_ref as NR
import mesh_ref as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
UP = np.array(NR.UP)
DIMS, CENTRE = (9, 11, 13), (4.0, 5.0, 6.0)
NEAR, FAR = 2.0, 6.0


def _normals(v, t):
    from nerf_pl_amd.extract import vertex_normals
    dv, dt = torch.from_numpy(v).to(DEV), torch.from_numpy(t).to(DEV)
    a = vertex_normals(dv, dt)
    b = vertex_normals(dv, dt)
    assert a.dtype == torch.float64 and a.shape == (len(v), 3) and a.device.type == "cuda"
    assert torch.equal(a, b)                       # atomic-free: two runs, one result
    return a.cpu().numpy()


def _check(v, t, max_bad=0):
    """the kernel against the restatement; returns the kernel's normals"""
    got = _normals(v, t)
    q, m, mag = NR.vertex_normals_ref(v, t)
    good = NR.well_conditioned(m, mag)
    n_bad = int((~good).sum())
    err = np.abs(got[good] - q[good]).max() if good.any() else 0.0
    print(f"V = {len(v)}, T = {len(t)}: {n_bad} below the bound, max error {err:.3g}")
    assert n_bad <= max_bad
    assert err <= 1e-12
    up = (q == UP).all(1) & good
    np.testing.assert_array_equal(got[up], q[up])               # (0, 0, 1) exactly
    rest = got[~good]
    unit = np.abs(np.sqrt((rest * rest).sum(1)) - 1.0) <= 1e-12
    assert (unit | (rest == UP).all(1)).all()
    assert np.isfinite(got).all()
    return got


def _mc(sigma):
    from nerf_pl_amd.extract import marching_cubes
    v, t = marching_cubes(torch.from_numpy(np.ascontiguousarray(sigma)).to(DEV), 0.0)
    return v.cpu().numpy(), t.cpu().numpy()


@pytest.mark.parametrize("name", sorted(NR.HAND_CASES))
def test_hand_cases(name):
    v, t, want = NR.HAND_CASES[name]()
    got = _check(v, t)
    np.testing.assert_allclose(got, want, rtol=0, atol=4 * np.finfo(np.float64).eps)
    exact = (np.abs(want) == 1).any(1)
    np.testing.assert_array_equal(got[exact], want[exact])


def test_fan_above_one_wave():
    v, t, _ = NR.fan(70)
    off, _ = NR.csr(t, len(v))
    assert off[1] - off[0] == 70 > 64
    _check(v, t)


@pytest.mark.parametrize("n_vertices", [257, 513])
def test_strips_across_the_blocks(n_vertices):
    v, t, _ = NR.strip(n_vertices)
    got = _check(v, t)
    assert not (got == UP).all(1).any()


def test_nan_and_inf_vertices_and_empty_meshes():
    from nerf_pl_amd.extract import vertex_normals
    v, t, want = NR.two_areas()
    for poison in (np.nan, np.inf):
        w = v.copy()
        w[2, 1] = poison            # the sums of vertices 0, 1, 2 hold NaN: (0, 0, 1)
        got = _check(w, t, max_bad=3)
        np.testing.assert_array_equal(got, np.array([UP, UP, UP, (1.0, 0.0, 0.0)]))
    # no triangle at all: (0, 0, 1) everywhere, and the two null pointers are accepted
    got = _normals(v, np.zeros((0, 3), np.int32))
    np.testing.assert_array_equal(got, np.broadcast_to(UP, (4, 3)))
    e = vertex_normals(torch.empty(0, 3, device=DEV),
                       torch.empty(0, 3, dtype=torch.int32, device=DEV))
    assert e.shape == (0, 3) and e.dtype == torch.float64
    with pytest.raises(ValueError):
        vertex_normals(torch.from_numpy(v).to(DEV), torch.tensor([[0, 1, 4]], dtype=torch.int32,
                                                                 device=DEV))


@pytest.mark.parametrize("name,max_bad", [("open_sphere", 0), ("sphere", 0), ("torus", 0),
                                          ("noise_5_7_9", 0.01), ("noise_24", 0.01)])
def test_marching_cubes_meshes(name, max_bad):
    sigma = {"open_sphere": lambda: R.sphere_field((7, 8, 9), (3.0, 3.5, 4.0), 4.3),
             "sphere": lambda: R.sphere_field(DIMS, CENTRE, 3.5),
             "torus": lambda: R.torus_field(DIMS, CENTRE, 3.0, 1.5),
             "noise_5_7_9": lambda: R.random_field((5, 7, 9), 1),
             "noise_24": lambda: R.random_field((24, 24, 24), 2)}[name]()
    v, t = _mc(sigma)
    assert len(t) > 0
    got = _check(v, t, max_bad=int(max_bad * len(v)))
    if name == "sphere":            # marching_cubes winds towards the empty side: outwards
        assert ((got * (v.astype(np.float64) - np.asarray(CENTRE))).sum(1) > 0).all()


def test_garbage_csr_list_stays_inside_the_buffers():
    """The guards, not a fault: every index the kernel forms from the list is
    range-checked before it is used, so offsets beyond 3T, negative offsets,
    incident indices of -1 and n_triangles, and triangles naming vertices -1
    and V are skipped.  The output rows are finite and the row allocated after
    them keeps its sentinel."""
    from nerf_pl_amd import _lib_mesh_normals
    from nerf_pl_amd._lib import ptr, stream_of
    v, t, _ = NR.strip(257)
    n_v, n_t = len(v), len(t)
    g = np.random.Generator(np.random.PCG64(9))
    off, inc = NR.csr(t, n_v)
    off = off.copy()
    inc = inc.copy()
    off[g.permutation(n_v + 1)[:60]] = g.choice([-5, -1, 3 * n_t + 1, 3 * n_t + 1000, 2 ** 40], 60)
    inc[g.permutation(3 * n_t)[:200]] = g.choice([-1, n_t, n_t + 7, -2 ** 31, 2 ** 31 - 1], 200)
    t = t.copy()
    t[5] = (-1, 6, 7)
    t[100] = (100, n_v, 102)
    t[200] = (200, 201, 2 ** 31 - 1)
    dv, dt = torch.from_numpy(v).to(DEV), torch.from_numpy(t).to(DEV)
    doff, dinc = torch.from_numpy(off).to(DEV), torch.from_numpy(inc).to(DEV)
    out = torch.full((n_v + 1, 3), 7.0, dtype=torch.float64, device=DEV)
    _lib_mesh_normals.call("nr_mesh_vertex_normals", ptr(dv), ptr(dt), ptr(doff), ptr(dinc), n_v,
                           n_t, ptr(out), stream_of(DEV))
    res = out.cpu().numpy()
    assert (res[n_v] == 7.0).all()
    rows = res[:n_v]
    assert np.isfinite(rows).all()
    unit = np.abs(np.sqrt((rows * rows).sum(1)) - 1.0) <= 1e-12
    assert unit.all()               # a unit vector, (0, 0, 1) included


@pytest.mark.parametrize("inward", [True, False])
@pytest.mark.parametrize("near_t", [1.0, 0.5])
def test_normal_rays_bit_for_bit(inward, near_t):
    from nerf_pl_amd.extract import normal_rays, vertex_normals
    v, t, _ = NR.strip(513)
    dv = torch.from_numpy(v).to(DEV)
    dn = vertex_normals(dv, torch.from_numpy(t).to(DEV))
    dn[7] = torch.tensor(NR.UP, dtype=torch.float64)  # the fallback row: its zeros keep their signs
    rays = normal_rays(dv, dn, NEAR, FAR, near_t, inward)
    assert rays.dtype == torch.float32 and rays.shape == (513, 8)
    want = NR.normal_rays_ref(v, dn.cpu().numpy(), NEAR, FAR, near_t, inward)
    assert torch.equal(rays.cpu(), torch.from_numpy(want))
    assert rays.cpu().numpy().tobytes() == want.tobytes()      # signed zeros too
    e = normal_rays(dv[:0], dn[:0], NEAR, FAR, near_t, inward)
    assert e.shape == (0, 8)


# ---------------------------------------------------------------------------
# the coarse + fine render along the normals
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    from nerf_pl_amd import NeRF
    out = []
    for seed in (1, 2):
        m = NeRF().to(DEV)
        m.load_state_dict(O.make_params(seed, sigma_bias=0.5))
        out.append(m)
    return out


@pytest.fixture(scope="module")
def sphere_mesh():
    """the closed sphere, centred on the origin, radius 0.875"""
    v, t = _mc(R.sphere_field(DIMS, CENTRE, 3.5))
    w = ((v - np.asarray(CENTRE, dtype=np.float32)) * np.float32(0.25)).astype(np.float32)
    return torch.from_numpy(w).to(DEV), torch.from_numpy(t).to(DEV)


@pytest.mark.parametrize("chunk", [None, 100])
def test_color_by_vertex_normals_is_the_chunk_loop(models, sphere_mesh, chunk):
    from nerf_pl_amd import Embedding, render_rays
    from nerf_pl_amd.extract import (FUSE_CHUNK, color_by_vertex_normals, normal_rays,
                                     vertex_normals)
    v, t = sphere_mesh
    n = len(v)
    c = FUSE_CHUNK if chunk is None else chunk
    assert (c >= n) if chunk is None else (n > c and n % c != 0)
    rays = normal_rays(v, vertex_normals(v, t), NEAR, FAR)
    # inward: every ray looks from the surface towards the centre
    assert ((rays[:, 3:6] * v).sum(1) < 0).all()
    torch.manual_seed(5)
    want = torch.cat([render_rays(models, [Embedding(3, 10), Embedding(3, 4)], rays[i:i + c], 8,
                                  False, 0, 0, 8, c, False, test_time=True)["rgb_fine"]
                      for i in range(0, n, c)], 0)
    torch.manual_seed(5)
    kw = {} if chunk is None else {"chunk": chunk}
    colors, rgb = color_by_vertex_normals(models, v, t, NEAR, FAR, N_samples=8, N_importance=8,
                                          return_rgb=True, **kw)
    assert rgb.dtype == torch.float32 and rgb.shape == (n, 3)
    assert colors.dtype == torch.uint8 and colors.shape == (n, 3)
    assert torch.equal(rgb, want)
    assert torch.equal(colors, (want * 255).to(torch.uint8))
    torch.manual_seed(5)
    only = color_by_vertex_normals(models, v, t, NEAR, FAR, N_samples=8, N_importance=8, **kw)
    assert torch.equal(only, colors)
    # the outward rays are the other rays
    out = normal_rays(v, vertex_normals(v, t), NEAR, FAR, inward=False)
    assert torch.equal(out[:, 3:6], -rays[:, 3:6])


def test_color_by_vertex_normals_of_an_empty_mesh(models):
    from nerf_pl_amd.extract import color_by_vertex_normals
    v = torch.empty(0, 3, device=DEV)
    t = torch.empty(0, 3, dtype=torch.int32, device=DEV)
    colors, rgb = color_by_vertex_normals(models, v, t, NEAR, FAR, 8, 8, return_rgb=True)
    assert colors.shape == (0, 3) and colors.dtype == torch.uint8
    assert rgb.shape == (0, 3) and rgb.dtype == torch.float32


def test_extract_color_mesh_by_vertex_normals_end_to_end(models, tmp_path):
    from nerf_pl_amd.extract import (color_by_vertex_normals, extract_color_mesh, grid_to_world,
                                     largest_cluster, marching_cubes, sigma_grid, vertex_normals,
                                     write_ply)
    from nerf_pl_amd.rays import pose_spherical
    coarse, fine = models
    N, rng = 16, (-1.2, 1.2)
    sigma = sigma_grid(fine, N, rng, rng, rng)
    thr = float(sigma.median())
    common = dict(N=N, x_range=rng, y_range=rng, z_range=rng, sigma_threshold=thr, N_samples=8)
    torch.manual_seed(3)
    verts, tris, colors = extract_color_mesh(fine, None, None, None, NEAR, **common,
                                             use_vertex_normal=True, model_coarse=coarse, far=FAR,
                                             N_importance=8)
    v0, t0 = marching_cubes(sigma, thr)
    ev, et = largest_cluster(grid_to_world(v0, N, rng, rng, rng), t0)
    n = len(ev)
    assert n > 0 and len(et) > 0
    assert torch.equal(verts, ev) and verts.dtype == torch.float32
    assert torch.equal(tris, et) and tris.dtype == torch.int32
    assert colors.shape == (n, 3) and colors.dtype == torch.uint8
    torch.manual_seed(3)
    want = color_by_vertex_normals([coarse, fine], ev.contiguous(), et, NEAR, FAR, 8, 8)
    assert torch.equal(colors, want)
    for missing in ({"model_coarse": coarse}, {"far": FAR}, {}):
        with pytest.raises(ValueError):
            extract_color_mesh(fine, None, None, None, NEAR, **common, use_vertex_normal=True,
                               **missing)
    # the PLY with the normals the colours were taken along
    p = tmp_path / "mesh.ply"
    write_ply(p, verts, tris, colors, normals=vertex_normals(verts.contiguous(), tris))
    assert p.stat().st_size > n * 27
    # flag off: the new keywords change nothing
    poses = torch.stack([pose_spherical(th, ph, 4.0) for th, ph in ((0.0, -30.0), (120.0, -10.0))])
    g = np.random.Generator(np.random.PCG64(11))
    images = torch.from_numpy(g.integers(0, 256, size=(2, 12, 16, 3)).astype(np.uint8)).to(DEV)
    a = extract_color_mesh(fine, poses, images, 20.0, NEAR, **common)
    b = extract_color_mesh(fine, poses, images, 20.0, NEAR, **common, use_vertex_normal=False,
                           model_coarse=coarse, far=FAR, N_importance=8, near_t=0.5, inward=False)
    assert len(a) == len(b) == 3 and all(torch.equal(x, y) for x, y in zip(a, b))
