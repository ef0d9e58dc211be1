"""The mesh-extraction kernels (csrc/mesh.hip) and nerf_pl_amd.extract on the
device against the float64 restatements of tests/mesh_ref.py.

Bounds (none taken from the kernels' output):
  * marching cubes: triangles and V equal as integers; a vertex coordinate is
    within 2 ulp_fp32(max Di) of the float64 reference -- t = (thr - s0) /
    (s1 - s0) takes three float32 roundings (<= 3 * 2^-24 on t <= 1) and
    i + t one more;
  * view kernel: ray rows and depth within 4 float32 ulp of the float64
    reference, colours within 255 * 4 * ulp_fp32(max(W, H)) (2 ulp of
    coordinate error per axis times the steepest bilinear slope, 255 per pixel);
  * fusion: the float64 sums equal the reference to 1e-12 relative, given the
    same depth, colour and opacity arrays.
"""
import math

import numpy as np
import pytest
import torch

import mesh_ref as R
from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)


def _mc(sigma, thr):
    from nerf_pl_amd.extract import marching_cubes
    v, t = marching_cubes(torch.from_numpy(np.ascontiguousarray(sigma)).to(DEV), thr)
    assert v.dtype == torch.float32 and t.dtype == torch.int32
    assert v.dim() == 2 and v.shape[1] == 3 and t.dim() == 2 and t.shape[1] == 3
    return v.cpu().numpy(), t.cpu().numpy()


def _check_against_ref(sigma, thr):
    v, t = _mc(sigma, thr)
    rv, rt, owners = R.marching_cubes_ref(sigma, thr)
    assert len(v) == len(rv) == R.count_sign_changes(sigma, thr)
    np.testing.assert_array_equal(t, rt)
    tol = 2 * R.ulp32(max(sigma.shape))
    both_nan = np.isnan(v) & np.isnan(rv)
    assert (both_nan | (np.abs(v - rv) <= tol)).all(), np.nanmax(np.abs(v - rv))
    # the owning edge, exactly: off-axis coordinates are the owner's, the axis
    # coordinate lies on the edge (floor, or the far end when t rounds to 1)
    for a in range(3):
        on = owners[:, 3] == a
        p = owners[on][:, :3].astype(np.float64)
        g = v[on].astype(np.float64)
        off = [x for x in range(3) if x != a]
        np.testing.assert_array_equal(g[:, off], p[:, off])
        ga = g[:, a]
        ok = np.isnan(ga) | (np.floor(ga) == p[:, a]) | (ga == p[:, a] + 1)
        assert ok.all()
    return v, t


def test_marching_cubes_one_cell_all_256_cases():
    b = np.arange(8)
    for case in range(256):
        empty = (case >> b) & 1
        s = np.where(empty, -(0.5 + 0.07 * b), 1.0 + 0.1 * b).astype(np.float32)
        # corner b sits at offset (b & 1, b >> 1 & 1, b >> 2 & 1): axis 0 is the low bit
        s = np.ascontiguousarray(s.reshape(2, 2, 2).transpose(2, 1, 0))
        v, t = _check_against_ref(s, 0.0)
        assert len(v) == sum(((case >> i) & 1) != ((case >> j) & 1)
                             for i in range(8) for j in range(i + 1, 8)
                             if bin(i ^ j).count("1") == 1)


@pytest.mark.parametrize("dims,seed", [((5, 7, 9), 1), ((24, 24, 24), 2), ((2, 9, 33), 3),
                                       ((33, 2, 3), 4)])
def test_marching_cubes_random_fields(dims, seed):
    v, t = _check_against_ref(R.random_field(dims, seed), 0.0)
    assert len(t) > 0


def test_marching_cubes_surface_crossing_every_side():
    s = R.sphere_field((7, 8, 9), (3.0, 3.5, 4.0), 4.3)
    b = s < 0
    for ax in range(3):
        for side in (0, -1):
            f = np.take(b, side, axis=ax)
            assert f.any() and not f.all()
    _check_against_ref(s, 0.0)


def test_marching_cubes_nan_and_exact_ties():
    s = R.random_field((5, 7, 9), 7)
    g = np.random.Generator(np.random.PCG64(0))
    idx = g.permutation(s.size)
    thr = 0.25
    s.reshape(-1)[idx[:25]] = np.nan
    s.reshape(-1)[idx[25:60]] = np.float32(thr)
    v, t = _check_against_ref(s, thr)
    assert np.isnan(v).any() and len(t) > 0


def test_marching_cubes_misses_the_grid():
    s = R.random_field((5, 7, 9), 1)
    for thr in (float(s.max()) + 1.0, float(s.min()) - 1.0):
        v, t = _mc(s, thr)
        assert v.shape == (0, 3) and t.shape == (0, 3)
    with pytest.raises(ValueError):
        _mc(np.zeros((1, 4, 4), np.float32), 0.0)


def test_marching_cubes_is_deterministic():
    s = R.random_field((24, 24, 24), 2)
    a, b = _mc(s, 0.0), _mc(s, 0.0)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_marching_cubes_topology_on_the_device():
    dims, c = (9, 11, 13), (4.0, 5.0, 6.0)
    v, t = _mc(R.sphere_field(dims, c, 3.5), 0.0)
    assert R.is_closed_oriented(t) and R.euler_characteristic(len(v), t) == 2
    vol = R.signed_volume(v, t)
    # the shell bound of tests/test_mesh_ref.py: within sqrt(3) cells of the sphere
    assert 4 * math.pi * (3.5 - math.sqrt(3)) ** 3 / 3 <= vol <= 4 * math.pi * (3.5 + math.sqrt(3)) ** 3 / 3
    v, t = _mc(R.torus_field(dims, c, 3.0, 1.5), 0.0)
    assert R.is_closed_oriented(t) and R.euler_characteristic(len(v), t) == 0
    assert R.signed_volume(v, t) > 0


# ---------------------------------------------------------------------------
# the two view kernels
# ---------------------------------------------------------------------------
W, H, FOCAL, NEAR = 16, 12, 20.0, 2.0


def _views():
    from nerf_pl_amd.rays import pose_spherical
    poses = np.stack([pose_spherical(th, ph, 4.0).numpy() for th, ph in
                      ((0.0, -30.0), (120.0, -10.0), (250.0, -60.0))]).astype(np.float64)
    g = np.random.Generator(np.random.PCG64(11))
    images = g.integers(0, 256, size=(3, H, W, 3)).astype(np.uint8)
    return poses, images


def _vertices(n, poses):
    g = np.random.Generator(np.random.PCG64(n))
    v = g.uniform(-0.25, 0.25, size=(n, 3))
    if n >= 16:
        # off the image on each side of each view, and behind the first camera
        for k, pose in enumerate(poses):
            right, up, o = pose[:, 0], pose[:, 1], pose[:, 3]
            v[4 * k + 0] = 3.0 * right
            v[4 * k + 1] = -3.0 * right
            v[4 * k + 2] = 3.0 * up
            v[4 * k + 3] = -3.0 * up
        v[12] = 1.5 * poses[0][:, 3]
        v[13] = 0.0                                   # the image centre
    return v.astype(np.float32)


def _ulps(got, ref):
    """|got - ref| in units of float32 spacing at |ref|"""
    ref = np.asarray(ref, dtype=np.float64)
    return np.abs(np.asarray(got, dtype=np.float64) - ref) / np.spacing(
        np.maximum(np.abs(ref), np.finfo(np.float32).tiny).astype(np.float32)).astype(np.float64)


def _opacity(n, view):
    g = np.random.Generator(np.random.PCG64(100 + view))
    o = g.uniform(0, 1, size=n).astype(np.float32)
    special = [np.nan, np.float32(0.2), np.nextafter(np.float32(0.2), np.float32(0)),
               np.nextafter(np.float32(0.2), np.float32(1)), 0.0, 1.0]
    o[:min(n, len(special))] = special[:n]
    return np.roll(o, view)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000])
def test_view_kernels(n):
    from nerf_pl_amd.extract import view_fuse, view_rays
    poses, images = _views()
    verts = _vertices(n, poses)
    dv = torch.from_numpy(verts).to(DEV)
    dimg = torch.from_numpy(images).to(DEV)
    csum = torch.zeros(n, 3, dtype=torch.float64, device=DEV)
    wsum = torch.zeros(n, dtype=torch.float64, device=DEV)
    rc, rw = np.zeros((n, 3)), np.zeros(n)
    outside = np.zeros(4, dtype=bool)
    behind = False
    for k in range(3):
        depth, pix, colour, rays = view_rays(dv, poses[k], FOCAL, NEAR, dimg[k])
        ref = R.view_rays(verts, poses[k], FOCAL, W, H, NEAR, images[k])
        d, p, c, r = (x.cpu().numpy() for x in (depth, pix, colour, rays))
        assert d.dtype == np.float64 and p.dtype == c.dtype == r.dtype == np.float32
        assert _ulps(d, ref["depth"]).max() <= 4
        assert _ulps(r, ref["rays"]).max() <= 4
        assert (p[:, 0] >= 0).all() and (p[:, 0] <= W - 1).all()
        assert (p[:, 1] >= 0).all() and (p[:, 1] <= H - 1).all()
        assert np.abs(p - ref["pix"]).max() <= 2 * R.ulp32(max(W, H))
        assert np.abs(c - ref["colour"]).max() <= 255 * 4 * R.ulp32(max(W, H))
        outside |= np.array([(ref["pix"][:, 0] == 0).any(), (ref["pix"][:, 0] == W - 1).any(),
                             (ref["pix"][:, 1] == 0).any(), (ref["pix"][:, 1] == H - 1).any()])
        behind |= bool((ref["depth"] < 0).any())
        # the fusion, on the kernel's own depth and colour: view order matters,
        # so the sums are compared after every view
        o = _opacity(n, k)
        view_fuse(depth, colour, torch.from_numpy(o).to(DEV), 0.2, csum, wsum)
        rc, rw = R.fuse(d, c, o, 0.2, rc, rw)
        scale_c = np.abs(rc).max() + 255 * np.abs(rw).max()
        np.testing.assert_allclose(csum.cpu().numpy(), rc, rtol=1e-12, atol=1e-12 * scale_c)
        np.testing.assert_allclose(wsum.cpu().numpy(), rw, rtol=1e-12, atol=1e-12 * np.abs(rw).max())
    if n >= 16:
        assert outside.all() and behind


# ---------------------------------------------------------------------------
# end to end
# ---------------------------------------------------------------------------
def test_extract_color_mesh_end_to_end(tmp_path):
    from nerf_pl_amd import NeRF
    from nerf_pl_amd.extract import (extract_color_mesh, grid_to_world, largest_cluster,
                                     marching_cubes, sigma_grid, write_ply)
    model = NeRF().to(DEV)
    model.load_state_dict(O.make_params(1, sigma_bias=0.5))
    N, rng = 16, (-1.2, 1.2)
    poses, images = _views()
    sigma = sigma_grid(model, N, rng, rng, rng)
    thr = float(sigma.median())
    cap = {}
    verts, tris, colors, colours64, opac = extract_color_mesh(
        model, torch.from_numpy(poses), torch.from_numpy(images).to(DEV), FOCAL, NEAR, N=N,
        x_range=rng, y_range=rng, z_range=rng, sigma_threshold=thr, N_samples=8,
        return_opacity=True, _capture=cap)
    # the mesh: marching cubes as in the reference run on the package's own grid ...
    _check_against_ref(sigma.cpu().numpy(), thr)
    v0, t0 = marching_cubes(sigma, thr)
    assert len(t0) > 0
    # ... then the two torch stages, which the CPU suite pins, on CPU tensors
    ev, et = largest_cluster(grid_to_world(v0.cpu(), N, rng, rng, rng), t0.cpu())
    assert torch.equal(tris.cpu(), et) and tris.dtype == torch.int32
    assert torch.equal(verts.cpu(), ev)
    n = len(ev)
    assert 0 < n <= len(v0) and opac.shape == (3, n) and colours64.shape == (n, 3)
    assert colours64.dtype == torch.float64 and colors.dtype == torch.uint8
    # colours: the float64 reference fed with the returned opacities (occlusion
    # flips cannot enter); all weights are positive here (the cameras sit
    # outside the grid), so the fused colour is a convex combination and
    # inherits the per-view colour bound
    vn = ev.numpy()
    rc, rw = np.zeros((n, 3)), np.zeros(n)
    for k in range(3):
        ref = R.view_rays(vn, poses[k], FOCAL, W, H, NEAR, images[k])
        assert (ref["depth"] > 0).all()
        assert _ulps(cap["rays"][k].cpu().numpy(), ref["rays"]).max() <= 4
        rc, rw = R.fuse(ref["depth"], ref["colour"], opac[k].cpu().numpy(), 0.2, rc, rw)
    want = rc / rw[:, None]
    assert np.abs(colours64.cpu().numpy() - want).max() <= 255 * 4 * R.ulp32(max(W, H))
    np.testing.assert_array_equal(colors.cpu().numpy(), colours64.cpu().numpy().astype(np.uint8))
    # PLY round trip
    p = tmp_path / "mesh.ply"
    write_ply(p, verts, tris, colors)
    _, pv, pc, pt = R.read_ply(p)
    np.testing.assert_array_equal(pv, verts.cpu().numpy())
    np.testing.assert_array_equal(pc, colors.cpu().numpy())
    np.testing.assert_array_equal(pt, tris.cpu().numpy())


def test_largest_cluster_on_the_device():
    from nerf_pl_amd.extract import largest_cluster, marching_cubes
    dims = (12, 12, 20)
    s = np.maximum(R.sphere_field(dims, (5.5, 5.5, 5.0), 3.6),
                   R.sphere_field(dims, (5.5, 5.5, 15.0), 2.2))
    v, t = marching_cubes(torch.from_numpy(s).to(DEV), 0.0)
    gv, gt = largest_cluster(v, t)
    cv, ct = largest_cluster(v.cpu(), t.cpu())
    assert gv.device.type == "cuda" and torch.equal(gv.cpu(), cv) and torch.equal(gt.cpu(), ct)
    assert 0 < len(ct) < len(t)
    assert R.is_closed_oriented(ct.numpy()) and R.euler_characteristic(len(cv), ct.numpy()) == 2
