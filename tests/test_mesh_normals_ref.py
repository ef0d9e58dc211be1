"""The vertex-normal contract on the CPU: tests/mesh_normals_ref.py (float64
numpy, the kernel's summation order) on the meshes of
tests/mesh_ref.marching_cubes_ref and on hand-made cases.  The device kernels
are compared with the same restatement in tests/test_gpu_mesh_normals.py.

Bounds: the identities are float64 sums of a few hundred to a few thousand
terms, asserted to 1e-12 of the sum of the terms' magnitudes (the project's
bound for float64 sums, tests/test_gpu_mesh.py)."""
import numpy as np
import pytest

import mesh_normals_ref as NR
import mesh_ref as R

DIMS = (9, 11, 13)
CENTRE = (4.0, 5.0, 6.0)
SPHERE_R = 3.5
TORUS = (3.0, 1.5)
# the open sphere of tests/test_gpu_mesh.py, crossing every side of its grid
OPEN_SPHERE = ((7, 8, 9), (3.0, 3.5, 4.0), 4.3)


def _mesh(sigma):
    v, t, _ = R.marching_cubes_ref(sigma, 0.0)
    return v.astype(np.float32), t


@pytest.fixture(scope="module")
def sphere():
    return _mesh(R.sphere_field(DIMS, CENTRE, SPHERE_R))


@pytest.fixture(scope="module")
def torus():
    return _mesh(R.torus_field(DIMS, CENTRE, *TORUS))


@pytest.fixture(scope="module")
def noise():
    return _mesh(R.random_field((5, 7, 9), 1))


@pytest.mark.parametrize("name", ["sphere", "torus", "noise"])
def test_vertex_sums_give_18_signed_volumes(name, request):
    """m_v = sum of (p1 - p0) x (p2 - p0) = p0 x p1 + p1 x p2 + p2 x p0 over the
    triangles at v, and each of a triangle's corners gives n_t . p_k =
    det(p0, p1, p2): sum_v m_v . p_v = 3 sum_t det_t = 18 V, closed or not."""
    v, t = request.getfixturevalue(name)
    m, _ = NR.vertex_sums(v, t)
    p = v.astype(np.float64)
    n = NR.triangle_normals(v, t)
    lhs = (m * p).sum()
    # the terms: every (triangle normal, corner) product, component by component
    scale = sum(np.abs(n * p[t[:, k]]).sum() for k in range(3))
    print(f"{name}: sum m.p = {lhs!r}, 18 V = {18 * R.signed_volume(v, t)!r}, scale {scale:.6g}")
    assert abs(lhs - 18.0 * R.signed_volume(v, t)) <= 1e-12 * scale


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_vertex_sums_of_a_closed_mesh_cancel(name, request):
    v, t = request.getfixturevalue(name)
    assert R.is_closed_oriented(t)
    m, mag = NR.vertex_sums(v, t)
    print(f"{name}: |sum m| = {np.abs(m.sum(0)).max():.3g}, scale {mag.sum():.6g}")
    assert np.abs(m.sum(0)).max() <= 1e-12 * mag.sum()


def test_sphere_normals_point_outwards(sphere):
    """marching_cubes_ref winds from the occupied side to the empty side"""
    v, t = sphere
    q, m, mag = NR.vertex_normals_ref(v, t)
    np.testing.assert_allclose(np.sqrt((q * q).sum(1)), 1.0, rtol=0, atol=1e-15)
    assert ((q * (v.astype(np.float64) - np.asarray(CENTRE))).sum(1) > 0).all()


@pytest.mark.parametrize("field", [R.sphere_field(DIMS, CENTRE, SPHERE_R),
                                   R.torus_field(DIMS, CENTRE, *TORUS),
                                   R.sphere_field(*OPEN_SPHERE)],
                         ids=["sphere", "torus", "open_sphere"])
def test_every_vertex_of_the_smooth_meshes_is_well_conditioned(field):
    """what tests/test_gpu_mesh_normals.py relies on when it asserts a count of 0"""
    v, t = _mesh(field)
    _, m, mag = NR.vertex_normals_ref(v, t)
    assert len(v) > 0 and NR.well_conditioned(m, mag).all()


def test_most_vertices_of_the_random_fields_are_well_conditioned():
    for dims, seed in (((5, 7, 9), 1), ((24, 24, 24), 2)):
        v, t = _mesh(R.random_field(dims, seed))
        _, m, mag = NR.vertex_normals_ref(v, t)
        bad = int((~NR.well_conditioned(m, mag)).sum())
        print(f"random_field({dims}, {seed}): {bad} of {len(v)} below the bound")
        assert bad <= 0.01 * len(v)


@pytest.mark.parametrize("name", sorted(NR.HAND_CASES))
def test_hand_cases(name):
    v, t, want = NR.HAND_CASES[name]()
    q, _, _ = NR.vertex_normals_ref(v, t)
    # exact for the axis-aligned rows; the 1:4 blend is one sqrt and one
    # division away from (4, 0, 1) / sqrt 17
    np.testing.assert_allclose(q, want, rtol=0, atol=4 * np.finfo(np.float64).eps)
    exact = (np.abs(want) == 1).any(1)
    np.testing.assert_array_equal(q[exact], want[exact])


def test_area_weights_are_told_from_uniform_ones():
    v, t, want = NR.two_areas()
    uniform = np.array([1.0, 0.0, 1.0]) / np.sqrt(2.0)
    assert np.abs(want[0] - uniform).max() > 0.2


def test_csr_lists_the_corners_in_order():
    v, t, _ = NR.fan()
    off, inc = NR.csr(t, len(v))
    assert off[0] == 0 and off[-1] == 3 * len(t) and (np.diff(off) >= 0).all()
    assert off[1] - off[0] == 70 and set(np.diff(off)[1:]) == {1, 2}
    for vi in (0, 1, 35, len(v) - 1):
        row = inc[off[vi]:off[vi + 1]]
        assert (np.diff(row) >= 0).all() and all(vi in t[k] for k in row)


def test_normal_rays_restate_the_reference_lines():
    """extract_color_mesh.py:190-193, 200 on torch CPU tensors, verbatim"""
    import torch
    g = np.random.Generator(np.random.PCG64(4))
    verts = g.uniform(-1, 1, size=(300, 3)).astype(np.float32)
    nrm = g.standard_normal((300, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    bounds = np.array([2.0, 6.0])
    for near_t in (1.0, 0.5):
        rays_d = torch.FloatTensor(nrm)
        near = bounds.min() * torch.ones_like(rays_d[:, :1])
        far = bounds.max() * torch.ones_like(rays_d[:, :1])
        rays_o = torch.FloatTensor(verts) - rays_d * near * near_t
        want = torch.cat([rays_o, rays_d, near, far], 1).numpy()
        got = NR.normal_rays_ref(verts, nrm, 2.0, 6.0, near_t, inward=False)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, want)
        flipped = NR.normal_rays_ref(verts, nrm, 2.0, 6.0, near_t, inward=True)
        np.testing.assert_array_equal(flipped[:, 3:6], -want[:, 3:6])
        np.testing.assert_array_equal(flipped, NR.normal_rays_ref(verts, -nrm, 2.0, 6.0, near_t,
                                                                 inward=False))
