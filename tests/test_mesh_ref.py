"""The marching-cubes contract on the CPU: tests/mesh_ref.marching_cubes_ref
(float64, plain loops, the package's table) on analytic fields, and the two
torch-only stages of nerf_pl_amd.extract (grid_to_world, largest_cluster) on
CPU tensors.  The device kernels are compared with the same reference in
tests/test_gpu_mesh.py."""
import math

import numpy as np
import pytest
import torch

import mesh_ref as R

DIMS = (9, 11, 13)
CENTRE = (4.0, 5.0, 6.0)
SPHERE_R = 3.5            # |corner - centre| >= 4 on every boundary plane: stays inside
TORUS = (3.0, 1.5)        # ring radius, tube radius: R + r = 4.5 < 5


@pytest.fixture(scope="module")
def sphere():
    s = R.sphere_field(DIMS, CENTRE, SPHERE_R)
    return (s,) + R.marching_cubes_ref(s, 0.0)


@pytest.fixture(scope="module")
def torus():
    s = R.torus_field(DIMS, CENTRE, *TORUS)
    return (s,) + R.marching_cubes_ref(s, 0.0)


@pytest.fixture(scope="module")
def noise():
    s = R.random_field((8, 8, 8), seed=5)
    return (s,) + R.marching_cubes_ref(s, 0.0)


@pytest.mark.parametrize("name", ["sphere", "torus", "noise"])
def test_one_vertex_per_sign_changing_edge(name, request):
    s, v, t, owners = request.getfixturevalue(name)
    if name == "noise":
        assert np.abs(s).min() >= np.float32(1e-3)      # kept away from the threshold
    assert len(v) == R.count_sign_changes(s, 0.0) > 0
    assert len(t) > 0 and t.min() == 0 and t.max() == len(v) - 1
    # ordering contract: (C-order point, axis) ascending; the vertex sits on its edge
    key = ((owners[:, 0] * s.shape[1] + owners[:, 1]) * s.shape[2] + owners[:, 2]) * 3 + owners[:, 3]
    assert (np.diff(key) > 0).all()
    d = v - owners[:, :3]
    for a in range(3):
        on = owners[:, 3] == a
        assert (d[on][:, a] >= 0).all() and (d[on][:, a] <= 1).all()
        assert (np.delete(d[on], a, axis=1) == 0).all()


@pytest.mark.parametrize("name,chi", [("sphere", 2), ("torus", 0)])
def test_closed_surface_topology(name, chi, request):
    s, v, t, _ = request.getfixturevalue(name)
    assert not R.touches_boundary(s, 0.0)
    assert R.is_closed_oriented(t)
    assert R.euler_characteristic(len(v), t) == chi


def test_open_surface_has_its_border_on_the_grid_boundary(noise):
    s, v, t, _ = noise
    c = R.directed_edge_counts(t)
    assert all(n == 1 for n in c.values())
    hi = np.asarray(s.shape) - 1
    for (a, b) in c:
        if (b, a) not in c:          # a border edge: both ends in one boundary plane
            both = ((v[a] == 0) & (v[b] == 0)) | ((v[a] == hi) & (v[b] == hi))
            assert both.any(), (a, b, v[a], v[b])


def test_sphere_volume_is_positive_and_within_the_discretisation_bound(sphere):
    """The field r - |x - c| is 1-Lipschitz and every triangle lies in a cell
    with corners on both sides, hence within one cell diagonal sqrt(3) h
    (h = 1) of a zero of the field: the surface stays in the shell
    r - sqrt(3) h <= |x - c| <= r + sqrt(3) h.  It is closed, oriented outwards
    (positive volume) and separates the occupied grid points from the empty
    ones, so its volume lies between the two balls' volumes."""
    s, v, t, _ = sphere
    vol = R.signed_volume(v, t)
    h = 1.0
    lo = 4 * math.pi * (SPHERE_R - math.sqrt(3) * h) ** 3 / 3
    hi = 4 * math.pi * (SPHERE_R + math.sqrt(3) * h) ** 3 / 3
    assert vol > 0
    assert lo <= vol <= hi, (lo, vol, hi)
    # the sharper one-sided fact: |x - c| is convex and every vertex lies on a
    # crossed edge within h of the sphere, so no triangle point leaves r + h
    assert np.linalg.norm(v - np.asarray(CENTRE), axis=1).max() <= SPHERE_R + h
    assert vol <= 4 * math.pi * (SPHERE_R + h) ** 3 / 3


def test_nan_and_ties_follow_the_comparison():
    """sigma == thr and NaN are both 'not below': occupied"""
    s = np.full((2, 2, 2), 1.0, dtype=np.float32)
    s[0, 0, 0] = 0.0                   # the only empty corner
    s[1, 1, 1] = np.nan
    s[1, 0, 0] = 0.5                   # tie with thr = 0.5
    v, t, owners = R.marching_cubes_ref(s, 0.5)
    assert len(v) == 3 and len(t) == 1
    assert v[0].tolist() == [1.0, 0.0, 0.0]      # t = (0.5 - 0) / (0.5 - 0)


# ---------------------------------------------------------------------------
# grid_to_world, largest_cluster (torch only: CPU tensors)
# ---------------------------------------------------------------------------
def test_grid_to_world_reproduces_the_reference_lines():
    from nerf_pl_amd.extract import grid_to_world
    g = np.random.Generator(np.random.PCG64(0))
    N = 37
    vertices = g.uniform(0, N - 1, size=(500, 3)).astype(np.float32)
    xr, yr, zr = (-1.2, 1.1), (-0.7, 0.9), (0.1, 2.3)
    # extract_color_mesh.py:148-154, verbatim arithmetic (mcubes returns float64)
    v_ = (vertices.astype(np.float64) / N).astype(np.float32)
    x_ = (yr[1] - yr[0]) * v_[:, 1] + yr[0]
    y_ = (xr[1] - xr[0]) * v_[:, 0] + xr[0]
    v_[:, 0] = x_
    v_[:, 1] = y_
    v_[:, 2] = (zr[1] - zr[0]) * v_[:, 2] + zr[0]
    got = grid_to_world(torch.from_numpy(vertices), N, xr, yr, zr)
    assert got.dtype == torch.float32
    np.testing.assert_array_equal(got.numpy(), v_)


def _components(n_v, tris):
    """brute-force union-find: component root per triangle"""
    parent = list(range(n_v))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    for a, b, c in tris:
        for x in (b, c):
            ra, rx = find(a), find(x)
            parent[max(ra, rx)] = min(ra, rx)
    return [find(t[0]) for t in tris]


def test_largest_cluster_keeps_the_bigger_sphere():
    from nerf_pl_amd.extract import largest_cluster
    dims = (12, 12, 20)
    s = np.maximum(R.sphere_field(dims, (5.5, 5.5, 5.0), 3.6), R.sphere_field(dims, (5.5, 5.5, 15.0), 2.2))
    v, t, _ = R.marching_cubes_ref(s, 0.0)
    comp = np.asarray(_components(len(v), t.tolist()))
    roots, counts = np.unique(comp, return_counts=True)
    assert len(roots) == 2 and counts[0] != counts[1]
    keep = comp == roots[np.argmax(counts)]
    used = np.zeros(len(v), dtype=bool)
    used[t[keep].reshape(-1)] = True
    v2, t2 = largest_cluster(torch.from_numpy(v.astype(np.float32)), torch.from_numpy(t))
    assert t2.dtype == torch.int32
    np.testing.assert_array_equal(v2.numpy(), v.astype(np.float32)[used])
    np.testing.assert_array_equal(t2.numpy(), (np.cumsum(used) - 1)[t[keep]])
    assert R.is_closed_oriented(t2.numpy()) and R.euler_characteristic(len(v2), t2.numpy()) == 2
    assert R.signed_volume(v2.numpy(), t2.numpy()) > 4 * math.pi * 2.2 ** 3 / 3 * 1.5


def test_largest_cluster_tie_and_compaction():
    """two tetrahedra of four triangles each: the one holding triangle 0 wins
    although its vertex indices are the higher ones; unreferenced vertices
    (0, 5, 10) and the loser's vertices go, order kept"""
    from nerf_pl_amd.extract import largest_cluster
    tet = [(0, 1, 2), (0, 3, 1), (1, 3, 2), (0, 2, 3)]
    hi = [6, 7, 8, 9]        # first in triangle order
    lo = [1, 2, 3, 4]
    tris = [tuple(hi[i] for i in t) for t in tet[:2]] + [tuple(lo[i] for i in t) for t in tet] + \
        [tuple(hi[i] for i in t) for t in tet[2:]]
    v = torch.arange(11 * 3, dtype=torch.float32).reshape(11, 3)
    v2, t2 = largest_cluster(v, torch.tensor(tris, dtype=torch.int32))
    np.testing.assert_array_equal(v2.numpy(), v.numpy()[hi])
    np.testing.assert_array_equal(t2.numpy(), np.asarray(tet, dtype=np.int32))
    # one more triangle on the other piece breaks the tie
    v3, t3 = largest_cluster(v, torch.tensor(tris + [(1, 2, 5)], dtype=torch.int32))
    np.testing.assert_array_equal(v3.numpy(), v.numpy()[[1, 2, 3, 4, 5]])
    assert len(t3) == 5
    # a long chain needs many rounds of hooking and jumping
    n = 300
    strip = torch.tensor([(i, i + 1, i + 2) for i in range(n)], dtype=torch.int32)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0))
    v4, t4 = largest_cluster(torch.zeros(n + 2, 3), strip[perm])
    assert len(v4) == n + 2 and torch.equal(t4, strip[perm])
    e = largest_cluster(torch.zeros(4, 3), torch.zeros(0, 3, dtype=torch.int32))
    assert e[0].shape == (0, 3) and e[1].shape == (0, 3)
