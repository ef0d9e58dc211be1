"""Float64 numpy restatements of the two kernels of csrc/mesh_normals.hip
(nerf_pl_amd.extract.vertex_normals / normal_rays) and the hand-made meshes
the CPU and GPU suites share.

``vertex_sums`` adds every triangle's unnormalised normal to its three
vertices with ``np.add.at`` over the corners in ``3t + k`` order -- the
kernel's per-vertex summation order; ``normal_rays_ref`` restates
extract_color_mesh.py:190-193, 200 in float32."""
import numpy as np


def triangle_normals(vertices, triangles):
    """(T,3) float64: (v1 - v0) x (v2 - v0) of the float32 vertices, unnormalised"""
    v = np.asarray(vertices, dtype=np.float32).astype(np.float64)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    a = v[t[:, 1]] - v[t[:, 0]]
    b = v[t[:, 2]] - v[t[:, 0]]
    with np.errstate(all="ignore"):                    # NaN / Inf vertices give NaN normals
        return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1],
                         a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                         a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def vertex_sums(vertices, triangles):
    """``(m (V,3), mag (V,))``: per vertex the sum of its triangles' normals and
    the sum of their Euclidean norms (what the sum could have been without
    cancellation)"""
    n_v = len(vertices)
    t = np.asarray(triangles, dtype=np.int64).reshape(-1, 3)
    n = triangle_normals(vertices, t)
    m = np.zeros((n_v, 3))
    mag = np.zeros(n_v)
    with np.errstate(all="ignore"):
        np.add.at(m, t.reshape(-1), np.repeat(n, 3, axis=0))
        np.add.at(mag, t.reshape(-1), np.repeat(np.sqrt((n * n).sum(1)), 3))
    return m, mag


def vertex_normals_ref(vertices, triangles):
    """``(normals (V,3) float64, m, mag)``: m / |m|, a NaN quotient -> (0, 0, 1)"""
    m, mag = vertex_sums(vertices, triangles)
    with np.errstate(all="ignore"):
        nrm = np.sqrt(m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1] + m[:, 2] * m[:, 2])
        q = m / nrm[:, None]
    q[np.isnan(q).any(1)] = (0.0, 0.0, 1.0)
    return q, m, mag


def well_conditioned(m, mag):
    """vertices whose sum kept at least 1e-6 of its terms' magnitude"""
    with np.errstate(all="ignore"):
        return np.sqrt((m * m).sum(1)) >= 1e-6 * mag


def csr(triangles, n_vertices):
    """``(inc_offsets (V+1) int64, inc_tris (3T) int32)``: per vertex the
    triangles that list it, in ascending corner index"""
    flat = np.asarray(triangles, dtype=np.int64).reshape(-1)
    order = np.argsort(flat, kind="stable")
    offsets = np.zeros(n_vertices + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(flat, minlength=n_vertices))
    return offsets, (order // 3).astype(np.int32)


def normal_rays_ref(vertices, normals, near, far, near_t=1.0, inward=True):
    """(V,8) float32 [o, d, near, far]: d = float32(normal) (negated when
    ``inward``), o = v - (d * near) * near_t, every step rounded to float32"""
    v = np.asarray(vertices, dtype=np.float32)
    d = np.asarray(normals, dtype=np.float64).astype(np.float32)
    if inward:
        d = -d
    near, far, near_t = np.float32(near), np.float32(far), np.float32(near_t)
    o = (v - ((d * near).astype(np.float32) * near_t).astype(np.float32)).astype(np.float32)
    n = len(v)
    return np.concatenate([o, d, np.full((n, 1), near, np.float32),
                           np.full((n, 1), far, np.float32)], 1)


# ---------------------------------------------------------------------------
# hand-made meshes: name -> (vertices (V,3) float32, triangles (T,3) int32,
# the exact normals (V,3) or None)
# ---------------------------------------------------------------------------
UP = (0.0, 0.0, 1.0)


def one_triangle():
    v = np.array([[1, 1, 1], [3, 1, 1], [1, 4, 1]], dtype=np.float32)
    return v, np.array([[0, 1, 2]], dtype=np.int32), np.array([UP] * 3)


def two_areas():
    """areas 1 (normal +z) and 4 (normal +x), planes at a right angle, sharing
    the edge 0-1: the shared vertices blend 1:4 by area -- uniform weights
    would give (1, 0, 1) / sqrt 2, and so would angle weights at vertex 0
    (both corners are right angles)"""
    v = np.array([[0, 0, 0], [0, 2, 0], [-1, 0, 0], [0, 0, -4]], dtype=np.float32)
    t = np.array([[0, 1, 2], [0, 3, 1]], dtype=np.int32)
    s = np.array([4.0, 0.0, 1.0]) / np.sqrt(17.0)
    return v, t, np.array([s, s, UP, (1.0, 0.0, 0.0)])


def zero_area():
    v = np.array([[0, 0, 0], [1, 2, 3], [2, 4, 6]], dtype=np.float32)
    return v, np.array([[0, 1, 2]], dtype=np.int32), np.array([UP] * 3)


def unreferenced():
    v = np.array([[9, 9, 9], [0, 0, 0], [0, 0, 2], [0, 3, 0], [5, 5, 5]], dtype=np.float32)
    return v, np.array([[1, 2, 3]], dtype=np.int32), np.array(
        [UP, (-1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), (-1.0, 0.0, 0.0), UP])


def fan(n_tris=70):
    """an open fan of ``n_tris`` triangles around vertex 0 (valence above one
    wave of 64); the rim vertices have valence 1 (the two ends) or 2"""
    g = np.random.Generator(np.random.PCG64(70))
    ang = np.linspace(0.0, 1.9 * np.pi, n_tris + 1)
    r = g.uniform(0.8, 1.3, size=n_tris + 1)
    rim = np.stack([r * np.cos(ang), r * np.sin(ang), g.uniform(-0.2, 0.2, size=n_tris + 1)], 1)
    v = np.concatenate([[[0.0, 0.0, 0.4]], rim]).astype(np.float32)
    t = np.array([[0, i + 1, i + 2] for i in range(n_tris)], dtype=np.int32)
    return v, t, None


def strip(n_vertices):
    """a zigzag triangle strip, consistently wound"""
    g = np.random.Generator(np.random.PCG64(n_vertices))
    i = np.arange(n_vertices)
    v = np.stack([0.5 * i, (i % 2).astype(np.float64), g.uniform(-0.3, 0.3, size=n_vertices)],
                 1).astype(np.float32)
    t = np.array([[k, k + 1, k + 2] if k % 2 == 0 else [k + 1, k, k + 2]
                  for k in range(n_vertices - 2)], dtype=np.int32)
    return v, t, None


HAND_CASES = {"one_triangle": one_triangle, "two_areas": two_areas, "zero_area": zero_area,
              "unreferenced": unreferenced}
