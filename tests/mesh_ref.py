"""CPU restatements of the mesh-extraction stages (nerf_pl_amd/extract.py,
csrc/mesh.hip) for the tests: marching cubes in float64 with plain loops and
the package's own table, the per-view projection / colour / ray and the
colour fusion of extract_color_mesh.py:221-277 in float64 numpy, a PLY
reader, and the topology checks shared by the CPU and GPU suites."""
import numpy as np

from nerf_pl_amd.mesh_tables import MC_CORNERS, MC_EDGE_CORNERS, MC_TRI_TABLE


def ulp32(x):
    """spacing of float32 at magnitude x"""
    return float(np.spacing(np.float32(x)))


def marching_cubes_ref(sigma, threshold):
    """(vertices (V,3) float64, triangles (T,3) int32, owners (V,4) int) of
    the float32 grid ``sigma``; the threshold is rounded to float32 like the
    kernel's argument, everything after that is float64.  Ordering contract of
    extract.marching_cubes: vertices by (C-order point, axis), triangles by
    (C-order cell, table position).  ``owners`` rows are (i, j, k, axis)."""
    s = np.asarray(sigma, dtype=np.float32)
    thr = np.float32(threshold)
    D = s.shape
    below = s < thr                                   # NaN: False
    index = {}
    verts, owners = [], []
    for i in range(D[0]):
        for j in range(D[1]):
            for k in range(D[2]):
                p = (i, j, k)
                for a in range(3):
                    if p[a] + 1 >= D[a]:
                        continue
                    q = list(p)
                    q[a] += 1
                    q = tuple(q)
                    if below[p] == below[q]:
                        continue
                    s0, s1 = float(s[p]), float(s[q])
                    with np.errstate(all="ignore"):
                        t = (np.float64(thr) - s0) / (np.float64(s1) - s0)
                    v = [float(i), float(j), float(k)]
                    v[a] += t
                    index[(p, a)] = len(verts)
                    verts.append(v)
                    owners.append((i, j, k, a))
    tris = []
    for i in range(D[0] - 1):
        for j in range(D[1] - 1):
            for k in range(D[2] - 1):
                case = 0
                for b, (di, dj, dk) in enumerate(MC_CORNERS):
                    case |= int(below[i + di, j + dj, k + dk]) << b
                row = MC_TRI_TABLE[case]
                for n in range(0, len(row) - 1, 3):
                    if row[n] < 0:
                        break
                    tri = []
                    for e in row[n:n + 3]:
                        di, dj, dk = MC_CORNERS[MC_EDGE_CORNERS[e][0]]
                        tri.append(index[((i + di, j + dj, k + dk), e // 4)])
                    tris.append(tri)
    return (np.asarray(verts, dtype=np.float64).reshape(-1, 3),
            np.asarray(tris, dtype=np.int32).reshape(-1, 3),
            np.asarray(owners, dtype=np.int64).reshape(-1, 4))


def count_sign_changes(sigma, threshold):
    """number of grid edges whose endpoints lie on different sides (numpy only)"""
    b = np.asarray(sigma, dtype=np.float32) < np.float32(threshold)
    return int((b[1:] != b[:-1]).sum() + (b[:, 1:] != b[:, :-1]).sum()
               + (b[:, :, 1:] != b[:, :, :-1]).sum())


def directed_edge_counts(triangles):
    """{(a, b): occurrences} over the directed edges of every triangle"""
    out = {}
    for t in np.asarray(triangles).tolist():
        for a, b in ((t[0], t[1]), (t[1], t[2]), (t[2], t[0])):
            out[(a, b)] = out.get((a, b), 0) + 1
    return out


def is_closed_oriented(triangles):
    """every undirected edge is used by exactly two triangles, once in each direction"""
    c = directed_edge_counts(triangles)
    return all(n == 1 and c.get((b, a), 0) == 1 for (a, b), n in c.items())


def euler_characteristic(n_vertices, triangles):
    c = directed_edge_counts(triangles)
    edges = {(min(a, b), max(a, b)) for a, b in c}
    return n_vertices - len(edges) + len(triangles)


def signed_volume(vertices, triangles):
    v = np.asarray(vertices, dtype=np.float64)
    t = np.asarray(triangles)
    return float(np.einsum("ij,ij->i", v[t[:, 0]], np.cross(v[t[:, 1]], v[t[:, 2]])).sum() / 6.0)


def touches_boundary(sigma, threshold):
    """does a crossed edge lie in a boundary plane of the grid?"""
    b = np.asarray(sigma, dtype=np.float32) < np.float32(threshold)
    for ax in range(3):
        for side in (0, -1):
            f = np.take(b, side, axis=ax)
            if f.any() and not f.all():
                return True
    return False


def sphere_field(dims, centre, radius):
    """sigma = radius - |x - centre|: occupied (>= 0) inside the sphere"""
    g = np.stack(np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij"), -1)
    return (radius - np.linalg.norm(g - np.asarray(centre, dtype=np.float64), axis=-1)).astype(
        np.float32)


def torus_field(dims, centre, R, r):
    """sigma = r - distance to the circle of radius R in the plane of axes (1, 2)"""
    g = np.stack(np.meshgrid(*[np.arange(d, dtype=np.float64) for d in dims], indexing="ij"), -1)
    g = g - np.asarray(centre, dtype=np.float64)
    q = np.sqrt(g[..., 1] ** 2 + g[..., 2] ** 2) - R
    return (r - np.sqrt(q ** 2 + g[..., 0] ** 2)).astype(np.float32)


def random_field(dims, seed, threshold=0.0, margin=1e-3):
    """seeded low-frequency field: a coarse random lattice, trilinearly
    upsampled; values closer than ``margin`` to the threshold are pushed away"""
    g = np.random.Generator(np.random.PCG64(seed))
    coarse = g.standard_normal((3, 3, 3))
    ax = [np.linspace(0, 2, d) for d in dims]
    out = np.zeros(dims)
    I, J, K = np.meshgrid(*ax, indexing="ij")
    i0, j0, k0 = (np.minimum(x.astype(int), 1) for x in (I, J, K))
    fi, fj, fk = I - i0, J - j0, K - k0
    for di in (0, 1):
        for dj in (0, 1):
            for dk in (0, 1):
                w = (fi if di else 1 - fi) * (fj if dj else 1 - fj) * (fk if dk else 1 - fk)
                out += w * coarse[i0 + di, j0 + dj, k0 + dk]
    near = np.abs(out - threshold) < margin
    out[near] = threshold + np.where(out[near] >= threshold, margin, -margin)
    return out.astype(np.float32)


# ---------------------------------------------------------------------------
# vertex colours
# ---------------------------------------------------------------------------
def w2c_of(pose):
    """(3,4) float64 world-to-camera of a (3,4) camera-to-world pose (line 220-221)"""
    c2w = np.concatenate([np.asarray(pose, dtype=np.float64), np.array([[0.0, 0.0, 0.0, 1.0]])], 0)
    return np.linalg.inv(c2w)[:3]


def bilinear(image, px, py):
    """exact bilinear sample (float64) of image (H,W,3) uint8 at float32 pixel
    coordinates already inside the image; neighbours clamped at the border"""
    H, W = image.shape[:2]
    px = px.astype(np.float64)
    py = py.astype(np.float64)
    x0 = np.floor(px).astype(np.int64)
    y0 = np.floor(py).astype(np.int64)
    x1 = np.minimum(x0 + 1, W - 1)
    y1 = np.minimum(y0 + 1, H - 1)
    ax = (px - x0)[:, None]
    ay = (py - y0)[:, None]
    im = image.astype(np.float64)
    return ((1 - ax) * (1 - ay) * im[y0, x0] + ax * (1 - ay) * im[y0, x1]
            + (1 - ax) * ay * im[y1, x0] + ax * ay * im[y1, x1])


def view_rays(vertices, pose, focal, W, H, near, image):
    """lines 221-262 for one view, float64: dict depth (n), pix (n,2) float32,
    colour (n,3), rays (n,8).  ``vertices`` float32 (n,3)."""
    v32 = np.asarray(vertices, dtype=np.float32)
    n = len(v32)
    K = np.array([[focal, 0, W / 2], [0, focal, H / 2], [0, 0, 1]]).astype(np.float32)
    homo = np.concatenate([v32, np.ones((n, 1))], 1)
    cam = w2c_of(pose) @ homo.T
    cam[1:] *= -1
    img = (K @ cam).T
    depth = img[:, -1:] + 1e-5
    with np.errstate(all="ignore"):
        pix = (img[:, :2] / depth).astype(np.float32)
    pix[:, 0] = np.clip(pix[:, 0], 0, W - 1)
    pix[:, 1] = np.clip(pix[:, 1], 0, H - 1)
    colour = bilinear(np.asarray(image), pix[:, 0], pix[:, 1])
    o = np.asarray(pose, dtype=np.float64)[:, 3].astype(np.float32).astype(np.float64)
    d = v32.astype(np.float64) - o
    d = d / np.linalg.norm(d, axis=-1, keepdims=True)
    rays = np.concatenate([np.broadcast_to(o, (n, 3)), d, np.full((n, 1), np.float32(near),
                                                                   dtype=np.float64),
                           depth.astype(np.float32).astype(np.float64)], 1)
    return dict(depth=depth[:, 0], pix=pix, colour=colour, rays=rays)


def fuse(depth, colour, opacity, occ_threshold, csum, wsum):
    """lines 269-277 for one view: returns the updated (csum (n,3), wsum (n))"""
    o = np.asarray(opacity, dtype=np.float32).copy()
    o[np.isnan(o)] = 0                      # np.nan_to_num(opacity, 1): NaN -> 0
    w = 0.1 / np.asarray(depth, dtype=np.float64) + (o < np.float32(occ_threshold))
    return csum + np.asarray(colour, dtype=np.float64) * w[:, None], wsum + w


# ---------------------------------------------------------------------------
# PLY
# ---------------------------------------------------------------------------
def read_ply(path):
    """(header lines, vertices (V,3) f4, colours (V,3) u1 or None, triangles (T,3) i4)"""
    raw = open(path, "rb").read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    header = raw[:end].decode("ascii").splitlines()
    nv = int([h for h in header if h.startswith("element vertex")][0].split()[-1])
    nf = int([h for h in header if h.startswith("element face")][0].split()[-1])
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    has_colour = "property uchar red" in header
    if has_colour:
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
    vt = np.dtype(fields)
    ft = np.dtype([("n", "u1"), ("idx", "<i4", (3,))])
    assert len(raw) == end + nv * vt.itemsize + nf * ft.itemsize
    v = np.frombuffer(raw, vt, nv, end)
    f = np.frombuffer(raw, ft, nf, end + nv * vt.itemsize)
    assert (f["n"] == 3).all()
    col = np.stack([v["red"], v["green"], v["blue"]], 1) if has_colour else None
    return header, np.stack([v["x"], v["y"], v["z"]], 1), col, f["idx"].copy()
