"""Dense sigma-grid query for mesh extraction (extract_color_mesh.py:114-141).

The reference embeds an N^3 grid chunk by chunk, runs the full fine NeRF with a
zero direction and keeps max(sigma, 0).  Here the sigma-only fused kernel
evaluates the grid with the positional encoding computed in-kernel (sigma does
not depend on the direction, nerf.py:112).

Colour mesh extraction (extract_color_mesh.py:142-297) follows on the device,
without mcubes, open3d, cv2 or plyfile: ``marching_cubes`` ->
``grid_to_world`` -> ``largest_cluster`` -> ``fuse_vertex_colors`` ->
``write_ply``, chained by ``extract_color_mesh`` (kernels: csrc/mesh.hip,
declared in include/nerf_pl_amd_mesh.h).  The ``--use_vertex_normal`` branch
(lines 187-204, 280-281) colours the same mesh from the two networks alone:
``vertex_normals`` -> ``normal_rays`` -> the coarse + fine ``render_rays``,
chained by ``color_by_vertex_normals`` (kernels: csrc/mesh_normals.hip,
declared in include/nerf_pl_amd_mesh_normals.h).  Five parities with the
replaced libraries are *unpinned*, because none of them is available to test
against: PyMCubes' vertex order and winding, open3d's triangle connectivity,
cv2.remap's fixed-point bilinear weights, open3d's vertex-normal rule, and
the side of the surface the reference's normal rays look at (it follows from
PyMCubes' winding); each function says what it does instead.
"""
from __future__ import annotations

import functools

import numpy as np
import torch

from . import _lib_mesh, _lib_mesh_normals, ops
from ._lib import ptr, stream_of
from .mesh_tables import MC_ROW, MC_TRI_TABLE


def grid_points(N, x_range, y_range, z_range, device) -> torch.Tensor:
    """The (N^3, 3) grid in the reference's order (np.meshgrid default 'xy'
    indexing, extract_color_mesh.py:119-123)."""
    x = np.linspace(x_range[0], x_range[1], N)
    y = np.linspace(y_range[0], y_range[1], N)
    z = np.linspace(z_range[0], z_range[1], N)
    return torch.tensor(np.stack(np.meshgrid(x, y, z), -1).reshape(-1, 3), dtype=torch.float32,
                        device=device)


@torch.no_grad()
def query_sigma(model, pts: torch.Tensor) -> torch.Tensor:
    """Raw sigma (n,) of ``model`` (a nerf_pl_amd.NeRF) at points (n,3)."""
    packed, _ = model.packed()
    return ops.sigma_points(packed, pts)


@torch.no_grad()
def sigma_grid(model, N=256, x_range=(-1.2, 1.2), y_range=(-1.2, 1.2), z_range=(-1.2, 1.2)):
    """max(sigma, 0) on the N^3 grid, shape (N, N, N) (extract_color_mesh.py:138-139)."""
    dev = model.flat_params().device
    sigma = query_sigma(model, grid_points(N, x_range, y_range, z_range, dev))
    return torch.clamp_min(sigma, 0).reshape(N, N, N)


# ---------------------------------------------------------------------------
# marching cubes (extract_color_mesh.py:144)
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _tri_table(device_index: int) -> torch.Tensor:
    """MC_TRI_TABLE as int8 (256, MC_ROW), uploaded once per device"""
    t = torch.tensor(MC_TRI_TABLE, dtype=torch.int8)
    assert t.shape == (256, MC_ROW)
    return t.to(torch.device("cuda", device_index))


@torch.no_grad()
def marching_cubes(sigma: torch.Tensor, threshold: float):
    """Indexed isosurface of a float32 device grid ``sigma`` (D0, D1, D2), every
    ``Di >= 2`` and fewer than 2^31 points: ``(vertices (V,3) float32 in
    array-index coordinates, triangles (T,3) int32)`` -- the call
    ``mcubes.marching_cubes(sigma, threshold)`` of extract_color_mesh.py:144.

    Classic marching cubes over the 256-case table of ``mesh_tables``.  A
    corner is *empty* iff ``sigma < threshold`` (a NaN is occupied); a grid
    edge is crossed iff its two corners differ, and carries one vertex, shared
    by every triangle that uses it, at ``p + t e_a`` with
    ``t = (threshold - s0) / (s1 - s0)`` in float32 (``threshold`` rounded to
    float32 first, ``s0`` the value at the edge's lower point ``p``).
    Vertices are ordered by (C-order index of ``p``, axis), triangles by
    (C-order index of the cell over (D0-1, D1-1, D2-1), position in the table
    row); nothing is atomic, so two runs give bit-identical tensors.  Every
    triangle's normal points from the occupied side to the empty side: the
    signed volume of a solid blob is positive.

    Parity with PyMCubes' own vertex order and winding is *unpinned* (the
    library is not available to compare with); the surface is the same
    piecewise-linear isosurface up to the choice on ambiguous faces.

    One host read-back (V, T) sizes the outputs; an isosurface that misses the
    grid returns (0,3) tensors without launching the emit kernels."""
    sigma = ops._dev(sigma, "sigma")
    if sigma.dim() != 3 or min(sigma.shape) < 2:
        raise ValueError(f"sigma: expected (D0, D1, D2) with every Di >= 2, got {tuple(sigma.shape)}")
    if sigma.numel() >= 2 ** 31:
        raise ValueError(f"sigma: {sigma.numel()} points, need fewer than 2^31")
    dev, st = sigma.device, stream_of(sigma.device)
    d0, d1, d2 = sigma.shape
    grid = (ptr(sigma), d0, d1, d2, float(threshold))
    table = _tri_table(dev.index)
    count = torch.empty(sigma.numel(), dtype=torch.int32, device=dev)
    mask = torch.empty(sigma.numel(), dtype=torch.uint8, device=dev)
    tcount = torch.empty((d0 - 1) * (d1 - 1) * (d2 - 1), dtype=torch.int32, device=dev)
    _lib_mesh.call("nr_mc_point_edges", *grid, ptr(count), ptr(mask), st)
    _lib_mesh.call("nr_mc_cell_tris", *grid, ptr(table), ptr(tcount), st)
    vend = torch.cumsum(count, 0, dtype=torch.int64)
    tend = torch.cumsum(tcount, 0, dtype=torch.int64)
    n_v, n_t = torch.stack([vend[-1], tend[-1]]).tolist()
    if n_v == 0 or n_t == 0:
        return (torch.empty(0, 3, device=dev), torch.empty(0, 3, dtype=torch.int32, device=dev))
    if n_v >= 2 ** 31:
        raise ValueError(f"marching_cubes: {n_v} vertices do not fit int32 indices")
    vbase, tbase = vend - count, tend - tcount
    vertices = torch.empty(n_v, 3, device=dev)
    triangles = torch.empty(n_t, 3, dtype=torch.int32, device=dev)
    _lib_mesh.call("nr_mc_vertices", *grid, ptr(mask), ptr(vbase), n_v, ptr(vertices), st)
    _lib_mesh.call("nr_mc_triangles", *grid, ptr(table), ptr(mask), ptr(vbase), ptr(tbase), n_v,
                   n_t, ptr(triangles), st)
    return vertices, triangles


def grid_to_world(vertices: torch.Tensor, N: int, x_range, y_range, z_range) -> torch.Tensor:
    """Array-index vertices -> world coordinates, extract_color_mesh.py:148-154
    with its quirks: the division is by ``N`` (not ``N - 1``), in float64 and
    then rounded to float32; columns 0 and 1 swap (``np.meshgrid``'s 'xy'
    indexing put y on axis 0 of the grid); the affine map runs in float32 with
    the range lengths rounded to float32.  Torch ops, any device."""
    v = (vertices.to(torch.float64) / N).to(torch.float32)

    def f32(s):
        return torch.tensor(s, dtype=torch.float32, device=v.device)

    x = f32(y_range[1] - y_range[0]) * v[:, 1] + f32(y_range[0])
    y = f32(x_range[1] - x_range[0]) * v[:, 0] + f32(x_range[0])
    z = f32(z_range[1] - z_range[0]) * v[:, 2] + f32(z_range[0])
    return torch.stack([x, y, z], 1)


@torch.no_grad()
def largest_cluster(vertices: torch.Tensor, triangles: torch.Tensor):
    """Keep the connected component with the most triangles, drop the
    vertices it does not reference (order kept) and re-index:
    extract_color_mesh.py:166-170.  Two triangles are connected when they
    share a vertex index.  On a tie the component holding the lowest triangle
    index wins, as ``np.argmax`` over clusters numbered by first triangle
    would choose.  Returns ``(vertices, triangles)``.

    Label propagation with pointer jumping in torch ops (any device): every
    vertex starts as its own label; each round hooks the labels of a
    triangle's three vertices onto their minimum and then halves the label
    chains, until every triangle is uniform and every label is a root.

    Parity with open3d's ``cluster_connected_triangles`` is *unpinned*: it
    joins triangles across shared edges, so two pieces that touch in a single
    vertex are one component here and may be two there."""
    n_v, n_t = vertices.shape[0], triangles.shape[0]
    if n_t == 0:
        return vertices[:0], triangles[:0]
    tri = triangles.to(torch.int64)
    flat = tri.reshape(-1)
    label = torch.arange(n_v, device=tri.device)
    while True:
        lt = label[tri]                                  # (T, 3)
        m = lt.min(1).values
        if bool((lt == m[:, None]).all()) and bool((label[label] == label).all()):
            break
        m3 = m[:, None].expand(-1, 3).reshape(-1)
        # hook the three vertices and their current roots onto the minimum
        label = label.scatter_reduce(0, flat, m3, "amin")
        label = label.scatter_reduce(0, lt.reshape(-1), m3, "amin")
        for _ in range(3):
            label = label[label]
    comp = label[tri[:, 0]]
    ids, inverse, counts = torch.unique(comp, return_inverse=True, return_counts=True)
    first = torch.full_like(ids, n_t).scatter_reduce(
        0, inverse, torch.arange(n_t, device=tri.device), "amin")
    best = counts == counts.max()
    winner = torch.where(best, first, torch.full_like(first, n_t)).argmin()
    keep = inverse == winner
    tri = tri[keep]
    used = torch.zeros(n_v, dtype=torch.bool, device=tri.device)
    used[tri.reshape(-1)] = True
    new_index = torch.cumsum(used, 0) - 1
    return vertices[used], new_index[tri].to(triangles.dtype)


# ---------------------------------------------------------------------------
# vertex colours (extract_color_mesh.py:177-284, the colour-average method)
# ---------------------------------------------------------------------------
FUSE_CHUNK = 32768          # vertices per occlusion render (the reference's --chunk)


def view_rays(vertices, pose, focal, near, image):
    """``nr_mesh_view_rays`` for one view: ``pose`` (3,4) camera-to-world
    (host, float64), ``image`` (H,W,3) uint8 on the device.  Returns ``(depth
    (n) float64, pix (n,2), colour (n,3), rays (n,8))``; see
    ``fuse_vertex_colors``."""
    vertices = ops._dev(vertices, "vertices", 3)
    dev, n = vertices.device, vertices.shape[0]
    if image.dtype != torch.uint8 or image.dim() != 3 or image.shape[-1] != 3 \
            or image.device != dev or not image.is_contiguous():
        raise ValueError("image: expected a contiguous (H, W, 3) uint8 tensor on the vertices' device")
    H, W = image.shape[:2]
    pose = np.asarray(pose, dtype=np.float64).reshape(3, 4)
    c2w = np.concatenate([pose, np.array([[0.0, 0.0, 0.0, 1.0]])], 0)
    w2c = np.ascontiguousarray(np.linalg.inv(c2w)[:3])           # line 221
    o = pose[:, 3].astype(np.float32)
    depth = torch.empty(n, dtype=torch.float64, device=dev)
    pix = torch.empty(n, 2, device=dev)
    colour = torch.empty(n, 3, device=dev)
    rays = torch.empty(n, 8, device=dev)
    _lib_mesh.call("nr_mesh_view_rays", ptr(vertices), n, w2c.ctypes.data, float(focal), W, H,
                   float(near), float(o[0]), float(o[1]), float(o[2]), ptr(image), ptr(depth),
                   ptr(pix), ptr(colour), ptr(rays), stream_of(dev))
    return depth, pix, colour, rays


def view_fuse(depth, colour, opacity, occ_threshold, colour_sum, weight_sum) -> None:
    """``nr_mesh_view_fuse``: add one view to the float64 sums, in place."""
    n = depth.shape[0]
    opacity = ops._dev(opacity, "opacity")
    if depth.dtype != torch.float64 or colour_sum.dtype != torch.float64 \
            or weight_sum.dtype != torch.float64:
        raise TypeError("view_fuse: depth and the two sums are float64")
    if colour.shape != (n, 3) or opacity.shape != (n,) or colour_sum.shape != (n, 3) \
            or weight_sum.shape != (n,):
        raise ValueError("view_fuse: shapes disagree")
    if not (depth.is_contiguous() and colour.is_contiguous() and colour_sum.is_contiguous()
            and weight_sum.is_contiguous()):
        raise ValueError("view_fuse: buffers must be contiguous")
    _lib_mesh.call("nr_mesh_view_fuse", ptr(depth), ptr(colour), ptr(opacity), n,
                   float(occ_threshold), ptr(colour_sum), ptr(weight_sum), stream_of(depth.device))


@torch.no_grad()
def fuse_vertex_colors(model_fine, vertices, poses, images, focal, near, N_samples=64,
                       occ_threshold=0.2, white_back=False, return_opacity=False, *,
                       _capture=None):
    """uint8 colours (n,3) of world-space ``vertices`` (n,3) averaged over
    the views ``poses`` (n_views,3,4) camera-to-world / ``images``
    (n_views,H,W,3) uint8 -- extract_color_mesh.py:206-284.

    Per view: the world-to-camera matrix is ``np.linalg.inv`` in float64 on
    the host (line 221); ``nr_mesh_view_rays`` projects every vertex in
    float64, takes ``depth = z + 1e-5``, clips the float32 pixel coordinates
    into the image, samples the colour and builds the ray from the camera to
    the vertex with ``far = depth``; ``render_rays([model_fine], ...,
    N_importance=0, test_time=True)`` gives the opacity accumulated on the
    way, ``FUSE_CHUNK`` vertices at a time; ``nr_mesh_view_fuse`` adds
    ``colour * w`` and ``w = 0.1 / depth + (opacity < occ_threshold)`` to
    float64 sums (a NaN opacity counts as 0: line 270 passes its ``1`` as
    ``copy``).  Views accumulate in order, one thread per vertex, so the
    result is deterministic.  The colour is ``(sum / weight).to(uint8)``.

    The colour sample is the exact bilinear interpolation with float32
    weights and border-clamped neighbours; ``cv2.remap``'s 1/32-pixel
    fixed-point weights and its rounding to uint8 per view are not
    reproduced -- parity *unpinned* (cv2 is not available to compare with).
    The ``--use_vertex_normal`` branch (lines 187-204) is
    ``color_by_vertex_normals``.

    ``return_opacity``: also return the float64 colours before quantisation
    (n,3) and the per-view opacities (n_views, n)."""
    from . import Embedding, render_rays
    vertices = ops._dev(vertices, "vertices", 3)
    dev = vertices.device
    n = vertices.shape[0]
    if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[-1] != 3:
        raise ValueError(f"images: expected (n_views, H, W, 3) uint8, got {tuple(images.shape)} "
                         f"{images.dtype}")
    images = images.to(dev).contiguous()
    n_views = images.shape[0]
    poses64 = np.asarray(torch.as_tensor(poses).detach().cpu().numpy(), dtype=np.float64)
    if poses64.shape != (n_views, 3, 4):
        raise ValueError(f"poses: expected ({n_views}, 3, 4), got {poses64.shape}")
    embeddings = [Embedding(3, 10), Embedding(3, 4)]
    csum = torch.zeros(n, 3, dtype=torch.float64, device=dev)
    wsum = torch.zeros(n, dtype=torch.float64, device=dev)
    opacities = []
    for v in range(n_views):
        depth, _, colour, rays = view_rays(vertices, poses64[v], focal, near, images[v])
        if n:
            opacity = torch.cat([
                render_rays([model_fine], embeddings, rays[i:i + FUSE_CHUNK], N_samples, False, 0,
                            0, 0, FUSE_CHUNK, white_back, test_time=True)["opacity_coarse"]
                for i in range(0, n, FUSE_CHUNK)], 0)
        else:
            opacity = torch.empty(0, device=dev)
        view_fuse(depth, colour, opacity, occ_threshold, csum, wsum)
        if return_opacity:
            opacities.append(opacity)
        if _capture is not None:
            _capture.setdefault("rays", []).append(rays)
    colours64 = csum / wsum[:, None]
    colors = colours64.to(torch.uint8)
    if return_opacity:
        return colors, colours64, (torch.stack(opacities, 0) if opacities
                                   else torch.empty(0, n, device=dev))
    return colors


# ---------------------------------------------------------------------------
# vertex colours along the vertex normals (extract_color_mesh.py:187-204, 280-281)
# ---------------------------------------------------------------------------
def _mesh(vertices, triangles):
    vertices = ops._dev(vertices, "vertices", 3)
    if not isinstance(triangles, torch.Tensor) or triangles.dtype != torch.int32 \
            or triangles.dim() != 2 or triangles.shape[1] != 3 \
            or triangles.device != vertices.device:
        raise ValueError("triangles: expected a (T, 3) int32 tensor on the vertices' device")
    if vertices.dim() != 2:
        raise ValueError(f"vertices: expected (V, 3), got {tuple(vertices.shape)}")
    return vertices, triangles.contiguous()


@torch.no_grad()
def vertex_normals(vertices: torch.Tensor, triangles: torch.Tensor) -> torch.Tensor:
    """Unit vertex normals (V,3) float64 of the indexed device mesh
    ``vertices`` (V,3) float32 / ``triangles`` (T,3) int32 with indices in
    ``[0, V)`` -- ``mesh.compute_vertex_normals()`` of
    extract_color_mesh.py:189.

    A triangle's normal is the unnormalised ``(v1 - v0) x (v2 - v0)`` in
    float64, so the sum over a vertex's triangles is area-weighted; the sum is
    divided by its Euclidean norm, and a NaN quotient -- a zero sum, a vertex
    no triangle lists, a sum holding NaN or Inf from NaN vertices -- becomes
    ``(0, 0, 1)``.  That is open3d's rule as recalled; parity with open3d is
    *unpinned* (the library is not available to compare with).

    The sum is a gather: a stable ``argsort`` of the corner list groups the
    corners by vertex in ascending corner index ``3t + k``, ``bincount`` and
    an exclusive ``cumsum`` give each vertex's row, and one kernel
    (``nr_mesh_vertex_normals``) has one thread per vertex add the cross
    products of its row in that order.  Nothing is atomic, so two runs give
    bit-identical tensors.  With ``marching_cubes``' winding the normals point
    from the occupied side to the empty side."""
    vertices, triangles = _mesh(vertices, triangles)
    dev, n_v, n_t = vertices.device, vertices.shape[0], triangles.shape[0]
    normals = torch.empty(n_v, 3, dtype=torch.float64, device=dev)
    if n_v == 0:
        return normals
    if n_v >= 2 ** 31 or 3 * n_t >= 2 ** 31:
        raise ValueError(f"vertex_normals: {n_v} vertices / {n_t} triangles do not fit int32 "
                         "indices")
    offsets = torch.zeros(n_v + 1, dtype=torch.int64, device=dev)
    inc = None
    if n_t:
        flat = triangles.reshape(-1).to(torch.int64)
        counts = torch.bincount(flat, minlength=n_v)           # raises on a negative index
        if counts.numel() != n_v:
            raise ValueError(f"triangles: vertex index {counts.numel() - 1} for {n_v} vertices")
        offsets[1:] = torch.cumsum(counts, 0)
        inc = (torch.argsort(flat, stable=True) // 3).to(torch.int32)
    _lib_mesh_normals.call("nr_mesh_vertex_normals", ptr(vertices),
                           ptr(triangles) if n_t else None, ptr(offsets),
                           ptr(inc) if n_t else None, n_v, n_t, ptr(normals), stream_of(dev))
    return normals


@torch.no_grad()
def normal_rays(vertices, normals, near, far, near_t=1.0, inward=True) -> torch.Tensor:
    """The rays (V,8) float32 ``[o, d, near, far]`` of
    extract_color_mesh.py:190-193, 200 for ``vertices`` (V,3) float32 and
    ``normals`` (V,3) float64 (``nr_mesh_normal_rays``, float32 in the
    reference's order): ``d = float32(normal)`` and
    ``o = v - d * near * near_t``, so the sample at ``z = near * near_t`` is
    the vertex itself and the ray travels on along ``d``.

    ``inward=True`` negates the normal first.  The reference's ray runs along
    ``+normal``, and the method sees the object's colour only if that
    direction enters the object; ``marching_cubes`` here winds every triangle
    so that the normal points from the occupied side to the empty side, and
    whether PyMCubes does is *unpinned*.  So the default points the ray into
    the occupied side; ``inward=False`` applies the reference's lines to the
    normals as they are."""
    vertices = ops._dev(vertices, "vertices", 3)
    n = vertices.shape[0]
    if not isinstance(normals, torch.Tensor) or normals.dtype != torch.float64 \
            or normals.shape != (n, 3) or normals.device != vertices.device:
        raise ValueError(f"normals: expected a ({n}, 3) float64 tensor on the vertices' device")
    normals = normals.contiguous()
    rays = torch.empty(n, 8, device=vertices.device)
    _lib_mesh_normals.call("nr_mesh_normal_rays", ptr(vertices), ptr(normals), n, float(near),
                           float(far), float(near_t), int(bool(inward)), ptr(rays),
                           stream_of(vertices.device))
    return rays


@torch.no_grad()
def color_by_vertex_normals(models, vertices, triangles, near, far, N_samples=64, N_importance=64,
                            near_t=1.0, white_back=False, inward=True, chunk=FUSE_CHUNK,
                            return_rgb=False, *, rng=None):
    """uint8 colours (V,3) of the mesh's vertices from ``models = [coarse,
    fine]`` alone -- the ``--use_vertex_normal`` branch,
    extract_color_mesh.py:187-204 and 280-284: one ray per vertex along its
    normal (``vertex_normals``, ``normal_rays``; see there for ``inward`` and
    the two unpinned parities), rendered coarse + fine with
    ``render_rays(models, ..., N_samples, False, 0, 0, N_importance, chunk,
    white_back, test_time=True, rng=rng)``, ``chunk`` vertices per call, in
    order; the colour is ``(rgb_fine * 255).to(uint8)``.  Nothing else draws
    from torch's generator.  ``return_rgb``: also return the float32
    ``rgb_fine`` (V,3)."""
    from . import Embedding, render_rays
    if len(models) != 2:
        raise ValueError("color_by_vertex_normals: models = [coarse, fine]")
    if chunk < 1:
        raise ValueError(f"color_by_vertex_normals: chunk = {chunk}")
    vertices, triangles = _mesh(vertices, triangles)
    n = vertices.shape[0]
    if n:
        rays = normal_rays(vertices, vertex_normals(vertices, triangles), near, far, near_t, inward)
        embeddings = [Embedding(3, 10), Embedding(3, 4)]
        rgb = torch.cat([
            render_rays(models, embeddings, rays[i:i + chunk], N_samples, False, 0, 0,
                        N_importance, chunk, white_back, test_time=True, rng=rng)["rgb_fine"]
            for i in range(0, n, chunk)], 0)
    else:
        rgb = torch.empty(0, 3, device=vertices.device)
    colors = (rgb * 255).to(torch.uint8)
    return (colors, rgb) if return_rgb else colors


@torch.no_grad()
def extract_color_mesh(model_fine, poses, images, focal, near, N=256, x_range=(-1.0, 1.0),
                       y_range=(-1.0, 1.0), z_range=(-1.0, 1.0), sigma_threshold=20.0,
                       N_samples=64, occ_threshold=0.2, white_back=False, return_opacity=False, *,
                       _capture=None, use_vertex_normal=False, model_coarse=None, far=None,
                       N_importance=64, near_t=1.0, inward=True):
    """extract_color_mesh.py:113-284 in one call: ``sigma_grid`` ->
    ``marching_cubes`` -> ``grid_to_world`` -> ``largest_cluster`` ->
    ``fuse_vertex_colors``.  Returns ``(vertices (V,3) float32 world,
    triangles (T,3) int32, colors (V,3) uint8)``; with ``return_opacity`` the
    float64 colours and per-view opacities of ``fuse_vertex_colors`` follow.
    Hand the first three to ``write_ply``.

    ``use_vertex_normal=True`` (the reference's ``--use_vertex_normal``) ends
    the chain with ``color_by_vertex_normals([model_coarse, model_fine], ...,
    near, far, N_samples, N_importance, near_t, white_back, inward)`` instead:
    ``model_coarse`` and ``far`` are then required, ``poses``, ``images`` and
    ``focal`` are not read and may be ``None``, and there are no opacities to
    return."""
    if use_vertex_normal:
        if model_coarse is None or far is None:
            raise ValueError("extract_color_mesh: use_vertex_normal needs model_coarse and far")
        if return_opacity:
            raise ValueError("extract_color_mesh: use_vertex_normal has no per-view opacities")
    sigma = sigma_grid(model_fine, N, x_range, y_range, z_range)
    vertices, triangles = marching_cubes(sigma, sigma_threshold)
    vertices = grid_to_world(vertices, N, x_range, y_range, z_range)
    vertices, triangles = largest_cluster(vertices, triangles)
    if use_vertex_normal:
        vertices = vertices.contiguous()
        colors = color_by_vertex_normals([model_coarse, model_fine], vertices, triangles, near, far,
                                         N_samples, N_importance, near_t, white_back, inward)
        return vertices, triangles, colors
    out = fuse_vertex_colors(model_fine, vertices.contiguous(), poses, images, focal, near,
                             N_samples, occ_threshold, white_back, return_opacity,
                             _capture=_capture)
    if return_opacity:
        return (vertices, triangles) + tuple(out)
    return vertices, triangles, out


def write_ply(path, vertices, triangles, colors=None, normals=None) -> None:
    """Binary little-endian PLY as extract_color_mesh.py:286-297 writes it
    through plyfile: vertex ``x y z`` float32 (+ ``red green blue`` uchar with
    ``colors``), face ``vertex_indices`` as ``list uchar int``.  With
    ``normals`` (V,3), ``nx ny nz`` follow ``x y z`` as float32, before the
    colours (the reference writes none).  numpy only; tensors (any device) or
    arrays."""
    def arr(a, dtype):
        if isinstance(a, torch.Tensor):
            a = a.detach().cpu().numpy()
        return np.ascontiguousarray(a, dtype=dtype)

    v = arr(vertices, "<f4").reshape(-1, 3)
    t = arr(triangles, "<i4").reshape(-1, 3)
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {len(v)}",
              "property float x", "property float y", "property float z"]
    if normals is not None:
        nrm = arr(normals, "<f4").reshape(-1, 3)
        if len(nrm) != len(v):
            raise ValueError(f"write_ply: {len(nrm)} normals for {len(v)} vertices")
        fields += [("nx", "<f4"), ("ny", "<f4"), ("nz", "<f4")]
        header += ["property float nx", "property float ny", "property float nz"]
    if colors is not None:
        c = arr(colors, "u1").reshape(-1, 3)
        if len(c) != len(v):
            raise ValueError(f"write_ply: {len(c)} colours for {len(v)} vertices")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {len(t)}", "property list uchar int vertex_indices", "end_header"]
    vert = np.empty(len(v), dtype=fields)
    for k, name in enumerate("xyz"):
        vert[name] = v[:, k]
    if normals is not None:
        for k, name in enumerate(("nx", "ny", "nz")):
            vert[name] = nrm[:, k]
    if colors is not None:
        for k, name in enumerate(("red", "green", "blue")):
            vert[name] = c[:, k]
    face = np.empty(len(t), dtype=[("n", "u1"), ("vertex_indices", "<i4", (3,))])
    face["n"] = 3
    face["vertex_indices"] = t
    with open(path, "wb") as f:
        f.write(("\n".join(header) + "\n").encode("ascii"))
        f.write(vert.tobytes())
        f.write(face.tobytes())
