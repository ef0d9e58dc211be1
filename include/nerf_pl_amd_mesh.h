/* nerf_pl_amd -- C ABI of the colour-mesh extraction (extract_color_mesh.py:142-284).
 *
 * A second header of the same library (libnerf_pl_amd.so); the conventions of
 * nerf_pl_amd.h hold: every entry point returns int, 0 on success, a
 * hipError_t or NR_EINVAL (10001) with a message naming the entry point in
 * nr_last_error(); sizes and pointers are checked before the device is
 * touched; an empty problem is a no-op; buffers are the caller's device
 * memory (the one exception, `w2c`, is marked); work is enqueued on the
 * caller's `stream` and no call synchronises the host.
 *
 * Marching cubes (mcubes.marching_cubes, extract_color_mesh.py:144) on a
 * float32 grid `sigma` (d0, d1, d2), C order, every di >= 2 and
 * d0*d1*d2 < 2^31.  Corner b of a cell sits at offset (b&1, b>>1&1, b>>2&1);
 * its case bit is set iff sigma < threshold (a NaN compares false).  The
 * edge from grid point p along axis a is crossed iff its two corner bits
 * differ; its vertex is p + t e_a, t = (threshold - s0) / (s1 - s0) in
 * float32, s0 the value at p.  Vertices are ordered by (linear index of the
 * owning point, axis), triangles by (linear index of the cell over
 * (d0-1, d1-1, d2-1), position in the table row); no atomics, so two runs
 * give identical buffers.  The caller scans the two count arrays
 * (exclusive, int64) between the calls and sizes the outputs from their
 * totals.
 */
#ifndef NERF_PL_AMD_MESH_H
#define NERF_PL_AMD_MESH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per grid point: mask bit a set iff the edge to the +1 neighbour along axis
 * a exists and is crossed; count = number of set bits (0..3). */
int nr_mc_point_edges(const float* sigma, int d0, int d1, int d2, float threshold,
                      int32_t* count, uint8_t* mask, void* stream);

/* One vertex (3 floats, array-index coordinates) per crossed edge, written at
 * vbase[point] + rank of the axis among the point's crossed axes.  vbase is
 * the exclusive scan of nr_mc_point_edges' count, n_vertices its total; an
 * index outside [0, n_vertices) is never written. */
int nr_mc_vertices(const float* sigma, int d0, int d1, int d2, float threshold,
                   const uint8_t* mask, const int64_t* vbase, int64_t n_vertices,
                   float* vertices, void* stream);

/* Per cell: the number of triangles of its case.  tri_table is
 * nerf_pl_amd.mesh_tables.MC_TRI_TABLE as int8 (256, 16): triples of cube-edge
 * ids (e = 4*axis + u + 2*v, (u, v) the offsets along the two other axes),
 * -1 after the last triangle. */
int nr_mc_cell_tris(const float* sigma, int d0, int d1, int d2, float threshold,
                    const int8_t* tri_table, int32_t* count, void* stream);

/* Per cell: its table row as int32 vertex indices, at tbase[cell] (the
 * exclusive scan of nr_mc_cell_tris' count; n_triangles its total).  A cube
 * edge's vertex is vbase[owner point] + axis rank within mask[owner point].
 * Triangle normals point from sigma >= threshold to sigma < threshold. */
int nr_mc_triangles(const float* sigma, int d0, int d1, int d2, float threshold,
                    const int8_t* tri_table, const uint8_t* mask, const int64_t* vbase,
                    const int64_t* tbase, int64_t n_vertices, int64_t n_triangles,
                    int32_t* triangles, void* stream);

/* One view of the vertex-colour fusion (extract_color_mesh.py:221-262) for
 * vertices (n, 3) in world coordinates.  w2c: 12 doubles in HOST memory, the
 * (3,4) world-to-camera matrix, read before the call returns.  In float64,
 * like the reference's numpy: cam = w2c @ [v, 1], rows 1-2 negated, then
 * K = [[focal, 0, W/2], [0, focal, H/2], [0, 0, 1]].
 *   depth  (n)   float64  z + 1e-5
 *   pix    (n,2) float32  (x, y) / depth, clipped to [0, W-1] x [0, H-1]
 *   colour (n,3) float32  bilinear sample of image (H, W, 3) uint8 at pix,
 *                         float32 weights, neighbours clamped at the border
 *   rays   (n,8) float32  [o, normalize(v - o), near, float32(depth)]
 * No vertex reads outside the image, wherever it projects. */
int nr_mesh_view_rays(const float* vertices, int64_t n, const double* w2c, float focal, int W,
                      int H, float near, float ox, float oy, float oz, const uint8_t* image,
                      double* depth, float* pix, float* colour, float* rays, void* stream);

/* Lines 269-277: w = 0.1 / depth + (opacity < occ_threshold), a NaN opacity
 * counting as 0; colour_sum (n,3) += colour * w and weight_sum (n) += w in
 * float64.  One thread per vertex: deterministic, views accumulate in call
 * order.  The float64 buffers must be 8-byte aligned. */
int nr_mesh_view_fuse(const double* depth, const float* colour, const float* opacity, int64_t n,
                      float occ_threshold, double* colour_sum, double* weight_sum, void* stream);

#ifdef __cplusplus
}
#endif

#endif
