/* nerf_pl_amd -- C ABI of colouring a mesh by its vertex normals
 * (extract_color_mesh.py:187-204, the --use_vertex_normal branch).
 *
 * A further header of the same library (libnerf_pl_amd.so); the conventions of
 * nerf_pl_amd_mesh.h hold: every entry point returns int, 0 on success, a
 * hipError_t or NR_EINVAL (10001) with a message naming the entry point in
 * nr_last_error(); sizes, null pointers and the 8-byte alignment of float64 /
 * int64 buffers are checked before the device is touched; an empty problem is
 * a no-op; buffers are the caller's device memory and the library allocates
 * nothing; work is enqueued on the caller's `stream` and no call synchronises
 * the host.
 */
#ifndef NERF_PL_AMD_MESH_NORMALS_H
#define NERF_PL_AMD_MESH_NORMALS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Unit vertex normals (n_vertices, 3) float64 of the indexed mesh `vertices`
 * (n_vertices, 3) float32 / `triangles` (n_triangles, 3) int32: open3d's
 * compute_vertex_normals() (line 189) as recalled.  A triangle's normal is the
 * unnormalised (v1 - v0) x (v2 - v0) in float64 (so the sum is area-weighted);
 * a vertex sums the normals of the triangles that list it and divides by the
 * Euclidean norm; a NaN quotient -- a zero sum, a vertex no triangle lists, a
 * sum that holds NaN or Inf -- becomes (0, 0, 1).
 *
 * The sum is a gather over a CSR list the caller builds: inc_offsets
 * (n_vertices + 1) int64, inc_tris (3 * n_triangles) int32 -- for each vertex
 * the triangles that list it, in ascending corner index 3t + k.  One thread
 * per vertex adds in that order: no atomics, two runs give identical buffers.
 * Offsets are clamped into [0, 3 * n_triangles], an entry outside
 * [0, n_triangles) and a triangle with a vertex index outside [0, n_vertices)
 * are skipped: whatever the list holds, nothing is read or written outside
 * the buffers.
 *
 * n_vertices and 3 * n_triangles must be below 2^31.  n_triangles == 0 with
 * n_vertices > 0 writes (0, 0, 1) everywhere; triangles and inc_tris may then
 * be null. */
int nr_mesh_vertex_normals(const float* vertices, const int32_t* triangles,
                           const int64_t* inc_offsets, const int32_t* inc_tris,
                           int64_t n_vertices, int64_t n_triangles, double* normals,
                           void* stream);

/* Lines 190-193 and the torch.cat of line 200 for n vertices, in float32 and
 * in the reference's order, nothing contracted: d = float32(normal), negated
 * when `inward` is non-zero; o = v - (d * near) * near_t; the row written to
 * rays (n, 8) is [o, d, near, far]. */
int nr_mesh_normal_rays(const float* vertices, const double* normals, int64_t n, float near,
                        float far, float near_t, int inward, float* rays, void* stream);

#ifdef __cplusplus
}
#endif

#endif
