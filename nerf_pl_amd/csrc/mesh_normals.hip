// Colouring a mesh by its vertex normals (extract_color_mesh.py:187-204, the
// --use_vertex_normal branch): the per-vertex work before the coarse + fine
// render.  Declared in include/nerf_pl_amd_mesh_normals.h.
//
//   nr_mesh_vertex_normals  per vertex: the area-weighted sum of the normals of
//                           its incident triangles, normalised (open3d's
//                           compute_vertex_normals, line 189, as recalled)
//   nr_mesh_normal_rays     per vertex: the ray [o, d, near, far] along the
//                           normal (lines 190-193 and the torch.cat of line 200)
//
// The sum over a vertex's triangles is a gather, not a scatter: the caller
// inverts the triangle list into a CSR list (per vertex, the triangles that
// list it, in ascending corner index 3t + k) and one thread per vertex walks
// its own row, recomputes each cross product in float64 and adds them in that
// order.  No atomics, so two runs give identical buffers, like the rest of
// csrc/mesh.hip.  Each cross product is computed up to three times; the
// vertices it reads (12 B each) come from the caches, marching cubes keeps a
// triangle's vertices close in index.
#include "common.h"

namespace {

// x clamped into [0, hi]
__device__ __forceinline__ int64_t clamp_to(int64_t x, int64_t hi) {
    return x < 0 ? 0 : (x > hi ? hi : x);
}

__global__ void __launch_bounds__(256) mesh_vertex_normals_kernel(
    const float* __restrict__ verts, const int* __restrict__ tris,
    const int64_t* __restrict__ inc_offsets, const int* __restrict__ inc_tris, int64_t nverts,
    int64_t ntris, double* __restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= nverts) return;
    // a foreign list can only shorten the walk or skip entries, never read outside
    const int64_t lim = 3 * ntris;
    const int64_t b = clamp_to(inc_offsets[v], lim);
    const int64_t e = clamp_to(inc_offsets[v + 1], lim);
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (int64_t c = b; c < e; ++c) {
        const int64_t t = inc_tris[c];
        if (t < 0 || t >= ntris) continue;
        const int64_t i0 = tris[t * 3 + 0], i1 = tris[t * 3 + 1], i2 = tris[t * 3 + 2];
        if (i0 < 0 || i0 >= nverts || i1 < 0 || i1 >= nverts || i2 < 0 || i2 >= nverts) continue;
        const double x0 = verts[i0 * 3 + 0], y0 = verts[i0 * 3 + 1], z0 = verts[i0 * 3 + 2];
        const double ax = (double)verts[i1 * 3 + 0] - x0, ay = (double)verts[i1 * 3 + 1] - y0,
                     az = (double)verts[i1 * 3 + 2] - z0;
        const double bx = (double)verts[i2 * 3 + 0] - x0, by = (double)verts[i2 * 3 + 1] - y0,
                     bz = (double)verts[i2 * 3 + 2] - z0;
        // (v1 - v0) x (v2 - v0), unnormalised: twice the area times the unit normal
        sx += ay * bz - az * by;
        sy += az * bx - ax * bz;
        sz += ax * by - ay * bx;
    }
    const double nrm = sqrt(sx * sx + sy * sy + sz * sz);
    double qx = sx / nrm, qy = sy / nrm, qz = sz / nrm;
    // open3d's rule: a NaN quotient (a zero sum, no triangle, or a sum that
    // already holds NaN or Inf) becomes (0, 0, 1)
    if (qx != qx || qy != qy || qz != qz) {
        qx = 0.0;
        qy = 0.0;
        qz = 1.0;
    }
    normals[v * 3 + 0] = qx;
    normals[v * 3 + 1] = qy;
    normals[v * 3 + 2] = qz;
}

__global__ void __launch_bounds__(256) mesh_normal_rays_kernel(const float* __restrict__ verts,
                                                               const double* __restrict__ normals,
                                                               int64_t n, float near, float far,
                                                               float near_t, int inward,
                                                               float* __restrict__ rays) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    float* r = rays + v * 8;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        float d = (float)normals[v * 3 + c];          // torch.FloatTensor(vertex_normals)
        if (inward) d = -d;
        // rays_o = vertices - rays_d * near * near_t, left to right in float32
        r[c] = nr_sub(verts[v * 3 + c], nr_mul(nr_mul(d, near), near_t));
        r[3 + c] = d;
    }
    r[6] = near;
    r[7] = far;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

inline bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

}  // namespace

NR_API int nr_mesh_vertex_normals(const float* vertices, const int32_t* triangles,
                                  const int64_t* inc_offsets, const int32_t* inc_tris,
                                  int64_t n_vertices, int64_t n_triangles, double* normals,
                                  void* stream) {
    NR_REQUIRE(n_vertices >= 0 && n_vertices < ((int64_t)1 << 31),
               "nr_mesh_vertex_normals: n_vertices = %lld", (long long)n_vertices);
    // compared before the product, which a huge count would overflow
    NR_REQUIRE(n_triangles >= 0 && n_triangles < (((int64_t)1 << 31) + 2) / 3,
               "nr_mesh_vertex_normals: n_triangles = %lld (3 * n_triangles must be below 2^31)",
               (long long)n_triangles);
    if (n_vertices == 0) return 0;
    NR_REQUIRE(vertices && inc_offsets && normals, "nr_mesh_vertex_normals: null pointer");
    NR_REQUIRE(n_triangles == 0 || (triangles && inc_tris),
               "nr_mesh_vertex_normals: null pointer (triangles / inc_tris with %lld triangles)",
               (long long)n_triangles);
    NR_REQUIRE(aligned8(inc_offsets) && aligned8(normals),
               "nr_mesh_vertex_normals: inc_offsets / normals is not 8-byte aligned");
    mesh_vertex_normals_kernel<<<blocks_of(n_vertices), 256, 0, (hipStream_t)stream>>>(
        vertices, triangles, inc_offsets, inc_tris, n_vertices, n_triangles, normals);
    NR_LAUNCH_CHECK("nr_mesh_vertex_normals");
    return 0;
}

NR_API int nr_mesh_normal_rays(const float* vertices, const double* normals, int64_t n, float near,
                               float far, float near_t, int inward, float* rays, void* stream) {
    NR_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "nr_mesh_normal_rays: n = %lld", (long long)n);
    if (n == 0) return 0;
    NR_REQUIRE(vertices && normals && rays, "nr_mesh_normal_rays: null pointer");
    NR_REQUIRE(aligned8(normals), "nr_mesh_normal_rays: normals is not 8-byte aligned");
    mesh_normal_rays_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(
        vertices, normals, n, near, far, near_t, inward, rays);
    NR_LAUNCH_CHECK("nr_mesh_normal_rays");
    return 0;
}
