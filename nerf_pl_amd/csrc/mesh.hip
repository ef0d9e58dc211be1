// Colour mesh extraction (extract_color_mesh.py:142-284) on the device:
// marching cubes on the dense sigma grid and the two per-view kernels of the
// vertex-colour fusion.  Declared in include/nerf_pl_amd_mesh.h.
//
// Marching cubes (replaces mcubes.marching_cubes, extract_color_mesh.py:144) is
// an indexed, deterministic, atomic-free pipeline; the caller scans between the
// kernels:
//   nr_mc_point_edges  per grid point: which of its three outgoing edges the
//                      isosurface crosses (mask) and how many (count)
//   -- exclusive scan of count -> vbase --
//   nr_mc_vertices     per grid point: one vertex per crossed edge, at
//                      vbase[point] + rank of the edge's axis among the crossed
//   nr_mc_cell_tris    per cell: the triangle count of its 256-way case
//   -- exclusive scan -> tbase --
//   nr_mc_triangles    per cell: the table row, each cube edge looked up as
//                      vbase[owner point] + axis rank
// Conventions of nerf_pl_amd/mesh_tables.py: corner b at offset (b&1, b>>1&1,
// b>>2&1); bit b set iff sigma[corner] < thr (NaN: clear); cube edge
// e = 4*axis + u + 2*v with (u, v) the offsets along the two other axes.
// The grid is C-ordered, k fastest, so consecutive lanes read consecutive
// floats; the +-1 neighbours of a point come from the same or adjacent lines
// and are served by the caches.
//
// Vertex colours (extract_color_mesh.py:213-277, the colour-average method):
//   nr_mesh_view_rays  per vertex: project into one view (float64, like the
//                      reference's numpy), bilinear colour, occlusion ray
//   -- the sigma-only render of the rays gives each vertex's opacity --
//   nr_mesh_view_fuse  per vertex: accumulate colour*w and w in float64
#include "common.h"

namespace {

struct Dims { int d0, d1, d2; };

__device__ __forceinline__ int64_t lin(Dims d, int i, int j, int k) {
    return ((int64_t)i * d.d1 + j) * d.d2 + k;
}

// exclusive prefix of the set bits of m below bit a
__device__ __forceinline__ int axis_rank(unsigned m, int a) {
    return __popc(m & ((1u << a) - 1u));
}

__global__ void __launch_bounds__(256) mc_point_edges_kernel(const float* __restrict__ sigma,
                                                             Dims d, float thr,
                                                             int* __restrict__ count,
                                                             uint8_t* __restrict__ mask) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t npts = (int64_t)d.d0 * d.d1 * d.d2;
    if (p >= npts) return;
    const int k = (int)(p % d.d2), j = (int)((p / d.d2) % d.d1), i = (int)(p / ((int64_t)d.d2 * d.d1));
    const bool b0 = sigma[p] < thr;
    unsigned m = 0;
    if (i + 1 < d.d0 && (sigma[p + (int64_t)d.d1 * d.d2] < thr) != b0) m |= 1u;
    if (j + 1 < d.d1 && (sigma[p + d.d2] < thr) != b0) m |= 2u;
    if (k + 1 < d.d2 && (sigma[p + 1] < thr) != b0) m |= 4u;
    count[p] = __popc(m);
    mask[p] = (uint8_t)m;
}

__global__ void __launch_bounds__(256) mc_vertices_kernel(const float* __restrict__ sigma, Dims d,
                                                          float thr,
                                                          const uint8_t* __restrict__ mask,
                                                          const int64_t* __restrict__ vbase,
                                                          int64_t nverts,
                                                          float* __restrict__ verts) {
    const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t npts = (int64_t)d.d0 * d.d1 * d.d2;
    if (p >= npts) return;
    const unsigned m = mask[p];
    if (!m) return;
    const int k = (int)(p % d.d2), j = (int)((p / d.d2) % d.d1), i = (int)(p / ((int64_t)d.d2 * d.d1));
    const float s0 = sigma[p];
    const int64_t step[3] = {(int64_t)d.d1 * d.d2, d.d2, 1};
    const int64_t base = vbase[p];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (!(m & (1u << a))) continue;
        // mc_point_edges sets a bit only where the neighbour exists; a foreign
        // mask must still not read past the grid
        if ((a == 0 ? i + 1 >= d.d0 : a == 1 ? j + 1 >= d.d1 : k + 1 >= d.d2)) continue;
        const float s1 = sigma[p + step[a]];
        const float t = nr_sub(thr, s0) / nr_sub(s1, s0);
        const int64_t v = base + axis_rank(m, a);
        if (v < 0 || v >= nverts) continue;      // an inconsistent scan must not write outside
        float x = (float)i, y = (float)j, z = (float)k;
        if (a == 0) x = nr_add(x, t);
        if (a == 1) y = nr_add(y, t);
        if (a == 2) z = nr_add(z, t);
        verts[v * 3 + 0] = x;
        verts[v * 3 + 1] = y;
        verts[v * 3 + 2] = z;
    }
}

// the 8 corner bits of the cell whose lowest corner is point (i, j, k)
__device__ __forceinline__ unsigned cell_case(const float* __restrict__ sigma, Dims d, float thr,
                                              int i, int j, int k) {
    unsigned c = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b)
        c |= (sigma[lin(d, i + (b & 1), j + ((b >> 1) & 1), k + ((b >> 2) & 1))] < thr ? 1u : 0u)
             << b;
    return c;
}

__global__ void __launch_bounds__(256) mc_cell_tris_kernel(const float* __restrict__ sigma, Dims d,
                                                           float thr,
                                                           const int8_t* __restrict__ table,
                                                           int* __restrict__ count) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c1 = d.d1 - 1, c2 = d.d2 - 1;
    const int64_t ncells = (int64_t)(d.d0 - 1) * c1 * c2;
    if (c >= ncells) return;
    const int k = (int)(c % c2), j = (int)((c / c2) % c1), i = (int)(c / ((int64_t)c2 * c1));
    const int8_t* row = table + 16 * cell_case(sigma, d, thr, i, j, k);
    int n = 0;
    while (n < 5 && row[3 * n] >= 0) ++n;
    count[c] = n;
}

__global__ void __launch_bounds__(256) mc_triangles_kernel(const float* __restrict__ sigma, Dims d,
                                                           float thr,
                                                           const int8_t* __restrict__ table,
                                                           const uint8_t* __restrict__ mask,
                                                           const int64_t* __restrict__ vbase,
                                                           const int64_t* __restrict__ tbase,
                                                           int64_t nverts, int64_t ntris,
                                                           int* __restrict__ tris) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c1 = d.d1 - 1, c2 = d.d2 - 1;
    const int64_t ncells = (int64_t)(d.d0 - 1) * c1 * c2;
    if (c >= ncells) return;
    const int k = (int)(c % c2), j = (int)((c / c2) % c1), i = (int)(c / ((int64_t)c2 * c1));
    const int8_t* row = table + 16 * cell_case(sigma, d, thr, i, j, k);
    if (row[0] < 0) return;
    const int64_t tb = tbase[c];
    for (int n = 0; n < 5 && row[3 * n] >= 0; ++n) {
        const int64_t t = tb + n;
        if (t < 0 || t >= ntris) return;
        for (int q = 0; q < 3; ++q) {
            const int e = min(row[3 * n + q] & 15, 11);     // 0..11 in a valid table
            const int a = e >> 2, u = e & 1, v = (e >> 1) & 1;
            // owner = the edge's corner with offset 0 along its own axis; (u, v) are
            // the offsets along the two other axes, ascending
            const int oi = a == 0 ? 0 : u;
            const int oj = a == 1 ? 0 : (a == 0 ? u : v);
            const int ok = a == 2 ? 0 : v;
            const int64_t p = lin(d, i + oi, j + oj, k + ok);   // <= the last point
            int64_t vi = vbase[p] + axis_rank(mask[p], a);
            // a malformed table or scan can only produce a wrong index, never a wild one
            if (vi < 0 || vi >= nverts) vi = 0;
            tris[t * 3 + q] = (int)vi;
        }
    }
}

struct View {
    double m[12];          // world-to-camera rows, (3,4) row-major
    float focal, cx, cy, near;
    float ox, oy, oz;
    int W, H;
};

__global__ void __launch_bounds__(256) mesh_view_rays_kernel(const float* __restrict__ verts,
                                                             int64_t n, View vw,
                                                             const uint8_t* __restrict__ image,
                                                             double* __restrict__ depth,
                                                             float* __restrict__ pix,
                                                             float* __restrict__ colour,
                                                             float* __restrict__ rays) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    const float xf = verts[v * 3 + 0], yf = verts[v * 3 + 1], zf = verts[v * 3 + 2];
    const double x = xf, y = yf, z = zf;
    // P_w2c @ [v, 1], rows 1-2 negated ("right down forward"), then K @ (lines 223-226)
    const double* m = vw.m;
    const double xc = m[0] * x + m[1] * y + m[2] * z + m[3];
    const double yc = -(m[4] * x + m[5] * y + m[6] * z + m[7]);
    const double zc = -(m[8] * x + m[9] * y + m[10] * z + m[11]);
    const double f = (double)vw.focal;
    const double ui = f * xc + (double)vw.cx * zc;
    const double vi = f * yc + (double)vw.cy * zc;
    const double dep = zc + 1e-5;
    depth[v] = dep;
    // float32 pixel coordinates clipped into the image (a NaN clips to 0, so the
    // fetch below stays inside the image whatever the vertex)
    float px = (float)(ui / dep), py = (float)(vi / dep);
    px = fminf(fmaxf(px, 0.0f), (float)(vw.W - 1));
    py = fminf(fmaxf(py, 0.0f), (float)(vw.H - 1));
    pix[v * 2 + 0] = px;
    pix[v * 2 + 1] = py;
    // exact bilinear interpolation, neighbours clamped at the border
    const float fx0 = floorf(px), fy0 = floorf(py);
    const int x0 = (int)fx0, y0 = (int)fy0;
    const int x1 = min(x0 + 1, vw.W - 1), y1 = min(y0 + 1, vw.H - 1);
    const float ax = nr_sub(px, fx0), ay = nr_sub(py, fy0);
    const float w00 = nr_mul(nr_sub(1.0f, ax), nr_sub(1.0f, ay)), w10 = nr_mul(ax, nr_sub(1.0f, ay));
    const float w01 = nr_mul(nr_sub(1.0f, ax), ay), w11 = nr_mul(ax, ay);
    const uint8_t* r0 = image + ((int64_t)y0 * vw.W) * 3;
    const uint8_t* r1 = image + ((int64_t)y1 * vw.W) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float s = nr_add(nr_add(nr_mul(w00, (float)r0[x0 * 3 + c]),
                                      nr_mul(w10, (float)r0[x1 * 3 + c])),
                               nr_add(nr_mul(w01, (float)r1[x0 * 3 + c]),
                                      nr_mul(w11, (float)r1[x1 * 3 + c])));
        colour[v * 3 + c] = s;
    }
    // [o, normalize(v - o), near, float32(depth)] (lines 255-262)
    const float dx = nr_sub(xf, vw.ox), dy = nr_sub(yf, vw.oy), dz = nr_sub(zf, vw.oz);
    // the norm in float64 (the kernel is in double anyway): each component is
    // then one rounding away from the quotient of the float32 difference
    const double nrm = sqrt((double)dx * dx + (double)dy * dy + (double)dz * dz);
    float* r = rays + v * 8;
    r[0] = vw.ox;
    r[1] = vw.oy;
    r[2] = vw.oz;
    r[3] = (float)(dx / nrm);
    r[4] = (float)(dy / nrm);
    r[5] = (float)(dz / nrm);
    r[6] = vw.near;
    r[7] = (float)dep;
}

__global__ void __launch_bounds__(256) mesh_view_fuse_kernel(const double* __restrict__ depth,
                                                             const float* __restrict__ colour,
                                                             const float* __restrict__ opacity,
                                                             int64_t n, float occ_threshold,
                                                             double* __restrict__ csum,
                                                             double* __restrict__ wsum) {
    const int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (v >= n) return;
    float o = opacity[v];
    if (o != o) o = 0.0f;          // np.nan_to_num(opacity, 1): NaN -> 0 (line 270)
    const double w = 0.1 / depth[v] + (o < occ_threshold ? 1.0 : 0.0);
#pragma unroll
    for (int c = 0; c < 3; ++c) csum[v * 3 + c] += (double)colour[v * 3 + c] * w;
    wsum[v] += w;
}

int check_dims(const char* name, int d0, int d1, int d2) {
    NR_REQUIRE(d0 >= 2 && d1 >= 2 && d2 >= 2, "%s: grid (%d, %d, %d): every dimension must be >= 2",
               name, d0, d1, d2);
    NR_REQUIRE((int64_t)d0 * d1 * d2 < ((int64_t)1 << 31), "%s: grid (%d, %d, %d) has 2^31 points or more",
               name, d0, d1, d2);
    return 0;
}

inline unsigned blocks_of(int64_t n) { return (unsigned)((n + 255) / 256); }

inline bool aligned8(const void* p) { return ((uintptr_t)p & 7u) == 0; }

}  // namespace

NR_API int nr_mc_point_edges(const float* sigma, int d0, int d1, int d2, float threshold,
                             int32_t* count, uint8_t* mask, void* stream) {
    if (int rc = check_dims("nr_mc_point_edges", d0, d1, d2)) return rc;
    NR_REQUIRE(sigma && count && mask, "nr_mc_point_edges: null pointer");
    const Dims d = {d0, d1, d2};
    mc_point_edges_kernel<<<blocks_of((int64_t)d0 * d1 * d2), 256, 0, (hipStream_t)stream>>>(
        sigma, d, threshold, count, mask);
    NR_LAUNCH_CHECK("nr_mc_point_edges");
    return 0;
}

NR_API int nr_mc_vertices(const float* sigma, int d0, int d1, int d2, float threshold,
                          const uint8_t* mask, const int64_t* vbase, int64_t n_vertices,
                          float* vertices, void* stream) {
    if (int rc = check_dims("nr_mc_vertices", d0, d1, d2)) return rc;
    NR_REQUIRE(n_vertices >= 0 && n_vertices < ((int64_t)1 << 31) &&
                   n_vertices <= 3 * (int64_t)d0 * d1 * d2,
               "nr_mc_vertices: %lld vertices for a (%d, %d, %d) grid", (long long)n_vertices, d0,
               d1, d2);
    if (n_vertices == 0) return 0;
    NR_REQUIRE(sigma && mask && vbase && vertices, "nr_mc_vertices: null pointer");
    NR_REQUIRE(aligned8(vbase), "nr_mc_vertices: vbase is not 8-byte aligned");
    const Dims d = {d0, d1, d2};
    mc_vertices_kernel<<<blocks_of((int64_t)d0 * d1 * d2), 256, 0, (hipStream_t)stream>>>(
        sigma, d, threshold, mask, vbase, n_vertices, vertices);
    NR_LAUNCH_CHECK("nr_mc_vertices");
    return 0;
}

NR_API int nr_mc_cell_tris(const float* sigma, int d0, int d1, int d2, float threshold,
                           const int8_t* tri_table, int32_t* count, void* stream) {
    if (int rc = check_dims("nr_mc_cell_tris", d0, d1, d2)) return rc;
    NR_REQUIRE(sigma && tri_table && count, "nr_mc_cell_tris: null pointer");
    const Dims d = {d0, d1, d2};
    const int64_t ncells = (int64_t)(d0 - 1) * (d1 - 1) * (d2 - 1);
    mc_cell_tris_kernel<<<blocks_of(ncells), 256, 0, (hipStream_t)stream>>>(sigma, d, threshold,
                                                                            tri_table, count);
    NR_LAUNCH_CHECK("nr_mc_cell_tris");
    return 0;
}

NR_API int nr_mc_triangles(const float* sigma, int d0, int d1, int d2, float threshold,
                           const int8_t* tri_table, const uint8_t* mask, const int64_t* vbase,
                           const int64_t* tbase, int64_t n_vertices, int64_t n_triangles,
                           int32_t* triangles, void* stream) {
    if (int rc = check_dims("nr_mc_triangles", d0, d1, d2)) return rc;
    const int64_t ncells = (int64_t)(d0 - 1) * (d1 - 1) * (d2 - 1);
    NR_REQUIRE(n_vertices >= 0 && n_vertices < ((int64_t)1 << 31) &&
                   n_vertices <= 3 * (int64_t)d0 * d1 * d2,
               "nr_mc_triangles: %lld vertices for a (%d, %d, %d) grid", (long long)n_vertices, d0,
               d1, d2);
    NR_REQUIRE(n_triangles >= 0 && n_triangles <= 5 * ncells,
               "nr_mc_triangles: %lld triangles for a (%d, %d, %d) grid", (long long)n_triangles,
               d0, d1, d2);
    if (n_triangles == 0) return 0;
    NR_REQUIRE(n_vertices > 0, "nr_mc_triangles: triangles without vertices");
    NR_REQUIRE(sigma && tri_table && mask && vbase && tbase && triangles,
               "nr_mc_triangles: null pointer");
    NR_REQUIRE(aligned8(vbase) && aligned8(tbase),
               "nr_mc_triangles: vbase / tbase is not 8-byte aligned");
    const Dims d = {d0, d1, d2};
    mc_triangles_kernel<<<blocks_of(ncells), 256, 0, (hipStream_t)stream>>>(
        sigma, d, threshold, tri_table, mask, vbase, tbase, n_vertices, n_triangles, triangles);
    NR_LAUNCH_CHECK("nr_mc_triangles");
    return 0;
}

NR_API int nr_mesh_view_rays(const float* vertices, int64_t n, const double* w2c, float focal,
                             int W, int H, float near, float ox, float oy, float oz,
                             const uint8_t* image, double* depth, float* pix, float* colour,
                             float* rays, void* stream) {
    NR_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "nr_mesh_view_rays: n = %lld", (long long)n);
    NR_REQUIRE(W >= 1 && H >= 1 && (int64_t)W * H < ((int64_t)1 << 29),
               "nr_mesh_view_rays: image %d x %d", W, H);
    if (n == 0) return 0;
    NR_REQUIRE(vertices && w2c && image && depth && pix && colour && rays,
               "nr_mesh_view_rays: null pointer");
    NR_REQUIRE(aligned8(depth), "nr_mesh_view_rays: depth is not 8-byte aligned");
    View vw;
    for (int i = 0; i < 12; ++i) vw.m[i] = w2c[i];       // w2c is host memory
    vw.focal = focal;
    vw.cx = (float)W / 2;                                 // K of lines 179-181 (float32)
    vw.cy = (float)H / 2;
    vw.near = near;
    vw.ox = ox;
    vw.oy = oy;
    vw.oz = oz;
    vw.W = W;
    vw.H = H;
    mesh_view_rays_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(vertices, n, vw, image,
                                                                         depth, pix, colour, rays);
    NR_LAUNCH_CHECK("nr_mesh_view_rays");
    return 0;
}

NR_API int nr_mesh_view_fuse(const double* depth, const float* colour, const float* opacity,
                             int64_t n, float occ_threshold, double* colour_sum,
                             double* weight_sum, void* stream) {
    NR_REQUIRE(n >= 0 && n < ((int64_t)1 << 31), "nr_mesh_view_fuse: n = %lld", (long long)n);
    if (n == 0) return 0;
    NR_REQUIRE(depth && colour && opacity && colour_sum && weight_sum,
               "nr_mesh_view_fuse: null pointer");
    NR_REQUIRE(aligned8(depth) && aligned8(colour_sum) && aligned8(weight_sum),
               "nr_mesh_view_fuse: a float64 buffer is not 8-byte aligned");
    mesh_view_fuse_kernel<<<blocks_of(n), 256, 0, (hipStream_t)stream>>>(
        depth, colour, opacity, n, occ_threshold, colour_sum, weight_sum);
    NR_LAUNCH_CHECK("nr_mesh_view_fuse");
    return 0;
}
