// Camera-pose gradients (include/nerf_pl_amd_posegrad.h): the
// transpose of gen_rays_kernel (rays.hip).  The reference's get_rays /
// get_ndc_rays (datasets/ray_utils.py:27-93) are plain PyTorch and
// differentiate in c2w; here d loss / d rays (n, 8) is pulled back through the
// per-ray chain -- NDC transform, normalisation, rotation -- and summed per
// pose into (n_poses, 3, 4), with one focal partial per pose.  Runs only when
// c2w or focal requires grad.
#include "common.h"

namespace {

struct PoseGradArgs {
    const float* c2w;  // (n_poses, 3, 4)
    int64_t n_poses; int H, W;
    float w_half, h_half, focal;
    int ndc; float ndc_near, ndc_cw, ndc_ch, ndc_2near;
    const int64_t* sel; int64_t n;
    const float* g_rays;    // (n, 8); columns 6..7 are not read
    float* g_c2w;           // (n_poses, 3, 4)
    double* g_focal_pose;   // (n_poses) or null
};

constexpr int kTerms = 13;      // 12 entries of the pose + the focal partial
constexpr int kThreads = 256;

// Ray k of pose p, pixel pix: adds its 13 terms to acc.  Everything in double
// from the fp32 inputs; m is the pose's 12 entries.
__device__ __forceinline__ void pg_ray(const PoseGradArgs& a, const double* m, int64_t pix,
                                       int64_t k, double* acc) {
    const f32x4* gp = reinterpret_cast<const f32x4*>(a.g_rays + k * 8);
    const f32x4 g0 = gp[0], g1 = gp[1];
    double go[3] = {g0.x, g0.y, g0.z};
    double gd[3] = {g0.w, g1.x, g1.y};
    const double f = a.focal;
    const double i = (double)(pix % a.W), j = (double)(pix / a.W);
    const double dc[3] = {(i - (double)a.w_half) / f, -((j - (double)a.h_half) / f), -1.0};
    double d[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) d[r] = dc[0] * m[r * 4] + dc[1] * m[r * 4 + 1] + dc[2] * m[r * 4 + 2];
    const double nrm = sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]);
    d[0] /= nrm; d[1] /= nrm; d[2] /= nrm;
    double gf = 0.0;
    if (a.ndc) {
        // get_ndc_rays (:75-93) backwards, node by node: the NDC origin and
        // direction -> ox, oy, the quotients, the shifted origin, t -> (o, d)
        const double cw = a.ndc_cw, ch = a.ndc_ch, near = a.ndc_near, near2 = a.ndc_2near;
        const double o[3] = {m[3], m[7], m[11]};
        const double t = -(near + o[2]) / d[2];
        const double s0 = o[0] + t * d[0], s1 = o[1] + t * d[1], s2 = o[2] + t * d[2];
        const double ox = s0 / s2, oy = s1 / s2;
        const double q0 = d[0] / d[2], q1 = d[1] / d[2];
        const double g_o2 = go[2] - gd[2];                    // d2 = 1 - o2
        const double g_ox = cw * (go[0] - gd[0]), g_oy = ch * (go[1] - gd[1]);
        const double g_q0 = cw * gd[0], g_q1 = ch * gd[1];
        // ndc_cw = -2 f / W, ndc_ch = -2 f / H: d ndc_c* / d f = ndc_c* / f
        gf = (ox * go[0] + (q0 - ox) * gd[0]) * cw / f + (oy * go[1] + (q1 - oy) * gd[1]) * ch / f;
        const double gs0 = g_ox / s2, gs1 = g_oy / s2;
        const double gs2 = -(g_ox * ox + g_oy * oy) / s2 - g_o2 * near2 / (s2 * s2);
        const double g_t = gs0 * d[0] + gs1 * d[1] + gs2 * d[2];
        go[0] = gs0; go[1] = gs1; go[2] = gs2 - g_t / d[2];
        gd[0] = g_q0 / d[2] + t * gs0;
        gd[1] = g_q1 / d[2] + t * gs1;
        gd[2] = -(g_q0 * q0 + g_q1 * q1) / d[2] + t * gs2 - g_t * t / d[2];
    }
    // d = d_un / |d_un|
    const double dot = d[0] * gd[0] + d[1] * gd[1] + d[2] * gd[2];
    double gu[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) gu[r] = (gd[r] - d[r] * dot) / nrm;
    double gdc[2] = {0.0, 0.0};
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        acc[r * 4 + 0] += gu[r] * dc[0];
        acc[r * 4 + 1] += gu[r] * dc[1];
        acc[r * 4 + 2] += gu[r] * dc[2];
        acc[r * 4 + 3] += go[r];
        gdc[0] += m[r * 4] * gu[r];
        gdc[1] += m[r * 4 + 1] * gu[r];
    }
    acc[12] += gf - (gdc[0] * dc[0] + gdc[1] * dc[1]) / f;
}

// One workgroup per pose.  Thread t takes candidates t, t + 256, ... in index
// order (the batch when sel is given, else the pose's own pixel range), keeps
// the rays of its pose and sums 13 doubles; the lanes of a wave meet in an xor
// butterfly and the four waves are added in wave order: a fixed order, no
// floating-point atomics.
__global__ void __launch_bounds__(kThreads) pose_grad_kernel(PoseGradArgs a) {
    __shared__ double part[kThreads / 64][kTerms];
    const int64_t p = blockIdx.x;
    const int tid = threadIdx.x;
    const int64_t hw = (int64_t)a.H * a.W;
    double m[12];
#pragma unroll
    for (int c = 0; c < 12; ++c) m[c] = (double)a.c2w[p * 12 + c];   // p < n_poses: the grid
    double acc[kTerms];
#pragma unroll
    for (int c = 0; c < kTerms; ++c) acc[c] = 0.0;
    if (a.sel) {
        for (int64_t k = tid; k < a.n; k += kThreads) {
            const int64_t g = a.sel[k];
            // an out-of-range selection (nr_gen_rays wrote it as NaN) belongs to no pose
            if (g < p * hw || g >= (p + 1) * hw) continue;
            pg_ray(a, m, g - p * hw, k, acc);
        }
    } else {
        const int64_t end = a.n < (p + 1) * hw ? a.n : (p + 1) * hw;
        for (int64_t k = p * hw + tid; k < end; k += kThreads) pg_ray(a, m, k - p * hw, k, acc);
    }
#pragma unroll
    for (int c = 0; c < kTerms; ++c) {
        double v = acc[c];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d);
        acc[c] = v;
    }
    if ((tid & 63) == 0) {
#pragma unroll
        for (int c = 0; c < kTerms; ++c) part[tid >> 6][c] = acc[c];
    }
    __syncthreads();
    if (tid < kTerms) {
        double v = part[0][tid];
        for (int w = 1; w < kThreads / 64; ++w) v += part[w][tid];
        if (tid < 12) a.g_c2w[p * 12 + tid] = (float)v;
        else if (a.g_focal_pose) a.g_focal_pose[p] = v;
    }
}

constexpr int64_t kMaxN = (int64_t)1 << 31;

}  // namespace

NR_API int nr_gen_rays_posegrad(const float* c2w, int64_t n_poses, int H, int W, float w_half,
                                float h_half, float focal, int ndc, float ndc_near, float ndc_cw,
                                float ndc_ch, float ndc_2near, const int64_t* sel, int64_t n,
                                const float* g_rays, float* g_c2w, double* g_focal_pose,
                                void* stream) {
    NR_REQUIRE(n >= 0 && n < kMaxN, "nr_gen_rays_posegrad: n out of range");
    NR_REQUIRE(n_poses > 0 && n_poses < kMaxN && H > 0 && W > 0, "nr_gen_rays_posegrad: bad sizes");
    // compared before the product, which a huge pose count would overflow
    NR_REQUIRE(n_poses <= INT64_MAX / ((int64_t)H * W) - 1,
               "nr_gen_rays_posegrad: n_poses * H * W overflows");
    NR_REQUIRE(c2w && g_rays && g_c2w, "nr_gen_rays_posegrad: null pointer");
    NR_REQUIRE(((uintptr_t)g_rays & 15) == 0, "nr_gen_rays_posegrad: g_rays must be 16-byte aligned");
    NR_REQUIRE(((uintptr_t)g_c2w & 3) == 0 && ((uintptr_t)g_focal_pose & 7) == 0,
               "nr_gen_rays_posegrad: misaligned output");
    NR_REQUIRE(focal != 0.f, "nr_gen_rays_posegrad: focal must not be 0");
    NR_REQUIRE(sel || n <= n_poses * H * W, "nr_gen_rays_posegrad: n exceeds the pixel count");
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) {       // the output is a gradient: the caller expects zeros
        hipError_t e = hipMemsetAsync(g_c2w, 0, (size_t)n_poses * 12 * sizeof(float), st);
        if (e == hipSuccess && g_focal_pose)
            e = hipMemsetAsync(g_focal_pose, 0, (size_t)n_poses * sizeof(double), st);
        if (e != hipSuccess) {
            nr_set_error("nr_gen_rays_posegrad: memset failed: %s", hipGetErrorString(e));
            return (int)e;
        }
        return 0;
    }
    PoseGradArgs a{c2w, n_poses, H, W, w_half, h_half, focal, ndc, ndc_near, ndc_cw, ndc_ch,
                   ndc_2near, sel, n, g_rays, g_c2w, g_focal_pose};
    pose_grad_kernel<<<(unsigned)n_poses, kThreads, 0, st>>>(a);
    NR_LAUNCH_CHECK("nr_gen_rays_posegrad");
    return 0;
}
