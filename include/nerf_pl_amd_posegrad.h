/* nerf_pl_amd -- C ABI of the camera-pose gradient of on-device ray generation.
 *
 * A fifth header of the same library (libnerf_pl_amd.so); the conventions of
 * nerf_pl_amd.h hold: every entry point returns int, 0 on success, a
 * hipError_t or NR_EINVAL (10001) with a message naming the entry point in
 * nr_last_error(); sizes, pointers and alignment are checked before the device
 * is touched; buffers are the caller's device memory; work is enqueued on the
 * caller's `stream` and no call synchronises the host.
 *
 * The reference's get_rays / get_ndc_rays (datasets/ray_utils.py:27-93) are
 * plain PyTorch and differentiate in the camera-to-world matrices.  nr_gen_rays
 * (nerf_pl_amd.h) builds a batch straight from them; this is its transpose.
 */
#ifndef NERF_PL_AMD_POSEGRAD_H
#define NERF_PL_AMD_POSEGRAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* d loss / d c2w from d loss / d rays.  The geometry arguments are
 * nr_gen_rays's, as they were passed to the forward call: ray k is global
 * pixel g = sel[k] (or k when sel is null) = pose * H*W + row * W + col.
 * g_rays (n, 8) fp32, 16-byte aligned: columns 0..2 the origin's gradient,
 * 3..5 the direction's; columns 6..7 (near, far: constants of the call) are
 * not read.  Per ray the forward chain is recomputed in double from the fp32
 * c2w, the pixel and focal, and transposed: the NDC transform when ndc, the
 * normalisation d = R dc / |R dc| and the rotation, dc = ((i - w_half) / focal,
 * -(j - h_half) / focal, -1).
 * g_c2w (n_poses, 3, 4) fp32: every row is written; a pose that no ray selects
 * gets zeros.  g_focal_pose (n_poses) double, or null: per pose, the sum of
 * d loss / d focal over its rays (through dc and, when ndc, through
 * ndc_cw = -2 focal / W and ndc_ch = -2 focal / H); the caller adds the poses.
 * A ray whose sel entry is outside [0, n_poses*H*W) contributes nothing and no
 * c2w is read for it (nr_gen_rays wrote that ray as NaN).
 * The per-pose sums run in double in a fixed order, without floating-point
 * atomics: two runs give identical buffers.  One workgroup per pose walks the
 * batch, so the cost is n_poses * n index reads with sel, n without.
 * n == 0 is not a no-op: the outputs are gradients and the caller expects
 * zeros, so g_c2w (and g_focal_pose) are cleared by a memset on `stream`.
 * 0 <= n < 2^31, 0 < n_poses < 2^31, n_poses * H * W < 2^63, focal != 0,
 * n <= n_poses * H * W when sel is null. */
int nr_gen_rays_posegrad(const float* c2w, int64_t n_poses, int H, int W, float w_half,
                         float h_half, float focal, int ndc, float ndc_near, float ndc_cw,
                         float ndc_ch, float ndc_2near, const int64_t* sel, int64_t n,
                         const float* g_rays, float* g_c2w, double* g_focal_pose, void* stream);

#ifdef __cplusplus
}
#endif

#endif
