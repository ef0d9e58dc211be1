/* nerf_pl_amd -- C ABI of the gradients with respect to the rays.
 *
 * A third header of the same library (libnerf_pl_amd.so); the conventions of
 * nerf_pl_amd.h hold: every entry point returns int, 0 on success, a
 * hipError_t or NR_EINVAL (10001) with a message naming the entry point in
 * nr_last_error(); sizes, pointers and alignment are checked before the device
 * is touched; an empty problem is a no-op; buffers are the caller's device
 * memory; work is enqueued on the caller's `stream` and no call synchronises
 * the host.
 *
 * The reference's render_rays (models/rendering.py) is differentiable in its
 * (N, 8) ray tensor [o, d, near, far].  These entry points carry d loss /
 * d rays through the stages of the fused render, one per stage; each writes
 * its own (n_rays, 8) contribution (columns it does not reach are zero) and
 * per-sample depth gradients, which the caller adds.  Every per-ray sum runs
 * in double over the sample index in a fixed order: no floating-point
 * atomics, two runs give identical buffers.
 */
#ifndef NERF_PL_AMD_RAYGRAD_H
#define NERF_PL_AMD_RAYGRAD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The MLP's input gradient, from the buffer nr_mlp_bwd* left in grad_ws
 * (dz1, dz5 and, unless sigma_only, dz_dir as true fp32 values) and the
 * model's flat fp32 parameters `params` (named_parameters order).  layout:
 * 0 the exact-fp32 object's block-native rows, 1 the split-operand objects'
 * N16 rows, 2 the bf16 object's N16 rows.  samples / count: the device-side
 * list and length the matching nr_mlp_bwd*_active / *_listed call ran over
 * (grad_ws rows are then packed by list position), or both null for every
 * sample; grad_ws is read at positions below the count only.
 * g_samples (n, 8), 16-byte aligned: row s = [g_x (3), d . g_x, g_dd (3), 0]
 * for every listed sample s, x = o + d z; rows of unlisted samples are left
 * as they are (the caller zeroes the buffer when it passes a list).
 * n = n_rays * samples_per_ray < 2^31. */
int nr_raygrad_mlp(const float* params, const float* grad_ws, const float* rays, const float* z,
                   int64_t n, int samples_per_ray, int64_t n_rays, int layout, int sigma_only,
                   const int32_t* samples, const int32_t* count, float* g_samples, void* stream);

/* g_rays (n_rays, 8) from nr_raygrad_mlp's rows: columns 0..2 the sum of g_x,
 * 3..5 the sum of z g_x + g_dd, 6..7 zero. */
int nr_raygrad_reduce(const float* g_samples, const float* z, int64_t n_rays, int samples_per_ray,
                      float* g_rays, void* stream);

/* Compositing (rendering.py:169-198) in the depths and the direction's norm;
 * the arguments of nr_composite_disp_bwd (g_disp, depth, opacity null without
 * a disparity gradient; noise null: the Philox draws of (seed, rng_stream)).
 * g_z (n_rays, n_samples); g_rays (n_rays, 8): columns 3..5, zero elsewhere. */
int nr_composite_raygrad(const float* raw, int raw_stride, int sig_col, const float* z,
                         const float* rays, const float* noise, float noise_std, uint64_t seed,
                         int rng_stream, int64_t n_rays, int n_samples, int white_back,
                         const float* g_rgb, const float* g_depth, const float* g_opacity,
                         const float* g_disp, const float* depth, const float* opacity,
                         float* g_z, float* g_rays, void* stream);

/* The merge z_fine = sort(cat[z_coarse, z_pdf]) (rendering.py:257), z_pdf
 * detached: g_zcoarse[i] = g_zfine[pos(i)], pos(i) the place nr_sample_pdf
 * gave coarse depth i (before every importance depth that is not smaller). */
int nr_merge_raygrad(const float* z_coarse, const float* z_fine, const float* g_zfine,
                     int64_t n_rays, int n_samples, int n_importance, float* g_zcoarse,
                     void* stream);

/* The stratified depths of nr_coarse_z (same arguments) in near and far:
 * g_rays (n_rays, 8): columns 6..7, zero elsewhere. */
int nr_coarse_z_raygrad(const float* rays, const float* tlin, int64_t n_rays, int n_samples,
                        int use_disp, float perturb, const float* u, uint64_t seed,
                        const float* g_z, float* g_rays, void* stream);

#ifdef __cplusplus
}
#endif

#endif
