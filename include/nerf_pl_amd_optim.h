/* nerf_pl_amd -- C ABI of the fused SGD, RAdam and Ranger steps.
 *
 * A sixth header of the same library (libnerf_pl_amd.so); the conventions of
 * nerf_pl_amd.h hold: every entry point returns int, 0 on success, a
 * hipError_t or NR_EINVAL (10001) with a message naming the entry point in
 * nr_last_error(); sizes and pointers are checked before the device is
 * touched; buffers are the caller's device memory; work is enqueued on the
 * caller's `stream` and no call synchronises the host.
 *
 * The reference offers --optimizer sgd|adam|radam|ranger (opt.py,
 * utils/__init__.py:10-30).  nr_adam_step (nerf_pl_amd.h) is the second; these
 * are the other three.  As there, the tables (params, grads, ...) are HOST
 * arrays of `count` device pointers to fp32 tensors of numel[k] elements; they
 * travel in the kernel arguments, one launch updates every tensor, and each
 * element is read once and written once.  A tensor may start at any 4-byte
 * aligned address and have any length: tensors whose pointers are all 16-byte
 * aligned move in 16-byte accesses (a shorter tail element by element), the
 * others element by element.  Arithmetic is unfused fp32, op for op the
 * optimizer's; scalars are formed in double and rounded to fp32 where torch
 * rounds them.  count == 0 (or no element at all) returns 0 without a launch.
 */
#ifndef NERF_PL_AMD_OPTIM_H
#define NERF_PL_AMD_OPTIM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The largest `count` of one call (48: the NeRF pair has 48 tensors). */
int nr_optim_max_tensors(void);

/* torch.optim.SGD with dampening = 0, nesterov = False, per element:
 *   g += weight_decay * p                        (when weight_decay != 0)
 *   buf = g when first, else momentum * buf + g  (when momentum != 0)
 *   p += (-lr) * buf                             (g itself when momentum == 0)
 * With momentum == 0 the momentum_buf table may be null and is not touched.
 * `first` (0 or 1): the buffers hold nothing yet and are written, not read.
 * 0 <= count <= nr_optim_max_tensors(), numel[k] >= 0. */
int nr_sgd_step(float* const* params, const float* const* grads, float* const* momentum_buf,
                const int64_t* numel, int count, double lr, double momentum,
                double weight_decay, int first, void* stream);

/* RAdam and Ranger (the reference's utils/optimizers.py:6-95 and :266-405),
 * per element, in the reference's op order:
 *   v = v * beta2 + (1 - beta2) * g * g
 *   m = m * beta1 + (1 - beta1) * g
 * then by `mode`:
 *   NR_RADAM_RECTIFIED (0)  p += (-weight_decay * lr) * p  (when weight_decay != 0)
 *                           p += (-step_size * lr) * m / (sqrt(v) + eps)
 *   NR_RADAM_SGD (1)        the same decay, then p += (-step_size * lr) * m
 *   NR_RADAM_SKIP (2)       the moments are updated, p is neither read nor written
 * and, when lookahead_sync (Ranger, every k-th step):
 *   slow += lookahead_alpha * (p - slow);  p = slow
 * `slow` may be null only when lookahead_sync is 0.
 * step_size is formed here in double from `step`, beta1 and beta2 as the
 * reference forms it: with beta2_t = beta2^step, N_max = 2 / (1 - beta2) - 1 and
 * N = N_max - 2 * step * beta2_t / (1 - beta2_t),
 *   rectified  sqrt((1 - beta2_t) * (N - 4) / (N_max - 4) * (N - 2) / N
 *                   * N_max / (N_max - 2)) / (1 - beta1^step)
 *   sgd-like   1 / (1 - beta1^step)
 * The caller chooses `mode` (RAdam: rectified when N >= 5; Ranger: when
 * N > N_sma_threshhold); the rectified mode where the radicand is not positive
 * (N <= 4) is NR_EINVAL.
 * 0 <= count <= nr_optim_max_tensors(), numel[k] >= 0, step >= 1,
 * 0 <= beta1, beta2 < 1, 0 <= lookahead_alpha <= 1, lookahead_sync 0 or 1. */
int nr_radam_step(float* const* params, const float* const* grads, float* const* exp_avg,
                  float* const* exp_avg_sq, float* const* slow, const int64_t* numel, int count,
                  double lr, double beta1, double beta2, double eps, double weight_decay,
                  int64_t step, int mode, double lookahead_alpha, int lookahead_sync,
                  void* stream);

#ifdef __cplusplus
}
#endif

#endif
