"""Joint RGB + shadow-map render path -- models/rendering_rgb_sm.py
(train_rgb_sm_juntos.py: colour and shadow map trained from one full-MLP
render, loss ``rgb_weight * MSE(rgb_*) + sm_weight * SMMSE(sm_*)``), executed by
the HIP kernels.

* ``render_rays(models, embeddings, rays, N_samples, use_disp, perturb,
  noise_std, N_importance, chunk, white_back, test_time)`` -- :84-277:
  ``rendering.render_rays`` plus ``disp_map_coarse`` / ``disp_map_fine`` =
  1 / max(1e-10, depth / opacity) (:197; not for the coarse pass under
  ``test_time``), produced and differentiated by the compositing kernels
  (``nr_composite_disp_fwd`` / ``nr_composite_disp_bwd``).  Same positional
  order, result keys and RNG draw order as the reference; the shared keys carry
  ``rendering.render_rays``' bits.  A host batch runs nerf_pl_amd.host.
* ``depth_only=True`` (added keyword, HIP-device batches only): the joint
  trainer's light render consumes only ``depth_*`` (train_rgb_sm_juntos.py:
  156-176) yet the reference runs the full MLP over every light ray.  With it
  the same models run their sigma-only graph (what ``rendering_shadows.
  render_rays`` runs): ``depth_*``, ``opacity_*``, ``disp_map_*`` and no
  ``rgb_*``; differentiable (``--grad_on_light``), and the rgb head gets no
  gradient.  The default is the reference's behaviour.
* ``efficient_sm(...)`` -- :359-480: ``rendering_shadows.efficient_sm`` writing
  ``sm_coarse`` / ``sm_fine`` (= shadow + 1e-5) and leaving ``rgb_*`` alone.

The reference module's legacy ``shadow_mapping()`` (:280-350) is not provided.
"""
from __future__ import annotations

from .rendering import _render_rays, sample_pdf
from .rendering_shadows import _efficient_sm

__all__ = ["render_rays", "efficient_sm", "sample_pdf"]


def render_rays(models, embeddings, rays, N_samples=64, use_disp=False, perturb=0, noise_std=1,
                N_importance=0, chunk=1024 * 32, white_back=False, test_time=False, *, rng=None,
                depth_only=False, _capture=None):
    return _render_rays(models, embeddings, rays, N_samples, use_disp, perturb, noise_std,
                        N_importance, chunk, white_back, test_time, rng, _capture, disp=True,
                        depth_only=depth_only)


def efficient_sm(cam_pixels, light_pixels, cam_results, light_results, ppc, light_ppc,
                 image_shape, fine_sampling, Light_N_importance, shadow_method):
    """rendering_rgb_sm.py:359-480: the shadow maps of the camera depths against
    the light's depth map, written to ``sm_coarse`` (and ``sm_fine``) of
    ``cam_results``, which is returned; every other entry is left as it is."""
    return _efficient_sm(cam_pixels, light_pixels, cam_results, light_results, ppc, light_ppc,
                         image_shape, fine_sampling, Light_N_importance, shadow_method, "sm")
