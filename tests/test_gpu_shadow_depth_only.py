"""rendering_shadows.render_rays is rendering_rgb_sm.render_rays(depth_only=True):
the sigma-only render exists once (rendering._render_rays) and the two entry
points must stay bit-identical -- every result map, the captured depths and
coarse weights, and after a backward of a fixed linear loss over depth_* and
opacity_* every parameter gradient with the same None pattern, whether or not
the joint path's fine pass runs on the side stream.

23 rays of 16 (+ 24) samples: 368 and 920 samples, a partial 128-sample
workgroup and a last 32-sample block that is not full.  disp_map_* is compared
in the forward only (bit-equal on these inputs): the shadow path computes it in
torch, the joint path in the compositing kernel, and their backwards round
differently (tests/test_gpu_rgb_sm.py bounds the latter).
"""
import pytest
import torch

from oracle import nerf_oracle as O

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
N_RAYS, N_SAMPLES, SEED = 23, 16, 20240611
CAPTURED = ("z_coarse", "z_fine", "weights_coarse")


def _models():
    from nerf_pl_amd import NeRF
    models = []
    for seed in (1, 2):
        m = NeRF()
        m.load_state_dict(O.make_params(seed, sigma_bias=0.5))
        models.append(m.to(DEV))
    return models


def _rays():
    from nerf_pl_amd.rays import blender_rays
    return blender_rays(16, 1, near=2.0, far=6.0)[7:7 + 11 * N_RAYS:11].contiguous().to(DEV)


def _render(fn, models, n_importance, test_time, **kw):
    from nerf_pl_amd import Embedding, PhiloxRNG
    cap = {}
    with torch.set_grad_enabled(not test_time):
        res = fn(models, [Embedding(3, 10), Embedding(3, 4)], _rays(), N_SAMPLES, False, 1, 1,
                 n_importance, 32768, False, test_time, rng=PhiloxRNG(SEED), _capture=cap, **kw)
    return res, cap


def _fixed_loss(maps):
    g = torch.Generator().manual_seed(5)
    return sum((maps[k] * torch.randn(N_RAYS, generator=g).to(DEV)).sum()
               for k in sorted(maps) if not k.startswith("disp_map_"))


@pytest.mark.parametrize("fine_stream", [True, False], ids=["side_stream", "one_stream"])
@pytest.mark.parametrize("n_importance", [0, 24])
def test_training_render_and_gradients(monkeypatch, n_importance, fine_stream):
    from nerf_pl_amd import rendering, rendering_rgb_sm, rendering_shadows
    from nerf_pl_amd.functions import _SIGMA_ONLY_UNUSED
    monkeypatch.setattr(rendering, "FINE_STREAM", fine_stream)
    runs = []
    for fn, kw in ((rendering_shadows.render_rays, {}),
                   (rendering_rgb_sm.render_rays, {"depth_only": True})):
        models = _models()
        maps, cap = _render(fn, models, n_importance, False, **kw)
        _fixed_loss(maps).backward()
        torch.cuda.synchronize()
        runs.append((maps, cap, {(i, name): p.grad for i, m in enumerate(models)
                                 for name, p in m.named_parameters()}))
    (maps_a, cap_a, grads_a), (maps_b, cap_b, grads_b) = runs
    levels = ("coarse", "fine") if n_importance else ("coarse",)
    assert sorted(maps_a) == sorted(maps_b) == sorted(f"{q}_{lv}" for lv in levels
                                                       for q in ("depth", "opacity", "disp_map"))
    for k in maps_a:
        assert torch.equal(maps_a[k], maps_b[k]), k
    for k in CAPTURED if n_importance else CAPTURED[:1]:
        assert torch.equal(cap_a[k], cap_b[k]), k
    for (i, name), ga in grads_a.items():
        gb = grads_b[i, name]
        # the sigma-only graph of each model that rendered a level, nothing else
        reached = i < len(levels) and name not in _SIGMA_ONLY_UNUSED
        assert (ga is not None) == (gb is not None) == reached, (i, name)
        if reached:
            assert ga.any() and torch.equal(ga, gb), (i, name)


@pytest.mark.parametrize("n_importance", [0, 24])
def test_test_time_render(n_importance):
    from nerf_pl_amd import rendering_rgb_sm, rendering_shadows
    maps_a, cap_a = _render(rendering_shadows.render_rays, _models(), n_importance, True)
    maps_b, cap_b = _render(rendering_rgb_sm.render_rays, _models(), n_importance, True,
                            depth_only=True)
    fine = ["depth_fine", "opacity_fine", "disp_map_fine"]
    want = ["opacity_coarse"] + (fine if n_importance else [])
    assert sorted(maps_a) == sorted(maps_b) == sorted(want)
    for k in maps_a:
        assert torch.equal(maps_a[k], maps_b[k]), k
    for k in CAPTURED if n_importance else CAPTURED[:1]:
        assert torch.equal(cap_a[k], cap_b[k]), k


def test_empty_batch_renders_empty_maps():
    """a rank's slice in render_rays_sharded may be empty: the shadow path
    renders it to empty maps (rendering.render_rays raises, like the reference)"""
    from nerf_pl_amd import rendering_shadows
    for n_importance in (0, 24):
        with torch.no_grad():
            res = rendering_shadows.render_rays(_models(), None, _rays()[:0], N_SAMPLES, False,
                                                1, 1, n_importance)
        levels = ("coarse", "fine") if n_importance else ("coarse",)
        assert list(res) == [f"{q}_{lv}" for lv in levels for q in ("depth", "opacity", "disp_map")]
        assert all(v.shape == (0,) for v in res.values())
