"""Times of the ray-gradient kernels and of a training step with and without
ray gradients: cfg2-sized batch, 4096 rays, 64 + 128 samples.
    python dev/raygrad_times.py
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nerf_pl_amd import Embedding, NeRF, functions, ops, render_rays
from nerf_pl_amd._lib import ptr, stream_of
from nerf_pl_amd._lib_raygrad import call as rcall
from nerf_pl_amd.rays import blender_rays

DEV = torch.device("cuda", 0)
R, S, I = 4096, 64, 128


def timed(fn, reps=3, warm=2):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), ts


def main():
    torch.manual_seed(0)
    rays = blender_rays(64, 1, near=2.0, far=6.0, device=DEV)[:R].contiguous()
    models = [NeRF().to(DEV), NeRF().to(DEV)]
    emb = [Embedding(3, 10), Embedding(3, 4)]
    target = torch.rand(R, 3, device=DEV)

    def step(req):
        r = rays.clone().requires_grad_(req)
        for m in models:
            m.zero_grad(set_to_none=True)
        res = render_rays(models, emb, r, S, False, 1.0, 1.0, I, 32768, False)
        loss = ((res["rgb_coarse"] - target) ** 2).mean() + ((res["rgb_fine"] - target) ** 2).mean()
        loss.backward()

    print(f"MATH {ops.MATH}")
    for req in (False, True, False, True):
        med, ts = timed(lambda: step(req))
        print(f"step rays.requires_grad={req}: median {med:.3f} ms  {['%.3f' % t for t in ts]}")

    # the kernels alone, fine-pass size (4096 x 192 samples), every sample listed
    SF = S + I
    n = R * SF
    z = (2 + 4 * torch.rand(R, SF, device=DEV)).sort(1)[0].contiguous()
    functions._DEBUG = {}
    r = rays.clone().requires_grad_(True)
    out = functions.mlp_apply(models[1], rays=r, z=z, spr=SF)
    gout = torch.randn_like(out)
    (out * gout).sum().backward()
    grad_ws = functions._DEBUG["grad_ws"]
    flat = models[1].flat_params()
    arith = ops.MATH
    layout = ops._RAYGRAD_LAYOUT[arith]
    g_smp = torch.empty(n, 8, device=DEV)
    g_rays = torch.empty(R, 8, device=DEV)
    st = stream_of(DEV)
    med, ts = timed(lambda: rcall("nr_raygrad_mlp", ptr(flat), ptr(grad_ws), ptr(rays), ptr(z), n, SF,
                                  R, layout, 0, None, None, ptr(g_smp), st))
    print(f"nr_raygrad_mlp n={n} layout {layout}: median {med:.3f} ms {['%.3f' % t for t in ts]}")
    med, ts = timed(lambda: rcall("nr_raygrad_reduce", ptr(g_smp), ptr(z), R, SF, ptr(g_rays), st))
    print(f"nr_raygrad_reduce: median {med:.3f} ms {['%.3f' % t for t in ts]}")
    raw = torch.randn(n, 4, device=DEV)
    noise = torch.randn(R, SF, device=DEV)
    g = [torch.randn(R, 3, device=DEV), torch.randn(R, device=DEV), torch.randn(R, device=DEV)]
    med, ts = timed(lambda: ops.composite_ray_gradient(raw, z, rays, noise, 1.0, 0, 4, False, *g))
    print(f"nr_composite_raygrad ({R}, {SF}): median {med:.3f} ms {['%.3f' % t for t in ts]}")
    zc = ops.coarse_z(rays, S, False, 1.0, u=torch.rand(R, S, device=DEV))
    w = torch.rand(R, S, device=DEV)
    _, zf = ops.sample_pdf(w, rays, I, u=torch.rand(R, I, device=DEV),
                           jitter=torch.rand(R, I, device=DEV), z_coarse=zc, merge=True)
    gzf = torch.randn(R, SF, device=DEV)
    med, ts = timed(lambda: ops.merge_ray_gradient(zc, zf, gzf))
    print(f"nr_merge_raygrad ({R}, {S}+{I}): median {med:.3f} ms {['%.3f' % t for t in ts]}")
    u = torch.rand(R, S, device=DEV)
    gz = torch.randn(R, S, device=DEV)
    med, ts = timed(lambda: ops.coarse_z_ray_gradient(rays, S, False, 1.0, u, 0, gz))
    print(f"nr_coarse_z_raygrad ({R}, {S}): median {med:.3f} ms {['%.3f' % t for t in ts]}")


if __name__ == "__main__":
    main()
