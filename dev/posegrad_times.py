"""Times of the camera-pose gradient kernel, for information:
the cfg2-shaped batch (4,096 shuffled rays of 100 poses at 400 x 400) and one
whole 400 x 400 image, with and without the focal partials; beside them the
forward nr_gen_rays launch of the same batch.
    python dev/posegrad_times.py
"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nerf_pl_amd._lib import ptr, stream_of
from nerf_pl_amd._lib_posegrad import call
from nerf_pl_amd.rays import blender_focal, generate_rays, pose_spherical

DEV = torch.device("cuda", 0)
IMG, N_POSES, BATCH = 400, 100, 4096


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
    focal = blender_focal(IMG)
    poses = torch.stack([pose_spherical(-180.0 + 3.6 * k, -30.0, 4.0) for k in range(N_POSES)]).to(DEV)
    st = stream_of(DEV)
    geom = (IMG, IMG, IMG / 2, IMG / 2, focal, 0, 1.0, -2 * focal / IMG, -2 * focal / IMG, 2.0)
    sel = torch.randint(0, N_POSES * IMG * IMG, (BATCH,), generator=torch.Generator().manual_seed(0)).to(DEV)
    cases = [("cfg2 batch: 4096 rays of 100 poses", poses, sel, BATCH),
             ("one 400 x 400 image of one pose", poses[:1].contiguous(), None, IMG * IMG)]
    for what, P, s, n in cases:
        n_poses = P.shape[0]
        g_rays = torch.randn(n, 8, device=DEV)
        g_c2w = torch.empty(n_poses, 3, 4, device=DEV)
        g_f = torch.empty(n_poses, dtype=torch.float64, device=DEV)
        med, ts = timed(lambda: generate_rays(P, IMG, IMG, focal, 2.0, 6.0, s))
        print(f"{what}: generate_rays (forward) median {med:.3f} ms {['%.3f' % t for t in ts]}")
        for label, gf in (("poses", None), ("poses + focal", g_f)):
            med, ts = timed(lambda: call("nr_gen_rays_posegrad", ptr(P), n_poses, *geom, ptr(s), n,
                                         ptr(g_rays), ptr(g_c2w), ptr(gf), st))
            print(f"{what}: nr_gen_rays_posegrad ({label}) median {med:.3f} ms "
                  f"{['%.3f' % t for t in ts]}")


if __name__ == "__main__":
    main()
