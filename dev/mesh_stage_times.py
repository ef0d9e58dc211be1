"""Per-stage device time of nerf_pl_amd.extract.extract_color_mesh at the
reference's default grid (N = 256), on a sigma-biased random network.

Each stage is run once to warm up and then ``--repeats`` times between HIP
events; the median is printed.  The threshold is a quantile of the grid so
that the (untrained, noisy) field still yields a mesh of a realistic size; V
and T are printed beside the times.  One JSON line on stdout.

    python dev/mesh_stage_times.py [--N 256] [--quantile 0.99] [--views 4]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nerf_pl_amd import NeRF, extract  # noqa: E402
from nerf_pl_amd.rays import blender_focal, pose_spherical  # noqa: E402
from oracle import nerf_oracle as O  # noqa: E402


def timed(fn, repeats):
    """(result, median ms, all ms) of fn() between device events, after one warm-up"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, statistics.median(ms), ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--N", type=int, default=256)
    ap.add_argument("--quantile", type=float, default=0.99)
    ap.add_argument("--views", type=int, default=4)
    ap.add_argument("--img", type=int, default=400)
    ap.add_argument("--N_samples", type=int, default=64)
    ap.add_argument("--N_importance", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mesh_stage_times: needs a HIP device")
    dev = torch.device("cuda", 0)
    model = NeRF().to(dev)
    model.load_state_dict(O.make_params(1, sigma_bias=0.5))
    rng = (-1.2, 1.2)
    g = np.random.Generator(np.random.PCG64(0))
    images = torch.from_numpy(g.integers(0, 256, size=(a.views, a.img, a.img, 3)).astype(np.uint8)).to(dev)
    poses = torch.stack([pose_spherical(360.0 * k / a.views, -30.0, 4.0) for k in range(a.views)])
    focal = blender_focal(a.img)
    res = {"N": a.N, "quantile": a.quantile, "views": a.views, "img": a.img,
           "N_samples": a.N_samples, "N_importance": a.N_importance, "repeats": a.repeats,
           "ms": {}, "all_ms": {}}

    def stage(name, fn):
        out, med, ms = timed(fn, a.repeats)
        res["ms"][name] = round(med, 3)
        res["all_ms"][name] = [round(x, 3) for x in ms]
        return out

    sigma = stage("sigma_grid", lambda: extract.sigma_grid(model, a.N, rng, rng, rng))
    thr = float(sigma.reshape(-1).sort().values[int(a.quantile * (sigma.numel() - 1))])
    v, t = stage("marching_cubes", lambda: extract.marching_cubes(sigma, thr))
    res["threshold"], res["V"], res["T"] = thr, len(v), len(t)
    w = stage("grid_to_world", lambda: extract.grid_to_world(v, a.N, rng, rng, rng))
    cv, ct = stage("largest_cluster", lambda: extract.largest_cluster(w, t))
    res["V_cluster"], res["T_cluster"] = len(cv), len(ct)
    # colours for every vertex of the mesh (the largest piece of a noise field is small)
    w = w.contiguous()
    stage("fuse_vertex_colors", lambda: extract.fuse_vertex_colors(
        model, w, poses, images, focal, 2.0, a.N_samples))
    # the --use_vertex_normal branch on the same vertices: the CSR list and the
    # normals kernel, the ray kernel, then all of it with the coarse + fine render
    coarse = NeRF().to(dev)
    coarse.load_state_dict(O.make_params(2, sigma_bias=0.5))
    normals = stage("vertex_normals", lambda: extract.vertex_normals(w, t))
    stage("normal_rays", lambda: extract.normal_rays(w, normals, 2.0, 6.0))
    stage("color_by_vertex_normals", lambda: extract.color_by_vertex_normals(
        [coarse, model], w, t, 2.0, 6.0, a.N_samples, a.N_importance))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
