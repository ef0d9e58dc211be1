"""Optimizer fixtures from the REFERENCE's own ``RAdam`` and ``Ranger``
(utils/optimizers.py:6-95, :266-405) and its ``GradualWarmupScheduler``
(utils/warmup_scheduler.py), run on the CPU in fp32.

    NERF_REFERENCE=<checkout of the reference> python tests/golden/make_golden_optim.py

The two files are loaded by path (``utils/__init__.py`` needs cv2) and only
here.  Inputs (tests/optim_ref.py holds the layout): six tensors, the shapes
``SHAPES`` with lengths 5 and 1 among them, parameters from a seeded
``torch.randn``, 14 steps of gradients ``randn * 10^(k % 4 - 2)`` for tensor k;
the first three columns of tensor 0 get no gradient signal (v = 0 meets eps) and
tensor 4 gets no gradient at all in the first 3 steps, so it crosses the
N_sma threshold (step 6 of its own) later than the others.  Output, plain arrays
only, under tests/golden/optim/ (a directory of their own, as every fixture
family after the render cases has: the top level is the render cases' list):

  optim_inputs.npz   p{k}, g{step}_{k}
  optim_<case>.npz   for the five cases of optim_ref.CASES: p{step}_{k} after
                     steps 5, 6, 7, 12 and 14; s{step}_{k}_{key} and
                     s{step}_{k}_step after steps 7 and 14
  optim_warmup.npz   the lr of the reference's warm-up class at epochs
                     0..total_epoch (its values after warm-up are artefacts of
                     the class on today's torch and are not recorded: DESIGN.md 21)

Before writing, the script checks what tests/test_optim_ref.py then asserts:
every checkpoint within 4 ulp max(1, |p|) + 1% of lr of the float64 restatement.
"""
from __future__ import annotations

import importlib.util
import os
import sys
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import optim_ref as R  # noqa: E402


def _load(rel, name):
    ref = os.environ.get("NERF_REFERENCE")
    if not ref:
        raise SystemExit("set NERF_REFERENCE to a checkout of the reference")
    spec = importlib.util.spec_from_file_location(name, os.path.join(ref, *rel.split("/")))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def make_inputs():
    g = torch.Generator().manual_seed(2024)
    arrs = {}
    for k, s in enumerate(R.SHAPES):
        arrs[f"p{k}"] = torch.randn(s, generator=g).numpy()
    for step in range(1, R.STEPS + 1):
        for k, s in enumerate(R.SHAPES):
            gr = torch.randn(s, generator=g) * (10.0 ** (k % 4 - 2))
            if k == 0:
                gr[:, :3] = 0.0
            if k == R.LATE and step < R.LATE_FROM:
                continue
            arrs[f"g{step}_{k}"] = gr.numpy()
    return arrs


def run_reference(mod, case, params, grads):
    cls, kw = R.CASES[case]
    ps = [torch.tensor(p).requires_grad_(True) for p in params]
    opt = getattr(mod, cls)(ps, lr=R.LR, **kw)
    arrs = {}
    for step, gs in enumerate(grads, start=1):
        for p, g in zip(ps, gs):
            p.grad = None if g is None else torch.tensor(g)
        opt.step()
        if step in R.CHECKPOINTS:
            for k, p in enumerate(ps):
                arrs[f"p{step}_{k}"] = p.detach().numpy().copy()
        if step in R.STATE_AT:
            for k, p in enumerate(ps):
                st = opt.state[p]
                arrs[f"s{step}_{k}_step"] = np.array(int(st["step"]), np.int64)
                for key in R.STATE_KEYS[cls]:
                    arrs[f"s{step}_{k}_{key}"] = st[key].detach().numpy().copy()
    return arrs


def check_against_float64(case, arrs, params, grads):
    at, _ = R.run(case, params, grads)
    worst = 0.0
    for step, ps in at.items():
        for k, p in enumerate(ps):
            d = np.abs(arrs[f"p{step}_{k}"].astype(np.float64) - p)
            worst = max(worst, float((d - 4 * 2.0 ** -23 * np.maximum(1.0, np.abs(p))).max()))
    print(f"{case}: the reference's fp32 run is {worst / R.LR:.4f} lr beyond 4 ulp of float64")
    assert worst <= 0.01 * R.LR, worst


def warmup_values(mod):
    arrs = {}
    base, total = 5e-4, 3
    for i, mult in enumerate((1.0, 2.0)):
        p = torch.zeros(1, requires_grad=True)
        opt = torch.optim.Adam([p], lr=base)
        after = torch.optim.lr_scheduler.MultiStepLR(opt, milestones=[5, 7], gamma=0.5)
        sch = mod.GradualWarmupScheduler(opt, multiplier=mult, total_epoch=total,
                                         after_scheduler=after)
        lrs = [opt.param_groups[0]["lr"]]
        for _ in range(total):
            opt.step()
            sch.step()
            lrs.append(opt.param_groups[0]["lr"])
        arrs[f"w{i}_cfg"] = np.array([base, mult, total], np.float64)
        arrs[f"w{i}_lr"] = np.array(lrs, np.float64)
    arrs["n_cases"] = np.array(2)
    return arrs


def main():
    warnings.simplefilter("ignore")          # the reference's deprecated add_(alpha, t) forms
    torch.set_num_threads(1)
    mod = _load("utils/optimizers.py", "reference_optimizers")
    inputs = make_inputs()
    params, grads = R.inputs_of(inputs)
    out = {"optim_inputs": inputs}
    for case in R.CASES:
        arrs = run_reference(mod, case, params, grads)
        check_against_float64(case, arrs, params, grads)
        out[f"optim_{case}"] = arrs
    out["optim_warmup"] = warmup_values(_load("utils/warmup_scheduler.py", "reference_warmup"))
    os.makedirs(os.path.join(HERE, "optim"), exist_ok=True)
    for name, arrs in out.items():
        path = os.path.join(HERE, "optim", name + ".npz")
        np.savez_compressed(path, **arrs)
        print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
