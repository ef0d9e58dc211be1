"""Times of the optimizer steps on the 48 tensors of the NeRF pair (1,191,688
floats), for information.  Each of SGD (momentum 0.9), RAdam and
Ranger three ways, in one process and alternating, so that the figures share
whatever else the machine is doing:

  fused   the optimizer's step() (one nr_sgd_step / nr_radam_step launch), and
          the bare launch with the tables built once (the kernel and its enqueue)
  torch   the same rule as per-tensor torch ops on the device: what a user of
          --optimizer sgd|radam|ranger has without this package (for SGD
          torch.optim.SGD itself, single-tensor and foreach)
  adam    FusedAdam's step() and bare nr_adam_step launch, in the same rounds

A window is STEPS steps between two HIP events on an otherwise idle stream,
after WARM steps (so every RAdam/Ranger step is past the rectification
threshold; a Ranger window of 120 steps holds 20 lookahead syncs); ROUNDS rounds
give the median and the spread.
    python dev/optim_times.py
"""
import ctypes
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from nerf_pl_amd import NeRF, _lib, _lib_optim
from nerf_pl_amd.optim import FusedAdam, FusedRAdam, FusedRanger, FusedSGD, n_sma

DEV = torch.device("cuda", 0)
STEPS, WARM, ROUNDS = 120, 12, 7
LR = 5e-4


def pair():
    torch.manual_seed(0)
    ps = [p for m in (NeRF().to(DEV), NeRF().to(DEV)) for p in m.parameters()]
    g = torch.Generator(device=DEV).manual_seed(1)
    for p in ps:
        p.grad = torch.randn(p.shape, device=DEV, generator=g) * 1e-3
    return ps


class TorchRAdam:
    """the RAdam / Ranger rule as per-tensor torch ops (about ten launches per
    tensor and step), written from include/nerf_pl_amd_optim.h"""

    def __init__(self, ps, betas, eps, lookahead):
        self.ps, self.betas, self.eps, self.lookahead = ps, betas, eps, lookahead
        self.m = [torch.zeros_like(p) for p in ps]
        self.v = [torch.zeros_like(p) for p in ps]
        self.slow = [p.detach().clone() for p in ps] if lookahead else None
        self.t = 0

    @torch.no_grad()
    def step(self):
        self.t += 1
        b1, b2 = self.betas
        t = self.t
        n, nmax, b2t = n_sma(b2, t), 2 / (1 - b2) - 1, b2 ** t
        rect = n > 5
        size = 1.0 / (1 - b1 ** t)
        if rect:
            size *= math.sqrt((1 - b2t) * (n - 4) / (nmax - 4) * (n - 2) / n * nmax / (nmax - 2))
        for k, p in enumerate(self.ps):
            g, m, v = p.grad, self.m[k], self.v[k]
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            m.mul_(b1).add_(g, alpha=1 - b1)
            if rect:
                p.addcdiv_(m, v.sqrt().add_(self.eps), value=-size * LR)
            else:
                p.add_(m, alpha=-size * LR)
            if self.lookahead and t % 6 == 0:
                s = self.slow[k]
                s.add_(p - s, alpha=0.5)
                p.copy_(s)


def bare(name, ps, extra_cols, tail):
    """the entry point with its tables built once: (callable, keep-alive)"""
    k = len(ps)
    col = lambda ts: (ctypes.c_void_p * k)(*[t.data_ptr() for t in ts])  # noqa: E731
    state = [[torch.zeros_like(p) for p in ps] for _ in range(extra_cols)]
    tabs = [col(ps), col([p.grad for p in ps])] + [col(s) for s in state]
    numel = (ctypes.c_int64 * k)(*[p.numel() for p in ps])
    st = _lib.stream_of(DEV)
    fn = getattr(_lib_optim.lib() if name != "nr_adam_step" else _lib.lib(), name)

    def go():
        rc = fn(*tabs, numel, k, *tail, st)
        assert rc == 0, _lib.last_error()
    return go, (state, tabs, numel)


def window(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(STEPS):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / STEPS * 1e3          # microseconds per step


def main():
    variants, keep = {}, []

    def add(label, fn):
        variants[label] = fn

    ps = pair()
    add("adam   fused step()", FusedAdam(ps, lr=LR).step)
    go, k = bare("nr_adam_step", pair(), 2, (LR, 0.9, 0.999, 1e-8, 0.0, 100))
    keep.append(k)
    add("adam   bare launch", go)

    add("sgd    fused step()", FusedSGD(pair(), lr=LR, momentum=0.9).step)
    go, k = bare("nr_sgd_step", pair(), 1, (LR, 0.9, 0.0, 0))
    keep.append(k)
    add("sgd    bare launch", go)
    add("sgd    torch.optim.SGD single-tensor",
        torch.optim.SGD(pair(), lr=LR, momentum=0.9, foreach=False).step)
    add("sgd    torch.optim.SGD foreach",
        torch.optim.SGD(pair(), lr=LR, momentum=0.9, foreach=True).step)

    add("radam  fused step()", FusedRAdam(pair(), lr=LR).step)
    go, k = bare("nr_radam_step", pair(), 3, (LR, 0.9, 0.999, 1e-8, 0.0, 100, 0, 0.0, 0))
    keep.append(k)
    add("radam  bare launch", go)
    add("radam  per-tensor torch ops", TorchRAdam(pair(), (0.9, 0.999), 1e-8, False).step)

    add("ranger fused step()", FusedRanger(pair(), lr=LR, eps=1e-8).step)
    go, k = bare("nr_radam_step", pair(), 3, (LR, 0.95, 0.999, 1e-8, 0.0, 100, 0, 0.5, 1))
    keep.append(k)
    add("ranger bare launch, every step a sync", go)
    add("ranger per-tensor torch ops", TorchRAdam(pair(), (0.95, 0.999), 1e-8, True).step)

    for fn in variants.values():
        for _ in range(WARM):
            fn()
    times = {label: [] for label in variants}
    for _ in range(ROUNDS):
        for label, fn in variants.items():
            times[label].append(window(fn))
    n = sum(p.numel() for p in ps)
    print(f"{len(ps)} tensors, {n} floats; microseconds per step, {STEPS} steps per window, "
          f"{ROUNDS} rounds: median [min .. max]")
    for label, ts in times.items():
        print(f"  {label:42s} {statistics.median(ts):9.1f}  [{min(ts):9.1f} .. {max(ts):9.1f}]")


if __name__ == "__main__":
    main()
