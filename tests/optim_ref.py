"""Float64 restatement of the four update rules behind nerf_pl_amd.optim's
FusedSGD, FusedRAdam and FusedRanger (and of N_sma / step_size), written from
the papers' formulas and the rules as include/nerf_pl_amd_optim.h states them:

  SGD     g += wd p;  buf = g (first) | momentum buf + g;  p -= lr buf
  RAdam   v = b2 v + (1 - b2) g^2;  m = b1 m + (1 - b1) g
          N = N_max - 2 t b2^t / (1 - b2^t),  N_max = 2 / (1 - b2) - 1
          N >= 5:  p -= wd lr p;  p -= lr r m / (sqrt(v) + eps) / (1 - b1^t),
                   r = sqrt((1 - b2^t) (N-4)/(N_max-4) (N-2)/N N_max/(N_max-2))
          else, degenerated to SGD:  p -= wd lr p;  p -= lr m / (1 - b1^t)
          else:    p unchanged
  Ranger  RAdam's with the rule N > threshold, the decay in both branches, and
          every k-th step of a parameter  slow += alpha (p - slow);  p = slow
          (slow: the parameter before its first step)

Everything is numpy float64; a parameter whose gradient is None is skipped and
keeps its own step count.  The tests compare the reference's fp32 fixtures
(tests/golden/optim/optim_*.npz) and the fused kernels against this."""
from __future__ import annotations

import math

import numpy as np

RECTIFIED, SGD_LIKE, SKIP = 0, 1, 2


def n_sma_max(beta2):
    return 2.0 / (1.0 - beta2) - 1.0


def n_sma(beta2, step):
    b2t = beta2 ** step
    return n_sma_max(beta2) - 2.0 * step * b2t / (1.0 - b2t)


def step_size(beta1, beta2, step, mode):
    """the factor of lr: rectification over the first-moment bias correction"""
    if mode == SKIP:
        return 0.0
    bc1 = 1.0 - beta1 ** step
    if mode == SGD_LIKE:
        return 1.0 / bc1
    n, nmax, b2t = n_sma(beta2, step), n_sma_max(beta2), beta2 ** step
    return math.sqrt((1.0 - b2t) * (n - 4.0) / (nmax - 4.0) * (n - 2.0) / n * nmax
                     / (nmax - 2.0)) / bc1


def radam_mode(beta2, step, degenerated_to_sgd=True):
    if n_sma(beta2, step) >= 5:
        return RECTIFIED
    return SGD_LIKE if degenerated_to_sgd else SKIP


def ranger_mode(beta2, step, threshold=5):
    return RECTIFIED if n_sma(beta2, step) > threshold else SGD_LIKE


class _Base:
    def __init__(self, params):
        self.params = [np.array(p, dtype=np.float64) for p in params]
        self.state = [dict() for _ in params]

    def step(self, grads):
        for k, g in enumerate(grads):
            if g is not None:
                self._update(k, np.asarray(g, dtype=np.float64))


class SGD(_Base):
    def __init__(self, params, lr, momentum=0.0, weight_decay=0.0):
        super().__init__(params)
        self.lr, self.momentum, self.wd = lr, momentum, weight_decay

    def _update(self, k, g):
        p, st = self.params[k], self.state[k]
        g = g + self.wd * p
        if self.momentum != 0:
            st["momentum_buffer"] = g.copy() if "momentum_buffer" not in st \
                else self.momentum * st["momentum_buffer"] + g
            g = st["momentum_buffer"]
        p -= self.lr * g


class RAdam(_Base):
    def __init__(self, params, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 degenerated_to_sgd=True):
        super().__init__(params)
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.degenerated_to_sgd = degenerated_to_sgd

    def _mode(self, step):
        return radam_mode(self.betas[1], step, self.degenerated_to_sgd)

    def _moments(self, k, g):
        p, st = self.params[k], self.state[k]
        if not st:
            st.update(step=0, exp_avg=np.zeros_like(p), exp_avg_sq=np.zeros_like(p))
            self._first(k)
        b1, b2 = self.betas
        st["exp_avg_sq"] = b2 * st["exp_avg_sq"] + (1.0 - b2) * g * g
        st["exp_avg"] = b1 * st["exp_avg"] + (1.0 - b1) * g
        st["step"] += 1
        return st

    def _first(self, k):
        pass

    def _move(self, k, st, mode):
        p = self.params[k]
        if mode == SKIP:
            return
        if self.wd != 0:
            p -= self.wd * self.lr * p
        s = step_size(self.betas[0], self.betas[1], st["step"], mode) * self.lr
        if mode == RECTIFIED:
            p -= s * st["exp_avg"] / (np.sqrt(st["exp_avg_sq"]) + self.eps)
        else:
            p -= s * st["exp_avg"]

    def _update(self, k, g):
        st = self._moments(k, g)
        self._move(k, st, self._mode(st["step"]))


class Ranger(RAdam):
    def __init__(self, params, lr, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999),
                 eps=1e-5, weight_decay=0.0):
        super().__init__(params, lr, betas, eps, weight_decay)
        self.alpha, self.k, self.threshold = alpha, k, N_sma_threshhold

    def _mode(self, step):
        return ranger_mode(self.betas[1], step, self.threshold)

    def _first(self, k):
        self.state[k]["slow_buffer"] = self.params[k].copy()

    def _update(self, k, g):
        super()._update(k, g)
        st = self.state[k]
        if st["step"] % self.k == 0:
            st["slow_buffer"] += self.alpha * (self.params[k] - st["slow_buffer"])
            self.params[k][...] = st["slow_buffer"]


# ---------------------------------------------------------------------------
# the fixtures' layout (tests/golden/make_golden_optim.py writes it, the tests
# read it)
# ---------------------------------------------------------------------------
SHAPES = [(32, 63), (32,), (1, 32), (3, 40), (5,), (1,)]
STEPS = 14
LATE, LATE_FROM = 4, 4                  # tensor 4 gets its first gradient at step 4
CHECKPOINTS = (5, 6, 7, 12, 14)         # parameters stored after these steps
STATE_AT = (7, 14)                      # ... and the full state after these
LR = 5e-4
# case -> (class name, keyword arguments beside lr); eps as get_optimizer passes it
CASES = {
    "radam": ("RAdam", dict(eps=1e-8)),
    "radam_wd": ("RAdam", dict(eps=1e-8, weight_decay=1e-2)),
    "radam_nosgd": ("RAdam", dict(eps=1e-8, degenerated_to_sgd=False)),
    "ranger": ("Ranger", dict(eps=1e-8)),
    "ranger_wd": ("Ranger", dict(eps=1e-8, weight_decay=1e-2)),
}
STATE_KEYS = {"RAdam": ("exp_avg", "exp_avg_sq"),
              "Ranger": ("exp_avg", "exp_avg_sq", "slow_buffer")}


def inputs_of(fx):
    """(initial parameters, [per step: list of gradient or None]) of optim_inputs.npz"""
    params = [fx[f"p{k}"] for k in range(len(SHAPES))]
    grads = [[fx.get(f"g{s}_{k}") for k in range(len(SHAPES))] for s in range(1, STEPS + 1)]
    return params, grads


def run(case, params, grads, lr=LR):
    """the restatement over the fixture's steps: {step: [params]}, {step: [state]}"""
    cls, kw = CASES[case]
    opt = {"RAdam": RAdam, "Ranger": Ranger}[cls](params, lr, **kw)
    at, states = {}, {}
    for s, gs in enumerate(grads, start=1):
        opt.step(gs)
        if s in CHECKPOINTS:
            at[s] = [p.copy() for p in opt.params]
        if s in STATE_AT:
            states[s] = [{k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}
                         for st in opt.state]
    return at, states
