"""Fused optimizers -- drop-ins for the four the reference
builds in ``utils/__init__.py:10-30`` from ``--optimizer sgd|adam|radam|ranger``
(lr 5e-4, eps 1e-8, weight_decay and momentum from opt.py).

``FusedAdam.step()`` updates every parameter tensor that has a gradient in
ONE ``nr_adam_step`` launch (up to ``nr_adam_max_tensors()`` tensors per
launch; the NeRF pair has 48), with torch's single-tensor Adam arithmetic.
Parameters without a gradient are skipped, like torch.  State keys
(``step``, ``exp_avg``, ``exp_avg_sq``) match torch's, so state dicts move
between the two optimizers.

``FusedSGD`` (``nr_sgd_step``: ``torch.optim.SGD``), ``FusedRAdam`` and
``FusedRanger`` (``nr_radam_step``: the reference's ``utils/optimizers.py``
``RAdam`` and ``Ranger``) do the same for the other three, with the state keys
of the class each replaces (``momentum_buffer``; ``step``, ``exp_avg``,
``exp_avg_sq``, ``slow_buffer``).  ``get_optimizer`` is the reference's
``get_optimizer`` over these four; ``nerf_pl_amd.schedule.get_scheduler`` is its
companion.
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib_optim
from ._lib import call, lib, stream_of

__all__ = ["FusedAdam", "FusedSGD", "FusedRAdam", "FusedRanger", "get_optimizer",
           "get_learning_rate"]


class FusedAdam(torch.optim.Optimizer):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 amsgrad=False):
        if amsgrad:
            raise NotImplementedError("nerf_pl_amd.FusedAdam: amsgrad is not supported")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        cap = int(lib().nr_adam_max_tensors())
        for group in self.param_groups:
            b1, b2 = group["betas"]
            batches = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                if p.grad.is_sparse or p.dtype != torch.float32 or p.device.type != "cuda":
                    raise RuntimeError("nerf_pl_amd.FusedAdam: dense fp32 HIP-device "
                                       "parameters only")
                st = self.state[p]
                if not st:
                    st["step"] = torch.tensor(0.0)
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.preserve_format)
                st["step"] += 1
                g = p.grad if p.grad.is_contiguous() else p.grad.contiguous()
                if not p.is_contiguous():
                    raise RuntimeError("nerf_pl_amd.FusedAdam: parameters must be contiguous")
                key = (int(st["step"].item()), p.device)
                batches.setdefault(key, []).append((p, g, st["exp_avg"], st["exp_avg_sq"]))
            for (step, dev), items in batches.items():
                for i in range(0, len(items), cap):
                    chunk = items[i:i + cap]
                    k = len(chunk)
                    arr = lambda xs: (ctypes.c_void_p * k)(*[x.data_ptr() for x in xs])  # noqa: E731
                    numel = (ctypes.c_int64 * k)(*[c[0].numel() for c in chunk])
                    call("nr_adam_step", arr([c[0] for c in chunk]), arr([c[1] for c in chunk]),
                         arr([c[2] for c in chunk]), arr([c[3] for c in chunk]), numel, k,
                         float(group["lr"]), float(b1), float(b2), float(group["eps"]),
                         float(group["weight_decay"]), step, stream_of(dev))
                # the kernel wrote through raw pointers: bump the version
                # counters like torch's in-place Adam does, so autograd sees
                # the modification and NeRF.packed() re-packs the new weights
                torch.autograd.graph.increment_version([c[0] for c in items])
        return loss


def _checked_grad(p, who):
    """the contiguous gradient of a parameter the kernels can take, or raise"""
    if p.grad.is_sparse or p.dtype != torch.float32 or p.device.type != "cuda":
        raise RuntimeError(f"nerf_pl_amd.{who}: dense fp32 HIP-device parameters only")
    if not p.is_contiguous():
        raise RuntimeError(f"nerf_pl_amd.{who}: parameters must be contiguous")
    return p.grad if p.grad.is_contiguous() else p.grad.contiguous()


def _launches(items):
    """``items`` (tuples of tensors, the parameter first; a column of ``None``
    is a null table) cut into the tables of one launch each"""
    cap = int(_lib_optim.lib().nr_optim_max_tensors())
    for i in range(0, len(items), cap):
        chunk = items[i:i + cap]
        k = len(chunk)
        cols = []
        for col in zip(*chunk):
            cols.append(None if col[0] is None
                        else (ctypes.c_void_p * k)(*[x.data_ptr() for x in col]))
        yield cols, (ctypes.c_int64 * k)(*[c[0].numel() for c in chunk]), k


def _closure_loss(closure):
    if closure is None:
        return None
    with torch.enable_grad():
        return closure()


class FusedSGD(torch.optim.Optimizer):
    """``torch.optim.SGD`` (momentum and weight decay; no dampening, no
    Nesterov) with one ``nr_sgd_step`` launch per step."""

    def __init__(self, params, lr=1e-3, momentum=0.0, dampening=0.0, weight_decay=0.0,
                 nesterov=False):
        if nesterov:
            raise NotImplementedError("nerf_pl_amd.FusedSGD: nesterov is not supported")
        if dampening != 0:
            raise NotImplementedError("nerf_pl_amd.FusedSGD: dampening is not supported")
        if lr < 0.0 or momentum < 0.0 or weight_decay < 0.0:
            raise ValueError(f"nerf_pl_amd.FusedSGD: negative lr {lr}, momentum {momentum} or "
                             f"weight_decay {weight_decay}")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening,
                                      weight_decay=weight_decay, nesterov=nesterov))

    @torch.no_grad()
    def step(self, closure=None):
        loss = _closure_loss(closure)
        for group in self.param_groups:
            if group["nesterov"] or group["dampening"] != 0:
                raise NotImplementedError("nerf_pl_amd.FusedSGD: nesterov and dampening are "
                                          "not supported")
            momentum = float(group["momentum"])
            batches = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = _checked_grad(p, "FusedSGD")
                buf, first = None, False
                if momentum != 0.0:
                    st = self.state[p]
                    first = st.get("momentum_buffer") is None
                    if first:        # written, not read, by its first launch
                        st["momentum_buffer"] = torch.empty_like(
                            p, memory_format=torch.contiguous_format)
                    buf = st["momentum_buffer"]
                batches.setdefault((first, p.device), []).append((p, g, buf))
            for (first, dev), items in batches.items():
                for (ps, gs, bufs), numel, k in _launches(items):
                    _lib_optim.call("nr_sgd_step", ps, gs, bufs, numel, k, float(group["lr"]),
                                    momentum, float(group["weight_decay"]), int(first),
                                    stream_of(dev))
                # raw-pointer writes: bump the version counters (see FusedAdam)
                torch.autograd.graph.increment_version([c[0] for c in items])
        return loss


def n_sma(beta2, step):
    """the length of the approximated simple moving average at ``step``
    (utils/optimizers.py:68-70), in Python doubles as the reference forms it"""
    beta2_t = beta2 ** step
    n_sma_max = 2 / (1 - beta2) - 1
    return n_sma_max - 2 * step * beta2_t / (1 - beta2_t)


class _RectifiedBase(torch.optim.Optimizer):
    """What FusedRAdam and FusedRanger share: the state, the batching by
    (step, device) and the ``nr_radam_step`` launches.  N_sma and the step size
    depend on the step and the group's own betas only, so they are computed per
    launch from those (the reference's ten-slot cache holds the same values --
    except that Ranger's single cache hands a group with other betas the first
    group's entry, which is not reproduced: DESIGN.md 21)."""

    _who = ""
    _lookahead = False

    def _mode(self, group, n):           # -> RECTIFIED / SGD_LIKE / SKIP
        raise NotImplementedError

    @torch.no_grad()
    def step(self, closure=None):
        loss = _closure_loss(closure)
        for group in self.param_groups:
            b1, b2 = group["betas"]
            batches = {}
            for p in group["params"]:
                if p.grad is None:
                    continue
                g = _checked_grad(p, self._who)
                st = self.state[p]
                if not st:
                    st["step"] = 0
                    st["exp_avg"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    st["exp_avg_sq"] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                    if self._lookahead:      # the weights before their first update
                        st["slow_buffer"] = p.detach().clone(
                            memory_format=torch.contiguous_format)
                st["step"] = int(st["step"]) + 1       # a loaded state may hold a tensor
                for key in ("exp_avg", "exp_avg_sq") + (("slow_buffer",) * self._lookahead):
                    t = st[key]
                    if t.dtype != torch.float32 or t.device != p.device or not t.is_contiguous():
                        raise RuntimeError(f"nerf_pl_amd.{self._who}: state {key} must be a "
                                           "contiguous fp32 tensor on the parameter's device")
                slow = st["slow_buffer"] if self._lookahead else None
                batches.setdefault((st["step"], p.device), []).append(
                    (p, g, st["exp_avg"], st["exp_avg_sq"], slow))
            for (step, dev), items in batches.items():
                mode = self._mode(group, n_sma(b2, step))
                sync = bool(self._lookahead and step % int(group["k"]) == 0)
                alpha = float(group["alpha"]) if self._lookahead else 0.0
                for (ps, gs, ms, vs, slows), numel, k in _launches(items):
                    _lib_optim.call("nr_radam_step", ps, gs, ms, vs, slows if sync else None,
                                    numel, k, float(group["lr"]), float(b1), float(b2),
                                    float(group["eps"]), float(group["weight_decay"]), step,
                                    mode, alpha, int(sync), stream_of(dev))
                # raw-pointer writes: bump the version counters (see FusedAdam)
                torch.autograd.graph.increment_version([c[0] for c in items])
        return loss


class FusedRAdam(_RectifiedBase):
    """The reference's ``RAdam`` (utils/optimizers.py:6-95) with one
    ``nr_radam_step`` launch per step: Adam's moments, the rectified step once
    N_sma >= 5, before that a momentum-SGD step (``degenerated_to_sgd``) or
    none."""

    _who = "FusedRAdam"

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0,
                 degenerated_to_sgd=True):
        if not 0.0 <= lr:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not 0.0 <= eps:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        self.degenerated_to_sgd = degenerated_to_sgd
        # `buffer` is the reference's cache slot: never read here, carried so
        # that a state dict saved from this class loads into the reference's
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                      buffer=[[None, None, None] for _ in range(10)]))

    def _mode(self, group, n):
        if n >= 5:
            return _lib_optim.RECTIFIED
        return _lib_optim.SGD_LIKE if self.degenerated_to_sgd else _lib_optim.SKIP


class FusedRanger(_RectifiedBase):
    """The reference's ``Ranger`` (utils/optimizers.py:266-405; RAdam plus
    Lookahead: every ``k``-th step of a parameter its slow copy moves ``alpha``
    of the way to it and replaces it) with one ``nr_radam_step`` launch per
    step."""

    _who = "FusedRanger"
    _lookahead = True

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(.95, 0.999),
                 eps=1e-5, weight_decay=0):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Invalid slow update rate: {alpha}")
        if not 1 <= k:
            raise ValueError(f"Invalid lookahead steps: {k}")
        if not lr > 0:
            raise ValueError(f"Invalid Learning Rate: {lr}")
        if not eps > 0:
            raise ValueError(f"Invalid eps: {eps}")
        super().__init__(params, dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas,
                                      N_sma_threshhold=N_sma_threshhold, eps=eps,
                                      weight_decay=weight_decay))
        self.N_sma_threshhold = N_sma_threshhold
        self.alpha = alpha
        self.k = k

    def _mode(self, group, n):
        return _lib_optim.RECTIFIED if n > group["N_sma_threshhold"] else _lib_optim.SGD_LIKE


def get_optimizer(hparams, models):
    """The reference's ``get_optimizer`` (utils/__init__.py:10-30) over the fused
    classes: ``hparams.optimizer`` in sgd | adam | radam | ranger, one optimizer
    over every model's parameters, eps 1e-8."""
    eps = 1e-8
    parameters = []
    for model in models:
        parameters += list(model.parameters())
    if hparams.optimizer == "sgd":
        return FusedSGD(parameters, lr=hparams.lr, momentum=hparams.momentum,
                        weight_decay=hparams.weight_decay)
    if hparams.optimizer == "adam":
        return FusedAdam(parameters, lr=hparams.lr, eps=eps, weight_decay=hparams.weight_decay)
    if hparams.optimizer == "radam":
        return FusedRAdam(parameters, lr=hparams.lr, eps=eps, weight_decay=hparams.weight_decay)
    if hparams.optimizer == "ranger":
        return FusedRanger(parameters, lr=hparams.lr, eps=eps, weight_decay=hparams.weight_decay)
    raise ValueError("optimizer not recognized!")


def get_learning_rate(optimizer):
    for param_group in optimizer.param_groups:
        return param_group["lr"]
