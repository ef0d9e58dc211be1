"""Learning-rate schedules: the reference's ``get_scheduler``
(utils/__init__.py:32-49) and a warm-up of our own in place of its
``GradualWarmupScheduler`` (utils/warmup_scheduler.py).  Host-only: no kernel
is involved, a schedule only writes ``param_group["lr"]``.

    optimizer = nerf_pl_amd.optim.get_optimizer(hparams, models)
    scheduler = nerf_pl_amd.schedule.get_scheduler(hparams, optimizer)

``hparams.lr_scheduler`` in steplr | cosine | poly gives torch's
``MultiStepLR(decay_step, decay_gamma)``, ``CosineAnnealingLR(T_max=num_epochs,
eta_min=1e-8)`` or a ``LambdaLR`` of ``(1 - epoch / num_epochs) ** poly_exp``
(the reference names ``LambdaLR`` without importing it, so its poly choice
raises; this one works).  The schedule is wrapped in the warm-up when
``warmup_epochs > 0`` and the optimizer is neither radam nor ranger: the
rectified optimizers warm up by themselves.

The warm-up is defined in closed form over the epoch e (the number of
``step()`` calls):

    e <= total_epoch:  lr = base * ((multiplier - 1) * e / total_epoch + 1)
    e >  total_epoch:  the wrapped schedule, started from base * multiplier,
                       evaluated at epoch e - total_epoch

Up to ``total_epoch`` these are the reference class's values
(tests/golden/optim/optim_warmup.npz).  After it the reference's class, run
on today's torch, calls the wrapped scheduler's recursive ``get_lr`` once
before it starts stepping it, so the wrapped schedule runs one epoch behind
(with total_epoch 3 the drop of MultiStepLR([5, 7]) lands at epoch 9, not 8)
and CosineAnnealingLR(T_max=10) first rises, from 5e-4 to 5.125e-4 at epoch 4;
those artefacts are not reproduced.
"""
from __future__ import annotations

from torch.optim.lr_scheduler import CosineAnnealingLR, LambdaLR, LRScheduler, MultiStepLR

__all__ = ["GradualWarmupScheduler", "get_scheduler"]


class GradualWarmupScheduler(LRScheduler):
    """Linear warm-up from ``base`` to ``base * multiplier`` over ``total_epoch``
    epochs, then ``after_scheduler`` (or the constant ``base * multiplier``).

    ``after_scheduler`` must be able to give its lr at an epoch in closed form:
    a ``LambdaLR``, or a torch scheduler with a closed form (MultiStepLR,
    CosineAnnealingLR, StepLR, ExponentialLR, ...).  It is built on the same
    optimizer before this one and is never stepped by the caller."""

    def __init__(self, optimizer, multiplier, total_epoch, after_scheduler=None):
        if multiplier < 1.0:
            raise ValueError("multiplier should be greater than or equal to 1.")
        if total_epoch < 1:
            raise ValueError("total_epoch should be at least 1")
        if after_scheduler is not None:
            if after_scheduler.optimizer is not optimizer:
                raise ValueError("after_scheduler drives another optimizer")
            if not (isinstance(after_scheduler, LambdaLR)
                    or hasattr(after_scheduler, "_get_closed_form_lr")):
                raise TypeError(f"{type(after_scheduler).__name__} has no closed form: it cannot "
                                "be evaluated at an epoch of the warm-up's choosing")
        self.multiplier = multiplier
        self.total_epoch = total_epoch
        self.after_scheduler = after_scheduler
        super().__init__(optimizer)

    def get_lr(self):
        e = self.last_epoch
        if e <= self.total_epoch:
            return [b * ((self.multiplier - 1.0) * e / self.total_epoch + 1.0)
                    for b in self.base_lrs]
        top = [b * self.multiplier for b in self.base_lrs]
        after = self.after_scheduler
        if after is None:
            return top
        after.base_lrs = top
        after.last_epoch = e - self.total_epoch
        if isinstance(after, LambdaLR):          # its get_lr is base * lambda(epoch)
            lrs = [b * f(after.last_epoch) for f, b in zip(after.lr_lambdas, top)]
        else:
            lrs = list(after._get_closed_form_lr())
        after._last_lr = lrs
        return lrs

    _get_closed_form_lr = get_lr                 # step(epoch) evaluates the same form

    def state_dict(self):
        sd = {k: v for k, v in self.__dict__.items()
              if k not in ("optimizer", "after_scheduler")}
        sd["after_scheduler"] = (None if self.after_scheduler is None
                                 else self.after_scheduler.state_dict())
        return sd

    def load_state_dict(self, state_dict):
        sd = dict(state_dict)
        after = sd.pop("after_scheduler", None)
        if after is not None and self.after_scheduler is not None:
            self.after_scheduler.load_state_dict(after)
        self.__dict__.update(sd)


def get_scheduler(hparams, optimizer):
    eps = 1e-8
    if hparams.lr_scheduler == "steplr":
        scheduler = MultiStepLR(optimizer, milestones=hparams.decay_step,
                                gamma=hparams.decay_gamma)
    elif hparams.lr_scheduler == "cosine":
        scheduler = CosineAnnealingLR(optimizer, T_max=hparams.num_epochs, eta_min=eps)
    elif hparams.lr_scheduler == "poly":
        scheduler = LambdaLR(optimizer,
                             lambda epoch: (1 - epoch / hparams.num_epochs) ** hparams.poly_exp)
    else:
        raise ValueError("scheduler not recognized!")

    if hparams.warmup_epochs > 0 and hparams.optimizer not in ["radam", "ranger"]:
        scheduler = GradualWarmupScheduler(optimizer, multiplier=hparams.warmup_multiplier,
                                           total_epoch=hparams.warmup_epochs,
                                           after_scheduler=scheduler)
    return scheduler
