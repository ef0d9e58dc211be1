"""nerf_pl_amd.schedule (get_scheduler, the closed-form warm-up) and
nerf_pl_amd.optim.get_optimizer on the host: no kernel runs, the optimizers
are only built and the schedulers only write ``param_group["lr"]``.

Tolerance of the lr comparisons: everything is a handful of double operations,
and torch's recursive forms (CosineAnnealingLR) drift from the closed form by
rounding only, so 1e-9 relative."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch.optim.lr_scheduler import CosineAnnealingLR, LambdaLR, MultiStepLR

from conftest import GOLDEN, load_golden_path

BASE = 5e-4
RTOL = 1e-9


def _hp(**k):
    d = dict(optimizer="adam", lr=BASE, momentum=0.9, weight_decay=0.0, lr_scheduler="steplr",
             decay_step=[5, 7], decay_gamma=0.5, num_epochs=10, poly_exp=0.9, warmup_epochs=0,
             warmup_multiplier=1.0)
    d.update(k)
    return SimpleNamespace(**d)


def _opt(lr=BASE):
    return torch.optim.Adam([torch.zeros(1, requires_grad=True)], lr=lr)


def _sequence(opt, sch, n):
    lrs = [opt.param_groups[0]["lr"]]
    for _ in range(n):
        opt.step()
        sch.step()
        lrs.append(opt.param_groups[0]["lr"])
    return np.array(lrs)


def _torch_schedule(kind, opt, hp):
    if kind == "steplr":
        return MultiStepLR(opt, milestones=hp.decay_step, gamma=hp.decay_gamma)
    if kind == "cosine":
        return CosineAnnealingLR(opt, T_max=hp.num_epochs, eta_min=1e-8)
    return LambdaLR(opt, lambda e: (1 - e / hp.num_epochs) ** hp.poly_exp)


@pytest.mark.parametrize("kind", ["steplr", "cosine", "poly"])
def test_get_scheduler_without_warmup_is_torchs_scheduler(kind):
    from nerf_pl_amd.schedule import get_scheduler
    hp = _hp(lr_scheduler=kind)
    opt = _opt()
    sch = get_scheduler(hp, opt)
    assert type(sch) is {"steplr": MultiStepLR, "cosine": CosineAnnealingLR,
                         "poly": LambdaLR}[kind]
    ref_opt = _opt()
    got = _sequence(opt, sch, 10)
    want = _sequence(ref_opt, _torch_schedule(kind, ref_opt, hp), 10)
    assert np.array_equal(got, want)
    if kind == "cosine":
        assert sch.T_max == 10 and sch.eta_min == 1e-8
    if kind == "steplr":
        assert got[4] == BASE and got[5] == BASE / 2 and got[7] == BASE / 4


@pytest.mark.parametrize("kind", ["steplr", "cosine", "poly"])
@pytest.mark.parametrize("mult", [1.0, 2.0])
def test_warmup_is_the_closed_form(kind, mult):
    """e <= total: base ((m - 1) e / total + 1); after: torch's scheduler started
    from base m, at epoch e - total"""
    from nerf_pl_amd.schedule import GradualWarmupScheduler, get_scheduler
    total = 3
    hp = _hp(lr_scheduler=kind, warmup_epochs=total, warmup_multiplier=mult)
    opt = _opt()
    sch = get_scheduler(hp, opt)
    assert type(sch) is GradualWarmupScheduler
    got = _sequence(opt, sch, total + 10)
    for e in range(total + 1):
        assert got[e] == pytest.approx(BASE * ((mult - 1.0) * e / total + 1.0), rel=1e-15)
    ref_opt = _opt(BASE * mult)
    want = _sequence(ref_opt, _torch_schedule(kind, ref_opt, hp), 10)
    np.testing.assert_allclose(got[total:], want, rtol=RTOL, atol=0)
    assert sch.get_last_lr() == [got[-1]]
    if kind == "steplr":        # the drops land at total + 5 and total + 7, not later
        assert got[total + 4] == pytest.approx(BASE * mult)
        assert got[total + 5] == pytest.approx(BASE * mult / 2)
        assert got[total + 7] == pytest.approx(BASE * mult / 4)
    if kind == "cosine":        # and the cosine never rises above where the warm-up ended
        assert (np.diff(got[total:]) < 0).all()


def test_warmup_matches_the_reference_class_up_to_total_epoch():
    fx = load_golden_path(os.path.join(GOLDEN, "optim", "optim_warmup.npz"))
    from nerf_pl_amd.schedule import GradualWarmupScheduler
    assert int(fx["n_cases"]) == 2
    for i in range(2):
        base, mult, total = fx[f"w{i}_cfg"]
        opt = _opt(float(base))
        after = MultiStepLR(opt, milestones=[5, 7], gamma=0.5)
        sch = GradualWarmupScheduler(opt, multiplier=float(mult), total_epoch=int(total),
                                     after_scheduler=after)
        got = _sequence(opt, sch, int(total))
        assert len(fx[f"w{i}_lr"]) == int(total) + 1
        np.testing.assert_allclose(got, fx[f"w{i}_lr"], rtol=1e-15, atol=0)


def test_warmup_without_after_scheduler_and_at_an_epoch():
    from nerf_pl_amd.schedule import GradualWarmupScheduler
    opt = _opt()
    sch = GradualWarmupScheduler(opt, multiplier=4.0, total_epoch=2)
    assert _sequence(opt, sch, 4).tolist() == pytest.approx([BASE, 2.5 * BASE, 4 * BASE,
                                                             4 * BASE, 4 * BASE])
    with pytest.raises(ValueError):
        GradualWarmupScheduler(_opt(), multiplier=0.5, total_epoch=2)
    with pytest.raises(ValueError):
        GradualWarmupScheduler(_opt(), multiplier=2.0, total_epoch=2,
                               after_scheduler=MultiStepLR(_opt(), [1]))
    o = _opt()
    with pytest.raises(TypeError):
        GradualWarmupScheduler(o, multiplier=2.0, total_epoch=2,
                               after_scheduler=torch.optim.lr_scheduler.CyclicLR(
                                   o, 1e-4, 1e-3, cycle_momentum=False))


def test_warmup_state_dict_round_trip():
    from nerf_pl_amd.schedule import get_scheduler
    hp = _hp(lr_scheduler="cosine", warmup_epochs=3, warmup_multiplier=2.0)
    opt = _opt()
    sch = get_scheduler(hp, opt)
    full = _sequence(opt, sch, 5)
    sd = sch.state_dict()
    assert "optimizer" not in sd and isinstance(sd["after_scheduler"], dict)
    tail = _sequence(opt, sch, 4)
    opt2 = _opt()
    sch2 = get_scheduler(hp, opt2)
    sch2.load_state_dict(sd)
    opt2.param_groups[0]["lr"] = full[-1]
    assert np.array_equal(_sequence(opt2, sch2, 4), tail)


@pytest.mark.parametrize("name", ["radam", "ranger"])
def test_rectified_optimizers_get_no_warmup(name):
    from nerf_pl_amd.schedule import get_scheduler
    hp = _hp(optimizer=name, warmup_epochs=3, warmup_multiplier=2.0)
    assert type(get_scheduler(hp, _opt())) is MultiStepLR
    assert type(get_scheduler(_hp(optimizer="sgd", warmup_epochs=3), _opt())) is not MultiStepLR


def test_unknown_scheduler_raises():
    from nerf_pl_amd.schedule import get_scheduler
    with pytest.raises(ValueError):
        get_scheduler(_hp(lr_scheduler="plateau"), _opt())


def test_get_optimizer_builds_the_fused_classes():
    from nerf_pl_amd import optim
    models = [torch.nn.Linear(3, 2), torch.nn.Linear(2, 1)]
    want = {"sgd": optim.FusedSGD, "adam": optim.FusedAdam, "radam": optim.FusedRAdam,
            "ranger": optim.FusedRanger}
    for name, cls in want.items():
        o = optim.get_optimizer(_hp(optimizer=name, weight_decay=1e-2), models)
        assert type(o) is cls
        g = o.param_groups[0]
        assert len(g["params"]) == 4 and g["lr"] == BASE and g["weight_decay"] == 1e-2
        assert optim.get_learning_rate(o) == BASE
        if name == "sgd":
            assert g["momentum"] == 0.9 and "eps" not in g
        else:
            assert g["eps"] == 1e-8        # Ranger's own default is 1e-5
    assert optim.get_optimizer(_hp(optimizer="ranger"), models).param_groups[0]["betas"] == \
        (.95, .999)
    with pytest.raises(ValueError):
        optim.get_optimizer(_hp(optimizer="lamb"), models)


def test_constructor_defaults_and_refusals():
    from nerf_pl_amd import optim
    p = [torch.nn.Parameter(torch.zeros(2))]
    r = optim.FusedRAdam(p)
    assert r.defaults["betas"] == (0.9, 0.999) and r.defaults["eps"] == 1e-8 \
        and r.degenerated_to_sgd is True
    g = optim.FusedRanger(p).defaults
    assert (g["alpha"], g["k"], g["N_sma_threshhold"], g["betas"], g["eps"]) == \
        (0.5, 6, 5, (.95, .999), 1e-5)
    with pytest.raises(NotImplementedError):
        optim.FusedSGD(p, nesterov=True, momentum=0.9)
    with pytest.raises(NotImplementedError):
        optim.FusedSGD(p, dampening=0.1)
    with pytest.raises(ValueError):
        optim.FusedRanger(p, alpha=1.5)
    # host parameters raise at the step, like FusedAdam's
    p[0].grad = torch.ones(2)
    for o in (optim.FusedSGD(p), optim.FusedRAdam(p), optim.FusedRanger(p)):
        with pytest.raises(RuntimeError, match="HIP-device"):
            o.step()
    assert set(optim.__all__) == {"FusedAdam", "FusedSGD", "FusedRAdam", "FusedRanger",
                                  "get_optimizer", "get_learning_rate"}
