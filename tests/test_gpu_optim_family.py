"""FusedSGD, FusedRAdam and FusedRanger (nr_sgd_step, nr_radam_step) on the
device.

RAdam and Ranger against the reference's own classes through the fixtures
(tests/golden/optim/: the reference's fp32 CPU run of 14 steps on six small
tensors, lengths 5 and 1 among them, one tensor joining at step 4).  Tolerance,
that of tests/test_gpu_optim.py for Adam: parameters within 4 ulp * max(1, |p|)
plus 2% of one step (lr) -- four times what the reference itself needs against
float64 (tests/test_optim_ref.py) -- moments and slow weights within 1e-5 of the
tensor's max, step counts equal.  FusedSGD against torch.optim.SGD
(single-tensor, CPU) under the same bound.

State interchange.  The fused run and the reference's differ by ulps at step 7
(torch's CPU kernels fuse some multiply-adds), so a run continued from the
FIXTURE's step-7 state cannot be bitwise equal to the straight fused run; the
test therefore checks both halves of the hand-over: the fixture's state (the
reference's keys, Python-int steps, host arrays) loaded into a fresh FusedRanger
and continued to step 14 meets the reference's step-14 fixture within the
tolerance, and the straight fused run's own step-7 state, taken to the host in
that same form and loaded into a fresh FusedRanger, continues to step 14 bit
for bit like the straight run."""
import functools
import os

import numpy as np
import pytest
import torch

import optim_ref as R
from conftest import GOLDEN, load_golden_path

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
ULP = 2.0 ** -23


@functools.lru_cache(maxsize=None)
def _fx(name):
    return load_golden_path(os.path.join(GOLDEN, "optim", name + ".npz"))


def _inputs():
    return R.inputs_of(_fx("optim_inputs"))


def _make(case, params):
    from nerf_pl_amd.optim import FusedRAdam, FusedRanger
    cls, kw = R.CASES[case]
    return {"RAdam": FusedRAdam, "Ranger": FusedRanger}[cls](params, lr=R.LR, **kw)


def _feed(opt, ps, grads, first_step, record):
    for step, gs in enumerate(grads, start=first_step):
        for p, g in zip(ps, gs):
            p.grad = None if g is None else torch.from_numpy(g).to(DEV)
        opt.step()
        record(step)


def _run(case):
    """one fused run over the fixture's 14 steps: parameters after every step,
    the state (host copies) after the fixture's state steps and after step 5"""
    params, grads = _inputs()
    ps = [torch.nn.Parameter(torch.from_numpy(p).to(DEV)) for p in params]
    opt = _make(case, ps)
    out = {"p": {}, "s": {}}

    def record(step):
        out["p"][step] = [p.detach().cpu() for p in ps]
        if step in R.STATE_AT or step == 5:
            out["s"][step] = [{k: (v.cpu() if torch.is_tensor(v) else v)
                               for k, v in opt.state[p].items()} for p in ps]
    _feed(opt, ps, grads, 1, record)
    torch.cuda.synchronize()
    return out


_first_run = functools.lru_cache(maxsize=None)(_run)       # shared by the tests below


def _excess(got, want):
    """how far beyond 4 ulp * max(1, |want|) the difference goes (<= 0: within)"""
    got, want = got.double(), torch.as_tensor(want).double()
    return float(((got - want).abs() - 4 * ULP * want.abs().clamp_min(1.0)).max())


def _check_state(case, states, fx, step):
    cls = R.CASES[case][0]
    for k, st in enumerate(states):
        assert int(st["step"]) == int(fx[f"s{step}_{k}_step"]) == step - (3 if k == R.LATE else 0)
        for key in R.STATE_KEYS[cls]:
            a, b = st[key], torch.from_numpy(fx[f"s{step}_{k}_{key}"])
            if key == "slow_buffer":            # a parameter: the parameters' bound
                assert _excess(a, b) <= 0.02 * R.LR, (step, k, key)
            else:
                assert (a - b).abs().max() <= 1e-5 * b.abs().max(), (step, k, key)


@pytest.mark.parametrize("case", list(R.CASES))
def test_fused_matches_the_reference_fixture(case):
    fx = _fx("optim_" + case)
    run = _first_run(case)
    worst = -1.0
    for step in R.CHECKPOINTS:
        for k, p in enumerate(run["p"][step]):
            worst = max(worst, _excess(p, fx[f"p{step}_{k}"]))
    print(f"{case}: max param diff beyond 4 ulps, in units of lr: {worst / R.LR:.4f}")
    assert worst <= 0.02 * R.LR
    for step in R.STATE_AT:
        _check_state(case, run["s"][step], fx, step)
    assert int(run["s"][14][R.LATE]["step"]) == 11
    assert set(run["s"][14][0]) == {"step"} | set(R.STATE_KEYS[R.CASES[case][0]])


def test_radam_without_sgd_leaves_parameters_bitwise_alone_through_step_5():
    params, _ = _inputs()
    run = _first_run("radam_nosgd")
    for step in range(1, 6):
        for k, p in enumerate(run["p"][step]):
            assert torch.equal(p, torch.from_numpy(params[k])), (step, k)
    for k, st in enumerate(run["s"][5]):
        assert st["exp_avg"].abs().max() > 0 and st["exp_avg_sq"].abs().max() > 0
        assert int(st["step"]) == (2 if k == R.LATE else 5)
    moved = [not torch.equal(p, torch.from_numpy(params[k])) for k, p in enumerate(run["p"][6])]
    assert moved == [k != R.LATE for k in range(len(params))]


@pytest.mark.parametrize("case", ["radam_wd", "ranger_wd"])
def test_two_runs_are_bitwise_equal(case):
    a, b = _first_run(case), _run(case)
    for step in (5, 6, 12, 14):
        for x, y in zip(a["p"][step], b["p"][step]):
            assert torch.equal(x, y)
    for sa, sb in zip(a["s"][14], b["s"][14]):
        for key in R.STATE_KEYS[R.CASES[case][0]]:
            assert torch.equal(sa[key], sb[key])


def _continue_from(case, params7, states7, grads):
    """a fresh optimizer on the step-7 parameters, the step-7 state loaded through
    load_state_dict in the reference's form (its keys, Python-int steps, host
    tensors), run over steps 8..14"""
    ps = [torch.nn.Parameter(torch.as_tensor(p).clone().to(DEV)) for p in params7]
    opt = _make(case, ps)
    sd = opt.state_dict()
    sd["state"] = {k: {key: (int(v) if key == "step" else torch.as_tensor(v).clone())
                       for key, v in st.items()} for k, st in enumerate(states7)}
    opt.load_state_dict(sd)
    out = {}

    def record(step):
        if step == 14:
            out["p"] = [p.detach().cpu() for p in ps]
            out["s"] = [{k: (v.cpu() if torch.is_tensor(v) else v)
                         for k, v in opt.state[p].items()} for p in ps]
    _feed(opt, ps, grads[7:], 8, record)
    return out


def test_ranger_state_moves_both_ways():
    case = "ranger_wd"
    fx = _fx("optim_" + case)
    _, grads = _inputs()
    keys = ("step",) + R.STATE_KEYS["Ranger"]
    n = len(R.SHAPES)
    # the reference's state into the fused optimizer: parity with the reference at 14
    got = _continue_from(case, [fx[f"p7_{k}"] for k in range(n)],
                         [{key: fx[f"s7_{k}_{key}"] for key in keys} for k in range(n)], grads)
    worst = max(_excess(p, fx[f"p14_{k}"]) for k, p in enumerate(got["p"]))
    print(f"continued from the reference's state: {worst / R.LR:.4f} lr beyond 4 ulps")
    assert worst <= 0.02 * R.LR
    _check_state(case, got["s"], fx, 14)
    # the fused optimizer's own state through the same form: bit for bit the straight run
    run = _first_run(case)
    again = _continue_from(case, run["p"][7], run["s"][7], grads)
    for k in range(n):
        assert torch.equal(again["p"][k], run["p"][14][k]), k
        for key in R.STATE_KEYS["Ranger"]:
            assert torch.equal(again["s"][k][key], run["s"][14][k][key]), (k, key)
        assert again["s"][k]["step"] == run["s"][14][k]["step"]


@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("wd", [0.0, 1e-2])
def test_fused_sgd_matches_torch(momentum, wd):
    from nerf_pl_amd.optim import FusedSGD
    params, grads = _inputs()
    ref = [torch.from_numpy(p).clone().requires_grad_(True) for p in params]
    ours = [torch.nn.Parameter(torch.from_numpy(p).to(DEV)) for p in params]
    o_ref = torch.optim.SGD(ref, lr=R.LR, momentum=momentum, weight_decay=wd, foreach=False)
    o_our = FusedSGD(ours, lr=R.LR, momentum=momentum, weight_decay=wd)
    for gs in grads[:6]:                     # tensor 4 joins at step 4: its buffer's first step
        for r, q, g in zip(ref, ours, gs):
            r.grad = None if g is None else torch.from_numpy(g)
            q.grad = None if g is None else torch.from_numpy(g).to(DEV)
        o_ref.step()
        o_our.step()
    worst = max(_excess(q.detach().cpu(), r.detach()) for r, q in zip(ref, ours))
    print("max param diff beyond 4 ulps, in units of lr:", worst / R.LR)
    assert worst <= 0.02 * R.LR
    assert not torch.equal(ours[0].detach().cpu(), torch.from_numpy(params[0]))
    for r, q in zip(ref, ours):
        if momentum == 0.0:
            assert "momentum_buffer" not in o_our.state[q]
        else:
            a, b = o_our.state[q]["momentum_buffer"].cpu(), o_ref.state[r]["momentum_buffer"]
            assert (a - b).abs().max() <= 1e-5 * b.abs().max()


def _many_tensors():
    """50 tensors of 1..7 elements and an empty one; every other one is a slice
    of one buffer at an offset that is no multiple of 4 elements, so whole
    chunks of misaligned tensors (element by element) sit beside aligned ones"""
    g = torch.Generator().manual_seed(7)
    sizes = [1 + (k * 3) % 7 for k in range(50)] + [0]
    flat_p = torch.randn(4 * len(sizes) * 8, generator=g).to(DEV)
    ps, off = [], 1
    for k, n in enumerate(sizes):
        if k % 2:
            ps.append(torch.nn.Parameter(flat_p[off:off + n]))
            off += n + (2 if (off + n + 2) % 4 else 3)
        else:
            ps.append(torch.nn.Parameter(torch.randn(n, generator=g).to(DEV)))
    assert any(p.data_ptr() % 16 and p.numel() >= 4 for p in ps)
    assert any(p.data_ptr() % 16 == 0 and p.numel() >= 4 for p in ps)
    grads = [[torch.randn(n, generator=g) * 10.0 ** (k % 4 - 2) for k, n in enumerate(sizes)]
             for _ in range(7)]
    return ps, grads


@pytest.mark.parametrize("kind", ["sgd", "radam", "ranger"])
def test_more_tensors_than_one_launch_takes(kind):
    from nerf_pl_amd import _lib_optim
    from nerf_pl_amd.optim import FusedRAdam, FusedRanger, FusedSGD
    ps, grads = _many_tensors()
    assert len(ps) == 51 > _lib_optim.lib().nr_optim_max_tensors()
    init = [p.detach().cpu().numpy() for p in ps]
    if kind == "sgd":
        opt, ref = (FusedSGD(ps, lr=R.LR, momentum=0.9, weight_decay=1e-2),
                    R.SGD(init, R.LR, momentum=0.9, weight_decay=1e-2))
    elif kind == "radam":
        opt, ref = (FusedRAdam(ps, lr=R.LR, weight_decay=1e-2),
                    R.RAdam(init, R.LR, weight_decay=1e-2))
    else:
        opt, ref = (FusedRanger(ps, lr=R.LR, eps=1e-8, weight_decay=1e-2),
                    R.Ranger(init, R.LR, eps=1e-8, weight_decay=1e-2))
    for gs in grads:                                   # 7 steps: a lookahead sync at 6
        for p, g in zip(ps, gs):
            p.grad = g.to(DEV)
        opt.step()
        ref.step([g.numpy() for g in gs])
    worst = max([_excess(p.detach().cpu(), torch.from_numpy(r))
                 for p, r in zip(ps, ref.params) if r.size])
    print(f"{kind}: max param diff beyond 4 ulps, in units of lr: {worst / R.LR:.4f}")
    assert worst <= 0.02 * R.LR
    assert all(not np.array_equal(p.detach().cpu().numpy(), i) for p, i in zip(ps, init) if i.size)
    assert all(p._version >= 7 for p in ps)            # the raw-pointer writes are announced


def _train(pipelined, steps, optimizer, **kw):
    """the setting of tests/test_gpu_pipeline.py: 1,024 rays, 64 + 64 samples"""
    from nerf_pl_amd import Embedding, NeRF, optim, render_rays
    from nerf_pl_amd.losses import MSELoss
    from nerf_pl_amd.pipeline import PipelinedStep
    from nerf_pl_amd.rays import RaySampler, blender_focal, pose_spherical
    W = 64
    poses = torch.stack([pose_spherical(-180.0 + 45.0 * k, -30.0, 4.0) for k in range(8)]).to(DEV)
    torch.manual_seed(1234)
    pool = torch.rand(8 * W * W, 3, device=DEV)
    sampler = RaySampler(poses, W, W, blender_focal(W), 1.0, 200.0, rgb_pool=pool, seed=99)
    torch.manual_seed(0)
    models = [NeRF().to(DEV), NeRF().to(DEV)]
    init = [p.detach().clone() for m in models for p in m.parameters()]
    emb = [Embedding(3, 10), Embedding(3, 4)]
    loss_fn = MSELoss()
    torch.manual_seed(4321)

    def step_loss():
        rays, rgbs = sampler.next(1024)
        res = render_rays(models, emb, rays, 64, False, 1.0, 1.0, 64, 32768, False, False)
        return loss_fn(res, rgbs)

    losses = []
    cls = {"sgd": optim.FusedSGD, "radam": optim.FusedRAdam, "ranger": optim.FusedRanger}[optimizer]
    if pipelined:
        ps = PipelinedStep(models, lr=5e-4, eps=1e-8, optimizer=optimizer, **kw)
        assert type(ps.opt_c) is type(ps.opt_f) is cls
        try:
            for _ in range(steps):
                losses.append(ps(step_loss).detach())
        finally:
            ps.remove()
    else:
        if optimizer != "sgd":
            kw = dict(kw, eps=1e-8)
        opt = cls([p for m in models for p in m.parameters()], lr=5e-4, **kw)
        for _ in range(steps):
            loss = step_loss()
            opt.zero_grad(set_to_none=True)
            loss.backward()
            opt.step()
            losses.append(loss.detach())
    torch.cuda.synchronize()
    return [p.detach().clone() for m in models for p in m.parameters()], torch.stack(losses), init


@pytest.mark.parametrize("optimizer,kw", [("ranger", {}), ("sgd", {"momentum": 0.9})],
                         ids=["ranger", "sgd"])
def test_pipelined_step_with_another_optimizer_matches_sequential_bitwise(optimizer, kw):
    ref, ref_loss, init = _train(False, 7, optimizer, **kw)     # 7 steps: a sync at 6
    got, got_loss, _ = _train(True, 7, optimizer, **kw)
    assert torch.equal(ref_loss, got_loss), (ref_loss, got_loss)
    assert len(ref) == len(got) == 48
    for i, (a, b) in enumerate(zip(ref, got)):
        assert torch.equal(a, b), f"parameter {i}: max |diff| {float((a - b).abs().max()):.3g}"
    assert any(not torch.equal(a, b) for a, b in zip(init, got))


def test_pipelined_step_refuses_what_it_does_not_know():
    models = [torch.nn.Linear(2, 2).to(DEV), torch.nn.Linear(2, 2).to(DEV)]
    from nerf_pl_amd.pipeline import PipelinedStep
    with pytest.raises(ValueError, match="lamb"):
        PipelinedStep(models, optimizer="lamb")
    with pytest.raises(TypeError):
        PipelinedStep(models, momentum=0.9)             # Adam takes no such argument
