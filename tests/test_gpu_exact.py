"""The fused MLP kernels (forward, data gradient, weight gradient) bit for bit
on integer-valued networks (tests/exact_net.py; DESIGN.md 3 "Exactness
contract").

On certified inputs every product the kernels form is exact and every fp32
partial sum is a multiple of one quantum below 2^24 quanta, so the result does
not depend on the summation order -- split-K slabs, the every-sample, active
and deferred paths, the LDS-DMA or the register-staged weight gradient, any
arithmetic -- and the float64 reference is the exact answer.  Every comparison
here is ``==`` on every entry of every parameter gradient, output and saved
activation: no tolerance, no ReLU-kink screening (a pre-activation of exactly
0 is "off" on both sides).  A reordering optimisation keeps passing; a wrong
index, mask bit, tail, scale or dropped term (or a dropped lo piece: the
"frac" and "wide*" families) fails.  Each test asserts the certificate before
it launches anything.

Two comparisons are inexact by nature, with the project's own bounds: the rgb
output of the "general" network (a sigmoid; 2e-5, the bound of
test_mlp_forward_embedded_and_sigma_only) and, in the ray input, the weight
gradient's zero-weight sin / cos columns (sum dz sin; 2e-4 max|ref|, the bound
of test_mlp_backward_matches_autograd).

n = 31,049 (the integer family only) runs in the combinations of
exact_net.LARGE: f16x3 embedded active, fp32 embedded every-sample, bf16
embedded every-sample, f16x3 rays every-sample, f16x3 rays active with the
register-staged weight gradient, bf16x6 rays deferred.
"""
import numpy as np
import pytest
import torch

import exact_net as E

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _exact(label, got, ref):
    """got == ref on every entry; on a mismatch the message gives the count,
    the largest difference in quanta (lowest set bit of the reference tensor)
    and its position"""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    if torch.equal(got, ref):
        return
    d = (got - ref).abs()
    d[got != got] = float("inf")
    i = int(d.argmax())
    pos = tuple(int(v) for v in np.unravel_index(i, tuple(ref.shape))) if ref.dim() else ()
    quantum = E.lowbit(ref) if bool(ref.any()) else 1.0
    raise AssertionError(
        f"{label}: {int((d != 0).sum())} of {ref.numel()} entries differ; largest |diff| "
        f"{d.reshape(-1)[i].item():.6g} = {d.reshape(-1)[i].item() / quantum:.6g} quanta at {pos}: "
        f"got {got.reshape(-1)[i].item()!r}, reference {ref.reshape(-1)[i].item()!r}")


def _model(p):
    from nerf_pl_amd import NeRF
    m = NeRF()
    m.load_state_dict({k: v.float() for k, v in p.items()})
    return m.to(DEV)


def _inputs(c):
    """keyword arguments of mlp_apply / mlp_forward for a case"""
    if "rays" in c:
        return dict(rays=c["rays"].float().to(DEV), z=c["z"].float().to(DEV)), c["spr"]
    return dict(x=c["x"].float().to(DEV)), 0


def _check_out(c, out, kind):
    ref = c["ref"]["out"]
    _exact("sigma", out[:, 3], ref[:, 3])
    if kind == "twin":
        assert torch.all(out[:, :3] == 0.5), "twin rgb must be exactly 0.5"
    else:
        err = (out[:, :3].cpu().double() - ref[:, :3]).abs().max().item()
        assert err < 2e-5, f"general rgb: {err:.3g} from float64"


def _check_save(c, sv, n, arith):
    """h1..h8 and hdir exact; the PE / dir slots exact where the input is (the
    embedded input: every channel; rays: the raw coordinates)"""
    from nerf_pl_amd import ops, packing
    seg = ops.save_segments(sv.cpu(), n)
    acts = c["ref"]["acts"]
    for i in range(1, 9):
        _exact(f"saved h{i}", ops.saved_rows(seg[f"h{i}"], n, 256), acts[f"h{i}"])
    _exact("saved hdir", ops.saved_rows(seg["hdir"], n, 128), acts["hdir"])
    x = c["x"]
    if arith == "fp32":      # packed k order: column 32h + g / 16h + g (mlp_fwd.hip ROWS)
        maps = (("pe", 64, [(32 * h + g, packing.PE_MAP[g, h]) for g in range(32) for h in (0, 1)], 0),
                ("dirpe", 32, [(16 * h + g, packing.DIR_MAP[g, h]) for g in range(16) for h in (0, 1)],
                 E.XYZ_CH))
    else:
        maps = (("pe", 64, list(enumerate(packing.PE16_MAP)), 0),
                ("dirpe", 32, list(enumerate(packing.DIR16_MAP)), E.XYZ_CH))
    for name, w, slots, x0 in maps:
        rows = ops.saved_rows(seg[name], n, w)
        for col, f in slots:
            if f < 0:
                assert torch.count_nonzero(rows[:, col]) == 0, (name, col)
            elif "rays" not in c or f < 3:
                _exact(f"saved {name} slot {col}", rows[:, col], x[:, x0 + f])


@pytest.mark.parametrize("s", E.forward_specs(), ids=E.spec_id)
def test_forward_is_exact(s, monkeypatch):
    """the inference call, the training call with a save buffer, the
    sigma_only inference call and (rays) sigma_points at the sample positions"""
    from nerf_pl_amd import functions, ops
    c = E.spec_case(s)
    cert = E.certify_case(s["arith"], c)
    assert cert.ok, cert.failures
    monkeypatch.setattr(ops, "MATH", s["arith"])
    m = _model(c["p"])
    kw, spr = _inputs(c)
    n = s["n"]
    with torch.no_grad():
        out = functions.mlp_apply(m, spr=spr, **kw)
    assert out.shape == (n, 4)
    _check_out(c, out, s["kind"])
    packed, _ = m.packed()
    assert ops.arith_of(packed) == s["arith"]
    out_t, sv = ops.mlp_forward(packed, samples_per_ray=spr, save=True, **kw)
    _check_out(c, out_t, s["kind"])
    if s["arith"] != "bf16":      # bf16 stores its save in bf16: ops.saved_rows does not decode it
        _check_save(c, sv, n, s["arith"])
    if "x" in kw:
        kw = dict(x=kw["x"][:, :E.XYZ_CH].contiguous())
    out_s, _ = ops.mlp_forward(packed, samples_per_ray=spr, sigma_only=True, **kw)
    assert out_s.shape == (n, 1)
    _exact("sigma_only sigma", out_s[:, 0], c["ref"]["out"][:, 3])
    if "rays" in c:      # integer points, zero trig weights
        sig = ops.sigma_points(packed, c["x"][:, :3].float().contiguous().to(DEV))
        _exact("sigma_points", sig, c["ref"]["out"][:, 3])


def _bf16_trig(c, name):
    """float64 weight gradient of a first-layer / skip / dir weight with the
    input operand rounded once to bf16, as the bf16 arithmetic documents
    (wgrad operands rb(dz), rb(x); dz is bf16-exact by the
    certificate): the reference of the inexact sin / cos columns there, whose
    2^-9 operand rounding is the arithmetic, not an error"""
    dz = c["ref"]["dz"][{"xyz_encoding_1.0.weight": "h1", "xyz_encoding_5.0.weight": "h5",
                         "dir_encoding.0.weight": "hdir"}[name]]
    x = c["x"][:, E.XYZ_CH:] if name.startswith("dir") else c["x"][:, :E.XYZ_CH]
    g = dz.T @ x.to(torch.bfloat16).double()
    out = c["ref"]["grads"][name].clone()
    if name.startswith("dir"):
        out[:, E.W:] = g
    else:
        out[:, :E.XYZ_CH] = g
    return out


@pytest.mark.parametrize("s", E.backward_specs(), ids=E.spec_id)
def test_backward_is_exact(s, monkeypatch):
    """all 24 parameter gradients (sigma-only graph: 18, the other six None)
    against the float64 reference, entry for entry"""
    from nerf_pl_amd import functions, ops
    c = E.spec_case(s)
    cert = E.certify_case(s["arith"], c)
    assert cert.ok, cert.failures
    monkeypatch.setattr(ops, "MATH", s["arith"])
    monkeypatch.setattr(functions, "ACTIVE_SAMPLES", s["path"] != "every")
    monkeypatch.setattr(functions, "DEFER_SAVE", "all" if s["path"] == "deferred" else "none")
    monkeypatch.setattr(functions, "SIGMA_TRAIN_KERNELS", s["so_kernels"])
    if s["arith"] == "f16x3":
        monkeypatch.setenv("NR_WGRAD_W4", str(s["w4"]))
    m = _model(c["p"])
    kw, spr = _inputs(c)
    so = s["sigma_only"]
    out = functions.mlp_apply(m, spr=spr, sigma_only=so, **kw)
    assert m.__dict__["_nr_defer_last"] == (s["path"] == "deferred")
    if so:
        _exact("sigma", out[:, 0], c["ref"]["out"][:, 0])
    else:
        _check_out(c, out.detach(), s["kind"])
    out.backward(c["g"].float().to(DEV))
    torch.cuda.synchronize()
    ref = c["ref"]["grads"]
    checked = 0
    for name, q in m.named_parameters():
        if so and name in E.SIGMA_ONLY_UNUSED:
            assert q.grad is None, name
            continue
        got = q.grad.detach().cpu().double()
        trig = E.trig_columns(name) if "rays" in c else None
        if trig is None:
            _exact(name, got, ref[name])
        else:
            # the ray input's sin / cos channels are inexact (their weights are
            # zero, their gradient columns sum dz sin): the raw-coordinate and
            # hidden-unit columns are exact, the trig columns bounded
            keep = torch.from_numpy(~trig)
            _exact(name, got[:, keep], ref[name][:, keep])
            want = _bf16_trig(c, name) if s["arith"] == "bf16" else ref[name]
            err = (got - want)[:, ~keep].abs().max().item()
            bound = 2e-4 * ref[name].abs().max().item()
            assert err <= bound, f"{name} trig columns: {err:.3g} from float64, bound {bound:.3g}"
        checked += 1
    assert checked == (18 if so else 24)
