"""The f16x3 MLP kernels across their documented range contract:
|w| < 255, activations < 65504, max-norm growth of every W^T in the
data-gradient chain < 2^9, per-product error <= 3 * 2^-22 relative plus 2^-25
absolute per operand element.  The networks come from tests/range_net.py
(regimes near each clause, and three just past one clause each); everything
goes through ``functions.mlp_apply`` alone -- values that may be non-finite
never reach the sampling or compositing kernels.

Reference: float64 autograd of the oracle MLP (for the f16x3 legs at
``repr_h3`` of the packed weights).  Bound, per parameter tensor and per output
column, normwise:

    |ours - g64| / |g64|  <=  16 * max(floor32, 2^-23)

with floor32 the CPU fp32 oracle's own distance from float64 over the ten
floor points of tests/grad64.py.  bf16x6 and fp32 have no range limits and run
as controls.  Samples inside the kink band (range_net.KINK_BAND) get no output
gradient; the ReLU masks the forward saved must equal float64's on every other
sample, except within range_net.FLIP_BAND of a kink (dropped, counted, <= 1 %).

Largest measured deviation / bound per regime (MI355X, every-sample path,
(23, 37); the tensor it occurred on is in DESIGN.md 3):

    regime   f16x3   bf16x6  fp32
    init     0.155   0.180   0.227
    grown    0.098   0.111   0.143
    swing    0.155   0.188   0.227
    spiky    0.174   0.193   0.255
    hot      0.171   0.197   0.221
    tiny     0.776   0.167   0.214     (f16x3: layers 1-2, the 2^-25 floor on dz3's B values)

f16x3 on the other paths (sample list / deferred save / sigma-only): grown
0.086 / 0.086 / 0.083, swing 0.190 / 0.190 / 0.130; grown at (509, 61) 0.251.
tiny's per-entry floor ratio: 0.486.  Outside the contract (f16x3): over_w --
every output row NaN; over_act -- the 299 of 851 rows past 65504 NaN, the rest
within the bound; over_growth -- the gradients of layers 1-3 non-finite, the
rest within the bound (worst 0.57).

What these regimes do not pin: with this output gradient the data gradient
realises a growth of 2^5.2 per layer (swing, hot) against the max-norm bound of
2^8.8, so a kGT of 8 instead of 6 (mlp_bwd3.hip) still passes; dropping the
lo * hi product or packing with kWScale = 0 fails every f16x3 leg.
"""
import functools

import numpy as np
import pytest
import torch

import range_net as R
from grad64 import FLOOR_POINTS

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)

SMALL, LARGE = (23, 37), (509, 61)
MATHS = ("f16x3", "bf16x6", "fp32")
MASKED = [f"h{i}" for i in range(1, 9)] + ["hdir"]


def _flat(p):
    from nerf_pl_amd import packing
    return torch.cat([p[k].reshape(-1) for k in packing.param_shapes()]).to(DEV)


@functools.lru_cache(maxsize=None)
def _case(regime, size, half, sigma_only, n_points):
    """parameters, inputs, the screened output gradient (with ``half``: about
    half of the samples zeroed as well, as test_gpu_active's scattered case)
    and the fp32 floors -- computed once, shared, left unchanged"""
    inp = R.inputs(*size)
    p = R.build(regime)
    kink = R.certificate(p, inp["x64"])["kink"]
    assert kink.float().mean() <= 0.10, kink.sum()
    gout = inp["gout"].clone()
    gout[kink] = 0
    if half:
        gout[torch.rand(inp["n"], generator=torch.Generator().manual_seed(5)) < 0.5] = 0
    entry = {}
    floor, fout = R.floors(p, inp["x32"], inp["x64"], gout, points=FLOOR_POINTS[:n_points],
                           sigma_only=sigma_only, entry=entry)
    return dict(p=p, inp=inp, kink=kink, gout=gout, floor=floor, fout=fout, entry=entry)


def _reference_params(p, math):
    p64 = R.params64(p, math)
    if not all(torch.isfinite(v).all() for v in p64.values()):     # over_w: repr_h3(256)
        p64 = R.to64(p)
    return p64


def _net(p):
    from nerf_pl_amd import NeRF
    net = NeRF()
    net.load_state_dict(p)
    return net.to(DEV)


def _saved_masks(net, inp, monkeypatch):
    """the ReLU masks of a training forward (h > 0 of the saved activations,
    as grad64.mlp_flips reads them; every path's forward computes the same
    layers bit for bit)"""
    from nerf_pl_amd import functions, ops
    monkeypatch.setattr(functions, "_DEBUG", {})
    monkeypatch.setattr(functions, "DEFER_SAVE", "none")
    functions.mlp_apply(net, rays=inp["rays"].to(DEV), z=inp["z"].to(DEV), spr=inp["spr"])
    save, n, _ = functions._DEBUG["fwd_saves"][-1]
    seg = ops.save_segments(save, n)
    masks = {k: ops.saved_rows(seg[k], n, 128 if k == "hdir" else 256).cpu() > 0 for k in MASKED}
    monkeypatch.setattr(functions, "_DEBUG", None)
    return masks


def _run(regime, math, monkeypatch, size=SMALL, path="every", sigma_only=False, half=False,
         n_points=len(FLOOR_POINTS), check_masks=True):
    """one leg: (ours: out, grads), (float64: out, grads, records), case, dropped"""
    from nerf_pl_amd import functions, ops
    c = _case(regime, size, half, sigma_only, n_points)
    inp, p = c["inp"], c["p"]
    monkeypatch.setattr(ops, "MATH", math)
    net = _net(p)
    p64 = _reference_params(p, math)
    gout, dropped = c["gout"], 0
    if check_masks:
        bad, drop = R.flips(_saved_masks(net, inp, monkeypatch), p64, inp["x64"], c["kink"])
        assert not bad.any(), (f"{regime} {math}: saved ReLU masks differ from float64 outside the "
                               f"kink band on samples {torch.nonzero(bad).flatten()[:8].tolist()}")
        dropped = int(drop.sum())
        print(f"{regime} {math} {path}: {dropped} of {inp['n']} samples dropped (mask flips within 2^-16)")
        assert dropped <= 0.01 * inp["n"]
        if dropped:
            gout = gout.clone()
            gout[drop] = 0
    monkeypatch.setattr(functions, "ACTIVE_SAMPLES", path != "every")
    monkeypatch.setattr(functions, "DEFER_SAVE", "all" if path == "deferred" else "none")
    out = functions.mlp_apply(net, rays=inp["rays"].to(DEV), z=inp["z"].to(DEV), spr=inp["spr"],
                              sigma_only=sigma_only)
    assert net.__dict__["_nr_defer_last"] == (path == "deferred")
    out.backward((gout[:, 3:4] if sigma_only else gout).contiguous().to(DEV))
    torch.cuda.synchronize()
    ours = {k: q.grad.detach().cpu() for k, q in net.named_parameters() if q.grad is not None}
    o64, g64, recs = R.evaluate(p64, inp["x64"], gout, torch.float64, sigma_only, keep=True)
    assert set(ours) == set(g64)
    return (out.detach().cpu(), ours), (o64, g64, recs), c, dropped


def _forward_rows(out, o64, fout, sigma_only, finite_only=False):
    """[(deviation / bound, column, deviation, bound)] per output column"""
    rows = []
    for j, col in (((0, 3),) if sigma_only else tuple((c, c) for c in range(4))):
        got, ref = out[:, j].double(), o64[:, col]
        if finite_only:
            ok = torch.isfinite(got)
            if not ok.any():
                continue
            got, ref = got[ok], ref[ok]
        dev = ((got - ref).norm() / ref.norm()).item()
        rows.append((dev / R.bound(fout[col]), f"out[:, {col}]", dev, R.bound(fout[col])))
    return rows


def _assert_within(label, rows):
    rows = sorted(rows, key=lambda r: -r[0] if r[0] == r[0] else -np.inf)
    for r, k, dev, b in rows[:3]:
        print(f"RANGE {label} {k}: {dev:.3g} from float64, bound {b:.3g}, {r:.3f} of it")
    for r, k, dev, b in rows:
        assert dev <= b, f"{label} {k}: {dev:.3g} from float64, bound {b:.3g} ({r:.2f} of it)"


@pytest.mark.parametrize("regime", ["spiky", "tiny", "hot"])
def test_pack_h3_pieces_on_regime_weights(regime):
    """test_pack_h3_pieces' comparison on regime weights: fp32 head block
    (layer biases x 2^8), then for every weight w' = 256 w its pieces
    hi = f16(w'), lo = f16(w' - hi), bit for bit against torch's fp16 casts --
    254 (w' = 65024, the largest the contract admits), tiny's subnormal lo
    pieces and hot's large biases among them"""
    from nerf_pl_amd import ops, packing
    p = R.build(regime)
    flat = _flat(p)
    buf = ops.pack_fwd3(flat, math="f16x3").cpu()
    m, hm = packing.build_fwd3_map(2)
    head = buf[:packing.HEAD_BYTES].view(torch.float32).numpy()
    fl = flat.cpu().numpy()
    sc = np.where(np.arange(hm.size) < 8 * 256 + 256 + 128, 256.0, 1.0).astype(np.float32)
    np.testing.assert_array_equal(head, np.where(hm >= 0, fl[np.maximum(hm, 0)] * sc, 0))
    raw = buf[packing.HEAD_BYTES:].view(torch.int16).numpy()
    pieces = buf[packing.HEAD_BYTES:].view(torch.float16).float().numpy()
    assert pieces.size == m.size
    w = torch.from_numpy(fl) * 256
    hi = w.to(torch.float16)
    lo = (w - hi.float()).to(torch.float16)
    ref16 = torch.stack([hi, lo], 1)
    ref = ref16.float().numpy()
    ok = m >= 0
    np.testing.assert_array_equal(pieces[ok], ref[m[ok] >> 2, m[ok] & 3])
    # the bit patterns too (a float comparison takes -0 for 0)
    refbits = ref16.view(torch.int16).numpy()
    nz = ok & (pieces != 0)
    np.testing.assert_array_equal(raw[nz], refbits[m[nz] >> 2, m[nz] & 3])
    assert np.all(pieces[~ok] == 0)
    assert np.isfinite(pieces).all()
    # the packed weights (not the biases and heads, which stay fp32): hi + lo
    # is w to 2^-22 relative, 2^-33 absolute where lo is subnormal
    wi = np.unique(m[ok] >> 2)
    recon = ref.astype(np.float64).sum(1)[wi] / 256
    assert np.all(np.abs(recon - fl[wi]) <= 2.0 ** -22 * np.abs(fl[wi]) + 2.0 ** -33)
    np.testing.assert_array_equal(recon, R.repr_h3(torch.from_numpy(fl[wi])).numpy())
    if regime == "spiky":
        assert (pieces == 65024.0).sum() >= 2 and fl.max() == 254.0      # layers 3 and 6
    if regime == "tiny":
        sub = (pieces != 0) & (np.abs(pieces) < 2.0 ** -14)
        assert sub.sum() > 50000, sub.sum()      # most of layer 4's 65,536 lo pieces
    if regime == "hot":
        assert np.abs(head).max() > 1e5          # 256 x the cumulative-product biases


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("regime", R.IN_CONTRACT)
def test_forward_and_gradients_in_contract(regime, math, monkeypatch):
    """every in-contract regime x arithmetic at (23, 37): 851 samples, 26 full
    blocks and a ragged one, every-sample path; forward and all 24 parameter
    gradients against the bound"""
    (out, ours), (o64, g64, _), c, _ = _run(regime, math, monkeypatch)
    label = f"{regime} {math} every {SMALL}"
    assert len(g64) == 24
    _assert_within(label + " forward", _forward_rows(out, o64, c["fout"], False))
    _assert_within(label, R.deviations(ours, g64, c["floor"]))


@pytest.mark.parametrize("regime,path,size", [
    ("grown", "active", SMALL), ("grown", "deferred", SMALL), ("grown", "sigma_only", SMALL),
    ("swing", "active", SMALL), ("swing", "deferred", SMALL), ("swing", "sigma_only", SMALL),
    ("grown", "active", LARGE)])
def test_other_paths_f16x3(regime, path, size, monkeypatch):
    """f16x3 through the sample list, the deferred save and the sigma-only
    graph, with about half of the output gradient's rows zeroed; grown once at
    (509, 61) = 31,049 samples, where the weight gradient's per-layer scale
    meets the split-K slabs (floor over three points there)"""
    so = path == "sigma_only"
    (out, ours), (o64, g64, _), c, _ = _run(
        regime, "f16x3", monkeypatch, size=size, path="active" if so else path, sigma_only=so,
        half=True, n_points=3 if size == LARGE else len(FLOOR_POINTS))
    label = f"{regime} f16x3 {path} {size}"
    assert len(g64) == (18 if so else 24)
    _assert_within(label + " forward", _forward_rows(out, o64, c["fout"], so))
    _assert_within(label, R.deviations(ours, g64, c["floor"]))


def test_tiny_weight_gradient_meets_the_absolute_floor(monkeypatch):
    """The contract's absolute floor where it bites: in ``tiny`` the h-columns
    of xyz_encoding_5.0.weight's gradient are sum_s dz5[s, i] h4[s, k] with h4
    ~ 5e-5, below fp16's normal range, so the unscaled activation operand is
    split on fp16's subnormal grid (spacing 2^-24).  Per entry

        |ours - g64| <= 2^-25 sum_s |dz5[s, i]| + 3 * 2^-22 sum_s |dz5[s, i] h4[s, k]|
                        + C * (the fp32 oracle's own error on that entry),

    dz5 and h4 from float64: the documented floor, not exceeded."""
    (_, ours), (_, g64, recs), c, _ = _run("tiny", "f16x3", monkeypatch)
    name, hin, pre = recs[4]
    assert name == "h5"
    dz5 = pre.grad.abs()                       # (n, 256)
    h4 = hin.detach()[:, R.XYZ_CH:].abs()      # (n, 256)
    assert 0 < h4.max() < 2.0 ** -14
    key = "xyz_encoding_5.0.weight"
    err = (ours[key].double() - g64[key])[:, R.XYZ_CH:].abs()
    floor_term = 2.0 ** -25 * dz5.sum(0)[:, None].expand(-1, 256)
    prod_term = 3 * 2.0 ** -22 * (dz5.T @ h4)
    bound = floor_term + prod_term + R.C * c["entry"][key][:, R.XYZ_CH:]
    ratio = (err / bound).max().item()
    rel = (err.norm() / g64[key][:, R.XYZ_CH:].norm()).item()
    share = (floor_term / bound).median().item()
    print(f"RANGE tiny floor: worst |ours - g64| / bound = {ratio:.3f}; the h-columns are {rel:.3g} "
          f"from float64 normwise; the 2^-25 term is {share:.2f} of the bound (median)")
    assert (err <= bound).all(), ratio


@pytest.mark.parametrize("math", MATHS)
@pytest.mark.parametrize("regime", R.OUT_OF_CONTRACT)
def test_outside_the_contract_is_loud(regime, math, monkeypatch):
    """one clause broken each: bf16x6 and fp32 (no range limits) meet the
    ordinary bound; for f16x3 every output entry is non-finite or within the
    bound, and every gradient tensor holds a non-finite entry or is within
    the bound -- never a finite wrong value"""
    (out, ours), (o64, g64, _), c, _ = _run(regime, math, monkeypatch, check_masks=False)
    label = f"{regime} {math} every {SMALL}"
    assert torch.isfinite(c["gout"]).all()
    if math != "f16x3":
        _assert_within(label + " forward", _forward_rows(out, o64, c["fout"], False))
        _assert_within(label, R.deviations(ours, g64, c["floor"]))
        return
    bad_rows = int((~torch.isfinite(out)).any(1).sum())
    loud = sorted(k for k, v in ours.items() if not torch.isfinite(v).all())
    print(f"RANGE {label}: {bad_rows} of {out.shape[0]} output rows non-finite; "
          f"{len(loud)} of 24 gradient tensors non-finite: {loud}")
    _assert_within(label + " forward (finite entries)",
                   _forward_rows(out, o64, c["fout"], False, finite_only=True))
    quiet = {k: v for k, v in ours.items() if k not in loud}
    _assert_within(label, R.deviations(quiet, {k: g64[k] for k in quiet}, c["floor"]))
