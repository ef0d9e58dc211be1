"""The range regimes of tests/range_net.py, checked on the host: where each
network sits in the f16x3 contract, how many samples its kink
band screens, that the float64 reference and the fp32 floor are usable, and
what repr_h3 represents."""
import numpy as np
import pytest
import torch

import range_net as R

SMALL, LARGE = (23, 37), (509, 61)

# regime: max |w|, max activation, max W^T growth in the data-gradient chain
# (float64, at the (23, 37) inputs), to three significant digits
TABLE = {
    "init": (0.126, 2.33, 8.86),
    "grown": (0.630, 1539, 44.3),
    "swing": (4.03, 74.5, 448),
    "spiky": (254, 207, 262),
    "hot": (31.5, 27280, 437),
    "tiny": (0.126, 2.33, 8.86),
    "over_w": (256, 207, 264),
    "over_act": (126, 1.09e5, 437),
    "over_growth": (112, 237, 1.6e4),
}
BROKEN = {"over_w": "w", "over_act": "act", "over_growth": "growth"}


def _sig3(v):
    return float(f"{v:.3g}")


@pytest.fixture(scope="module")
def certs():
    x = R.inputs(*SMALL)["x64"]
    return {r: R.certificate(R.build(r), x) for r in R.REGIMES}


@pytest.mark.parametrize("regime", R.REGIMES)
def test_certificate_matches_the_table(regime, certs):
    c = certs[regime]
    got = (c["max_w"], c["max_act"], c["max_growth"])
    assert tuple(map(_sig3, got)) == tuple(map(_sig3, TABLE[regime])), got
    broken = [k for k, v in R.clauses(c).items() if v]
    if regime in R.IN_CONTRACT:
        assert broken == []
        assert c["max_act"] < 32768
    else:
        assert broken == [BROKEN[regime]]


def test_regimes_are_what_they_say(certs):
    """swing is the same function as init; tiny's h4 lies below fp16's
    smallest normal and its 256 w have subnormal lo pieces; spiky holds 254
    exactly; grown's sigma reaches 262"""
    x = R.inputs(*SMALL)["x64"]
    with torch.no_grad():
        o_init = R.layers64(R.to64(R.build("init")), x)[0]
        o_swing = R.layers64(R.to64(R.build("swing")), x)[0]
    # (x 56 and / 56 round the fp32 weights: ~6e-8 relative each)
    assert (o_init - o_swing).abs().max() < 1e-6
    assert 0 < certs["tiny"]["acts"]["h4"] < 2.0 ** -14
    s = R.build("tiny")["xyz_encoding_4.0.weight"] * 256
    lo = s - s.half().float()
    assert ((lo != 0) & (lo.abs() < 2.0 ** -14)).float().mean() > 0.9
    assert (R.build("spiky")["xyz_encoding_3.0.weight"] == 254).sum() == 1
    assert (R.build("over_w")["xyz_encoding_3.0.weight"] == 256).sum() == 1
    assert _sig3(certs["grown"]["sigma"]) == 262


@pytest.mark.parametrize("size", [SMALL, LARGE])
def test_screened_share(size):
    x = R.inputs(*size)["x64"]
    for r in R.REGIMES:
        share = R.certificate(R.build(r), x)["kink"].float().mean().item()
        print(f"{size} {r}: {100 * share:.2f} % screened")
        assert 0 < share <= 0.10, (r, share)


@pytest.mark.parametrize("regime", R.REGIMES)
def test_reference_and_floor_are_usable(regime, certs):
    """with the screened gradient every float64 tensor norm is nonzero and
    every floor finite (and nonzero: the fp32 oracle is not float64)"""
    inp = R.inputs(*SMALL)
    p = R.build(regime)
    gout = inp["gout"].clone()
    gout[certs[regime]["kink"]] = 0
    for math in ("fp32", "f16x3"):
        if math == "f16x3" and regime == "over_w":
            continue      # repr_h3(256) is non-finite: that leg has no f16x3 reference
        out, g64, _ = R.evaluate(R.params64(p, math), inp["x64"], gout, torch.float64)
        assert len(g64) == 24
        assert all(torch.isfinite(v).all() and v.norm() > 0 for v in g64.values())
        assert torch.isfinite(out).all() and (out.norm(dim=0) > 0).all()
    floor, fout = R.floors(p, inp["x32"], inp["x64"], gout, points=R.FLOOR_POINTS[:3])
    assert all(np.isfinite(v) and v > 0 for v in floor.values()), floor
    assert np.isfinite(fout).all() and (fout > 0).all()
    print(regime, "floor32 min / median / max",
          f"{min(floor.values()):.3g} {np.median(list(floor.values())):.3g} {max(floor.values()):.3g}")


def test_repr_h3():
    g = torch.Generator().manual_seed(0)
    # identity on values of at most 22 significant bits in range: 11 + 11 bits
    m = torch.randint(2 ** 21, 2 ** 22, (4096,), generator=g).double()
    # (256 w >= 2^-3 keeps the lo piece's last bit at or above fp16's 2^-24)
    e = torch.randint(-30, -14, (4096,), generator=g).double()      # |w| in [2^-9, 2^7)
    wd = m * torch.exp2(e) * (torch.randint(0, 2, (4096,), generator=g) * 2 - 1)
    w = wd.float()
    assert torch.equal(w.double(), wd)
    assert torch.equal(R.repr_h3(w), wd)
    assert R.repr_h3(254.0).item() == 254.0
    assert R.repr_h3(torch.tensor([-254.0, 0.0])).tolist() == [-254.0, 0.0]
    assert not torch.isfinite(R.repr_h3(256.0)).any()
    # any fp32 weight of the contract: within 2^-22 |w| + 2^-33
    w = (torch.randn(1 << 16, generator=g) * torch.exp2(torch.randint(-40, 8, (1 << 16,), generator=g))).float()
    w = w[w.abs() < 255]
    err = (R.repr_h3(w) - w.double()).abs()
    assert (err <= 2.0 ** -22 * w.double().abs() + 2.0 ** -33).all()
    for r in ("spiky", "tiny", "hot"):
        for k in R.SPLIT_WEIGHTS:
            w = R.build(r)[k]
            assert ((R.repr_h3(w) - w.double()).abs() <= 2.0 ** -22 * w.double().abs() + 2.0 ** -33).all()
