"""tests/exact_net.py on the CPU: the float64 reference against torch autograd
of the oracle MLP entry for entry, the certificate on every case the GPU file
(tests/test_gpu_exact.py) runs and on one deliberately inadmissible input per
rule, and the non-degeneracy of the networks (conditions on the reference:
an exact comparison of a dead network would prove nothing)."""
import pytest
import torch

import exact_net as E
from oracle import nerf_oracle as O


def _autograd(p, x, g, sigma_only=False):
    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    out = O.nerf_forward(pr, x[:, :63].contiguous() if sigma_only else x, sigma_only=sigma_only)
    (out * g).sum().backward()
    return out.detach(), {k: v.grad for k, v in pr.items()}


@pytest.mark.parametrize("kind,inp,mode,sigma_only", [
    ("general", "emb", "mixed", False), ("general", "emb", "sigma", False),
    ("twin", "emb", "mixed", False), ("twin", "emb", "rgb", False),
    ("twin", "rays", "mixed", False), ("twin", "rays", "mixed", True),
    ("general", "rays", "sigma", True)])
def test_reference_equals_float64_autograd(kind, inp, mode, sigma_only):
    """all 24 (sigma-only: 18) parameter gradients and the output, entry for
    entry; the six a sigma-only graph does not reach stay None in autograd"""
    c = E.case("int", 851, kind, inp, mode, "scattered", sigma_only)
    out, grads = _autograd(c["p"], c["x"], c["g"], sigma_only)
    assert torch.equal(out, c["ref"]["out"])
    for k in c["p"]:
        if sigma_only and k in E.SIGMA_ONLY_UNUSED:
            assert grads[k] is None and k not in c["ref"]["grads"], k
        else:
            assert torch.equal(grads[k], c["ref"]["grads"][k]), k
    assert len(c["ref"]["grads"]) == (18 if sigma_only else 24)


@pytest.mark.parametrize("family", ["frac", "wide8", "wide5", "widedir"])
def test_reference_equals_float64_autograd_wide_operands(family):
    c = E.case(family, 129)
    out, grads = _autograd(c["p"], c["x"], c["g"])
    assert torch.equal(out, c["ref"]["out"])
    for k in c["p"]:
        assert torch.equal(grads[k], c["ref"]["grads"][k]), k


def test_certificate_holds_for_every_gpu_case():
    specs = E.backward_specs() + E.forward_specs()
    assert len({E.spec_id(s) for s in specs}) == len(specs)
    for s in specs:
        assert s["arith"] in E.FAMILIES[s["family"]][0] and s["n"] in E.FAMILIES[s["family"]][1]
        cert = E.certify_case(s["arith"], E.spec_case(s))
        assert cert.ok, (E.spec_id(s), cert.failures)
    # the large size runs in the combinations named in exact_net.LARGE only
    assert sorted((s["arith"], s["inp"], s["path"], s["w4"]) for s in E.backward_specs()
                  if s["n"] > 1000) == sorted(E.LARGE)


def _refused(arith, p, x, g, needle):
    cert = E.certify(arith, p, x, g)
    assert not cert.ok and any(needle in f for f in cert.failures), (needle, cert.failures)


def _widths_pass(arith, p, x):
    return not any("operand widths" in f for f in E.certify(arith, p, x, None).failures)


def test_certificate_refuses_one_input_per_rule():
    n = 129
    c = E.case("int", n)
    p, x, g = c["p"], c["x"], c["g"]
    assert all(E.certify(a, p, x, g) for a in E.ARITHS)
    # widths.  f16x3: a 23-bit input (> 22); 12-bit inputs against the 12-bit
    # weights of a wide family (both > 11: lo*lo is dropped).  bf16x6: a 17-bit
    # input against 12-bit weights (outside (16, 16) and (24, 8)).  bf16: a
    # 9-bit input
    x23 = x.clone()
    x23[0, 0] = 1 + 2.0 ** -22
    _refused("f16x3", p, x23, g, "fwd xyz_encoding_1.0: operand widths")
    x12 = x.clone()
    x12[:, :63] = E.embedded_input(n, 11, seed=5)[:, :63]
    pw = E.net("twin", wide="xyz_encoding_5.0")
    _refused("f16x3", pw, x12, g, "fwd xyz_encoding_5.0: operand widths")
    x17 = x.clone()
    x17[0, 1] = 1 + 2.0 ** -16
    _refused("bf16x6", pw, x17, g, "fwd xyz_encoding_5.0: operand widths")
    assert _widths_pass("bf16x6", p, x17)                  # (8, 24): +-1 weights
    x9 = x.clone()
    x9[0, 0] = 1 - 2.0 ** -9
    _refused("bf16", p, x9, g, "fwd xyz_encoding_1.0: operand widths")
    assert _widths_pass("bf16x6", p, x9)
    # the sum of |term|: q = 6 holds at n = 851 and fails at 31,049 -- shown
    # here on the gradient, 2^13 times larger at n = 129
    for a in E.ARITHS:
        _refused(a, p, x, g * 2.0 ** 13 + g, "sum of |term|")
    # ranges
    big = {k: v.clone() for k, v in p.items()}
    big["xyz_encoding_3.0.weight"][0, 0] = 255.0
    _refused("f16x3", big, x, g, "|w| reaches")
    xb = x.clone()
    xb[0, 0] = 65504.0
    _refused("f16x3", p, xb, None, "activation reaches")
    grow = {k: v.clone() for k, v in p.items()}
    grow["xyz_encoding_4.0.weight"][:, 7] = 2.0            # a column of W: a row of W^T
    _refused("f16x3", grow, x, g, "max-norm growth")
    tiny = x.clone()
    tiny[0, 0] = 2.0 ** -25
    _refused("f16x3", p, tiny, None, "lowest set bit")
    assert not any("lowest set bit" in f for f in E.certify("bf16x6", p, tiny, None).failures)


@pytest.mark.parametrize("family,n,kind,inp,mode", [
    ("int", 851, "twin", "emb", "mixed"), ("int", 851, "twin", "emb", "rgb"),
    ("int", 851, "twin", "emb", "sigma"), ("int", 851, "general", "emb", "sigma"),
    ("int", 851, "twin", "rays", "mixed"), ("int", 31049, "twin", "emb", "mixed"),
    ("frac", 851, "twin", "emb", "mixed"), ("int", 33, "twin", "emb", "mixed"),
    ("wide8", 129, "twin", "emb", "mixed")])
def test_networks_are_not_degenerate(family, n, kind, inp, mode):
    c = E.case(family, n, kind, inp, mode)
    r = c["ref"]
    for k, h in r["acts"].items():
        if k != "feat":
            on = (h > 0).double().mean().item()
            assert 0.2 <= on <= 0.8, (k, on)
    if kind == "twin":
        assert torch.count_nonzero(r["pre_rgb"]) == 0
        assert torch.all(r["out"][:, :3] == 0.5)
    if n >= 851:
        unreached = set()
        if mode == "sigma":      # a zero rgb gradient reaches neither final, dir nor rgb
            unreached = set(E.SIGMA_ONLY_UNUSED)
        if mode == "rgb":
            unreached = {"sigma.weight", "sigma.bias"}
        for k, gk in r["grads"].items():
            if k in unreached:
                assert torch.count_nonzero(gk) == 0, k
                continue
            m = E.trig_columns(k) if inp == "rays" else None
            gk = gk if m is None else gk[:, ~torch.from_numpy(m)]
            nz = (gk != 0).double().mean().item()
            assert nz >= 0.25, (k, nz)


def test_wide_operands_where_intended():
    """the fractional family's activations and the wide families' weights,
    downstream activations and upstream gradients exceed one 11-bit piece"""
    for n in E.FAMILIES["frac"][1]:
        r = E.case("frac", n)["ref"]
        assert max(E.width(r["acts"][f"h{i}"]) for i in range(1, 9)) >= 12
        assert E.width(r["acts"]["hdir"]) >= 12
        assert max(E.width(v) for v in r["dz"].values()) <= 11
    for fam, layer, down, up in (("wide8", "xyz_encoding_8.0", "h8", "h7"),
                                 ("wide5", "xyz_encoding_5.0", "h5", "h4"),
                                 ("widedir", "dir_encoding.0", "hdir", "feat")):
        c = E.case(fam, 129)
        assert E.width(c["p"][layer + ".weight"]) == 12
        assert E.width(c["ref"]["acts"][down]) >= 12
        assert E.width(c["ref"]["dz"][up]) >= 12
        src = "h8" if fam == "widedir" else f"h{int(layer[13]) - 1}"
        assert E.width(c["ref"]["acts"][src]) <= 11
