"""The numpy model of the in-kernel draws (tests/philox_ref.py) against the
published Philox4x32-10 known-answer vectors of Random123 (kat_vectors), and
the statistics of its draws for the seeds tests/test_gpu_philox.py uses.

The GPU uniforms must equal the model's bit for bit and the GPU normals sit
within 2^-20 (1 + radius) of the model's, so the figures checked here are the
kernels' own: each over N = 2^20 consecutive draws of a (seed, stream), inside
five standard deviations of its sampling distribution,

    uniform mean     0.5 +- 5 / sqrt(12 N)        (variance 1/12)
    normal mean      0   +- 5 / sqrt(N)
    normal variance  1   +- 5 sqrt(2 / N)         (var of a squared normal: 2)
    correlation      0   +- 5 / sqrt(N)           streams 2, 3 (u, jitter) and
                                                  1, 4 (coarse, fine noise)

with every uniform in [0, 1) and |normal| <= sqrt(48 ln 2) = 5.768, the
Box-Muller radius at the smallest u1 = 2^-24.
"""
import numpy as np
import pytest

import philox_ref as P

SEEDS = (0, 7, 2 ** 62 - 12345, 0x9E3779B97F4A7C15)
N = 1 << 20

KAT = [
    ((0x00000000,) * 4, (0x00000000,) * 2, "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("counter,key,expected", KAT, ids=["zeros", "ones", "pi"])
def test_known_answer_vectors(counter, key, expected):
    out = P.philox4x32(counter, key)
    assert " ".join(f"{int(w):08x}" for w in out) == expected


def test_known_answers_vectorised():
    """the same three through one array call (the way every test uses the model)"""
    ctr = [np.array([c[0][j] for c in KAT]) for j in range(4)]
    key = [np.array([c[1][j] for c in KAT]) for j in range(2)]
    out = np.stack(P.philox4x32(ctr, key), 1)
    exp = np.array([[int(w, 16) for w in c[2].split()] for c in KAT], dtype=np.uint64)
    np.testing.assert_array_equal(out, exp)


def test_contract_layout():
    """index words, stream, kind and seed words land where the header says"""
    seed, idx = 0x0123456789ABCDEF, (5 << 32) | 9
    for kind in (P.UNIFORM, P.NORMAL):
        got = P.words(seed, 3, [idx], kind)
        exp = P.philox4x32((9, 5, 3, kind), (0x89ABCDEF, 0x01234567))
        assert [int(a[0]) for a in got] == [int(b) for b in exp]
    x = int(P.words(seed, 3, [idx], P.UNIFORM)[0][0])
    u = P.uniform(seed, 3, [idx])
    assert u.dtype == np.float32 and float(u[0]) == (x >> 8) / 2.0 ** 24
    x, y = (int(w[0]) for w in P.words(seed, 3, [idx], P.NORMAL)[:2])
    r = np.sqrt(-2.0 * np.log(((x >> 8) + 1) / 2.0 ** 24))
    assert P.radius64(seed, 3, [idx])[0] == r
    assert P.normal64(seed, 3, [idx])[0] == r * np.cos(2.0 * np.pi * ((y >> 8) / 2.0 ** 24))


@pytest.mark.parametrize("seed", SEEDS, ids=hex)
def test_draw_statistics(seed):
    idx = np.arange(N, dtype=np.uint64)
    uni = {s: P.uniform(seed, s, idx).astype(np.float64) for s in P.STREAMS}
    nrm = {s: P.normal64(seed, s, idx) for s in P.STREAMS}
    band = 5.0 / np.sqrt(N)
    for s in P.STREAMS:
        u, g = uni[s], nrm[s]
        assert u.min() >= 0.0 and u.max() < 1.0, (s, u.min(), u.max())
        assert abs(u.mean() - 0.5) <= band / np.sqrt(12.0), (s, u.mean())
        assert np.isfinite(g).all()
        assert abs(g.mean()) <= band, (s, g.mean())
        assert abs(g.var() - 1.0) <= 5.0 * np.sqrt(2.0 / N), (s, g.var())
        assert np.abs(g).max() <= P.RADIUS_MAX, (s, np.abs(g).max())
    for a, b, draws in ((2, 3, uni), (1, 4, nrm)):
        r = np.corrcoef(draws[a], draws[b])[0, 1]
        assert abs(r) <= band, (a, b, r)
    # uniform and normal of one (stream, idx) differ in the counter's last word only
    assert abs(np.corrcoef(uni[1], nrm[1])[0, 1]) <= band


def test_radius_bounds():
    assert P.RADIUS_MAX == pytest.approx(np.sqrt(48.0 * np.log(2.0)), rel=1e-15)
    assert 5.76 < P.RADIUS_MAX < 5.77
