"""Numpy model of the in-kernel random draws (test infrastructure, like
composite64.py): Philox4x32-10 as Salmon et al. define it ("Parallel random
numbers: as easy as 1, 2, 3", SC'11; the Random123 library), and the contract
the kernels put on top of it (include/nerf_pl_amd.h, nr_probe_rand):

    counter = (idx mod 2^32, idx >> 32, stream, 0 uniform | 1 normal)
    key     = (seed mod 2^32, seed >> 32)
    uniform = (x >> 8) * 2^-24                       x, y: output words 0, 1
    normal  = sqrt(-2 ln u1) cos(2 pi u2),  u1 = ((x >> 8) + 1) * 2^-24,
                                            u2 = (y >> 8) * 2^-24

Philox-4x32: one round maps the counter (c0, c1, c2, c3) under the round key
(k0, k1) through two 32x32 -> 64 bit products, p0 = M0 c0 and p1 = M1 c2, to

    (hi(p1) ^ c1 ^ k0,  lo(p1),  hi(p0) ^ c3 ^ k1,  lo(p0));

ten rounds, the key advanced by the Weyl constants (W0, W1) mod 2^32 between
rounds.  M0, M1 are the paper's multipliers, W0 = floor(2^32 (golden ratio -
1)) and W1 = floor(2^32 (sqrt(3) - 1)).

The uniform is exact in fp32 (24 bits times a power of two), so the model's
float32 is the kernel's bit for bit; the normal is evaluated in float64 from
the exact u1, u2 and is the reference the kernel's fp32 logf / sqrtf / cosf are
measured against (tests/test_gpu_philox.py).
"""
import numpy as np

ROUNDS = 10
MULTIPLIERS = (0xD2511F53, 0xCD9E8D57)
WEYL = (0x9E3779B9, 0xBB67AE85)
STREAMS = range(5)        # nerf_pl_amd.rng.STREAM_*
UNIFORM, NORMAL = 0, 1    # the counter's fourth word

_U64 = np.uint64
_LOW = _U64(0xFFFFFFFF)
_32 = _U64(32)


def _mulhilo(m, c):
    """(high, low) words of the 64-bit product of two 32-bit values"""
    p = _U64(m) * c
    return p >> _32, p & _LOW


def _round(ctr, key):
    hi0, lo0 = _mulhilo(MULTIPLIERS[0], ctr[0])
    hi1, lo1 = _mulhilo(MULTIPLIERS[1], ctr[2])
    return (hi1 ^ ctr[1] ^ key[0], lo1, hi0 ^ ctr[3] ^ key[1], lo0)


def _bump(key):
    return tuple((k + _U64(w)) & _LOW for k, w in zip(key, WEYL))


def philox4x32(counter, key, rounds=ROUNDS):
    """The four output words (uint64 arrays holding 32-bit values) of counter
    (four words) under key (two words); words broadcast against each other."""
    ctr = tuple(np.asarray(c, dtype=_U64) & _LOW for c in counter)
    key = tuple(np.asarray(k, dtype=_U64) & _LOW for k in key)
    for r in range(rounds):
        if r:
            key = _bump(key)
        ctr = _round(ctr, key)
    return ctr


def words(seed, stream, idx, kind):
    """Output words of the draw ``kind`` (UNIFORM / NORMAL) of ``stream`` at the
    64-bit indices ``idx`` under the 64-bit ``seed``"""
    seed = int(seed)
    assert 0 <= seed < 2 ** 64, seed
    idx = np.asarray(idx, dtype=_U64)
    return philox4x32((idx & _LOW, idx >> _32, stream, kind), (seed & 0xFFFFFFFF, seed >> 32))


def mantissa(word):
    """the 24 bits a draw keeps of an output word"""
    return (word >> _U64(8)).astype(np.int64)


def uniform(seed, stream, idx):
    """float32 in [0, 1), the kernels' value bit for bit"""
    x = words(seed, stream, idx, UNIFORM)[0]
    return (mantissa(x).astype(np.float64) * 2.0 ** -24).astype(np.float32)


def _u1_u2(seed, stream, idx):
    w = words(seed, stream, idx, NORMAL)
    return (mantissa(w[0]) + 1) * 2.0 ** -24, mantissa(w[1]) * 2.0 ** -24


def radius64(seed, stream, idx):
    """sqrt(-2 ln u1) in float64: 0 at u1 = 1, at most RADIUS_MAX"""
    u1, _ = _u1_u2(seed, stream, idx)
    return np.sqrt(-2.0 * np.log(u1))


def normal64(seed, stream, idx):
    """the Box-Muller normal in float64 from the exact u1, u2"""
    u1, u2 = _u1_u2(seed, stream, idx)
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(2.0 * np.pi * u2)


# the largest radius, at u1 = 2^-24: sqrt(48 ln 2) = 5.768...
RADIUS_MAX = float(np.sqrt(-2.0 * np.log(2.0 ** -24)))
