"""References and case lists for the helper kernels at the end of csrc/mdbn_kernels.hip (TEST-ONLY, no GPU needed to
import): tests/test_helpers_twin.py pins them on the CPU, tests/test_gpu_helpers.py holds the kernels to them.

    round_half_away(x)   tensor.round, exact in any dtype (oracle/rbm_np.py; restated here in rationals for the pin)
    bf16_rne_bits(u32)   float32 -> bfloat16 with round-to-nearest-even, in integer arithmetic on the bit patterns

The case lists are bit patterns (uint32): what the kernels are asked about is decided by single bits."""
from fractions import Fraction

import numpy as np

from oracle.rbm_np import round_half_away        # noqa: F401  (the reference the tests import from here)


def f32(bits):
    """uint32 patterns -> float32, bit for bit."""
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def bits32(x):
    """float32 -> uint32 patterns (a copy)."""
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()


def round_up4(n):
    return (int(n) + 3) // 4 * 4


# ------------------------------------------------------------------ tensor.round

BELOW_HALF = 0x3EFFFFFF          # the largest float32 below 0.5: 0.5 - 2^-25; + 0.5f is a tie that rounds to 1.0f

# magnitudes of the edge list; every one is used with both signs
ROUND_EDGE_BITS = np.array([
    0x00000000,                  # 0
    BELOW_HALF,
    0x3F000000,                  # 0.5
    0x3F000001,                  # the next float32 above 0.5
    0x3FC00000,                  # 1.5
    0x40200000,                  # 2.5
    0x3F400000,                  # 0.75
    0x4AFFFFFF,                  # 8388607.5 = 2^23 - 0.5, the last float32 with a fraction
    0x4B000000,                  # 8388608 = 2^23
    0x4B000001,                  # 8388609: + 0.5f is a tie that rounds to the even 8388610
    0x4B7FFFFF,                  # 16777215 = 2^24 - 1
    0x4B800000,                  # 16777216
    int(np.float32(3e38).view(np.uint32)),
    0x00800000,                  # the smallest normal
    0x00000123,                  # a subnormal
    0x7F800000,                  # inf
    0x7FC00000,                  # NaN
], dtype=np.uint32)


def round_edges():
    """The edge list as float32, every magnitude followed by its negative (34 values)."""
    return f32(np.stack([ROUND_EDGE_BITS, ROUND_EDGE_BITS | np.uint32(0x80000000)], axis=1).ravel())


def cyclic(values, rows, cols, start=0):
    """[rows, cols] filled row-major from `values`, cyclically."""
    values = np.asarray(values)
    return values[(start + np.arange(rows * cols)) % len(values)].reshape(rows, cols)


def round_half_away_exact(v):
    """One finite float, in rational arithmetic: (sign is negative, |result| as an int).  Independent of
    round_half_away: floor(|x| + 1/2) on Fractions has no rounding of its own."""
    q = Fraction(float(v))
    mag = abs(q) + Fraction(1, 2)
    return bool(np.signbit(v)), mag.numerator // mag.denominator


# ------------------------------------------------------------------ bfloat16 wire format

def bf16_rne_bits(u):
    """uint32 float32 patterns -> uint16 bfloat16 patterns, round to nearest even: add 0x7FFF plus the lowest kept bit and
    drop the lower half (a carry out of the mantissa moves the exponent up, FLT_MAX's neighbourhood becomes inf).  A NaN
    stays a NaN of the same sign (the quiet bit is set, so that a payload in the dropped half cannot turn it into inf)."""
    u = np.asarray(u, dtype=np.uint32).astype(np.uint64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, (u >> 16) | 0x0040, r).astype(np.uint16)


def is_nan_bf16(b):
    return (np.asarray(b, dtype=np.uint16) & 0x7FFF) > 0x7F80


def is_nan_f32_bits(u):
    return (np.asarray(u, dtype=np.uint32) & 0x7FFFFFFF) > 0x7F800000


# upper halves of the tie cases: even and odd, at 1.0, at the smallest normal exponent, next to FLT_MAX and mid-range
_TIE_UPPERS = (0x3F80, 0x3F81, 0x0080, 0x0081, 0x4000, 0x4001, 0x7F7E, 0x7F7D)
_QNAN, _SNAN, _SNAN_LOW = 0x7FC00000, 0x7FA00000, 0x7F800001     # the last: a payload in the dropped half only


def bf16_cases():
    """The float32 patterns of the narrowing tests (normal numbers, zeros, inf, NaNs; no subnormals): the special cases with
    both signs first, then 4096 random normal patterns, so that every length from 72 upwards meets every special case."""
    mags = [0x00000000]
    for up in _TIE_UPPERS:
        mags += [(up << 16) | low for low in (0x7FFF, 0x8000, 0x8001)]
    mags += [0x7F7FFFFF,         # FLT_MAX: rounds up to inf
             0x7F7F7FFF,         # the largest pattern that stays finite
             0x7F800000, _QNAN, _SNAN, _SNAN_LOW,
             0x00800000]         # the smallest normal
    mags = np.array(mags, dtype=np.uint32)
    special = np.stack([mags, mags | np.uint32(0x80000000)], axis=1).ravel()
    rs = np.random.RandomState(11)
    exp = rs.randint(1, 255, 4096).astype(np.uint32)              # normal numbers only
    rnd = (rs.randint(0, 2, 4096).astype(np.uint32) << 31) | (exp << 23) | rs.randint(0, 1 << 23, 4096).astype(np.uint32)
    return np.concatenate([special, rnd]).astype(np.uint32)


BF16_LENGTHS = (0, 1, 7, 8, 9, 2047, 2048, 2049, 6149)           # the 8-wide body/tail switch and the 2048-element block
BF16_SUBNORMAL_BITS = np.array([0x00000001, 0x00008000, 0x00018000, 0x007FFFFF], dtype=np.uint32)
BF16_GUARD = 0x7F7F


# ------------------------------------------------------------------ tanh

TANH_MAGNITUDES = (0.0, 1e-30, 2.0 ** -12, 0.5, 1.0, 5.0, 9.01, 20.0, 89.0, 1e30, np.inf)
TANH_SMALL = 2.0 ** -10          # below it the absolute bound says nothing: the relative error is measured instead


def tanh_values(n, seed):
    """n float32 arguments: h = (n - 1) // 2 magnitudes -- the listed ones, 2^-k (1 + U(0, 1)) for k = 11 .. 40 and
    |N(0, 2)| noise --, then their negatives in the same order (so that out[h + i] must be -out[i] bit for bit), then NaN."""
    rs = np.random.RandomState(seed)
    h = (n - 1) // 2
    small = [2.0 ** -k * (1 + rs.uniform()) for k in range(11, 41)]
    pos = np.concatenate([TANH_MAGNITUDES, small, np.abs(rs.normal(0, 2, max(0, h)))])[:h].astype(np.float32)
    return np.concatenate([pos, -pos, np.full(n - 2 * h, np.nan, dtype=np.float32)]).astype(np.float32), h
