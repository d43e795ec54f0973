"""torch_utils/ops/_exact_common.py, the numpy statement of the fixed-order sums and of fmaf that every bit-for-bit test of the SWD, MS-SSIM
and spectrum tools rests on: the sums against a scalar emulation of csrc/reduce.h and csrc/merge.h (one Python addition per device
addition), fma32 against exact rational arithmetic rounded once.  No library is loaded."""
import math
from fractions import Fraction

import numpy as np
import pytest

from style_big_gan_amd.torch_utils.ops._exact_common import NT, block_sum_np, chunked_sum_np, fma32, strided_sum_np

SIZES = [1, 255, 256, 257, 513, 1000]
ROWS = 8


def _bits(v):
    v = np.ascontiguousarray(v)
    return v.view({4: np.int32, 8: np.int64}[v.dtype.itemsize])


def _spread(rng, shape, dtype):
    """magnitudes over 1e-6 .. 1e6: almost every addition rounds, and differently in another order"""
    return (rng.randn(*shape) * 10.0 ** rng.uniform(-6, 6, shape)).astype(dtype)


def _block_sum_scalar(lanes):
    """reduce.h block_sum<256>, one value at a time: the xor butterfly with offsets 32 .. 1 in each wave of 64 (every lane adds its
    partner's value of the step before), then the four waves' values left to right"""
    assert len(lanes) == NT
    waves = []
    for w in range(NT // 64):
        v = list(lanes[64 * w:64 * w + 64])
        for off in (32, 16, 8, 4, 2, 1):
            v = [v[i] + v[i ^ off] for i in range(64)]
        waves.append(v[0])
    s = waves[0]
    for w in waves[1:]:
        s = s + w
    return s


def _strided_sum_scalar(v):
    """merge.h: lane t adds the elements t, t + 256, ... in ascending order from 0, then block_sum"""
    lanes = [v.dtype.type(0)] * NT
    for i, x in enumerate(v):
        lanes[i % NT] = lanes[i % NT] + x
    return _block_sum_scalar(lanes)


def _left_to_right(v):
    s = v.dtype.type(0)
    for x in v:
        s = s + x
    return s


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_block_sum_is_the_butterfly_then_the_waves_in_order(dtype):
    lanes = _spread(np.random.RandomState(0), (ROWS, NT), dtype)
    got = block_sum_np(lanes)
    want = np.array([_block_sum_scalar(list(row)) for row in lanes])
    assert got.dtype == dtype and want.dtype == dtype and got.shape == (ROWS,)
    assert np.array_equal(_bits(got), _bits(want))
    other = np.array([_left_to_right(row) for row in lanes])
    assert (_bits(other) != _bits(got)).any()            # the inputs tell the butterfly from a plain loop


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_strided_sum_is_lane_strided_then_block_sum(dtype):
    rng = np.random.RandomState(0)
    told_apart = 0
    for n in SIZES:
        v = _spread(rng, (ROWS, n), dtype)
        got = strided_sum_np(v)
        want = np.array([_strided_sum_scalar(row) for row in v])
        assert got.dtype == dtype and want.dtype == dtype and got.shape == (ROWS,), n
        assert np.array_equal(_bits(got), _bits(want)), n
        assert np.array_equal(_bits(strided_sum_np(v.reshape(2, ROWS // 2, n))), _bits(got).reshape(2, ROWS // 2)), n      # leading axes are batch
        other = np.array([_left_to_right(row) for row in v])
        told_apart += int((_bits(other) != _bits(got)).sum())
    assert told_apart > 0                                   # a left-to-right sum gives other bits: the inputs can tell orders apart


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_chunked_sum_is_the_strided_sum_of_strided_chunk_sums(dtype):
    """a ragged last chunk and more than 256 chunks (a lane of the second stage adds two chunk sums)"""
    v = _spread(np.random.RandomState(1), (2, 257 * 48 + 5), dtype)
    got = chunked_sum_np(v, 48)
    assert got.dtype == dtype and got.shape == (2,)
    for q in range(2):
        chunk_sums = np.array([_strided_sum_scalar(v[q, i:i + 48]) for i in range(0, v.shape[1], 48)])
        assert len(chunk_sums) == 258
        assert _bits(got[q:q + 1])[0] == _bits(np.array([_strided_sum_scalar(chunk_sums)]))[0]


def _round_to_f32(x):
    """a rational number -> the nearest float32, ties to even (one rounding); no overflow in these tests"""
    if x == 0:
        return np.float32(0.0)
    sign, x = (-1.0 if x < 0 else 1.0), abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    e = max(e, -126)                                        # below 2^-126 the spacing stays 2^-149
    q = x / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    rest = q - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(sign * math.ldexp(float(n), e - 23))


def test_fma32_rounds_the_exact_value_once():
    rng = np.random.RandomState(0)
    a, b = _spread(rng, (2000,), np.float32) * 1e-3, _spread(rng, (2000,), np.float32) * 1e-3
    c = (-(a.astype(np.float64) * b.astype(np.float64))).astype(np.float32)                # c close to -a b: the sum cancels
    for _ in range(2):
        c = np.where(rng.randint(0, 2, c.shape) == 1, np.nextafter(c, np.float32(np.inf)), c)
    got = fma32(a, b, c)
    assert got.dtype == np.float32
    want = np.array([_round_to_f32(Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))) for x, y, z in zip(a, b, c)])
    assert np.array_equal(_bits(got), _bits(want))
    assert (got != 0).sum() > 1900                          # the cancellation leaves a rounding error to round, not zeros
    unfused = a * b + c
    assert (_bits(unfused) != _bits(got)).any()             # a rounded product is another function


def test_fma32_does_not_round_twice():
    """a = b = 1 + 2^-12, c = 2^-80: a b + c = 1 + 2^-11 + 2^-24 + 2^-80 lies just above the middle of two floats and rounds up; rounded to
    float64 first it is the middle itself and goes to the even neighbour"""
    a = np.array([1 + 2.0 ** -12], dtype=np.float32)
    c = np.array([2.0 ** -80], dtype=np.float32)
    assert float(fma32(a, a, c)[0]) == 1 + 2.0 ** -11 + 2.0 ** -23
    assert _round_to_f32(Fraction(float(a[0])) ** 2 + Fraction(float(c[0]))) == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)
    naive = (a.astype(np.float64) * a.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    assert float(naive[0]) == 1 + 2.0 ** -11
