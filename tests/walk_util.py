"""Shared pieces of the latent-walk tests: an independent fmaf (exact rational arithmetic, rounded once to fp32, signed zeros by the IEEE rule),
the scalar restatement of `blend_table` built on it, the key tables and tap tables of the test shapes, the CPU results computed once per
session, and a reader of the animations the tool writes (frames expanded by their duration, a still image to the frames expected)."""
import functools
import math
from fractions import Fraction

import numpy as np
import PIL.Image
import torch

from directions_util import ExactGenerator, same_bits  # noqa: F401  (re-exported to the tests)
from style_big_gan_amd.torch_utils.ops import walk as ops

# (K, L, D, T, loop): the shapes of the issue; SHAPES[:3] run on the CPU against the restatement, all of them on the device against the CPU path
SHAPES = [(2, 1, 1, 3, False), (3, 6, 24, 7, False), (5, 14, 40, 33, True), (3, 18, 512, 130, False), (4, 1, 512, 64, False), (2, 3, 1024, 5, False)]


def _round_to_f32(x, negative_zero):
    """an exact rational -> the nearest float32, ties to even, subnormals included; an exact zero takes the sign given"""
    if x == 0:
        return np.float32(-0.0 if negative_zero else 0.0)
    sign, x = (-1.0, -x) if x < 0 else (1.0, x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if Fraction(2) ** e > x:
        e -= 1
    assert Fraction(2) ** e <= x < Fraction(2) ** (e + 1)
    e = max(e, -126)
    q = x / Fraction(2) ** (e - 23)
    n = q.numerator // q.denominator
    rest = q - n
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and n % 2 == 1):
        n += 1
    return np.float32(sign * math.ldexp(float(n), e - 23))


def fmaf(a, b, c):
    """float32 a b + c with one rounding.  An exact zero result is -0.0 only when the product and c are both negative zeros (or the product
    is a negative zero and so is c); a cancellation gives +0.0 (round to nearest)."""
    a, b, c = float(a), float(b), float(c)
    product_negative = math.copysign(1.0, a) * math.copysign(1.0, b) < 0
    both_zero = (a == 0 or b == 0) and c == 0
    return _round_to_f32(Fraction(a) * Fraction(b) + Fraction(c), both_zero and product_negative and math.copysign(1.0, c) < 0)


def restate_blend(keys, index, weight, layers=None, hold=None):
    """every element on its own: one rounded product, then three fmaf in tap order; a layer left out copies keys[hold[t]]"""
    k, l, d = keys.shape
    t = index.shape[0]
    out = np.empty([t, l, d], dtype=np.float32)
    for ti in range(t):
        for li in range(l):
            for di in range(d):
                if layers is not None and li not in layers:
                    out[ti, li, di] = keys[hold[ti], li, di]
                    continue
                acc = np.float32(weight[ti, 0]) * np.float32(keys[index[ti, 0], li, di])
                for j in (1, 2, 3):
                    acc = fmaf(weight[ti, j], keys[index[ti, j], li, di], acc)
                out[ti, li, di] = acc
    return out


@functools.lru_cache(maxsize=None)
def key_table(k, l, d):
    """fp32 [K, L, D]: normal values; every 7th element a subnormal, every 11th -0.0, every 13th +0.0"""
    rng = np.random.RandomState(100 * k + 10 * l + d)
    keys = rng.randn(k, l, d).astype(np.float32)
    flat = keys.reshape(-1)
    flat[::7] = (rng.randint(-(1 << 22), 1 << 22, [len(flat[::7])]).astype(np.float64) * 2.0 ** -149).astype(np.float32)
    flat[::11] = np.float32(-0.0)
    flat[::13] = np.float32(0.0)
    keys.setflags(write=False)
    return keys


@functools.lru_cache(maxsize=None)
def taps(k, t, loop, method="cubic"):
    """(index int32 [T, 4], weight fp32 [T, 4], hold int32 [T]) of a walk through K keys: the LAST T frames of the shortest walk with at least T
    (the last segment's fold, or the wrap of a loop, is always among them; with T frames exactly, the first segment's too)"""
    n = 1
    while (k * n if loop else (k - 1) * n + 1) < t:
        n += 1
    omega = np.random.RandomState(k + t).rand(k if loop else k - 1) * 2 + 0.5 if method == "slerp" else None
    index, weight, _, _ = ops.walk_weights(method, k, n, loop, omega)
    index, weight = np.ascontiguousarray(index[-t:]), np.ascontiguousarray(weight[-t:])
    hold = (np.arange(t, dtype=np.int32) * 3) % np.int32(k)
    for v in (index, weight, hold):
        v.setflags(write=False)
    return index, weight, hold


def odd_layers(l):
    return list(range(1, l, 2))


def case_method(k, l, d):
    return "slerp" if (l, d) == (1, 512) else "cubic"              # the Z table


@functools.lru_cache(maxsize=None)
def cpu_table(k, l, d, t, loop, masked):
    """the op's CPU path on a test shape, computed once per session and read-only"""
    index, weight, hold = taps(k, t, loop, case_method(k, l, d))
    h = lambda v: torch.from_numpy(v.copy())
    out = ops.blend_table(h(key_table(k, l, d)), h(index), h(weight), odd_layers(l) if masked else None, h(hold) if masked else None).numpy()
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def byte_rows(n, f, seed=0):
    rng = np.random.RandomState(1000 * n + f % 1000 + seed)
    rows = rng.randint(0, 256, [n, f], dtype=np.uint8)
    rows.setflags(write=False)
    return rows


def sqdiff_np(a, b):
    diff = a.astype(np.int64) - b.astype(np.int64)
    return (diff * diff).sum(axis=1)


def read_animation(path, fps, frames, mode="RGB"):
    """-> uint8 [T, H, W(, 3)]: every stored frame repeated round(duration / (1000 / fps)) times (the writers merge identical consecutive frames);
    a file of one still image (all frames identical: the duration is lost) is expanded to `frames`"""
    im = PIL.Image.open(path)
    count = getattr(im, "n_frames", 1)
    out = []
    for i in range(count):
        im.seek(i)
        pixels = np.array(im.convert(mode))             # decoding sets the frame's duration
        repeat = frames if count == 1 else int(round(im.info["duration"] / (1000 / fps)))
        out += [pixels] * repeat
    return np.stack(out)
