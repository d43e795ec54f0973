"""Arithmetic of the variation tool (csrc/moments_u8.hip; variation.py): running moments of uint8 images, the exact numerator
of the per-pixel variance and its heat maps.  Every function has ONE definition for both devices: device tensors run the HIP kernels, CPU tensors
run the same integer arithmetic in numpy int64 -- the results are equal bit for bit, not close.  On the device an unsupported input is an error,
never a quiet fallback.

    accumulate(images, sum, sumsq)     uint8 [G, N, F] (dense in F; the N and G strides are free, so a slice of a larger batch is fine), running
                                       int64 [G, F] sums, updated in place and returned:
                                         sum[g, f] += sum_n images[g, n, f];  sumsq[g, f] += sum_n images[g, n, f]^2.
                                       N = 0 changes nothing.  More than MAX_N rows are fed in several calls.
    numerator(sum, sumsq, n)           int64 [G, C, P], the count n -> int64 [G, P]: sum_c (n sumsq - sum^2), exact, never negative for the moments of
                                       n bytes; num / (C n (n - 1)) is the channel mean of the unbiased variance.  n above numerator_max_n(C) is refused.
    render(num, thresholds, table)     int64 [G, P], 255 ascending int64 thresholds and a uint8 [256, 3] table (both on the host) ->
                                       (heat uint8 [G, 3, P], dominant uint8 [P]): heat[g, :, p] = table[number of thresholds <= num[g, p]];
                                       dominant[p] = the g of the largest num[g, p], ties to the lower g, 255 where every group is 0.
    std_thresholds(max_std, C, n)      host: the 255 thresholds of a scale on which level L begins at a per-pixel std of L max_std / 255.
    pixel_std(num, C, n)               host, float64: sqrt(num / (C n (n - 1))); everything floating happens here, on both devices.

All refusals happen on the host, before any launch, with a message naming shapes, dtypes and devices.
"""
import math

import numpy as np
import torch

from ... import _lib

MAX_N = 32768                   # rows per call: a work-item's uint32 partials cannot overflow while 255^2 N < 2^32 (N <= 66051); a factor of two is left
MAX_F = 1 << 26
MAX_G = 65535
MAX_C = 1024
MAX_RENDER_G = 255
TILE, TARGET_BLOCKS, MIN_ROWS = 4096, 1024, 16


def _describe(**tensors):
    return ', '.join(f'{name} {t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}' for name, t in tensors.items() if t is not None)


def accumulate_splits(g, n, f):
    """the split rule of include/sbg_hip.h: workgroups over N of one accumulate call (the launch record's fourth entry); 0 for N = 0"""
    g, n, f = int(g), int(n), int(f)
    if n == 0:
        return 0
    tiles = -(-f // TILE)
    want = max(1, min(-(-TARGET_BLOCKS // (g * tiles)), -(-n // MIN_ROWS)))
    rows = -(-n // want)
    return -(-n // rows)


def _strides(images):
    """(row_stride, group_stride) in bytes as the library gets them: a single row or group has no stride of its own"""
    g, n, f = images.shape
    row = int(images.stride(1)) if n > 1 else f
    return row, (int(images.stride(0)) if g > 1 else n * row)


def load_width(images):
    """bytes per load of the accumulate kernel for this tensor (the launch record's fifth entry)"""
    row, group = _strides(images)
    strides = row | (group if images.shape[0] > 1 else 0)
    return 16 if strides % 16 == 0 else 4 if strides % 4 == 0 else 1


def numerator_max_n(c):
    """the largest count n with n^2 * 65025 * C < 2^63"""
    c = int(c)
    n = math.isqrt(((1 << 63) - 1) // (65025 * c))
    while n * n * 65025 * c >= 1 << 63:
        n -= 1
    while (n + 1) * (n + 1) * 65025 * c < 1 << 63:
        n += 1
    return n


# ---------------------------------------------------------------------------------------------------------------- accumulate

def accumulate(images, sum, sumsq):
    what = 'moments_u8.accumulate'
    said = _describe(images=images, sum=sum, sumsq=sumsq)
    if images.dtype != torch.uint8 or images.ndim != 3:
        raise RuntimeError(f'{what}: images must be a uint8 [G, N, F] tensor; got {said}')
    g, n, f = images.shape
    if not 1 <= g <= MAX_G or not 1 <= f <= MAX_F:
        raise RuntimeError(f'{what}: [G, N, F] = [{g}, {n}, {f}] is not within 1 <= G <= {MAX_G}, 1 <= F <= 2^26; got {said}')
    for name, t in (('sum', sum), ('sumsq', sumsq)):
        if t.dtype != torch.int64 or tuple(t.shape) != (g, f) or not t.is_contiguous() or t.device != images.device:
            raise RuntimeError(f'{what}: {name} must be a dense int64 [G, F] = [{g}, {f}] tensor on the device of images; got {said}')
    if sum.data_ptr() == sumsq.data_ptr():
        raise RuntimeError(f'{what}: sum and sumsq must be two tensors; got {said}')
    if n == 0:
        return sum, sumsq
    dense_rows = images.stride(2) == 1 or f == 1
    if not dense_rows or (n > 1 and images.stride(1) < f) or (g > 1 and images.stride(0) < (n - 1) * images.stride(1) + f):
        raise RuntimeError(f'{what}: images must be dense along F with rows and groups that do not overlap; got {said}')
    if images.device.type != 'cuda':
        x = images.numpy().astype(np.int64)
        sum.numpy()[...] += x.sum(axis=1)
        sumsq.numpy()[...] += (x * x).sum(axis=1)
        return sum, sumsq
    lib = _lib.load()
    row_stride, group_stride = _strides(images)
    for lo in range(0, n, MAX_N):
        rows = min(MAX_N, n - lo)
        part = images[:, lo:lo + rows]
        ws = _lib.workspace(lib.sbg_moments_accumulate_workspace(g, rows, f), images.device, 'sbg_moments_accumulate_workspace')
        _lib.check(lib.sbg_moments_accumulate(part.data_ptr(), row_stride, group_stride, sum.data_ptr(), sumsq.data_ptr(), ws.data_ptr(), g, rows, f,
                                              _lib.stream_ptr(images.device)), 'sbg_moments_accumulate')
    return sum, sumsq


# ---------------------------------------------------------------------------------------------------------------- numerator

def numerator(sum, sumsq, n):
    what = 'moments_u8.numerator'
    said = _describe(sum=sum, sumsq=sumsq)
    n = int(n)
    for t in (sum, sumsq):
        if t.dtype != torch.int64 or t.ndim != 3 or not t.is_contiguous():
            raise RuntimeError(f'{what}: expects two dense int64 [G, C, P] tensors; got {said}')
    if sum.shape != sumsq.shape or sum.device != sumsq.device:
        raise RuntimeError(f'{what}: sum and sumsq must have one shape and one device; got {said}')
    g, c, p = sum.shape
    if not 1 <= g <= MAX_G or not 1 <= c <= MAX_C or not 1 <= p <= MAX_F or g * c * p > 1 << 40:
        raise RuntimeError(f'{what}: [G, C, P] = [{g}, {c}, {p}] is not within 1 <= G <= {MAX_G}, 1 <= C <= {MAX_C}, 1 <= P <= 2^26, G C P <= 2^40; got {said}')
    if not 0 <= n <= numerator_max_n(c):
        raise RuntimeError(f'{what}: n = {n} is not within [0, {numerator_max_n(c)}], the counts with n^2 * 65025 * C < 2^63 at C = {c}; got {said}')
    if sum.device.type != 'cuda':
        s, q = sum.numpy(), sumsq.numpy()
        return torch.from_numpy((np.int64(n) * q - s * s).sum(axis=1))
    num = torch.empty([g, p], dtype=torch.int64, device=sum.device)
    _lib.check(_lib.load().sbg_moments_numerator(sum.data_ptr(), sumsq.data_ptr(), num.data_ptr(), g, c, p, n, _lib.stream_ptr(sum.device)),
               'sbg_moments_numerator')
    return num


# ---------------------------------------------------------------------------------------------------------------- render

def render(num, thresholds, table):
    what = 'moments_u8.render'
    said = _describe(num=num)
    if num.dtype != torch.int64 or num.ndim != 2 or not num.is_contiguous():
        raise RuntimeError(f'{what}: num must be a dense int64 [G, P] tensor; got {said}')
    g, p = num.shape
    if not 1 <= g <= MAX_RENDER_G or not 1 <= p <= MAX_F:
        raise RuntimeError(f'{what}: [G, P] = [{g}, {p}] is not within 1 <= G <= {MAX_RENDER_G}, 1 <= P <= 2^26; got {said}')
    thresholds = np.ascontiguousarray(thresholds)
    table = np.ascontiguousarray(table)
    if thresholds.dtype != np.int64 or thresholds.shape != (255,) or bool((np.diff(thresholds) < 0).any()):
        raise RuntimeError(f'{what}: thresholds must be 255 ascending int64 values on the host; got {thresholds.dtype} {thresholds.shape}')
    if table.dtype != np.uint8 or table.shape != (256, 3):
        raise RuntimeError(f'{what}: table must be a uint8 [256, 3] array on the host; got {table.dtype} {table.shape}')
    if num.device.type != 'cuda':
        v = num.numpy()
        level = np.searchsorted(thresholds, v, side='right')                # the number of thresholds <= v
        heat = np.ascontiguousarray(table[level].transpose(0, 2, 1))
        dominant = np.where(v.max(axis=0) > 0, np.argmax(v, axis=0), 255).astype(np.uint8)      # argmax: the first of equal values
        return torch.from_numpy(heat), torch.from_numpy(dominant)
    heat = torch.empty([g, 3, p], dtype=torch.uint8, device=num.device)
    dominant = torch.empty([p], dtype=torch.uint8, device=num.device)
    thr = torch.from_numpy(thresholds).to(num.device)
    tab = torch.from_numpy(table).to(num.device)
    _lib.check(_lib.load().sbg_moments_render(num.data_ptr(), thr.data_ptr(), tab.data_ptr(), heat.data_ptr(), dominant.data_ptr(), g, p,
                                              _lib.stream_ptr(num.device)), 'sbg_moments_render')
    return heat, dominant


# ---------------------------------------------------------------------------------------------------------------- host

def pixel_std(num, c, n):
    """int64 numerators (any shape, numpy) -> float64 per-pixel std in byte units: sqrt(num / (C n (n - 1))), the channel mean of the unbiased
    variance; zeros for n < 2"""
    num = np.asarray(num)
    if int(n) < 2:
        return np.zeros(num.shape, dtype=np.float64)
    return np.sqrt(np.maximum(num, 0).astype(np.float64) / np.float64(int(c) * int(n) * (int(n) - 1)))


def std_thresholds(max_std, c, n):
    """-> int64 [255] ascending: threshold L - 1 is the smallest numerator, at least 1, whose `pixel_std` reaches L max_std / 255 (L = 1 .. 255),
    judged by `pixel_std` itself, so a pixel whose std is max_std is on the top level; a numerator of 0 is level 0 on every scale"""
    c, n = int(c), max(int(n), 2)
    target = np.arange(1, 256, dtype=np.float64) * np.float64(max_std) / 255.0
    v = np.ceil(np.minimum(target * target * np.float64(c * n * (n - 1)), 2.0 ** 62)).astype(np.int64)
    for _ in range(4):                                                          # the float64 square is off by a few ulps at most
        v = np.where((v > 0) & (pixel_std(v - 1, c, n) >= target), v - 1, v)
    for _ in range(4):
        v = np.where(pixel_std(v, c, n) < target, v + 1, v)
    return np.maximum(v, 1)
