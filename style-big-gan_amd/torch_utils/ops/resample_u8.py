"""Exact uint8 image resizing as HIP kernels (csrc/resample_u8.hip): PIL's ``Image.resize`` with ``LANCZOS`` or ``BOX`` on 8-bit images,
which is the arithmetic of the reference's data set tool (stylegan2ada/dataset_tool.py:199-248).

PIL's routine is integer arithmetic: per output index a window ``(first, count)`` and coefficients rounded to 22 fractional bits, int32
accumulators, a horizontal pass whose result is rounded to uint8 before the vertical pass, and no pass at all along an axis whose extent
does not change.  ``coefficients`` restates the table on the host, ``resize_reference`` the two passes on CPU tensors, and ``resize``
runs the passes as kernels for a device tensor; all three give PIL's bytes.  CPU tensors take ``resize_reference`` so that the tool works
without a GPU; on the device an unsupported input is an error, never a quiet torch fallback.

``box = (left, upper, right, lower)`` is a crop in whole pixels, with the meaning of ``img[upper:lower, left:right]`` followed by the
resize (the pixels outside the box are not seen by the filter; this is what the tool's centre crops do).  On the device it is a pointer
offset and an extent, not a copy.
"""
import functools
import math

import numpy as np
import torch

from ... import _lib

FILTERS = ("box", "lanczos")
PRECISION_BITS = 22                     # 32 - 8 - 2
LDS_BUDGET = 60 * 1024                  # kLdsBudget of csrc/resample_u8.hip


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


_SUPPORT = {"lanczos": (_lanczos, 3.0), "box": (_box, 0.5)}


@functools.lru_cache(maxsize=256)
def _coefficients(in_size, out_size, filter, lo, hi):
    f, support = _SUPPORT[filter]
    n = hi - lo
    scale = filterscale = n / out_size
    if filterscale < 1.0:
        filterscale = 1.0
    support = support * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    bounds = np.zeros([out_size, 2], dtype=np.int32)
    coeffs = np.zeros([out_size, ksize], dtype=np.int32)
    for i in range(out_size):
        center = (i + 0.5) * scale
        first = max(int(center - support + 0.5), 0)
        count = min(int(center + support + 0.5), n) - first
        w = [f((x + first - center + 0.5) * ss) for x in range(count)]
        ww = 0.0
        for v in w:
            ww += v
        for x, v in enumerate(w):
            if ww != 0.0:
                v = v / ww
            coeffs[i, x] = int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS))
        bounds[i] = (first + lo, count)
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


def coefficients(in_size, out_size, filter, box=None):
    """-> (bounds int32 [out_size, 2] = (first, count) per output index, coeffs int32 [out_size, ksize], zero behind `count`): PIL's
    `precompute_coeffs` and `normalize_coeffs_8bpc` in double precision, with libm's sin as in PIL's C code.  `box = (lo, hi)` resamples
    the slice [lo, hi) of the axis: the windows are those of an axis of hi - lo samples, `first` counts from the uncropped origin.
    The arrays are shared and read-only."""
    if filter not in FILTERS:
        raise RuntimeError(f"resample_u8: unknown filter {filter!r} (one of {FILTERS})")
    in_size, out_size = int(in_size), int(out_size)
    lo, hi = (0, in_size) if box is None else (int(box[0]), int(box[1]))
    if in_size < 1 or out_size < 1 or not 0 <= lo < hi <= in_size:
        raise RuntimeError(f"resample_u8: cannot resample [{lo}, {hi}) of {in_size} samples to {out_size}")
    return _coefficients(in_size, out_size, filter, lo, hi)


# ---------------------------------------------------------------------------------------------------------------- checks shared by both paths

def _as_batch(img, what):
    """-> ([N, H, W, C] view, function restoring the caller's rank)"""
    if not isinstance(img, torch.Tensor):
        raise RuntimeError(f"{what}: expects a torch tensor, got {type(img).__name__}")
    if img.dtype != torch.uint8:
        raise RuntimeError(f"{what}: expects uint8 images, got {img.dtype}")
    if img.ndim == 2:
        x, back = img[None, :, :, None], lambda o: o[0, :, :, 0]
    elif img.ndim == 3:
        x, back = img[None], lambda o: o[0]
    elif img.ndim == 4:
        x, back = img, lambda o: o
    else:
        raise RuntimeError(f"{what}: expects [H, W], [H, W, C] or [N, H, W, C], got {list(img.shape)}")
    if x.shape[3] not in (1, 3) or x.numel() == 0:
        raise RuntimeError(f"{what}: expects non-empty images with C = 1 or 3 interleaved channels, got {list(img.shape)}")
    return x, back


def _check_target(x, width, height, filter, box, what):
    if filter not in FILTERS:
        raise RuntimeError(f"{what}: unknown filter {filter!r} (one of {FILTERS})")
    width, height = int(width), int(height)
    if width < 1 or height < 1:
        raise RuntimeError(f"{what}: the target size must be positive, got {width} x {height}")
    H, W = x.shape[1], x.shape[2]
    left, upper, right, lower = (0, 0, W, H) if box is None else [int(v) for v in box]
    if not (0 <= left < right <= W and 0 <= upper < lower <= H):
        raise RuntimeError(f"{what}: box {(left, upper, right, lower)} does not lie inside a {W} x {H} image")
    return width, height, (left, upper, right, lower)


# ---------------------------------------------------------------------------------------------------------------- the integer restatement (CPU)

def _pass_reference(a, bounds, coeffs, axis):
    """one pass over `axis` (1 rows / 2 columns) of uint8 [N, H, W, C]; int32 wraps like the C accumulators"""
    ksize = coeffs.shape[1]
    first = bounds[:, 0].astype(np.int64)
    shape = list(a.shape)
    shape[axis] = bounds.shape[0]
    bshape = [1, 1, 1, 1]
    bshape[axis] = -1
    out = np.empty(shape, dtype=np.uint8)
    for n in range(a.shape[0]):
        acc = np.full(shape[1:], 1 << (PRECISION_BITS - 1), dtype=np.int32)
        for k in range(ksize):
            ck = coeffs[:, k]
            if not ck.any():
                continue
            idx = np.minimum(first + k, a.shape[axis] - 1)          # behind `count` the coefficient is zero
            acc += np.take(a[n], idx, axis=axis - 1).astype(np.int32) * ck.reshape(bshape[1:])
        out[n] = np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)
    return out


def resize_reference(img, width, height, filter, box=None):
    """`PIL.Image.fromarray(img).resize((width, height), filter)` of CPU uint8 images [H, W], [H, W, C] or [N, H, W, C] (C = 1 or 3), by
    the integer algorithm; `box` crops first.  Returns a new tensor of the same rank."""
    what = "resample_u8 resize_reference"
    x, back = _as_batch(img, what)
    if x.device.type != "cpu":
        raise RuntimeError(f"{what}: expects CPU tensors, got {x.device}")
    width, height, (left, upper, right, lower) = _check_target(x, width, height, filter, box, what)
    a = x.numpy()[:, upper:lower, left:right]
    if right - left != width:
        a = _pass_reference(a, *coefficients(right - left, width, filter), axis=2)
    if lower - upper != height:
        a = _pass_reference(a, *coefficients(lower - upper, height, filter), axis=1)
    if (right - left, lower - upper) == (width, height):   # no pass ran: PIL returns a copy
        a = np.array(a, order="C")
    return back(torch.from_numpy(a))


# ---------------------------------------------------------------------------------------------------------------- the kernels

def _pitch4(row_bytes):
    return (row_bytes + 3) // 4 * 4


def strip_and_span(bounds, C):
    """-> (strip, span) for sbg_u8_resample_h: the largest power-of-two strip of output pixels in [16, 256] (no longer than needed)
    whose input span, `span` pixels of C bytes, fits the kernel's LDS; None when even 16 output pixels do not fit"""
    out = bounds.shape[0]
    first, last = bounds[:, 0].astype(np.int64), bounds[:, 0].astype(np.int64) + bounds[:, 1]
    strip = 16
    while strip < 256 and strip < out:
        strip *= 2
    while True:
        starts = np.arange(0, out, strip)
        ends = np.minimum(starts + strip, out) - 1
        span = int(max(1, (np.maximum.accumulate(last)[ends] - first[starts]).max()))
        if (span * C + 6) // 4 * 4 <= LDS_BUDGET:
            return strip, span
        if strip == 16:
            return None
        strip //= 2


_tables = {}


def _device_tables(in_size, out_size, filter, lo, hi, device, tap_major):
    key = (in_size, out_size, filter, lo, hi, str(device), tap_major)
    t = _tables.get(key)
    if t is None:
        bounds, coeffs = coefficients(in_size, out_size, filter, (lo, hi))
        bounds = bounds.copy()
        bounds[:, 0] -= lo                  # the kernels count from the pointer they are given, which is the box's origin
        c = np.ascontiguousarray(coeffs.T) if tap_major else coeffs
        table = torch.from_numpy(np.concatenate([bounds.reshape(-1), c.reshape(-1)])).to(device)
        if len(_tables) >= 64:
            _tables.clear()
        t = _tables[key] = (table, bounds, coeffs.shape[1])
    return t


def resize(img, width, height, filter, box=None):
    """`PIL.Image.fromarray(img).resize((width, height), filter)`, bit for bit, of uint8 images [H, W], [H, W, C] or [N, H, W, C] with
    C = 1 or 3 interleaved channels; `filter` is 'lanczos' or 'box'; `box = (left, upper, right, lower)` crops first.  A device tensor
    runs the kernels (horizontal pass, uint8 intermediate, vertical pass; a pass that keeps its extent is skipped) and may be any view
    whose pixels are dense: channels adjacent, pixels of a row adjacent, any row pitch and image stride.  A CPU tensor takes
    `resize_reference`.  Returns a new dense tensor of the same rank on the same device."""
    what = "resample_u8 resize"
    x, back = _as_batch(img, what)
    if x.device.type != "cuda":
        return resize_reference(img, width, height, filter, box)
    width, height, (left, upper, right, lower) = _check_target(x, width, height, filter, box, what)
    x = x.detach()
    N, H, W, C = x.shape
    sn, sh, sw, sc = x.stride()
    if (C > 1 and sc != 1) or (W > 1 and sw != C) or (H > 1 and sh < W * C) or (N > 1 and sn < 0):
        raise RuntimeError(f"{what}: the device path needs interleaved channels and dense rows (strides [n, h, w, c] = [any, >= W * C, C, 1]), "
                           f"got shape {list(x.shape)} with strides {list(x.stride())}; call .contiguous() first")
    sh = max(sh, W * C) if H > 1 else W * C
    bw, bh = right - left, lower - upper
    if bw == width and bh == height:
        return back(x[:, upper:lower, left:right].clone(memory_format=torch.contiguous_format))
    lib, dev, stream = _lib.load(), x.device, _lib.stream_ptr(x.device)
    src, src_n, src_pitch = x.data_ptr() + upper * sh + left * C, sn, sh
    rows = bh
    out = None
    if bw != width:
        table, bounds, ksize = _device_tables(bw, width, filter, 0, bw, dev, True)
        ss = strip_and_span(bounds, C)
        if ss is None:
            raise RuntimeError(f"{what}: {bw} -> {width} pixels needs more than {LDS_BUDGET} bytes of LDS for 16 output pixels; not supported on the device")
        if bh != height:
            pitch = _pitch4(width * C)
            out = torch.empty([N, rows, pitch], dtype=torch.uint8, device=dev)
        else:
            pitch = width * C
            out = torch.empty([N, rows, width, C], dtype=torch.uint8, device=dev)
        p = table.data_ptr()
        _lib.check(lib.sbg_u8_resample_h(src, src_n, src_pitch, out.data_ptr(), rows * pitch, pitch, N, rows, bw, width, C, p, p + 8 * width, ksize,
                                         ss[0], ss[1], stream), "sbg_u8_resample_h")
        if bh == height:
            return back(out)
        src, src_n, src_pitch = out.data_ptr(), rows * pitch, pitch
    row_bytes = width * C
    pitch = _pitch4(row_bytes)
    table, _, ksize = _device_tables(bh, height, filter, 0, bh, dev, False)
    dst = torch.empty([N, height, pitch], dtype=torch.uint8, device=dev)
    p = table.data_ptr()
    _lib.check(lib.sbg_u8_resample_v(src, src_n, src_pitch, dst.data_ptr(), height * pitch, pitch, N, row_bytes, bh, height, p, p + 8 * height, ksize,
                                     stream), "sbg_u8_resample_v")
    del out                                 # the intermediate stays allocated until here: both launches are on the current stream
    if pitch != row_bytes:
        dst = dst[:, :, :row_bytes].contiguous()
    return back(dst.reshape(N, height, width, C))
