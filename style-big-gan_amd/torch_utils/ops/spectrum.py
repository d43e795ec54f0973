"""Arithmetic of the average 2-D power spectrum of an image set (csrc/spectrum.hip; avg_spectra.py of Karras et al., "Alias-Free Generative
Adversarial Networks", NeurIPS 2021).  Every function takes its tables explicitly and has ONE definition for both devices: device tensors
run the HIP kernels, CPU tensors run the same value graph with numpy (meant for small sets) -- the results are equal bit for bit, not close
(DESIGN.md section 22 states every rounding and the order of the sums).

    tables(R, S, beta=8.0)                     window fp32 [R], twiddle fp32 [S/2, 2], built in float64 on the host
    normalisation(total, total_sq, count)      exact integer sums of the byte values -> (mean, std) as float64
    scale_shift(mean, std)                     (s, t) = (float32(1 / std), float32(-mean / std)):  v = fmaf(x, s, t)
    transform(images, s, t, window, twiddle)   CPU tensors: complex64 [B, C, S/2 + 1, S], the transform that accumulate squares and adds
    accumulate(acc, images, s, t, window, twiddle)     acc float64 [S/2 + 1, S] += the power of every image-channel, in order, in place
    full_spectrum(acc, count)                  float64 ndarray [S, S] = P[ky, kx], not shifted
    radial_profile(full), slices(full), compare(real_full, gen_full)       host arithmetic in float64
"""
import math

import numpy as np
import torch

from ... import _lib
from ._exact_common import fma32

PADS = (1, 2, 4)
MIN_SIDE, MAX_SIDE = 16, 1024
MAX_PIECE = 1 << 20         # image-channels per launch pair, whatever the workspace would hold
DB_FLOOR = 1e-30


def check_sizes(R, S, what="spectrum"):
    """R a power of two in [16, 1024], S = P R with P in (1, 2, 4) -> P"""
    R, S = int(R), int(S)
    if R < MIN_SIDE or R > MAX_SIDE or R & (R - 1):
        raise ValueError(f"{what}: the image side R={R} must be a power of two in [{MIN_SIDE}, {MAX_SIDE}]")
    if S % R or S // R not in PADS:
        raise ValueError(f"{what}: the spectrum side S={S} must be P * R with the padding factor P in {PADS}, R={R}")
    return S // R


def tables(R, S, beta=8.0):
    """-> (window fp32 [R], twiddle fp32 [S/2, 2]) on the host: the Kaiser window divided by the root of the sum of its squares, and
    (cos, -sin)(2 pi k / S); both evaluated in float64 and cast"""
    check_sizes(R, S, "spectrum.tables")
    w = np.kaiser(R, float(beta))
    w = w / np.sqrt(np.sum(w * w))
    k = np.arange(S // 2, dtype=np.float64)
    tw = np.stack([np.cos(2 * np.pi * k / S), -np.sin(2 * np.pi * k / S)], axis=1)
    return torch.from_numpy(w.astype(np.float32)), torch.from_numpy(tw.astype(np.float32))


def normalisation(total, total_sq, count):
    """the mean and the population std of `count` byte values from their exact integer sum and sum of squares (Python integers: no
    summation order enters) -> (mean, std) as floats"""
    total, total_sq, count = int(total), int(total_sq), int(count)
    if count < 1:
        raise ValueError(f"spectrum.normalisation: count={count} values")
    if count * 255 * 255 >= 1 << 63:
        raise OverflowError(f"spectrum.normalisation: the sum of squares of count={count} byte values does not fit the int64 range it is gathered in")
    var_num = count * total_sq - total * total          # count^2 * variance, exact
    if var_num <= 0:
        raise ValueError("spectrum.normalisation: the std of the real set is 0 (every byte has one value); the spectrum is not defined")
    return total / count, math.sqrt(var_num) / count


def scale_shift(mean, std):
    """-> (s, t) as Python floats holding float32 values"""
    if not std > 0:
        raise ValueError(f"spectrum.scale_shift: std={std} must be positive")
    return float(np.float32(1.0 / std)), float(np.float32(-mean / std))


_rev_cache, _stage_cache = {}, {}


def _bitrev(n):
    """int64 ndarray [n]: the bit reversal of 0 .. n - 1 over log2 n bits"""
    if n not in _rev_cache:
        bits = n.bit_length() - 1
        i = np.arange(n, dtype=np.int64)
        r = np.zeros(n, dtype=np.int64)
        for b in range(bits):
            r |= ((i >> b) & 1) << (bits - 1 - b)
        _rev_cache[n] = r
    return _rev_cache[n]


def _stage_index(S, device):
    """int64 [S - 1] on `device`: entry h - 1 + j = j S / (2 h), the twiddle of butterfly j of the stage of half-span h"""
    key = (S, str(device))
    if key not in _stage_cache:
        idx, h = [], 1
        while h < S:
            idx.append(np.arange(h, dtype=np.int64) * (S // (2 * h)))
            h *= 2
        _stage_cache[key] = torch.from_numpy(np.concatenate(idx)).to(device)
    return _stage_cache[key]


def _stages_np(re, im, stages, S, h0):
    """the butterflies of half-span h0, 2 h0, .., S/2 over the last axis (length S) of two fp32 arrays; `stages` fp32 [S - 1, 2]"""
    lead = re.shape[:-1]
    h = h0
    while h < S:
        shape = lead + (S // (2 * h), 2, h)
        re, im = re.reshape(shape), im.reshape(shape)
        ar, br, ai, bi = re[..., 0, :], re[..., 1, :], im[..., 0, :], im[..., 1, :]
        wr = np.broadcast_to(stages[h - 1:2 * h - 1, 0], br.shape)
        wi = np.broadcast_to(stages[h - 1:2 * h - 1, 1], br.shape)
        tr = fma32(br, wr, -(bi * wi))                 # the inner products are fp32 products: rounded before the fmaf
        ti = fma32(br, wi, bi * wr)
        re = np.stack([ar + tr, ar - tr], axis=-2).reshape(lead + (S,))
        im = np.stack([ai + ti, ai - ti], axis=-2).reshape(lead + (S,))
        h *= 2
    return re, im


def _transform_np(x, s, t, window, stages, S):
    """x fp32 ndarray [BC, R, R] -> (re, im) fp32 [BC, S/2 + 1, S]: the windowed transform Y[kx, ky] of every image-channel"""
    R = x.shape[2]
    P, rev = S // R, _bitrev(R)
    v = fma32(x, np.broadcast_to(np.float32(s), x.shape), np.broadcast_to(np.float32(t), x.shape))
    a = v * window[None, None, :]
    # the samples in bit-reversed order, each P times: what the stages h < P make of the zero padding
    re = np.repeat(a[:, :, rev], P, axis=2)
    re, im = _stages_np(re, np.zeros_like(re), stages, S, P)
    re, im = re[:, :, :S // 2 + 1] * window[None, :, None], im[:, :, :S // 2 + 1] * window[None, :, None]
    re = np.repeat(re.transpose(0, 2, 1)[:, :, rev], P, axis=2)            # [BC, kx, ky positions]
    im = np.repeat(im.transpose(0, 2, 1)[:, :, rev], P, axis=2)
    return _stages_np(np.ascontiguousarray(re), np.ascontiguousarray(im), stages, S, P)


def _checked(what, images, window, twiddle):
    """the checks `accumulate` and `transform` share -> (B, C, R, S)"""
    for name, v in (("images", images), ("window", window), ("twiddle", twiddle)):
        if not isinstance(v, torch.Tensor):
            raise RuntimeError(f"{what}: {name} must be a torch tensor, got {type(v).__name__}")
    if images.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"{what}: images must be uint8 or float32, got {images.dtype}")
    if images.ndim != 4 or images.shape[2] != images.shape[3]:
        raise ValueError(f"{what}: images must be square [B, C, R, R], got {tuple(images.shape)}")
    B, C, R = images.shape[0], images.shape[1], images.shape[3]
    if twiddle.dtype != torch.float32 or twiddle.ndim != 2 or twiddle.shape[1] != 2 or twiddle.shape[0] < 1:
        raise ValueError(f"{what}: twiddle must be float32 [S/2, 2], got {twiddle.dtype} {tuple(twiddle.shape)}")
    S = 2 * twiddle.shape[0]
    check_sizes(R, S, f"{what}: images {tuple(images.shape)} with a twiddle table of {twiddle.shape[0]} entries")
    if not 1 <= C <= 4:
        raise ValueError(f"{what}: images {tuple(images.shape)}: 1..4 channels are supported")
    if window.dtype != torch.float32 or tuple(window.shape) != (R,):
        raise ValueError(f"{what}: window must be float32 [{R}] for images {tuple(images.shape)}, got {window.dtype} {tuple(window.shape)}")
    for name, v in (("window", window), ("twiddle", twiddle)):
        if v.device != images.device:
            raise ValueError(f"{what}: {name} is on {v.device}, images on {images.device}")
    return B, C, R, S


def transform(images, s, t, window, twiddle):
    """CPU tensors only: the windowed fp32 transform of every image-channel, complex64 [B, C, S/2 + 1, S] = Y[kx, ky] -- what `accumulate`
    squares and adds.  The device path never materialises it (the column pass goes from LDS to the accumulator)."""
    B, C, R, S = _checked("spectrum.transform", images, window, twiddle)
    if images.device.type != "cpu":
        raise RuntimeError("spectrum.transform: CPU tensors only; on the device the transform exists per column in LDS, use accumulate")
    stages = twiddle.contiguous()[_stage_index(S, twiddle.device)].numpy()
    x = images.contiguous().reshape(B * C, R, R).to(torch.float32).numpy()
    re, im = _transform_np(x, float(np.float32(s)), float(np.float32(t)), window.contiguous().numpy(), stages, S)
    return torch.complex(torch.from_numpy(re), torch.from_numpy(im)).reshape(B, C, S // 2 + 1, S)


def accumulate(acc, images, s, t, window, twiddle, max_workspace_bytes=256 << 20):
    """acc (float64 [S/2 + 1, S], acc[kx, ky]) += the power spectrum of every image-channel of `images` (uint8 or fp32 [B, C, R, R]), one
    sequential float64 chain per entry in (image, channel) order; in place, returns acc.  `s`, `t`: the normalisation v = fmaf(x, s, t), given
    as numbers (they are rounded to float32); `window` fp32 [R] and `twiddle` fp32 [S/2, 2] as `tables` makes them, on the images' device.
    The batch is cut into pieces whose intermediate ([piece, S/2 + 1, R] float2) fits `max_workspace_bytes`: the result does not depend on
    the cut."""
    what = "spectrum.accumulate"
    if not isinstance(acc, torch.Tensor):
        raise RuntimeError(f"{what}: acc must be a torch tensor, got {type(acc).__name__}")
    B, C, R, S = _checked(what, images, window, twiddle)
    if acc.dtype != torch.float64 or tuple(acc.shape) != (S // 2 + 1, S) or not acc.is_contiguous():
        raise ValueError(f"{what}: acc must be a dense float64 [{S // 2 + 1}, {S}] for S={S}, got {acc.dtype} {tuple(acc.shape)}")
    if acc.device != images.device:
        raise ValueError(f"{what}: acc is on {acc.device}, images on {images.device}")
    if int(max_workspace_bytes) < 1:
        raise ValueError(f"{what}: max_workspace_bytes={max_workspace_bytes} must be positive")
    if B == 0:
        return acc
    s, t = float(np.float32(s)), float(np.float32(t))
    x = images.contiguous().reshape(B * C, R, R)
    window, twiddle = window.contiguous(), twiddle.contiguous()
    stages = twiddle[_stage_index(S, twiddle.device)]           # [S - 1, 2], stage-major: copies, no arithmetic
    per = 8 * (S // 2 + 1) * R
    piece = max(1, min(int(max_workspace_bytes) // per, MAX_PIECE, B * C))
    if images.device.type != "cuda":
        acc_np, w_np, st_np = acc.numpy(), window.numpy(), stages.numpy()
        for lo in range(0, B * C, piece):
            re, im = _transform_np(x[lo:lo + piece].to(torch.float32).numpy(), s, t, w_np, st_np, S)
            re, im = re.astype(np.float64), im.astype(np.float64)
            p = re * re + im * im
            for i in range(p.shape[0]):
                acc_np += p[i]
        return acc
    lib = _lib.load()
    if lib.sbg_spectrum_workspace(piece, R, S) < 0:
        _lib.check(1, "sbg_spectrum_workspace")
    ws = torch.empty([piece * per // 8, 2], dtype=torch.float32, device=images.device)
    stream = _lib.stream_ptr(images.device)
    for lo in range(0, B * C, piece):
        n = min(piece, B * C - lo)
        xs = x[lo:lo + n]
        _lib.check(lib.sbg_spectrum_rows(xs.data_ptr(), int(x.dtype == torch.uint8), window.data_ptr(), stages.data_ptr(), s, t, ws.data_ptr(), n, R, S,
                                         stream), "sbg_spectrum_rows")
        _lib.check(lib.sbg_spectrum_cols(ws.data_ptr(), window.data_ptr(), stages.data_ptr(), acc.data_ptr(), n, R, S, stream), "sbg_spectrum_cols")
    return acc


# ------------------------------------------------------------------------------------------------ host arithmetic (float64, numpy)

def _as_np(a):
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def half_spectrum(acc, count):
    """acc [S/2 + 1, S] (acc[kx, ky]) over `count` image-channels -> the mean power, float64 ndarray [S, S/2 + 1] = P[ky, kx]"""
    acc = _as_np(acc)
    if acc.dtype != np.float64 or acc.ndim != 2 or acc.shape[1] != 2 * (acc.shape[0] - 1) or acc.shape[0] < 2:
        raise ValueError(f"spectrum.half_spectrum: acc must be float64 [S/2 + 1, S], got {acc.dtype} {acc.shape}")
    if int(count) < 1:
        raise ValueError(f"spectrum.half_spectrum: count={count} image-channels")
    return np.ascontiguousarray(acc.T) / float(int(count))


def full_from_half(half):
    """float64 [S, S/2 + 1] -> [S, S]: P[ky, kx] = P[(S - ky) % S, (S - kx) % S], the spectrum of a real image"""
    half = _as_np(half)
    if half.dtype != np.float64 or half.ndim != 2 or half.shape[0] != 2 * (half.shape[1] - 1) or half.shape[1] < 2:
        raise ValueError(f"spectrum.full_from_half: expects float64 [S, S/2 + 1], got {half.dtype} {half.shape}")
    S = half.shape[0]
    full = np.empty([S, S], dtype=np.float64)
    full[:, :S // 2 + 1] = half
    ky = (S - np.arange(S)) % S
    kx = S - np.arange(S // 2 + 1, S)
    full[:, S // 2 + 1:] = half[ky][:, kx]
    return full


def full_spectrum(acc, count):
    """-> float64 ndarray [S, S], P[ky, kx], frequency 0 at [0, 0] (not shifted)"""
    return full_from_half(half_spectrum(acc, count))


def _square(full, what):
    full = _as_np(full)
    if full.dtype != np.float64 or full.ndim != 2 or full.shape[0] != full.shape[1] or full.shape[0] < 2 or full.shape[0] % 2:
        raise ValueError(f"{what}: expects a float64 [S, S] spectrum with an even S, got {full.dtype} {full.shape}")
    return full


def to_db(p):
    return 10.0 * np.log10(np.maximum(_as_np(p), DB_FLOOR))


def radial_profile(full):
    """-> float64 [S/2 + 1]: the mean of the spectrum over the bin r = floor(sqrt(fy^2 + fx^2) + 0.5), f = k for k <= S/2, else k - S"""
    full = _square(full, "spectrum.radial_profile")
    S = full.shape[0]
    k = np.arange(S)
    f = np.where(k <= S // 2, k, k - S).astype(np.float64)
    r = np.floor(np.sqrt(f[:, None] ** 2 + f[None, :] ** 2) + 0.5).astype(np.int64).ravel()
    sums = np.bincount(r, weights=full.ravel())[:S // 2 + 1]
    return sums / np.bincount(r)[:S // 2 + 1]


def slices(full):
    """-> (the 0 degree slice P[0, k], the 45 degree slice P[k, k]), k = 0 .. S/2"""
    full = _square(full, "spectrum.slices")
    k = np.arange(full.shape[0] // 2 + 1)
    return full[0, k].copy(), full[k, k].copy()


def compare(real_full, gen_full):
    """-> dict(lsd_db, hf_excess_db): the root mean square over r = 1 .. S/2, and the mean over S/4 < r <= S/2, of the difference of the
    radial profiles in dB (generated minus real)"""
    real_full, gen_full = _square(real_full, "spectrum.compare (real)"), _square(gen_full, "spectrum.compare (gen)")
    if real_full.shape != gen_full.shape:
        raise ValueError(f"spectrum.compare: the spectra have different sides, real {real_full.shape} and gen {gen_full.shape}")
    S = real_full.shape[0]
    d = to_db(radial_profile(gen_full)) - to_db(radial_profile(real_full))
    return dict(lsd_db=float(np.sqrt(np.mean(d[1:] ** 2))), hf_excess_db=float(np.mean(d[S // 4 + 1:])))
