"""Arithmetic of the network summary tool (csrc/act_stats.hip; network_summary.py): one record of counts and sums per
(sample, channel) plane of an activation tensor, the fold of such records into running per-channel records, and the numbers derived from them.
Every function has ONE definition for both devices: device tensors run the HIP kernels, CPU tensors run the same value graph in numpy, built from
``_exact_common`` -- the results are equal bit for bit, not close.  On the device an unsupported input is an error, never a quiet fallback or copy.

    planes(x)                          fp16 / bf16 / fp32 tensor of rank 4 ([N, C, H, W], dense NCHW or channels_last, or a batch / channel slice of
                                       one) or rank 2 ([N, F]: C = F, one pixel) -> (counts int64 [N, C, 70], values float64 [N, C, 4]) on x's
                                       device.  Every element is converted exactly to fp32.
                                         counts: [0] n = P, [1] n_zero (either sign), [2] n_nan, [3] n_posinf, [4] n_neginf, [5] n_peak (finite
                                           elements with |x| == the largest finite |x| of the plane; 0 without a finite element), [6 .. 69] the
                                           exponent histogram of the finite non-zero elements: bin = min(max(floor(log2 |x|), -32), 31) + 32,
                                           fp32 subnormals in bin 0.
                                         values: [0] sum and [1] sumsq of the finite elements in float64 ((double)x and its square are exact),
                                           added in the project's fixed order over the pixel index p whatever the layout: lane t of 256 adds
                                           p = t, t + 256, ... ascending from +0.0, then block_sum (``_exact_common.strided_sum_np``);
                                           [2] min and [3] max of the finite elements (a zero of either sign is +0.0), +inf / -inf without one.
    empty(C, device)                   -> running (counts int64 [C, 70], values float64 [C, 4]) of no sample: zeros, min = +inf, max = -inf.
    fold(counts, values, run_counts, run_values)
                                       adds the records [N, C, ...] into the running records [C, ...] in place, n ascending, and returns them:
                                       counts add; sum and sumsq add in sample order (so batching does not matter); min / max combine; n_peak
                                       follows the larger peak max(|min|, |max|) and adds on equal peaks.
    derive(counts, values)             host, float64: running records (numpy or tensors) -> dict of per-entry numbers and per-channel arrays.
                                       Everything floating beyond the two sums happens here, on both devices.

All refusals happen on the host, before any launch, with a message naming shape, strides, dtype and device.
"""
import numpy as np
import torch

from ... import _lib
from ._exact_common import strided_sum_np

COUNTS, VALUES, BINS, HIST0 = 70, 4, 64, 6
N_, N_ZERO, N_NAN, N_POSINF, N_NEGINF, N_PEAK = range(6)
SUM, SUMSQ, MIN, MAX = range(4)
MAX_P = (1 << 31) - 1 - 4096
MAX_PLANES = (1 << 31) - 1 - 256
FP16_MAX = 65504.0
FP16_OVERFLOW_BIN = 16 + 32         # binades e >= 16: |x| >= 65536 (see `derive` on the binade granularity)
FP16_SUBNORMAL_BIN = -14 + 32       # binades e < -14: |x| < 2^-14, below fp16's smallest normal


def _describe(**tensors):
    return ', '.join(f'{name} {t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}' for name, t in tensors.items() if t is not None)


def logical_strides(x):
    """x of rank 2 or 4 -> (N, C, P, sn, sc, sp): the [N, C, P] view the kernel reads, strides in elements.  Refuses (RuntimeError) what is no
    such view: another rank or dtype, pixels that are not one strided run, overlapping planes."""
    what = 'act_stats.planes'
    if not isinstance(x, torch.Tensor) or x.dtype not in (torch.float16, torch.bfloat16, torch.float32):
        raise RuntimeError(f'{what}: expects an fp16, bf16 or fp32 tensor; got {_describe(x=x) if isinstance(x, torch.Tensor) else type(x)}')
    said = _describe(x=x)
    if x.ndim == 2:
        n, c = x.shape
        p, sn, sc, sp = 1, x.stride(0), x.stride(1), 1
    elif x.ndim == 4:
        n, c, h, w = x.shape
        sn, sc, sh, sw = x.stride()
        p = h * w
        if w == 1:
            sp = sh
        elif h == 1 or sh == w * sw:
            sp = sw
        else:
            raise RuntimeError(f'{what}: the pixels of a plane must be one strided run (stride(2) == W * stride(3)); got {said}')
        if p == 1:
            sp = 1
    else:
        raise RuntimeError(f'{what}: expects a tensor of rank 2 ([N, F]) or 4 ([N, C, H, W]); got {said}')
    if n < 1 or c < 1 or p < 1 or p > MAX_P or n * c > MAX_PLANES:
        raise RuntimeError(f'{what}: [N, C, P] = [{n}, {c}, {p}] is not within 1 <= P < 2^31 - 4096, 1 <= N C < 2^31 - 256; got {said}')
    # no two elements may share an address: sort the axes of size > 1 by stride; each must step over the whole extent of the ones below it
    axes = sorted((s, k) for s, k in ((sp, p), (sc, c), (sn, n)) if k > 1)
    extent = 1
    for s, k in axes:
        if s < extent:
            raise RuntimeError(f'{what}: the elements overlap or a stride is not positive (unsupported strides); got {said}')
        extent = s * (k - 1) + extent
    # an axis of size 1 has no stride of its own
    return int(n), int(c), int(p), int(sn) if n > 1 else 0, int(sc) if c > 1 else 0, int(sp) if p > 1 else 0


def path(x):
    """the mapping `planes` takes for a device tensor (``_lib.ACT_STATS_PATHS``): the launch record's fifth entry"""
    n, c, p, sn, sc, sp = logical_strides(x)
    return _lib.ACT_STATS_PATHS[_lib.load().sbg_act_stats_path(x.data_ptr(), _lib.dtype_code(x.dtype), n, c, p, sn, sc, sp)]


def _plane_values(x, n, c, p, sn, sc, sp):
    """the fp32 values of a CPU tensor as a numpy [N, C, P] array (exact: fp16 and bf16 widen without rounding)"""
    flat = torch.as_strided(x, (n, c, p), (sn, sc, sp))
    return flat.to(torch.float32).numpy()


def planes_np(v):
    """the definition on the host: fp32 numpy [N, C, P] -> (counts int64 [N, C, 70], values float64 [N, C, 4])"""
    n, c, p = v.shape
    bits = v.view(np.uint32)
    mag = bits & np.uint32(0x7fffffff)
    nan = mag > 0x7f800000
    inf = mag == 0x7f800000
    neg = (bits >> np.uint32(31)).astype(bool)
    finite = mag < 0x7f800000
    zero = mag == 0
    counts = np.zeros([n, c, COUNTS], dtype=np.int64)
    counts[..., N_] = p
    counts[..., N_ZERO] = zero.sum(axis=2)
    counts[..., N_NAN] = nan.sum(axis=2)
    counts[..., N_POSINF] = (inf & ~neg).sum(axis=2)
    counts[..., N_NEGINF] = (inf & neg).sum(axis=2)
    absf = mag.view(np.float32)
    peak = np.where(finite, absf, np.float32(-1)).max(axis=2)
    counts[..., N_PEAK] = (finite & (absf == peak[..., None])).sum(axis=2)
    e = (mag >> np.uint32(23)).astype(np.int64) - 127
    bins = np.clip(e, -32, 31) + 32
    live = finite & ~zero
    for b in range(BINS):
        counts[..., HIST0 + b] = (live & (bins == b)).sum(axis=2)
    d = np.where(finite, v.astype(np.float64), 0.0)
    values = np.empty([n, c, VALUES], dtype=np.float64)
    values[..., SUM] = strided_sum_np(d)
    values[..., SUMSQ] = strided_sum_np(d * d)
    seen = np.where(zero, np.float32(0), v).astype(np.float64)          # a zero of either sign is +0.0
    values[..., MIN] = np.where(finite, seen, np.inf).min(axis=2)
    values[..., MAX] = np.where(finite, seen, -np.inf).max(axis=2)
    return counts, values


def planes(x):
    n, c, p, sn, sc, sp = logical_strides(x)
    if x.device.type != 'cuda':
        counts, values = planes_np(_plane_values(x.detach(), n, c, p, sn, sc, sp))
        return torch.from_numpy(counts), torch.from_numpy(values)
    counts = torch.empty([n, c, COUNTS], dtype=torch.int64, device=x.device)
    values = torch.empty([n, c, VALUES], dtype=torch.float64, device=x.device)
    _lib.check(_lib.load().sbg_act_stats_planes(x.data_ptr(), _lib.dtype_code(x.dtype), n, c, p, sn, sc, sp, counts.data_ptr(), values.data_ptr(),
                                                _lib.stream_ptr(x.device)), 'sbg_act_stats_planes')
    return counts, values


def empty(channels, device='cpu'):
    counts = torch.zeros([int(channels), COUNTS], dtype=torch.int64, device=device)
    values = torch.zeros([int(channels), VALUES], dtype=torch.float64, device=device)
    values[:, MIN] = float('inf')
    values[:, MAX] = float('-inf')
    return counts, values


def _peak_np(mn, mx):
    """the peak of records with these min / max: max(|min|, |max|), -1 where the record holds no finite element"""
    return np.where(mn <= mx, np.maximum(np.abs(mn), np.abs(mx)), -1.0)


def fold(counts, values, run_counts, run_values):
    what = 'act_stats.fold'
    said = _describe(counts=counts, values=values, run_counts=run_counts, run_values=run_values)
    if counts.dtype != torch.int64 or counts.ndim != 3 or counts.shape[2] != COUNTS or not counts.is_contiguous():
        raise RuntimeError(f'{what}: counts must be a dense int64 [N, C, {COUNTS}] tensor; got {said}')
    n, c = int(counts.shape[0]), int(counts.shape[1])
    for name, t, dtype, shape in (('values', values, torch.float64, (n, c, VALUES)), ('run_counts', run_counts, torch.int64, (c, COUNTS)),
                                  ('run_values', run_values, torch.float64, (c, VALUES))):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise RuntimeError(f'{what}: {name} must be a dense {dtype} {list(shape)} tensor; got {said}')
    if len({t.device for t in (counts, values, run_counts, run_values)}) != 1:
        raise RuntimeError(f'{what}: the four tensors must be on one device; got {said}')
    if c < 1 or n * c > MAX_PLANES or c * (COUNTS + VALUES) > MAX_PLANES:
        raise RuntimeError(f'{what}: [N, C] = [{n}, {c}] is not within 1 <= C, N C < 2^31 - 256, 74 C < 2^31 - 256; got {said}')
    if n == 0:
        return run_counts, run_values
    if counts.device.type != 'cuda':
        rc, rv, k, v = run_counts.numpy(), run_values.numpy(), counts.numpy(), values.numpy()
        for i in range(n):
            have, got = _peak_np(rv[:, MIN], rv[:, MAX]), _peak_np(v[i, :, MIN], v[i, :, MAX])
            npk = np.where(got > have, k[i, :, N_PEAK], np.where(got == have, rc[:, N_PEAK] + k[i, :, N_PEAK], rc[:, N_PEAK]))
            rc += k[i]
            rc[:, N_PEAK] = npk
            rv[:, SUM] = rv[:, SUM] + v[i, :, SUM]
            rv[:, SUMSQ] = rv[:, SUMSQ] + v[i, :, SUMSQ]
            rv[:, MIN] = np.minimum(rv[:, MIN], v[i, :, MIN])
            rv[:, MAX] = np.maximum(rv[:, MAX], v[i, :, MAX])
        return run_counts, run_values
    _lib.check(_lib.load().sbg_act_stats_fold(counts.data_ptr(), values.data_ptr(), run_counts.data_ptr(), run_values.data_ptr(), n, c,
                                              _lib.stream_ptr(counts.device)), 'sbg_act_stats_fold')
    return run_counts, run_values


# ---------------------------------------------------------------------------------------------------------------- host

def derive(counts, values):
    """running records counts [C, 70], values [C, 4] (numpy arrays or tensors of either device) -> dict, all float64 / int on the host.
    Per entry (all channels together): n, mean, rms, min, max, absmax (None without a finite element), zero_share, nonfinite (count), peak_share
    (elements on the largest |x| of the entry over the finite ones), fp16_overflow_share, fp16_subnormal_share, fp16_headroom_bits =
    log2(65504 / absmax), dead_channels (indices of the channels whose every element was zero), channel_rms_spread (largest over smallest rms
    of the channels that are not dead; None with fewer than two), hist (int [64]).  Per channel, under `channels`: mean, rms, absmax, zero_share,
    nonfinite, peak_share.
    THE FP16 SHARES HAVE THE GRANULARITY OF A BINADE: they are read from the exponent histogram.  Overflow counts the finite elements with
    floor(log2 |x|) >= 16, i.e. |x| >= 65536; the values in (65504, 65536), which also round to infinity in fp16, sit in binade 15 with values
    fp16 holds and are not counted.  Subnormal counts the non-zero elements with floor(log2 |x|) < -14, i.e. below fp16's smallest normal 2^-14
    (this includes what fp16 flushes to zero below 2^-24); binade -14 itself is normal in fp16.  Both shares, like
    zero_share and peak_share, are over the finite elements."""
    k = np.asarray(counts.cpu() if isinstance(counts, torch.Tensor) else counts).astype(np.int64)
    v = np.asarray(values.cpu() if isinstance(values, torch.Tensor) else values).astype(np.float64)
    n = k[:, N_]
    nonfinite = k[:, N_NAN] + k[:, N_POSINF] + k[:, N_NEGINF]
    finite = n - nonfinite
    hist = k[:, HIST0:HIST0 + BINS]
    has = v[:, MIN] <= v[:, MAX]
    absmax_c = np.where(has, np.maximum(np.abs(v[:, MIN]), np.abs(v[:, MAX])), np.nan)

    def share(a, b):
        return float(a) / float(b) if b else None

    with np.errstate(divide='ignore', invalid='ignore'):
        ch = dict(mean=np.where(finite > 0, v[:, SUM] / finite, np.nan), rms=np.where(finite > 0, np.sqrt(v[:, SUMSQ] / finite), np.nan), absmax=absmax_c,
                  zero_share=np.where(finite > 0, k[:, N_ZERO] / np.maximum(finite, 1), np.nan), nonfinite=nonfinite,
                  peak_share=np.where(finite > 0, k[:, N_PEAK] / np.maximum(finite, 1), np.nan))
    total, total_finite = int(n.sum()), int(finite.sum())
    any_finite = bool(has.any())
    absmax = float(np.nanmax(absmax_c)) if any_finite else None
    on_peak = int(k[:, N_PEAK][absmax_c == absmax].sum()) if any_finite else 0
    dead = [int(i) for i in np.nonzero((k[:, N_ZERO] == n) & (n > 0))[0]]
    alive = [float(r) for i, r in enumerate(ch['rms']) if i not in set(dead) and np.isfinite(r) and r > 0]
    all_hist = hist.sum(axis=0)
    out = dict(n=total, mean=share(v[:, SUM].sum(), total_finite), rms=float(np.sqrt(v[:, SUMSQ].sum() / total_finite)) if total_finite else None,
               min=float(v[:, MIN].min()) if any_finite else None, max=float(v[:, MAX].max()) if any_finite else None, absmax=absmax,
               zero_share=share(int(k[:, N_ZERO].sum()), total_finite), nonfinite=int(nonfinite.sum()), peak_share=share(on_peak, total_finite),
               fp16_overflow_share=share(int(all_hist[FP16_OVERFLOW_BIN:].sum()), total_finite),
               fp16_subnormal_share=share(int(all_hist[:FP16_SUBNORMAL_BIN].sum()), total_finite),
               fp16_headroom_bits=float(np.log2(FP16_MAX / absmax)) if absmax else None,
               dead_channels=dead, channel_rms_spread=max(alive) / min(alive) if len(alive) >= 2 else None,
               hist=[int(h) for h in all_hist], channels=ch)
    return out
