"""End of a training phase over a flat fp32 gradient bucket (csrc/grad_finish.hip): scale, ``nan_to_num`` and gradient health in one pass.

The reference sanitises every parameter's gradient with ``misc.nan_to_num(param.grad, nan=0, posinf=1e5, neginf=-1e5)``
(train_parts/trainers.py:745-747) and keeps no record of what it erased.  One definition for both devices, per element of ``flat`` and a
scale ``s``:

    y = x * s            one fp32 multiply, skipped when s == 1
    z = nan -> +0, +inf -> 1e5, -inf -> -1e5, anything else y            written back in place
    health = [number of non-finite y, sum of z^2 in float64, max |z|]    float64 [3]

``sweep`` writes one record per chunk of the buffer (``records(n)`` of them, a function of n alone), ``merge`` adds a run of records --
those of several buffers laid out back to back -- in an order fixed by their number alone.  Device buffers run the kernels: they must be dense fp32 and 16-byte
aligned, anything else is an error, never a quiet torch path.  ``finish_cpu`` is the same definition in torch for CPU buckets.
"""
import ctypes

import torch

from ... import _lib


def records(n):
    """number of [count, sumsq, absmax] records a sweep over n elements writes"""
    r = _lib.load().sbg_grad_finish_records(int(n))
    if r < 0:
        raise RuntimeError(f"grad_finish: bad size n={n}")
    return int(r)


def sweep(flat, scale, partials):
    """flat: dense fp32 device buffer, sanitised in place; partials: float64 device tensor with room for records(n) * 3 values"""
    _lib.require_cuda(flat, "grad_finish.sweep")
    _lib.require_dtype(flat, torch.float32, "grad_finish.sweep")
    _lib.require_dtype(partials, torch.float64, "grad_finish.sweep (partials)")
    if flat.ndim != 1 or not flat.is_contiguous() or not partials.is_contiguous() or partials.device != flat.device:
        raise RuntimeError("grad_finish.sweep: expects a dense 1-d buffer and dense partials on its device")
    n = flat.numel()
    lib = _lib.load()
    need = 3 * lib.sbg_grad_finish_records(n)
    if partials.numel() < need:
        raise RuntimeError(f"grad_finish.sweep: partials hold {partials.numel()} values, {need} are written")
    _lib.check(lib.sbg_grad_finish_sweep(flat.data_ptr(), n, ctypes.c_float(float(scale)), partials.data_ptr(), _lib.stream_ptr(flat.device)),
               "sbg_grad_finish_sweep")
    return flat


def merge(partials, out=None):
    """partials: float64 [R, 3] (or flat [3 R]) records on the device -> float64 [3] = [sum count, sum sumsq, max absmax], summed in an order fixed by R alone"""
    _lib.require_cuda(partials, "grad_finish.merge")
    _lib.require_dtype(partials, torch.float64, "grad_finish.merge")
    if not partials.is_contiguous() or partials.numel() % 3:
        raise RuntimeError("grad_finish.merge: expects dense records of three float64 values")
    if out is None:
        out = torch.empty([3], dtype=torch.float64, device=partials.device)
    _lib.require_dtype(out, torch.float64, "grad_finish.merge (out)")
    if out.shape != (3,) or out.device != partials.device or not out.is_contiguous():
        raise RuntimeError("grad_finish.merge: out must be a dense float64 [3] on the records' device")
    lib = _lib.load()
    _lib.check(lib.sbg_grad_finish_merge(partials.data_ptr(), partials.numel() // 3, out.data_ptr(), _lib.stream_ptr(partials.device)),
               "sbg_grad_finish_merge")
    return out


def finish_cpu(flat, scale=1.0):
    """the definition above with torch ops (CPU buckets): flat is sanitised in place -> float64 [3]"""
    if scale != 1.0:
        flat.mul_(scale)
    count = (~torch.isfinite(flat)).sum().to(torch.float64)
    torch.nan_to_num(flat, nan=0, posinf=1e5, neginf=-1e5, out=flat)
    z = flat.to(torch.float64)
    absmax = z.abs().max() if z.numel() else torch.zeros([], dtype=torch.float64)
    return torch.stack([count, z.square().sum(), absmax])
