"""The numpy statement of the tool kernels' fixed-order sums and of fmaf: the ONE definition on the host, as csrc/reduce.h and csrc/merge.h are
on the device.  The CPU paths of swd.py, msssim.py and spectrum.py are built from these; the sums keep the dtype of
their input (float32 or float64), so a float32 kernel is restated in float32.

    block_sum_np(lanes)        [..., 256] -> [...]: reduce.h block_sum<256>
    strided_sum_np(v)          [..., n] -> [...]: lane t adds t, t + 256, ... in ascending order from 0, then block_sum (merge.h, div = 1)
    chunked_sum_np(v, chunk)   [Q, n] -> [Q]: chunks summed by strided_sum_np, the chunk sums by strided_sum_np again
    fma32(a, b, c)             float32 fmaf(a, b, c), one rounding
"""
import numpy as np

NT = 256                    # work-items of the summing workgroups


def block_sum_np(lanes):
    """csrc/reduce.h block_sum over the last axis of 256 lanes: the xor butterfly (offsets 32 .. 1) in each wave, the four waves left to right"""
    w = lanes.reshape(lanes.shape[:-1] + (NT // 64, 64))
    lane = np.arange(64)
    for off in (32, 16, 8, 4, 2, 1):
        w = w + w[..., lane ^ off]
    s = w[..., 0, 0]
    for i in range(1, NT // 64):
        s = s + w[..., i, 0]
    return s


def strided_sum_np(v):
    """v [..., n] -> [...]: lane t adds the elements t, t + 256, ... in ascending order, then block_sum"""
    n = v.shape[-1]
    rounds = -(-n // NT)
    if rounds * NT != n:
        v = np.concatenate([v, np.zeros(v.shape[:-1] + (rounds * NT - n,), dtype=v.dtype)], axis=-1)       # + 0.0 changes nothing
    v = v.reshape(v.shape[:-1] + (rounds, NT))
    acc = np.zeros(v.shape[:-2] + (NT,), dtype=v.dtype)
    for r in range(rounds):
        acc = acc + v[..., r, :]
    return block_sum_np(acc)


def chunked_sum_np(v, chunk):
    """v [Q, n] -> [Q]: chunks of `chunk` elements summed by strided_sum_np, the chunk sums by strided_sum_np again"""
    q, n = v.shape
    chunks = -(-n // chunk)
    if chunks * chunk != n:
        v = np.concatenate([v, np.zeros([q, chunks * chunk - n], dtype=v.dtype)], axis=1)
    return strided_sum_np(strided_sum_np(v.reshape(q, chunks, chunk)))


def fma32(a, b, c):
    """float32 arrays -> fmaf(a, b, c), one rounding: the product of two floats is exact in float64; the float64 sum is taken with its
    exact error (two-sum) and forced to an odd last bit when inexact, after which the rounding to float32 is the rounding of the exact value"""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = c.astype(np.float64)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    fix = (err != 0) & ((s.view(np.int64) & 1) == 0) & np.isfinite(s)
    if fix.any():
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)
