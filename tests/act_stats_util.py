"""What the act_stats tests share: an independent restatement of the record in plain numpy and Python (np.frexp for the bins, Python loops for the
counts and for the lane order -- nothing of torch_utils/ops/act_stats.py's CPU path or of _exact_common is imported), and the case builder."""
import math

import numpy as np
import torch

COUNTS, VALUES = 70, 4
DTYPES = {"fp16": torch.float16, "bf16": torch.bfloat16, "fp32": torch.float32}
LAYOUTS = ("nchw", "channels_last", "2d", "slice", "offset")
PLANE_SHAPES = {1: (1, 1), 16: (4, 4), 255: (15, 17), 256: (16, 16), 257: (1, 257), 1089: (33, 33)}
CHANNELS = (1, 3, 7, 8, 9, 72)
BATCHES = (1, 5)

# planted in random data wherever the dtype holds them exactly: zeros, fp16 and fp32 subnormals, powers of two on bin edges, the non-finite values
SPECIALS = [0.0, -0.0, 2.0 ** -20, -(2.0 ** -24), 2.0 ** -130, -(2.0 ** -133), 2.0 ** -140, 2.0 ** -33, 2.0 ** -32, -(2.0 ** -14), 2.0 ** 16, 2.0 ** 31,
            -(2.0 ** 32), float("inf"), float("-inf"), float("nan")]


def _holds(value, dtype):
    if math.isnan(value) or math.isinf(value):
        return True
    back = float(torch.tensor([value], dtype=torch.float64).to(dtype).to(torch.float64)[0])
    return back == value and (value == 0 or back != 0)


def plane_values(kind, p, dtype, rng):
    """one plane of `p` fp32 values of the given kind (0 random with the specials planted, 1 all zeros, 2 all NaN, 3 clamped to +-256 with
    several elements on the peak, 4 a negative peak, 5 random)"""
    v = (rng.standard_normal(p) * 3.0).astype(np.float32)
    if kind == 0:
        specials = [s for s in SPECIALS if _holds(s, dtype)]
        if p == 1:
            v[0] = specials[int(rng.integers(len(specials)))]
        else:
            for k, s in enumerate(specials):
                v[(k * 37 + 5) % p] = s
    elif kind == 1:
        v[:] = 0.0
        v[::2] = -0.0
    elif kind == 2:
        v[:] = np.nan
    elif kind == 3:
        v = np.clip(v * 200.0, -256.0, 256.0)
        v[:: max(p // 5, 1)] = 256.0
        v[p // 2] = -256.0
    elif kind == 4:
        v = np.clip(v, -7.5, 1.0)
        v[p // 3] = -7.5
        v[0] = -7.5
    return v


def build_case(dtype_name, layout, n, c, p, seed=0):
    """-> a CPU tensor of the dtype in the layout with logical shape [n, c, h, w] ([n, c] for '2d', which needs p == 1).  'slice' is [1:4] of a
    batch of 5 (n == 5 -> three samples) or [1:2] of 3 (n == 1); 'offset' starts one element into its buffer, so it is misaligned for 16-byte
    loads.  The kind of plane i is (i + seed) % 6."""
    dtype = DTYPES[dtype_name]
    rng = np.random.default_rng(1000 * seed + 17 * c + p + n)
    h, w = PLANE_SHAPES[p]
    if layout == "slice":
        total, lo, hi = (5, 1, 4) if n > 1 else (3, 1, 2)
    else:
        total, lo, hi = n, 0, n
    data = np.stack([plane_values((i + seed) % 6, p, dtype, rng) for i in range(total * c)]).reshape(total, c, h, w)
    x = torch.from_numpy(data).to(dtype)
    if layout == "2d":
        assert p == 1
        return x.reshape(total, c).clone()
    if layout == "channels_last":
        x = x.contiguous(memory_format=torch.channels_last)
        if c == 1 or p == 1:            # torch calls such a tensor contiguous in both formats: force the channel-minor strides
            x = torch.as_strided(x, x.shape, (c * h * w, 1, w * c, c))
        return x
    if layout == "offset":
        buf = torch.zeros([x.numel() + 1], dtype=dtype)
        buf[1:] = x.reshape(-1)
        return buf[1:].view(total, c, h, w)
    return x[lo:hi]


def _fp32_planes(x):
    """any case tensor -> fp32 numpy [N, C, P] in logical order (exact widening)"""
    v = x.to(torch.float32)
    return v.reshape(v.shape[0], v.shape[1], -1).numpy().copy()


def _lane_sum(values):
    """float64 list -> the fixed-order sum: lane t of 256 adds t, t + 256, ... ascending from +0.0; in each wave of 64 lanes a butterfly with the
    xor offsets 32, 16, 8, 4, 2, 1; then the four wave values left to right"""
    lanes = [0.0] * 256
    for t in range(256):
        acc = 0.0
        for i in range(t, len(values), 256):
            acc = acc + values[i]
        lanes[t] = acc
    waves = []
    for w in range(4):
        cur = lanes[64 * w:64 * w + 64]
        for off in (32, 16, 8, 4, 2, 1):
            cur = [cur[i] + cur[i ^ off] for i in range(64)]
        waves.append(cur[0])
    return ((waves[0] + waves[1]) + waves[2]) + waves[3]


def restate_planes(x):
    """-> (counts int64 [N, C, 70], values float64 [N, C, 4]) of a CPU tensor, from the statement of the record alone"""
    v = _fp32_planes(x)
    n, c, p = v.shape
    counts = np.zeros([n, c, COUNTS], dtype=np.int64)
    values = np.zeros([n, c, VALUES], dtype=np.float64)
    for i in range(n):
        for j in range(c):
            plane = [float(e) for e in v[i, j]]
            k = counts[i, j]
            k[0] = p
            finite = [e for e in plane if math.isfinite(e)]
            peak = max((abs(e) for e in finite), default=None)
            for e in plane:
                if math.isnan(e):
                    k[2] += 1
                elif e == math.inf:
                    k[3] += 1
                elif e == -math.inf:
                    k[4] += 1
                elif e == 0:
                    k[1] += 1
                else:
                    mantissa, exponent = np.frexp(e)        # |e| = |mantissa| 2^exponent, 0.5 <= |mantissa| < 1: floor(log2 |e|) = exponent - 1
                    k[6 + min(max(int(exponent) - 1, -32), 31) + 32] += 1
                if math.isfinite(e) and abs(e) == peak:
                    k[5] += 1
            kept = [e if math.isfinite(e) else 0.0 for e in plane]
            values[i, j, 0] = _lane_sum(kept)
            values[i, j, 1] = _lane_sum([e * e for e in kept])
            values[i, j, 2] = min((e + 0.0 for e in finite), default=math.inf) + 0.0
            values[i, j, 3] = max((e + 0.0 for e in finite), default=-math.inf) + 0.0
    return counts, values


def same_bits(a, b):
    """two tensors / arrays of one dtype (int64 or float64) are equal as bit patterns"""
    a, b = np.ascontiguousarray(np.asarray(a)), np.ascontiguousarray(np.asarray(b))
    return a.dtype == b.dtype and a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


def first_difference(a, b):
    a, b = np.asarray(a), np.asarray(b)
    where = np.argwhere(a.view(np.int64) != b.view(np.int64))
    return None if len(where) == 0 else (tuple(int(i) for i in where[0]), a[tuple(where[0])], b[tuple(where[0])], len(where))
