"""Arithmetic of the latent walk tool (csrc/walk.hip; interpolate.py).  Every function has ONE definition for both
devices: device tensors run the HIP kernels, CPU tensors run the same arithmetic in numpy (``_exact_common.fma32``) or torch int64 -- the results
are equal bit for bit, not close.  On the device an unsupported input is an error, never a quiet fallback.

    blend_table(keys, index, weight, layers=None, hold=None)
                                   fp32 [K, L, D], int32 [T, 4], fp32 [T, 4] -> fp32 [T, L, D].  On every layer in ``layers`` (default: all)
                                   element (t, l, d) is this fp32 chain and no other:
                                     1. acc = weight[t, 0] * keys[index[t, 0], l, d], one rounded product;
                                     2. acc = fmaf(weight[t, j], keys[index[t, j], l, d], acc) for j = 1, 2, 3, in that order.
                                   On a layer not in ``layers`` it is a copy of keys[hold[t], l, d]; ``hold`` (int32 [T]) is required exactly
                                   when ``layers`` leaves a layer out.  T = 0 gives an empty table without a launch.
    pair_sqdiff(a, b)              uint8 [N, F], uint8 [N, F] -> int64 [N]: row n is sum_f (a[n, f] - b[n, f])^2, exact.  Any F >= 1 and any
                                   row alignment; a and b may be slices along dimension 0 of one dense tensor.  N <= 2^24, F <= 2^26.
    walk_weights(method, K, frames_per_key, loop, omega=None)
                                   host, float64: the taps and weights of ONE walk through K >= 2 keys ->
                                   (index int32 [T, 4], weight fp32 [T, 4], segment int32 [T], tau float64 [T]); ``walk_weights64`` returns the
                                   weights before their one rounding to fp32.

Both ops refuse on the host, before any launch and with a message naming shapes, dtypes and devices: wrong dtypes, non-dense tensors, mixed
devices, D outside 1 .. MAX_D, T L D >= 2^31 and any index or hold value outside [0, K).  The range check reads ``index`` back: one small
synchronisation per table is the price of never launching a kernel that could read outside ``keys``.
"""
import numpy as np
import torch

from ... import _lib
from ._exact_common import fma32

MAX_D = 1024
MAX_N, MAX_F = 1 << 24, 1 << 26
CHUNK = 16384               # bytes of a row per workgroup of pair_sqdiff
METHODS = ('linear', 'cubic', 'slerp')
SLERP_EPS = 1e-6            # sin(omega) below this: the linear weights


# ---------------------------------------------------------------------------------------------------------------- weights

def walk_weights64(method, K, frames_per_key, loop, omega=None):
    """-> (index int32 [T, 4], weight float64 [T, 4], segment int32 [T], tau float64 [T]): the taps s - 1, s, s + 1, s + 2 of every frame.
    Open walk: T = (K - 1) n + 1, u = f / n, s = min(floor(u), K - 2), tau = u - s (the last frame is s = K - 2, tau = 1).  Loop: T = K n,
    s = floor(u), neighbours mod K.  A tap without a key (and the two taps linear and slerp do not use) points at s with weight 0."""
    K, n, loop = int(K), int(frames_per_key), bool(loop)
    if method not in METHODS:
        raise ValueError(f'--method={method}: one of {", ".join(METHODS)}')
    if K < 2:
        raise ValueError(f'a walk needs at least 2 keys, got {K}')
    if n < 1:
        raise ValueError(f'--frames-per-key={n}: must be at least 1')
    T = K * n if loop else (K - 1) * n + 1
    u = np.arange(T, dtype=np.float64) / np.float64(n)
    seg = np.floor(u).astype(np.int64)
    if not loop:
        seg = np.minimum(seg, K - 2)
    tau = u - seg
    taps = seg[:, None] + np.arange(-1, 3)[None, :]
    w = np.zeros([T, 4], dtype=np.float64)
    if method == 'cubic':
        t2, t3 = tau * tau, tau * tau * tau
        w[:, 0] = (-t3 + 2 * t2 - tau) / 2
        w[:, 1] = (3 * t3 - 5 * t2 + 2) / 2
        w[:, 2] = (-3 * t3 + 4 * t2 + tau) / 2
        w[:, 3] = (t3 - t2) / 2
        if not loop:                                    # the missing neighbour is the reflected one, folded in before rounding
            first, last = seg == 0, seg == K - 2
            w[first, 1] += 2 * w[first, 0]
            w[first, 2] -= w[first, 0]
            w[first, 0] = 0
            w[last, 2] += 2 * w[last, 3]
            w[last, 1] -= w[last, 3]
            w[last, 3] = 0
            taps[first, 0] = seg[first]
            taps[last, 3] = seg[last]
    else:
        w[:, 1], w[:, 2] = 1 - tau, tau
        if method == 'slerp':
            segments = K if loop else K - 1
            omega = None if omega is None else np.asarray(omega, dtype=np.float64)
            if omega is None or omega.shape != (segments,):
                raise ValueError(f'--method=slerp: needs the angle of each of the {segments} segments, got '
                                 f'{None if omega is None else omega.shape}')
            om = omega[seg]
            so = np.sin(om)
            ok = so >= SLERP_EPS
            so = np.where(ok, so, 1)
            w[:, 1] = np.where(ok, np.sin((1 - tau) * om) / so, w[:, 1])
            w[:, 2] = np.where(ok, np.sin(tau * om) / so, w[:, 2])
        taps[:, 0] = seg
        taps[:, 3] = seg
    taps = taps % K if loop else taps
    assert taps.min() >= 0 and taps.max() < K
    return taps.astype(np.int32), w, seg.astype(np.int32), tau


def walk_weights(method, K, frames_per_key, loop, omega=None):
    """`walk_weights64` with the weights rounded once to fp32"""
    index, w, seg, tau = walk_weights64(method, K, frames_per_key, loop, omega)
    return index, w.astype(np.float32), seg, tau


# ---------------------------------------------------------------------------------------------------------------- blend_table

def _describe(**tensors):
    return ', '.join(f'{name} {t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}' for name, t in tensors.items() if t is not None)


def blend_table(keys, index, weight, layers=None, hold=None):
    what = 'walk.blend_table'
    given = dict(keys=keys, index=index, weight=weight, hold=hold)
    said = _describe(**given)
    for name, t, dtype, ndim in (('keys', keys, torch.float32, 3), ('index', index, torch.int32, 2), ('weight', weight, torch.float32, 2),
                                 ('hold', hold, torch.int32, 1)):
        if t is None:
            continue
        if t.dtype != dtype or t.ndim != ndim or not t.is_contiguous():
            raise RuntimeError(f'{what}: {name} must be a dense {str(dtype).replace("torch.", "")} tensor of {ndim} dimensions; got {said}')
        if t.device != keys.device:
            raise RuntimeError(f'{what}: every tensor must be on the device of keys; got {said}')
    k, l, d = keys.shape
    t = index.shape[0]
    if k < 1 or l < 1 or not 1 <= d <= MAX_D or tuple(index.shape) != (t, 4) or tuple(weight.shape) != (t, 4) or (hold is not None and hold.shape[0] != t):
        raise RuntimeError(f'{what}: expects keys [K >= 1, L >= 1, 1 <= D <= {MAX_D}], index and weight [T, 4] and hold [T]; got {said}')
    if t * l * d >= 1 << 31:
        raise RuntimeError(f'{what}: a table of T L D = {t} x {l} x {d} = {t * l * d} elements is not below 2^31; got {said}')
    if layers is not None:
        layers = sorted({int(i) for i in layers})
        if not layers or layers[0] < 0 or layers[-1] >= l:
            raise RuntimeError(f'{what}: layers {layers} must be a non-empty set of indices in [0, {l}); got {said}')
        if len(layers) == l:
            layers = None
    if (layers is None) != (hold is None):
        raise RuntimeError(f'{what}: hold is required exactly when layers leaves a layer out (layers {layers if layers is not None else "all"}); got {said}')
    if t == 0:
        return torch.empty([0, l, d], dtype=torch.float32, device=keys.device)
    outside = (index < 0) | (index >= k)                # the read-back: nothing is launched on an index that leaves keys
    if bool(outside.any()) or (hold is not None and bool(((hold < 0) | (hold >= k)).any())):
        raise RuntimeError(f'{what}: an index or hold value lies outside [0, K = {k}); got {said}')
    if keys.device.type != 'cuda':
        kn, idx, wn = keys.numpy(), index.numpy(), weight.numpy()
        sel = slice(None) if layers is None else layers
        tap = lambda j: kn[idx[:, j]][:, sel]
        acc = wn[:, 0, None, None] * tap(0)             # one rounded fp32 product
        for j in (1, 2, 3):
            acc = fma32(np.broadcast_to(wn[:, j, None, None], acc.shape), tap(j), acc)
        if layers is None:
            return torch.from_numpy(acc)
        out = kn[hold.numpy()].copy()
        out[:, layers] = acc
        return torch.from_numpy(out)
    mask = None
    if layers is not None:
        mask = torch.zeros([l], dtype=torch.int32)
        mask[layers] = 1
        mask = mask.to(keys.device)
    out = torch.empty([t, l, d], dtype=torch.float32, device=keys.device)
    _lib.check(_lib.load().sbg_walk_blend(keys.data_ptr(), index.data_ptr(), weight.data_ptr(), _lib.ptr(mask), _lib.ptr(hold), out.data_ptr(),
                                          k, t, l, d, _lib.stream_ptr(keys.device)), 'sbg_walk_blend')
    return out


# ---------------------------------------------------------------------------------------------------------------- pair_sqdiff

def sqdiff_splits(n, f):
    """chunks a row of F bytes is cut into on the device (the launch record's last entry)"""
    return -(-int(f) // CHUNK)


def pair_sqdiff(a, b):
    what = 'walk.pair_sqdiff'
    said = _describe(a=a, b=b)
    for t in (a, b):
        if t.dtype != torch.uint8 or t.ndim != 2 or not t.is_contiguous():
            raise RuntimeError(f'{what}: expects two dense uint8 [N, F] tensors; got {said}')
    if a.shape != b.shape or a.device != b.device:
        raise RuntimeError(f'{what}: a and b must have one shape and one device; got {said}')
    n, f = a.shape
    if n > MAX_N or not 1 <= f <= MAX_F:
        raise RuntimeError(f'{what}: [N, F] = [{n}, {f}] is not within N <= 2^24, 1 <= F <= 2^26; got {said}')
    if n == 0:
        return torch.empty([0], dtype=torch.int64, device=a.device)
    if a.device.type != 'cuda':
        diff = a.to(torch.int64) - b.to(torch.int64)
        return (diff * diff).sum(dim=1)
    lib = _lib.load()
    ws = _lib.workspace(lib.sbg_walk_sqdiff_workspace(n, f), a.device, 'sbg_walk_sqdiff_workspace')
    out = torch.empty([n], dtype=torch.int64, device=a.device)
    _lib.check(lib.sbg_walk_sqdiff(a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), n, f, _lib.stream_ptr(a.device)), 'sbg_walk_sqdiff')
    return out
