"""Arithmetic of the sliced Wasserstein distance on Laplacian-pyramid patches (csrc/swd.hip; Karras et al., "Progressive Growing of GANs",
ICLR 2018, section 5).  Every function takes its tables explicitly (centres, ``s``, ``t``, directions) and has ONE definition for both
devices: device tensors run the HIP kernels, CPU tensors run the same arithmetic, in the same order, with torch / numpy -- the results
are equal bit for bit, not close (DESIGN.md section 21 states the orders).

    pyr_down(x)                    [B, C, S, S] -> [B, C, S/2, S/2]: separable [1,4,6,4,1]/16, mirrored boundaries, even samples kept
    pyr_lap(fine, coarse)          fine - up(coarse); up = zero insertion + separable [1,4,6,4,1]/8, mirrored boundaries
    laplacian_pyramid(x, levels)   [lap_0, ..., lap_{levels-2}, gauss_{levels-1}]
    gather_descriptors(level, centres, out, row_offset)    7 x 7 x C patches -> rows of the [M, 49 C] descriptor matrix
    channel_moments(desc, C)       float64 [C, 2]: sum and sum of squares per channel, fixed order
    project(desc, s, t, dirs)      fp32 [D, M]: acc = fmaf(fmaf(x, s_c, t_c), dir, acc) over k, from 0
    sorted_l1(a, b)                float64 [D]: sum_m |a[d, m] - b[d, m]| of two fp32 [D, M] arrays, fixed order
"""
import numpy as np
import torch

from ... import _lib
from ._exact_common import chunked_sum_np, fma32

PATCH = 7
PP = PATCH * PATCH          # values per channel in a descriptor row
MOMENT_ROWS = 1024          # descriptor rows per chunk of channel_moments
L1_CHUNK = 16384            # elements per chunk of sorted_l1


def _dense_f32(t, what, ndim):
    _lib.require_dtype(t, torch.float32, what)
    if t.ndim != ndim or not t.is_contiguous():
        raise RuntimeError(f"{what}: expects a dense {ndim}-d tensor, got shape {tuple(t.shape)} with strides {t.stride()}")
    return t


def _square_pow2(x, what):
    _dense_f32(x, what, 4)
    s = x.shape[3]
    if x.shape[2] != s or s < 4 or s & (s - 1):
        raise RuntimeError(f"{what}: expects square images with a power-of-two side >= 4, got {tuple(x.shape)}")
    return s


# ------------------------------------------------------------------------------------------------ pyramid

def _mirror_index(n, lo, hi, device):
    """indices lo..hi-1 of an axis of n samples, mirrored without repeating the edge sample"""
    i = torch.arange(lo, hi, device=device).abs()
    return torch.where(i >= n, 2 * (n - 1) - i, i)


def _chain5(a, w0, w1, w2):
    """csrc/swd.hip `chain5`: taps (w0, w1, w1 + w2, w1, w0) as five power-of-two steps, each rounded once"""
    r = w0 * a[0] + w1 * a[1]
    r = r + w1 * a[2]
    r = r + w2 * a[2]
    r = r + w1 * a[3]
    return r + w0 * a[4]


def _filter_cpu(x, step, w0, w1, w2):
    """the separable 5-tap chain over a mirrored image, rows filtered along x first, then along y; every `step`-th sample kept"""
    s = x.shape[3]
    idx = _mirror_index(s, -2, s + 2, x.device)
    xp = x[:, :, idx][:, :, :, idx]                        # [B, C, S + 4, S + 4]
    h = _chain5([xp[:, :, :, j:j + s:step] for j in range(5)], w0, w1, w2)
    return _chain5([h[:, :, j:j + s:step] for j in range(5)], w0, w1, w2)


def pyr_down(x):
    s = _square_pow2(x, "swd.pyr_down")
    if x.device.type != "cuda":
        return _filter_cpu(x, 2, 0.0625, 0.25, 0.125).contiguous()
    y = torch.empty([x.shape[0], x.shape[1], s // 2, s // 2], dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().sbg_swd_pyr_down(x.data_ptr(), y.data_ptr(), x.shape[0], x.shape[1], s, _lib.stream_ptr(x.device)), "sbg_swd_pyr_down")
    return y


def pyr_lap(fine, coarse, inplace=False):
    """fine - up(coarse); `inplace` writes the result over `fine`"""
    s = _square_pow2(fine, "swd.pyr_lap")
    _dense_f32(coarse, "swd.pyr_lap (coarse)", 4)
    if tuple(coarse.shape) != (fine.shape[0], fine.shape[1], s // 2, s // 2) or coarse.device != fine.device:
        raise RuntimeError(f"swd.pyr_lap: coarse {tuple(coarse.shape)} on {coarse.device} does not belong to fine {tuple(fine.shape)} on {fine.device}")
    if fine.device.type != "cuda":
        z = torch.zeros_like(fine)
        z[:, :, ::2, ::2] = coarse
        lap = fine - _filter_cpu(z, 1, 0.125, 0.5, 0.25)
        return fine.copy_(lap) if inplace else lap
    out = fine if inplace else torch.empty_like(fine)
    _lib.check(_lib.load().sbg_swd_pyr_lap(fine.data_ptr(), coarse.data_ptr(), out.data_ptr(), fine.shape[0], fine.shape[1], s,
                                           _lib.stream_ptr(fine.device)), "sbg_swd_pyr_lap")
    return out


def laplacian_pyramid(x, num_levels):
    """x fp32 [B, C, S, S] -> `num_levels` tensors of sides S, S/2, ...: Laplacian levels, the last one Gaussian"""
    s = _square_pow2(x, "swd.laplacian_pyramid")
    if num_levels < 1 or (s >> (num_levels - 1)) < 4:
        raise RuntimeError(f"swd.laplacian_pyramid: {num_levels} levels do not fit a side of {s}")
    gauss = [x]
    for _ in range(num_levels - 1):
        gauss.append(pyr_down(gauss[-1]))
    return [pyr_lap(gauss[i], gauss[i + 1]) for i in range(num_levels - 1)] + [gauss[-1]]


# ------------------------------------------------------------------------------------------------ descriptors

def gather_descriptors(level, centres, out, row_offset=0):
    """level fp32 [B, C, S, S]; centres int32 [B, P, 2] = (y, x) in [3, S - 4]; rows row_offset + b P + p of out fp32 [M, 49 C] are
    written in (c, dy, dx) order.  A centre outside the range gives a row of NaN on both devices."""
    _dense_f32(level, "swd.gather_descriptors", 4)
    _dense_f32(out, "swd.gather_descriptors (out)", 2)
    _lib.require_dtype(centres, torch.int32, "swd.gather_descriptors (centres)")
    b, c, s = level.shape[0], level.shape[1], level.shape[3]
    if centres.ndim != 3 or centres.shape[0] != b or centres.shape[2] != 2 or not centres.is_contiguous() or centres.shape[1] < 1:
        raise RuntimeError(f"swd.gather_descriptors: centres must be dense int32 [{b}, P, 2], got {tuple(centres.shape)}")
    p = centres.shape[1]
    if level.shape[2] != s or s < PATCH or not 1 <= c <= 4 or out.shape[1] != c * PP:
        raise RuntimeError(f"swd.gather_descriptors: level {tuple(level.shape)} / out {tuple(out.shape)}: square images of 1..4 channels, 49 C columns")
    if row_offset < 0 or row_offset + b * p > out.shape[0] or centres.device != level.device or out.device != level.device:
        raise RuntimeError(f"swd.gather_descriptors: rows [{row_offset}, +{b * p}) of {out.shape[0]}, or tensors on different devices")
    if level.device.type != "cuda":
        cy, cx = centres[..., 0].long(), centres[..., 1].long()
        ok = (cy >= 3) & (cy <= s - 4) & (cx >= 3) & (cx <= s - 4)
        cy, cx = cy.clamp(3, s - 4), cx.clamp(3, s - 4)
        d = torch.arange(-3, 4)
        yy = (cy[:, :, None, None] + d[None, None, :, None]).expand(b, p, PATCH, PATCH)
        xx = (cx[:, :, None, None] + d[None, None, None, :]).expand(b, p, PATCH, PATCH)
        bb = torch.arange(b)[:, None, None, None].expand_as(yy)
        patches = level[bb, :, yy, xx]                      # [B, P, 7, 7, C]
        rows = patches.permute(0, 1, 4, 2, 3).reshape(b * p, c * PP)
        rows = torch.where(ok.reshape(-1, 1), rows, torch.full_like(rows, float("nan")))
        out[row_offset:row_offset + b * p] = rows
        return out
    _lib.check(_lib.load().sbg_swd_gather(level.data_ptr(), centres.data_ptr(), out.data_ptr(), b, c, s, p, row_offset, out.shape[0],
                                          _lib.stream_ptr(level.device)), "sbg_swd_gather")
    return out


# ------------------------------------------------------------------------------------------------ fixed-order float64 sums

def channel_moments(desc, channels):
    """desc fp32 [M, 49 C] -> float64 [C, 2] on desc's device: per channel, the sum and the sum of squares of its M * 49 values.  Chunks of
    1024 descriptor rows; in a chunk lane t of 256 adds the values t, t + 256, ... (row-major inside the channel's [rows, 49] slab), the
    lanes are added as in csrc/reduce.h; the chunk sums are added the same way.  An order fixed by M alone."""
    _dense_f32(desc, "swd.channel_moments", 2)
    m = desc.shape[0]
    if m < 1 or not 1 <= channels <= 4 or desc.shape[1] != channels * PP:
        raise RuntimeError(f"swd.channel_moments: desc {tuple(desc.shape)} is not [M >= 1, 49 * {channels}] with 1..4 channels")
    if desc.device.type != "cuda":
        v = desc.numpy().astype(np.float64).reshape(m, channels, PP).transpose(1, 0, 2).reshape(channels, m * PP)
        both = np.concatenate([v, v * v], axis=0)           # [2 C, M * 49]: sums first, then squares
        sums = chunked_sum_np(both, MOMENT_ROWS * PP)
        return torch.from_numpy(np.stack([sums[:channels], sums[channels:]], axis=1).copy())
    lib = _lib.load()
    ws = _lib.workspace(lib.sbg_swd_moments_workspace(m, channels), desc.device, "sbg_swd_moments_workspace")
    out = torch.empty([channels, 2], dtype=torch.float64, device=desc.device)
    _lib.check(lib.sbg_swd_moments(desc.data_ptr(), out.data_ptr(), ws.data_ptr(), m, channels, _lib.stream_ptr(desc.device)), "sbg_swd_moments")
    return out


def sorted_l1(a, b):
    """a, b fp32 [D, M] (each row sorted by the caller) -> float64 [D]: sum_m |a - b|, difference and sum in float64.  Chunks of 16384
    elements of a row; lane t of 256 adds the elements t, t + 256, ... of a chunk, the lanes as in csrc/reduce.h; the chunk sums the same way."""
    _dense_f32(a, "swd.sorted_l1", 2)
    _dense_f32(b, "swd.sorted_l1 (b)", 2)
    if a.shape != b.shape or a.device != b.device or a.shape[0] < 1 or a.shape[1] < 1:
        raise RuntimeError(f"swd.sorted_l1: {tuple(a.shape)} on {a.device} against {tuple(b.shape)} on {b.device}")
    d, m = a.shape
    if a.device.type != "cuda":
        diff = np.abs(a.numpy().astype(np.float64) - b.numpy().astype(np.float64))
        return torch.from_numpy(chunked_sum_np(diff, L1_CHUNK).copy())
    lib = _lib.load()
    ws = _lib.workspace(lib.sbg_swd_l1_workspace(d, m), a.device, "sbg_swd_l1_workspace")
    out = torch.empty([d], dtype=torch.float64, device=a.device)
    _lib.check(lib.sbg_swd_l1(a.data_ptr(), b.data_ptr(), out.data_ptr(), ws.data_ptr(), d, m, _lib.stream_ptr(a.device)), "sbg_swd_l1")
    return out


# ------------------------------------------------------------------------------------------------ projection

def project(desc, s, t, dirs):
    """desc fp32 [M, 49 C], s / t fp32 [C], dirs fp32 [49 C, D] (any row pitch: a column slice of a wider table is taken as it is) ->
    fp32 [D, M], direction-major:  p[d, m] = the chain over k = 0 .. 49 C - 1 from 0 of  acc = fmaf(fmaf(desc[m, k], s[k // 49], t[k // 49]), dirs[k, d], acc)."""
    _dense_f32(desc, "swd.project", 2)
    for name, v in (("s", s), ("t", t), ("dirs", dirs)):
        _lib.require_dtype(v, torch.float32, f"swd.project ({name})")
        if v.device != desc.device:
            raise RuntimeError(f"swd.project: {name} is on {v.device}, desc on {desc.device}")
    m, k = desc.shape
    c = k // PP
    if m < 1 or k != c * PP or not 1 <= c <= 4 or tuple(s.shape) != (c,) or tuple(t.shape) != (c,) or not s.is_contiguous() or not t.is_contiguous():
        raise RuntimeError(f"swd.project: desc {tuple(desc.shape)} with s {tuple(s.shape)} / t {tuple(t.shape)}: 49 C columns, 1..4 channels, dense [C] tables")
    if dirs.ndim != 2 or dirs.shape[0] != k or dirs.shape[1] < 1 or dirs.stride(1) != 1 or dirs.stride(0) < dirs.shape[1]:
        raise RuntimeError(f"swd.project: dirs must be [{k}, D] with unit column stride, got {tuple(dirs.shape)} strides {dirs.stride()}")
    d = dirs.shape[1]
    if desc.device.type != "cuda":
        x, sn, tn, dn = desc.numpy(), s.numpy(), t.numpy(), dirs.numpy()
        acc = np.zeros([d, m], dtype=np.float32)
        for kk in range(k):
            xh = fma32(x[:, kk], np.broadcast_to(sn[kk // PP], [m]), np.broadcast_to(tn[kk // PP], [m]))
            acc = fma32(np.broadcast_to(xh[None, :], [d, m]), np.broadcast_to(dn[kk, :, None], [d, m]), acc)
        return torch.from_numpy(acc)
    out = torch.empty([d, m], dtype=torch.float32, device=desc.device)
    _lib.check(_lib.load().sbg_swd_project(desc.data_ptr(), s.data_ptr(), t.data_ptr(), dirs.data_ptr(), out.data_ptr(), m, c, d, dirs.stride(0),
                                           _lib.stream_ptr(desc.device)), "sbg_swd_project")
    return out
