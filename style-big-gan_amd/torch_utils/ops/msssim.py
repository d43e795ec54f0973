"""Arithmetic of multi-scale structural similarity between pairs of images (csrc/msssim.hip; Wang, Simoncelli, Bovik, "Multi-scale structural
similarity for image quality assessment", Asilomar 2003; the diversity tool diversity.py).  Every function has ONE definition for both
devices: device tensors run the HIP kernels, CPU tensors run the same arithmetic, in the same order, with torch / numpy float64 -- the results
are equal bit for bit, not close (DESIGN.md section 23 states the value graph and the order of the sums).

    window()               float64 [11]: g[k] = exp(-(k - 5)^2 / 4.5) divided by the left-to-right sum
    levels(S)              (the level sides [S, S/2, ...], the level weights float64 [L]); L = min(5, log2 S - 3)
    down(x)                [N, C, S, S] -> fp32 [N, C, S/2, S/2]: ((a + b) + (c + d)) * 0.25f
    level_terms(x, y)      float64 [N, C, 2]: the means of cs and of ssim over the (S - 10)^2 map of x[i, c] against y[i, c]
    pair_scores(x, y)      (float64 [N] the score of every pair, float64 [N, C, L] its per-level terms: cs, and ssim on the coarsest level)

Images are byte values 0..255 as fp32 [N, C, S, S]; uint8 is accepted and is the same input.  A pair's result does not depend on the
batch it is in.
"""
import numpy as np
import torch

from ... import _lib
from ._exact_common import NT, block_sum_np, strided_sum_np

TAPS = 11
SIGMA2X2 = 4.5                  # 2 sigma^2, sigma = 1.5
WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)      # Wang et al. 2003, finest level first
C1 = (0.01 * 255) ** 2
C2 = (0.03 * 255) ** 2
TILE_H, TILE_W = 16, 32         # map entries of one workgroup of the level kernel
MIN_SIDE, MAX_SIDE = 16, 16384


def window():
    k = np.arange(TAPS, dtype=np.float64)
    g = np.exp(-(k - (TAPS // 2)) ** 2 / SIGMA2X2)
    total = np.float64(0.0)
    for v in g:
        total = total + v
    return torch.from_numpy(g / total)


def check_side(s, what, lo=MIN_SIDE):
    if s < lo or s > MAX_SIDE or s & (s - 1):
        raise ValueError(f"{what}: S={s} must be a power of two in [{lo}, {MAX_SIDE}]")
    return s


def levels(s):
    """-> (sides, weights): L = min(5, log2(S) - 3) levels, the smallest side >= 16; the first L published weights, for L < 5 divided by
    their float64 sum taken left to right"""
    check_side(s, "msssim.levels")
    num = min(len(WEIGHTS), s.bit_length() - 1 - 3)
    w = np.array(WEIGHTS[:num], dtype=np.float64)
    if num < len(WEIGHTS):
        total = np.float64(0.0)
        for v in w:
            total = total + v
        w = w / total
    return [s >> i for i in range(num)], w


def _images(x, what, lo=MIN_SIDE):
    """a dense uint8 or float32 [N, C, S, S] tensor, C 1 or 3, S a power of two -> S"""
    if not isinstance(x, torch.Tensor):
        raise RuntimeError(f"{what}: must be a torch tensor, got {type(x).__name__}")
    if x.dtype not in (torch.uint8, torch.float32):
        raise RuntimeError(f"{what}: expects uint8 or float32, got {x.dtype}")
    if x.ndim != 4 or x.shape[2] != x.shape[3] or not x.is_contiguous():
        raise ValueError(f"{what}: expects dense square images [N, C, S, S], got shape {tuple(x.shape)} with strides {x.stride()}")
    if x.shape[1] not in (1, 3):
        raise ValueError(f"{what}: expects 1 or 3 channels, got {tuple(x.shape)}")
    return check_side(x.shape[3], what, lo)


def _pair(x, y, what):
    s = _images(x, what)
    _images(y, f"{what} (y)")
    if x.shape != y.shape or x.device != y.device or x.dtype != y.dtype:
        raise ValueError(f"{what}: x is {x.dtype} {tuple(x.shape)} on {x.device}, y is {y.dtype} {tuple(y.shape)} on {y.device}")
    return s


def down(x):
    s = _images(x, "msssim.down", lo=2)
    n, c = x.shape[0], x.shape[1]
    if x.device.type != "cuda":
        v = x.to(torch.float32)
        a, b, cc, d = v[:, :, 0::2, 0::2], v[:, :, 0::2, 1::2], v[:, :, 1::2, 0::2], v[:, :, 1::2, 1::2]
        return (((a + b) + (cc + d)) * 0.25).contiguous()
    y = torch.empty([n, c, s // 2, s // 2], dtype=torch.float32, device=x.device)
    _lib.check(_lib.load().sbg_msssim_down(x.data_ptr(), int(x.dtype == torch.uint8), y.data_ptr(), n * c, s, _lib.stream_ptr(x.device)), "sbg_msssim_down")
    return y


# ------------------------------------------------------------------------------------------------ the CPU statement of csrc/msssim.hip

def _filter_valid(v, g):
    """float64 [Q, S, S] -> [Q, S - 10, S - 10]: the chain acc = 0; acc = acc + g[k] v[k] along x, then along y"""
    n = v.shape[2] - (TAPS - 1)
    acc = torch.zeros([v.shape[0], v.shape[1], n], dtype=torch.float64)
    for k in range(TAPS):
        acc = acc + g[k] * v[:, :, k:k + n]
    out = torch.zeros([v.shape[0], n, n], dtype=torch.float64)
    for k in range(TAPS):
        out = out + g[k] * acc[:, k:k + n, :]
    return out


def _map_mean_np(m):
    """m float64 [Q, n, n] -> [Q]: the order of csrc/msssim.hip.  Tiles of 16 x 32 entries in row-major order; in a tile lane t of 256 adds
    the entries (t // 32 + 8 i, t % 32), i = 0, 1, from 0 (an entry outside the map is 0), the lanes are added as in csrc/reduce.h; lane t
    then adds the tile sums t, t + 256, ..., the lanes again as in reduce.h; the sum is divided by n n."""
    q, n = m.shape[0], m.shape[1]
    ty, tx = -(-n // TILE_H), -(-n // TILE_W)
    rows = NT // TILE_W
    pad = np.zeros([q, ty * TILE_H, tx * TILE_W], dtype=np.float64)
    pad[:, :n, :n] = m
    t = pad.reshape(q, ty, TILE_H // rows, rows, tx, TILE_W).transpose(0, 1, 4, 2, 3, 5).reshape(q, ty * tx, TILE_H // rows, NT)
    lanes = np.zeros([q, ty * tx, NT], dtype=np.float64)
    for i in range(TILE_H // rows):
        lanes = lanes + t[:, :, i]
    return strided_sum_np(block_sum_np(lanes)) / np.float64(float(n) * float(n))


def _level_terms_cpu(x, y, g):
    n, c, s = x.shape[0], x.shape[1], x.shape[3]
    a, b = x.to(torch.float64).reshape(n * c, s, s), y.to(torch.float64).reshape(n * c, s, s)
    m1, m2 = _filter_valid(a, g), _filter_valid(b, g)
    m11, m22, m12 = m1 * m1, m2 * m2, m1 * m2
    s11 = _filter_valid(a * a, g) - m11
    s22 = _filter_valid(b * b, g) - m22
    s12 = _filter_valid(a * b, g) - m12
    cs = (2.0 * s12 + C2) / ((s11 + s22) + C2)
    lum = (2.0 * m12 + C1) / ((m11 + m22) + C1)
    ssim = lum * cs
    out = np.stack([_map_mean_np(cs.numpy()), _map_mean_np(ssim.numpy())], axis=1)
    return torch.from_numpy(out.reshape(n, c, 2).copy())


# ------------------------------------------------------------------------------------------------

def level_terms(x, y):
    """x, y uint8 or fp32 [N, C, S, S] -> float64 [N, C, 2] on their device: (mean of cs, mean of ssim) of every image-channel pair"""
    s = _pair(x, y, "msssim.level_terms")
    n, c = x.shape[0], x.shape[1]
    g = window()
    if x.device.type != "cuda":
        return _level_terms_cpu(x, y, g.tolist()) if n else torch.zeros([0, c, 2], dtype=torch.float64)
    out = torch.empty([n, c, 2], dtype=torch.float64, device=x.device)
    if n == 0:
        return out
    lib = _lib.load()
    g = g.to(x.device)
    need = lib.sbg_msssim_workspace(n * c, s)
    if need < 0:
        raise ValueError(f"msssim.level_terms: {n * c} image-channels of side {s} are more than the 2^24 tiles of one launch; cut the batch")
    ws = _lib.workspace(need, x.device, "sbg_msssim_workspace")
    _lib.check(lib.sbg_msssim_level(x.data_ptr(), y.data_ptr(), int(x.dtype == torch.uint8), g.data_ptr(), C1, C2, out.data_ptr(), ws.data_ptr(), n * c, s,
                                    _lib.stream_ptr(x.device)), "sbg_msssim_level")
    return out


def pair_scores(x, y):
    """x, y uint8 or fp32 [N, C, S, S] -> (scores float64 [N], terms float64 [N, C, L]), both on the host.  terms[:, :, i] is the mean of cs on
    level i < L - 1 and the mean of ssim on level L - 1; per channel the score is the product over the levels of max(term, 0) ** weight,
    left to right (a non-positive mean makes it 0), and the pair's score is the mean over the channels, left to right."""
    s = _pair(x, y, "msssim.pair_scores")
    sides, w = levels(s)
    num = len(sides)
    terms = np.zeros([x.shape[0], x.shape[1], num], dtype=np.float64)
    for i in range(num):
        t = level_terms(x, y).cpu().numpy()
        terms[:, :, i] = t[:, :, 1 if i == num - 1 else 0]
        if i + 1 < num:
            x, y = down(x), down(y)
    prod = np.ones(terms.shape[:2], dtype=np.float64)
    for i in range(num):
        prod = prod * np.power(np.maximum(terms[:, :, i], 0.0), w[i])
    total = np.zeros([terms.shape[0]], dtype=np.float64)
    for ch in range(terms.shape[1]):
        total = total + prod[:, ch]
    return torch.from_numpy(total / np.float64(terms.shape[1])), torch.from_numpy(terms)
