"""Independent restatement of the sliced Wasserstein distance of Karras et al. ("Progressive Growing of GANs", ICLR 2018, section 5) in the
form of their metrics/sliced_wasserstein.py: scipy's mirrored 5 x 5 convolution for the pyramid, `ogrid` patch indexing, `finalize_descriptors`,
a float64 projection, `np.sort` and the mean absolute difference.  Nothing here imports torch_utils/ops/swd.py.  The only departures from the
published file: patch centres and directions are passed in (it draws them on the fly), a descriptor row is in (c, dy, dx) order (its two
patch axes are swapped), the pyramid's dtype is the caller's (float64 for the exact tests) and the projection is float64."""
import numpy as np
import scipy.ndimage

GAUSS = np.float64([1, 4, 6, 4, 1]) / 16.0
GAUSS2D = GAUSS[:, None] * GAUSS[None, :]


def pyr_down(x):
    return scipy.ndimage.convolve(x, GAUSS2D[None, None].astype(x.dtype), mode='mirror')[:, :, ::2, ::2]


def pyr_up(x):
    s = x.shape
    res = np.zeros((s[0], s[1], s[2] * 2, s[3] * 2), x.dtype)
    res[:, :, ::2, ::2] = x
    return scipy.ndimage.convolve(res, (GAUSS2D[None, None] * 4.0).astype(x.dtype), mode='mirror')


def laplacian_pyramid(x, num_levels, dtype=np.float64):
    pyramid = [np.asarray(x, dtype=dtype).copy()]
    for _ in range(1, num_levels):
        pyramid.append(pyr_down(pyramid[-1]))
        pyramid[-2] -= pyr_up(pyramid[-1])
    return pyramid


def descriptors(level, centres, nhood_size=7):
    """level [B, C, S, S], centres int [B, P, 2] = (y, x) -> [B * P, C, 7, 7]"""
    b, c, hh, ww = level.shape
    p = centres.shape[1]
    n, h = b * p, nhood_size // 2
    nhood, chan, y, x = np.ogrid[0:n, 0:c, -h:h + 1, -h:h + 1]
    img = nhood // p
    y = y + centres[..., 0].reshape(n, 1, 1, 1)
    x = x + centres[..., 1].reshape(n, 1, 1, 1)
    idx = ((img * c + chan) * hh + y) * ww + x
    return level.flat[idx]


def finalize_descriptors(desc):
    desc = desc.copy()
    desc -= np.mean(desc, axis=(0, 2, 3), keepdims=True)
    desc /= np.std(desc, axis=(0, 2, 3), keepdims=True)
    return desc.reshape(desc.shape[0], -1)


def projections(a, dirs):
    """a [M, K] (finalised), dirs [K, D] -> float64 [M, D]"""
    return np.matmul(a.astype(np.float64), dirs.astype(np.float64))


def sliced_wasserstein(a, b, dirs, dir_repeats, dirs_per_repeat):
    """a, b [M, K] finalised descriptors; dirs [K, dir_repeats * dirs_per_repeat], columns of repeat r at r * dirs_per_repeat ..."""
    assert a.ndim == 2 and a.shape == b.shape and dirs.shape == (a.shape[1], dir_repeats * dirs_per_repeat)
    results = []
    for r in range(dir_repeats):
        d = dirs[:, r * dirs_per_repeat:(r + 1) * dirs_per_repeat]
        pa, pb = np.sort(projections(a, d), axis=0), np.sort(projections(b, d), axis=0)
        results.append(np.mean(np.abs(pa - pb)))
    return float(np.mean(results))


def unit_directions(rs, k, d):
    dirs = rs.randn(k, d)
    dirs /= np.sqrt(np.sum(np.square(dirs), axis=0, keepdims=True))
    return dirs.astype(np.float32)


def score(real_u8, fake_u8, centres_per_level, dirs, dir_repeats, dirs_per_repeat, min_res=16):
    """the whole metric of one pair of image sets [N, C, R, R] (byte values): {resolution: 1e3 * distance}; centres_per_level[i] is
    int [N, P, 2] for the level of side R >> i.  Also returns, per level, the finalised descriptors of both sets."""
    res = real_u8.shape[3]
    levels = int(np.log2(res // min_res)) + 1
    pr, pf = laplacian_pyramid(real_u8, levels, np.float32), laplacian_pyramid(fake_u8, levels, np.float32)
    out, desc = dict(), dict()
    for i in range(levels):
        a = finalize_descriptors(descriptors(pr[i], centres_per_level[i]))
        b = finalize_descriptors(descriptors(pf[i], centres_per_level[i]))
        out[res >> i] = 1e3 * sliced_wasserstein(a, b, dirs, dir_repeats, dirs_per_repeat)
        desc[res >> i] = (a, b)
    return out, desc
