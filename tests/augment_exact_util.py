"""Plain float64 CPU references of the ADA augmentation ops (csrc/augment_ops.hip), written from the op definitions, for
tests/test_augment_kernels_gpu.py; tests/test_augment_kernels_cpu.py checks them against torch's own float64 ops.

* positions: `grid_positions` (normalised grid -> input pixel units, align_corners=False) and `affine_positions`, whose base grid
  is (2 j + 1) / W - 1 evaluated in float64 (F.affine_grid's float64 base grid, linspace(-1, 1, W) * (W - 1) / W, is not exact);
* `bilinear_sample`, `bilinear_adjoint`, `bilinear_dgrid`: bilinear sampling with zero padding from explicit positions, its adjoint
  with respect to the input and its gradient with respect to the normalised grid;
* `color_transform`: the per-sample 3x4 colour transform; `filter1d`: the per-sample 1-D correlation with zero padding and flip;
* `model_box`: a float32 model of the backward kernel's selection rule as DESIGN.md states it (the pre-image parallelogram's
  bounding box, batch-wide worst case), independent of the library's code.

Contract of the op for positions without a valid neighbour -- between two pixels outside, far outside, or not finite: they
contribute nothing, so `y`, their share of `dx` and their `dgrid` are exact zeros.  For finite positions this is what zero padding
gives by itself; for +-inf it is the stated contract (the arithmetic would give inf - inf), so `_corners` moves every non-finite
position to one without neighbours first."""
import numpy as np
import torch

F64 = torch.float64
GATHER_MAX_BOX, GATHER_MAX_C = 24, 4


def frac_bits(t):
    """smallest d with every finite element of the fp64 tensor t an integer multiple of 2^-d"""
    t = t[torch.isfinite(t)]
    for d in range(0, 80):
        s = t * 2.0 ** d
        if bool((s == s.round()).all()):
            return d
    raise AssertionError("operand is not dyadic")


def grid_positions(grid, ih, iw):
    """grid [N, OH, OW, 2] (x, y in [-1, 1], align_corners=False) -> (ix, iy) [N, OH, OW] in input pixel units"""
    grid = grid.to(F64)
    return ((grid[..., 0] + 1) * iw - 1) / 2, ((grid[..., 1] + 1) * ih - 1) / 2


def affine_grid(theta, oh, ow):
    """theta [N, 2, 3] -> normalised grid [N, OH, OW, 2] = theta @ [bx, by, 1], bx = (2 j + 1) / OW - 1"""
    theta = theta.to(F64)
    bx = ((2 * torch.arange(ow, dtype=F64) + 1) / ow - 1).reshape(1, 1, ow)
    by = ((2 * torch.arange(oh, dtype=F64) + 1) / oh - 1).reshape(1, oh, 1)
    t = theta.reshape(-1, 6, 1, 1)
    gx = t[:, 0] * bx + t[:, 1] * by + t[:, 2]
    gy = t[:, 3] * bx + t[:, 4] * by + t[:, 5]
    return torch.stack([gx, gy], dim=3)


def affine_positions(theta, ih, iw, oh, ow):
    return grid_positions(affine_grid(theta, oh, ow), ih, iw)


def _corners(ix, iy, ih, iw):
    """the four neighbours of every position: [(flat index [N, P], weight [N, P], d weight / d ix, d weight / d iy)] with the
    weight and its derivatives zeroed where the neighbour lies outside the image (zero padding)"""
    n = ix.shape[0]
    ix, iy = ix.to(F64).reshape(n, -1), iy.to(F64).reshape(n, -1)
    lost = ~(torch.isfinite(ix) & torch.isfinite(iy))
    ix, iy = torch.where(lost, torch.full_like(ix, -4.0), ix), torch.where(lost, torch.full_like(iy, -4.0), iy)
    x0, y0 = ix.floor(), iy.floor()
    tx, ty = ix - x0, iy - y0
    out = []
    for dy_, wy, gy in ((0, 1 - ty, -torch.ones_like(ty)), (1, ty, torch.ones_like(ty))):
        for dx_, wx, gx in ((0, 1 - tx, -torch.ones_like(tx)), (1, tx, torch.ones_like(tx))):
            xx, yy = x0 + dx_, y0 + dy_
            ok = ((xx >= 0) & (xx <= iw - 1) & (yy >= 0) & (yy <= ih - 1)).to(F64)
            idx = (yy.clamp(0, ih - 1) * iw + xx.clamp(0, iw - 1)).to(torch.int64)
            out.append((idx, wx * wy * ok, gx * wy * ok, wx * gy * ok))
    return out


def bilinear_sample(x, ix, iy):
    """x [N, C, IH, IW], positions [N, OH, OW] -> y [N, C, OH, OW] (fp64)"""
    n, c, ih, iw = x.shape
    xf = x.to(F64).reshape(n, c, ih * iw)
    y = torch.zeros([n, c, ix[0].numel()], dtype=F64)
    for idx, w, _, _ in _corners(ix, iy, ih, iw):
        y += xf.gather(2, idx.unsqueeze(1).expand(n, c, -1)) * w.unsqueeze(1)
    return y.reshape(n, c, *ix.shape[1:])


def bilinear_adjoint(dy, ix, iy, ih, iw):
    """dy [N, C, OH, OW] -> dx [N, C, IH, IW]: <bilinear_sample(x), dy> == <x, bilinear_adjoint(dy)>"""
    n, c = dy.shape[:2]
    df = dy.to(F64).reshape(n, c, -1)
    dx = torch.zeros([n, c, ih * iw], dtype=F64)
    for idx, w, _, _ in _corners(ix, iy, ih, iw):
        dx.scatter_add_(2, idx.unsqueeze(1).expand(n, c, -1), df * w.unsqueeze(1))
    return dx.reshape(n, c, ih, iw)


def bilinear_dgrid(x, dy, ix, iy):
    """d <bilinear_sample(x), dy> / d grid, [N, OH, OW, 2]: d ix / d gx = IW / 2, d iy / d gy = IH / 2"""
    n, c, ih, iw = x.shape
    xf, df = x.to(F64).reshape(n, c, ih * iw), dy.to(F64).reshape(n, c, -1)
    gix, giy = torch.zeros([n, df.shape[2]], dtype=F64), torch.zeros([n, df.shape[2]], dtype=F64)
    for idx, _, wgx, wgy in _corners(ix, iy, ih, iw):
        v = (xf.gather(2, idx.unsqueeze(1).expand(n, c, -1)) * df)
        gix += (v * wgx.unsqueeze(1)).sum(1)
        giy += (v * wgy.unsqueeze(1)).sum(1)
    return torch.stack([gix * iw / 2, giy * ih / 2], dim=2).reshape(n, *ix.shape[1:], 2)


def color_transform(x, m):
    """x [N, 3, H, W], m [N, 3, 4]: y[n, c] = sum_c' m[n, c, c'] x[n, c'] + m[n, c, 3]"""
    n, _, h, w = x.shape
    m = m.to(F64)
    y = torch.zeros([n, 3, h * w], dtype=F64)
    xf = x.to(F64).reshape(n, 3, h * w)
    for c in range(3):
        for k in range(3):
            y[:, c] += m[:, c, k].reshape(n, 1) * xf[:, k]
        y[:, c] += m[:, c, 3].reshape(n, 1)
    return y.reshape(n, 3, h, w)


def filter1d(x, taps, axis, pad, flip):
    """x [N, C, H, W], taps [N, T]: y[n, c, oy, ox] = sum_t x[n, c, oy, ox + t - pad] * taps[n, T - 1 - t if flip else t] along
    W (axis 0) or along H (axis 1); zeros outside; output length L + 2 pad - T + 1"""
    n, c, h, w = x.shape
    t = taps.shape[1]
    x, taps = x.to(F64), taps.to(F64)
    if axis == 1:
        return filter1d(x.transpose(2, 3), taps, 0, pad, flip).transpose(2, 3).contiguous()
    xp = torch.zeros([n, c, h, w + 2 * pad], dtype=F64)
    xp[..., pad:pad + w] = x
    ow = w + 2 * pad - t + 1
    y = torch.zeros([n, c, h, ow], dtype=F64)
    for k in range(t):
        y += xp[..., k:k + ow] * taps[:, t - 1 - k if flip else k].reshape(n, 1, 1, 1)
    return y


def model_box(theta, c, ih, iw, oh, ow, grid=False, dgrid=False):
    """Candidate box of the deterministic (gather) backward, 0 = atomic scatter.  DESIGN.md: each input pixel walks the bounding
    box of its pre-image parallelogram.  Output pixel o samples at A o + b with A = [[t00 IW / OW, t01 IW / OH], [t10 IH / OW,
    t11 IH / OH]] (from the base grid and the pixel-unit mapping above), so the pre-image of a 2 x 2 footprint has half extents
    ex = (|A11| + |A01|) / |det A|, ey = (|A10| + |A00|) / |det A|; box = 2 ceil(worst + 0.01) + 2 over the batch, used up to 24,
    for up to 4 channels, finite regular theta, affine positions and no grid gradient.  float32, in the order written here."""
    f = np.float32
    if grid or dgrid or c > GATHER_MAX_C or len(theta) == 0:
        return 0
    worst = f(0)
    for t in np.asarray(theta, dtype=np.float32).reshape(-1, 6):
        with np.errstate(all="ignore"):
            a00, a01, a10, a11 = t[0] * f(iw) / f(ow), t[1] * f(iw) / f(oh), t[3] * f(ih) / f(ow), t[4] * f(ih) / f(oh)
            det = f(a00 * a11) - f(a01 * a10)
            if not abs(det) > 0:                    # singular or NaN: no pre-image
                return 0
            ex, ey = (abs(a11) + abs(a01)) / abs(det), (abs(a10) + abs(a00)) / abs(det)
        if not (ex <= GATHER_MAX_BOX and ey <= GATHER_MAX_BOX):     # (also NaN / inf) larger than any usable box
            return 0
        worst = max(worst, ex, ey)
    box = 2 * int(np.ceil(f(worst + f(0.01)))) + 2
    return box if box <= GATHER_MAX_BOX else 0


# the affine cases of the exact tests: dyadic theta, power-of-two output sizes (see test_augment_kernels_gpu.py)
THETAS = {
    "identity": [[1, 0, 0], [0, 1, 0]],
    "shift": [[1, 0, 1 / 16], [0, 1, -3 / 16]],
    "xflip": [[-1, 0, 0], [0, 1, 0]],
    "rot90": [[0, -1, 0], [1, 0, 0]],
    "shear": [[1, .5, .25], [-.25, 1, 0]],
    "zoom_out": [[2, 0, 0], [0, 2, 0]],
    "zoom_in8": [[1 / 8, 0, 0], [0, 1 / 8, 0]],
    "zoom_in16": [[1 / 16, 0, 0], [0, 1 / 16, 0]],
    "shift4": [[1, 0, 4], [0, 1, 4]],
}
SINGULAR = [[0, 0, .25], [0, 0, -.125]]
AFFINE_SIZES = [(16, 16, 16, 16), (12, 20, 16, 8), (11, 12, 16, 16), (9, 11, 8, 16), (12, 12, 16, 16)]      # (IH, IW, OH, OW)


def theta64(name_or_rows, n=1):
    rows = THETAS[name_or_rows] if isinstance(name_or_rows, str) else name_or_rows
    return torch.tensor(rows, dtype=F64).reshape(1, 2, 3).repeat(n, 1, 1)
