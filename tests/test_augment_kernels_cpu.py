"""CPU: the float64 references of tests/augment_exact_util.py against torch's own float64 ops, and the host-side selection rule of
the grid-sample backward (`sbg_grid_sample2d_bwd_overwrites` reads only `theta_host` and the sizes) against a float32 model of
the rule written from its description in DESIGN.md."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import style_big_gan_amd  # noqa: F401
from style_big_gan_amd import _lib

import augment_exact_util as R
from exact_util import qint

F64 = torch.float64


def test_bilinear_references_match_torch_float64():
    gen = torch.Generator().manual_seed(11)
    for (n, c, ih, iw, oh, ow) in [(2, 3, 9, 11, 7, 13), (1, 1, 12, 20, 5, 3), (3, 4, 16, 16, 16, 16)]:
        x = torch.randn(n, c, ih, iw, generator=gen, dtype=F64).requires_grad_(True)
        grid = (torch.rand(n, oh, ow, 2, generator=gen, dtype=F64) * 2.8 - 1.4).requires_grad_(True)     # a good part falls outside
        dy = torch.randn(n, c, oh, ow, generator=gen, dtype=F64)
        yt = F.grid_sample(x, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
        dxt, dgt = torch.autograd.grad(yt, [x, grid], dy)
        ix, iy = R.grid_positions(grid.detach(), ih, iw)
        assert (R.bilinear_sample(x.detach(), ix, iy) - yt.detach()).abs().max() < 1e-12
        assert (R.bilinear_adjoint(dy, ix, iy, ih, iw) - dxt).abs().max() < 1e-12
        assert (R.bilinear_dgrid(x.detach(), dy, ix, iy) - dgt).abs().max() < 1e-12 * max(ih, iw)


def test_affine_positions_match_torch_affine_grid():
    """to 1e-12 only: F.affine_grid's float64 base grid is linspace(-1, 1, W) * (W - 1) / W, which is not exact"""
    gen = torch.Generator().manual_seed(12)
    theta = torch.eye(2, 3, dtype=F64).repeat(3, 1, 1) + 0.3 * torch.randn(3, 2, 3, generator=gen, dtype=F64)
    for (ih, iw, oh, ow) in [(9, 11, 7, 13), (16, 16, 16, 16), (12, 20, 16, 8)]:
        g = R.affine_grid(theta, oh, ow)
        assert (g - F.affine_grid(theta, [3, 1, oh, ow], align_corners=False)).abs().max() < 1e-12
        ix, iy = R.affine_positions(theta, ih, iw, oh, ow)
        assert torch.equal(ix, ((g[..., 0] + 1) * iw - 1) / 2) and torch.equal(iy, ((g[..., 1] + 1) * ih - 1) / 2)
    # the explicit base grid is exact for power-of-two sizes: pixel centres of an identity map at equal sizes
    ix, iy = R.affine_positions(R.theta64("identity"), 16, 16, 16, 16)
    assert torch.equal(ix[0, 3], torch.arange(16, dtype=F64)) and torch.equal(iy[0, :, 5], torch.arange(16, dtype=F64))


def test_bilinear_adjoint_identity_exact():
    """<S x, dy> == <x, S^T dy> with integer data and dyadic positions: every term is exact in float64, so the two sides are equal"""
    gen = torch.Generator().manual_seed(13)
    for name in ("shear", "zoom_in8", "rot90", "shift"):
        for (ih, iw, oh, ow) in R.AFFINE_SIZES:
            x, dy = qint(gen, [2, 3, ih, iw], 4), qint(gen, [2, 3, oh, ow], 4)
            ix, iy = R.affine_positions(R.theta64(name, 2), ih, iw, oh, ow)
            lhs = (R.bilinear_sample(x, ix, iy) * dy).sum()
            rhs = (x * R.bilinear_adjoint(dy, ix, iy, ih, iw)).sum()
            assert float(lhs) == float(rhs) and float(lhs) != 0.0
    # positions without a valid neighbour contribute nothing (the documented contract for +-inf)
    x = qint(gen, [1, 2, 5, 6], 4)
    ix = torch.tensor([[[float("inf"), -float("inf"), 1e30, -1.5, 6.5, 2.0]]], dtype=F64)
    iy = torch.tensor([[[1.0, 1.0, 1.0, 1.0, 1.0, -float("inf")]]], dtype=F64)
    dy = qint(gen, [1, 2, 1, 6], 4)
    assert not R.bilinear_sample(x, ix, iy).any() and not R.bilinear_adjoint(dy, ix, iy, 5, 6).any()
    assert not R.bilinear_dgrid(x, dy, ix, iy).any()


def test_color_and_filter_references_match_torch_float64():
    gen = torch.Generator().manual_seed(14)
    x = torch.randn(3, 3, 5, 7, generator=gen, dtype=F64)
    m = torch.randn(3, 3, 4, generator=gen, dtype=F64)
    want = (m[:, :, :3] @ x.reshape(3, 3, -1) + m[:, :, 3:]).reshape(3, 3, 5, 7)
    assert (R.color_transform(x, m) - want).abs().max() < 1e-12
    n, c, h, w = 3, 2, 9, 8
    x = torch.randn(n, c, h, w, generator=gen, dtype=F64)
    for t in (1, 2, 7, 12):
        taps = torch.randn(n, t, generator=gen, dtype=F64)
        for pad in sorted({0, t // 2, t - 1}):
            for axis in (0, 1):
                if (w if axis == 0 else h) + 2 * pad - t + 1 < 1:
                    continue
                for flip in (False, True):
                    k = (taps.flip(1) if flip else taps).unsqueeze(1).repeat(1, c, 1).reshape(n * c, 1, -1)
                    wgt = k.unsqueeze(2) if axis == 0 else k.unsqueeze(3)
                    padding = (0, pad) if axis == 0 else (pad, 0)
                    want = F.conv2d(x.reshape(1, n * c, h, w), wgt, groups=n * c, padding=padding).reshape(n, c, *R.filter1d(x, taps, axis, pad, flip).shape[2:])
                    assert (R.filter1d(x, taps, axis, pad, flip) - want).abs().max() < 1e-12, (t, pad, axis, flip)


def _overwrites(theta, c, ih, iw, oh, ow, grid=False, dgrid=False):
    """the library's answer; the device addresses are dummies (the function reads only theta_host and the sizes)"""
    th = torch.as_tensor(theta, dtype=torch.float32).reshape(-1, 2, 3).contiguous()
    p = _lib.GridSampleParams()
    p.N, p.C, p.IH, p.IW, p.OH, p.OW = th.shape[0], c, ih, iw, oh, ow
    p.dx, p.theta_host = 64, th.data_ptr()
    if grid:
        p.grid = 64
    else:
        p.theta = 64
    if dgrid:
        p.dgrid = 64
    return int(_lib.load().sbg_grid_sample2d_bwd_overwrites(ctypes.byref(p)))


ZOOM8, ZOOM16, SHEAR, ZOOM_OUT = (R.THETAS[k] for k in ("zoom_in8", "zoom_in16", "shear", "zoom_out"))
BOX_TABLE = [      # (theta, (IH, IW, OH, OW), box); 0 = atomic scatter
    (ZOOM8, (16, 16, 16, 16), 20), (ZOOM16, (16, 16, 16, 16), 0),
    (ZOOM8, (12, 20, 16, 8), 24), (ZOOM8, (12, 12, 16, 16), 24),           # the boundary, GATHER_MAX_BOX
    (ZOOM8, (11, 12, 16, 16), 0), (ZOOM8, (9, 11, 8, 16), 0),
    (SHEAR, (9, 11, 8, 16), 8), (SHEAR, (16, 16, 16, 16), 6), (SHEAR, (12, 20, 16, 8), 6), (SHEAR, (11, 12, 16, 16), 6), (SHEAR, (12, 12, 16, 16), 6),
] + [(ZOOM_OUT, s, 4) for s in R.AFFINE_SIZES] + [(R.SINGULAR, s, 0) for s in R.AFFINE_SIZES]


def test_selection_rule_matches_model():
    for theta, size, box in BOX_TABLE:
        for c in (1, 3, 4):
            assert R.model_box([theta], c, *size) == box, (theta, size)
            assert _overwrites([theta], c, *size) == int(box > 0), (theta, size, c)
        assert R.model_box([theta], 5, *size) == 0 and _overwrites([theta], 5, *size) == 0            # GATHER_MAX_C
        assert R.model_box([theta], 3, *size, grid=True) == 0 and _overwrites([theta], 3, *size, grid=True) == 0
        assert R.model_box([theta], 3, *size, dgrid=True) == 0 and _overwrites([theta], 3, *size, dgrid=True) == 0
    for bad in (float("nan"), float("inf"), -float("inf")):
        for slot in range(6):
            th = torch.tensor(R.THETAS["identity"], dtype=torch.float32).reshape(6).clone()
            th[slot] = bad
            for size in R.AFFINE_SIZES:
                if slot in (2, 5):      # the box does not depend on the translation; such a sample lands nowhere under either kernel
                    assert _overwrites(th, 3, *size) == int(R.model_box(th.numpy(), 3, *size) > 0), (bad, slot, size)
                else:
                    assert R.model_box(th.numpy(), 3, *size) == 0 and _overwrites(th, 3, *size) == 0, (bad, slot, size)
    # batch-wide worst case: one sample beyond the limit sends the whole launch to the atomic kernel, wherever it stands
    ident = R.THETAS["identity"]
    for batch in ([ident, ident, ZOOM16], [ZOOM16, ident, ident], [ident, R.SINGULAR], [ZOOM8, ident, SHEAR]):
        want = R.model_box(batch, 3, 16, 16, 16, 16)
        assert _overwrites(batch, 3, 16, 16, 16, 16) == int(want > 0)
    assert R.model_box([ZOOM8, ident, SHEAR], 3, 16, 16, 16, 16) == 20 and R.model_box([ident, ident, ZOOM16], 3, 16, 16, 16, 16) == 0
    # no host copy, no dx, an empty batch: atomic
    p = _lib.GridSampleParams()
    p.N, p.C, p.IH, p.IW, p.OH, p.OW, p.theta, p.dx = 1, 3, 16, 16, 16, 16, 64, 64
    assert _lib.load().sbg_grid_sample2d_bwd_overwrites(ctypes.byref(p)) == 0
    assert _lib.load().sbg_grid_sample2d_bwd_overwrites(None) == 0


def test_selection_rule_matches_model_on_a_dyadic_sweep():
    """thetas on a 1/16 lattice at every size of the exact tests: the model and the library agree on every one, and both kernels
    are selected often enough for the comparison to mean something"""
    gen = torch.Generator().manual_seed(15)
    taken = [0, 0]
    for size in R.AFFINE_SIZES + [(9, 11, 7, 13), (70, 64, 44, 52)]:
        for _ in range(60):
            th = torch.randint(-24, 25, [2, 2, 3], generator=gen).to(torch.float32) / 16
            if int(torch.randint(0, 3, [1], generator=gen)) == 0:
                th = th / 8
            want = int(R.model_box(th.numpy(), 3, *size) > 0)
            assert _overwrites(th, 3, *size) == want, (th, size)
            taken[want] += 1
    assert min(taken) >= 40, taken
