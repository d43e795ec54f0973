"""The 256 x 256 tile of conv_k64_kernel (two LDS stages, profiler code 1256256): stride-2 forward convolutions with Cout % 256 == 0 and at
least one 256 x 256 tile per CU, in exact mode (see exact_util) with the launch log asserting the kernel.

Operands are integers in {+-1, +-2}, so every partial sum is an integer below 2^24 and exact in fp32 in ANY order; the references are
therefore computed by the fp32 CPU convolution (several times faster than fp64 at these sizes) and widened to fp64 -- `assert_range` is the
precondition and `assert_exact` re-checks that the reference is an fp32 value.  One reference per shape is computed once and shared."""
import functools

import pytest
import torch
import torch.nn.functional as F

import style_big_gan_amd  # noqa: F401
from style_big_gan_amd.torch_utils.ops import conv2d_gradfix as CG

from exact_util import assert_exact, assert_range, expect_launch, qgrid, qint, qpow2

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF, F16 = torch.bfloat16, torch.float16


def code(c):
    return lambda d: d[6] == c


K64_256x256, K64_128x256 = code(1256256), code(1128256)

# first shape: N 4, Cin 72 (ragged last 64-channel slab), Cout 256, 257 x 257 input, 3 x 3, stride 2, pad 0 -> 128 x 128, P = 65536 = 256 tiles
N0, CIN0, COUT0, R0 = 4, 72, 256, 257


@functools.lru_cache(maxsize=None)
def _shape0():
    """(x, w, dy, y, dx, dw) of the first shape, fp64 CPU tensors (never modified)"""
    gen = torch.Generator().manual_seed(41)
    x, wt = qint(gen, (N0, CIN0, R0, R0)), qint(gen, (COUT0, CIN0, 3, 3))
    assert_range("forward", CIN0 * 9 * 4)
    assert_range("data gradient", COUT0 * 9 * 4)
    assert_range("weight gradient", N0 * R0 * R0 * 4)
    xr, wr = x.float().requires_grad_(True), wt.float().requires_grad_(True)
    yr = F.conv2d(xr, wr, stride=2)
    dy = qint(gen, tuple(yr.shape))
    gx, gw = torch.autograd.grad(yr, [xr, wr], dy.float())
    return x, wt, dy, yr.detach().double(), gx.double(), gw.double()


def _ref_forward(x, wt, stride=2):
    return F.conv2d(x.float(), wt.float(), stride=stride).double()


def test_stride2_cout256_exact(dev):
    """forward (1256256), dx and dw of the first shape, bit for bit"""
    x, wt, dy, yr, gxr, gwr = _shape0()
    xg = x.to(dev, BF).contiguous(memory_format=CL).requires_grad_(True)
    wg = wt.to(dev, BF).requires_grad_(True)
    with expect_launch("conv_igemm", K64_256x256, "forward"):
        y = CG.conv2d(xg, wg, stride=2, padding=0)
    assert_exact(y, yr, "forward")
    gx, gw = torch.autograd.grad(y, [xg, wg], dy.to(dev, BF).contiguous(memory_format=CL))
    assert_exact(gx, gxr, "dx")
    assert_exact(gw, gwr, "dw")


def test_f16(dev):
    """the f16 instantiation at the first shape"""
    x, wt, _, yr, _, _ = _shape0()
    with expect_launch("conv_igemm", K64_256x256, "f16 forward"), torch.no_grad():
        y = CG.conv2d(x.to(dev, F16).contiguous(memory_format=CL), wt.to(dev, F16), stride=2, padding=0)
    assert_exact(y, yr, "f16 forward")


def test_just_below_the_rule(dev):
    """the first two images of the first shape are 128 tiles of 256 x 256: fewer than the CUs, the launch keeps the 128 x 256 kernel"""
    x, wt, _, yr, _, _ = _shape0()
    with expect_launch("conv_igemm", K64_128x256, "N 2 forward"), torch.no_grad():
        y = CG.conv2d(x[:2].to(dev, BF).contiguous(memory_format=CL), wt.to(dev, BF), stride=2, padding=0)
    assert_exact(y, yr[:2], "N 2 forward")


def test_ragged_last_pixel_tile(dev):
    """257 x 259 input -> 128 x 129 output, P = 66048 = 258 tiles, the last one half empty; pixel tiles straddle rows and images"""
    gen = torch.Generator().manual_seed(42)
    x, wt = qint(gen, (N0, CIN0, 257, 259)), qint(gen, (COUT0, CIN0, 3, 3))
    assert_range("forward", CIN0 * 9 * 4)
    with expect_launch("conv_igemm", K64_256x256, "ragged forward"), torch.no_grad():
        y = CG.conv2d(x.to(dev, BF).contiguous(memory_format=CL), wt.to(dev, BF), stride=2, padding=0)
    assert tuple(y.shape) == (N0, COUT0, 128, 129)
    assert_exact(y, _ref_forward(x, wt), "ragged forward")


def test_cout512_two_channel_tiles(dev):
    """N 2, Cin 64, Cout 512 from 257^2: 128 pixel tiles x 2 channel tiles"""
    gen = torch.Generator().manual_seed(43)
    x, wt = qint(gen, (2, 64, 257, 257)), qint(gen, (512, 64, 3, 3))
    assert_range("forward", 64 * 9 * 4)
    with expect_launch("conv_igemm", K64_256x256, "Cout 512 forward"), torch.no_grad():
        y = CG.conv2d(x.to(dev, BF).contiguous(memory_format=CL), wt.to(dev, BF), stride=2, padding=0)
    assert_exact(y, _ref_forward(x, wt), "Cout 512 forward")


def test_transposed_layer_data_gradient(dev):
    """an up-sampling layer 256 -> 64 channels from 128^2 (N 4): its data gradient is the stride-2 convolution of the [N, 64, 257, 257] output
    gradient with Cout 256, P = 65536, and must take the 256 x 256 tile"""
    gen = torch.Generator().manual_seed(44)
    n, cin, cout, r = 4, 256, 64, 128
    x, wt = qint(gen, (n, cin, r, r)), qint(gen, (cin, cout, 3, 3))
    dy = qint(gen, (n, cout, 2 * r + 1, 2 * r + 1))
    assert_range("data gradient", cout * 9 * 4)
    gxr = _ref_forward(dy, wt)             # d/dx conv_transpose2d(x, w, stride 2) = conv2d(dy, w, stride 2), w read as [256, 64, 3, 3]
    xg = x.to(dev, BF).contiguous(memory_format=CL).requires_grad_(True)
    y = CG.conv_transpose2d(xg, wt.to(dev, BF), stride=2, padding=0)
    assert tuple(y.shape) == tuple(dy.shape)
    with expect_launch("conv_igemm", K64_256x256, "transposed layer dx"):
        gx, = torch.autograd.grad(y, [xg], dy.to(dev, BF).contiguous(memory_format=CL))
    assert_exact(gx, gxr, "transposed layer dx")


EPI_TAILS = [  # (act, gain, clamp, per-sample noise (None: no noise), oscale, bias)
    ("linear", 1.0, -1.0, None, False, False),
    ("lrelu", 2.0, 60.0, True, True, True),
    ("lrelu", 0.5, -1.0, False, True, True),
    ("relu", 2.0, 60.0, True, False, True),
]


def test_fused_epilogue_exact(dev):
    """y = clamp(act(conv * oscale[n, co] + noise + bias[co]) * gain) at the first shape: oscale in {1/4 .. 2}, noise per sample and constant
    (multiples of 1/4), bias = multiple of 1/4 + 1/8 (no pre-activation is 0), lrelu slope 1/4, gain 2 / 1/2, clamp 60 (never met exactly)"""
    x, wt, _, conv, _, _ = _shape0()
    n, cout, oh, ow = conv.shape
    gen = torch.Generator().manual_seed(45)
    assert_range("epilogue", CIN0 * 9 * 4 * 2 + 64, 7)
    xg, wg = x.to(dev, BF).contiguous(memory_format=CL), wt.to(dev, BF)
    for act, gain, clamp, per_sample, use_osc, use_bias in EPI_TAILS:
        osc = qpow2(gen, (n, cout)) if use_osc else None
        noise = None if per_sample is None else qgrid(gen, (n if per_sample else 1, 1, oh, ow), -4, 4, 0.25)
        bias = qgrid(gen, (cout,), -8, 8, 0.25) + 0.125 if use_bias else None
        v = conv * (osc[:, :, None, None] if osc is not None else 1)
        v = v + (noise if noise is not None else 0) + (bias[None, :, None, None] if bias is not None else 0)
        if act == "lrelu":
            v = torch.where(v > 0, v, v * 0.25)
        elif act == "relu":
            v = torch.where(v > 0, v, torch.zeros_like(v))
        v = v * gain
        if clamp >= 0:
            assert not bool((v.abs() == clamp).any())
            v = v.clamp(-clamp, clamp)
        epi = CG.Epilogue(oscale=None if osc is None else osc.to(dev, torch.float32), noise=None if noise is None else noise.to(dev, torch.float32),
                          bias=None if bias is None else bias.to(dev, torch.float32), act=act, alpha=0.25, gain=gain, clamp=clamp)
        what = f"{act} gain {gain} clamp {clamp} noise {per_sample}"
        with expect_launch("conv_igemm", K64_256x256, what):
            y = CG._conv_forward(xg, wg, (2, 2), (0, 0), epi=epi)
        assert_exact(y, v, what)


def test_accumulate_into_prefilled_fp32(dev):
    """conv2d_gradfix._igemm(accumulate=True) on a prefilled fp32 output at the first shape: y = prefill + conv (prefill: multiples of 1/2)"""
    x, wt, _, conv, _, _ = _shape0()
    n, cout, oh, ow = conv.shape
    gen = torch.Generator().manual_seed(46)
    pre = qgrid(gen, tuple(conv.shape), -64, 64, 0.5)
    assert_range("accumulate", CIN0 * 9 * 4 + 64, 1)
    xg = x.to(dev, BF).contiguous(memory_format=CL)
    wp = wt.permute(2, 3, 0, 1).reshape(9, cout, CIN0).to(dev, BF).contiguous()         # [taps, Cout, Cin]
    taps = [(i, j, i * 3 + j) for i in range(3) for j in range(3)]                      # pad 0
    y = pre.to(dev, torch.float32).contiguous(memory_format=CL)
    with expect_launch("conv_igemm", K64_256x256, "accumulate"):
        CG._igemm(xg, wp, y, taps, 2, oh, ow, accumulate=True)
    assert_exact(y, pre + conv, "accumulate")
