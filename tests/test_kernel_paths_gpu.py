"""Every convolution, weight-gradient and FIR kernel path against an exact or a bounded CPU reference, with the launch log asserting which
kernel served each launch.

Exact mode (most cases).  Operands are small nonzero integers ({+-1, +-2}, FIR inputs up to +-40); filter taps, output scales, noise, gains,
clamps and the lrelu slope are dyadic; every bias is offset by half the finest grid step, so no pre-activation is exactly 0.  Every product is
then exact, and every fp32 partial sum is exact in any order as long as its magnitude stays below 2^(24 - d), d = fractional bits (each case
asserts that precondition before comparing).  So the kernel's result must equal the fp64 reference rounded ONCE to the output dtype
(round-to-nearest-even), bit for bit -- a dropped, duplicated or misplaced term moves some element by at least one unit at any size, and
the results above 256 (odd integers there are bf16 ties) check the conversion's rounding.

Bound mode (the real non-dyadic constants, fp32 operands): element-wise bounds derived in each case's docstring; each such case also checks
that its bound rejects the reference with one 8-channel input slab or one border row removed.

Weight gradients run in exact mode and, besides, with support probes: a dy that is zero except on one region (first / last row and column,
last partial tile, last image, last channel tail), so that region alone produces the result.
"""
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import style_big_gan_amd  # noqa: F401
from style_big_gan_amd import _lib
from style_big_gan_amd.torch_utils.ops import conv2d_gradfix as CG, conv_bias_act, upfirdn2d as UP

import conv_plan_cases as PLAN
from exact_util import U32, U_OUT, assert_exact, assert_range, expect_launch, qgrid, qint, qpow2, within_bound

pytestmark = pytest.mark.gpu

CL = torch.channels_last


def code(c):
    return lambda d: d[6] == c


def thin(tcs=None):
    return lambda d: d[6] // 1000000 == 6 and d[6] % 1000000 < 1000 and (tcs is None or d[6] == 6000000 + 16 * tcs)


HALO, GATHER1, GATHER4, UP2 = code(3128256), code(4128256), code(8128256), code(9064256)
K64_64x256, K64_128x128, K64_128x256 = code(1064256), code(1128128), code(1128256)


def wg_rows(bca):
    return lambda d: d[6] == 1000000 + 1000 * bca + 64


def wg_thin(ta, tb):
    return lambda d: d[6] == 3000000 + 10 * ta + tb


WG_BIG, WG_64 = code(128128), code(64064)
SPLIT = lambda d: d[5] > 1              # noqa: E731  (conv_wgrad: dims[5] = pixel splits)


def fir(variant, up=1, down=1):
    return lambda d: d[6] == 10000 * variant + 16 * up + down


# the codes the library logs; FIR_TILE / FIR_TILE_EDGE are retired (the tile matrix-core kernel is gone) and no launch logs them any more
FIR_SLIDE, FIR_TILE, FIR_SLIDE_EDGE, FIR_TILE_EDGE, FIR_FIXED44, FIR_GENERIC, FIR_VEC8, FIR_SCALAR = range(1, 9)


def _ref_conv(x, w, stride, pad, transpose, opad=0):
    if transpose:
        return F.conv_transpose2d(x, w, stride=stride, padding=pad, output_padding=opad)
    return F.conv2d(x, w, stride=stride, padding=pad)


# ---------------------------------------------------------------------------------------------------------------- conv leaves

# (id, dtype, n, cin, cout, h, w, k, stride, pad, transpose, forward leaf, data-gradient leaf, weight-gradient leaf)
BF, F16 = torch.bfloat16, torch.float16
CONV_CASES = [
    # thin: Cout 3, Cin 8 / 24, ragged tiles; a transposed thin conv runs all phases in one launch
    ("thin_cout3", BF, 2, 8, 3, 37, 45, 3, 1, 1, False, thin(1), thin(1), wg_thin(1, 1)),
    ("thin_cin24_cout40", BF, 1, 24, 40, 70, 45, 3, 1, 1, False, thin(4), thin(2), WG_64),
    ("thin_transposed_phases", F16, 2, 32, 16, 24, 40, 3, 2, 0, True, thin(1), thin(2), wg_thin(2, 1)),
    # up2 + border: Cout % 128 == 8, N > 1, phase grids 8 x 32 (+1 row / column); its data gradient is a 64-channel stride-2 conv
    ("up2_border", BF, 2, 64, 136, 8, 32, 3, 2, 0, True, UP2, K64_64x256, wg_rows(64)),
    # multi-phase gather: 4x4 kernel (16 taps, 4 per phase) and a 3x3 pad-1 transposed conv whose phases have different grids and tap counts
    ("gather_phases_4x4", BF, 2, 72, 136, 24, 20, 4, 2, 1, True, GATHER4, K64_128x128, WG_64),
    ("gather_phases_ragged", BF, 2, 64, 136, 24, 24, 3, 2, 1, True, GATHER4, K64_64x256, WG_64),
    # halo 16x16 (Cin % 64 == 56, Cout % 128 == 8, 288 tiles on 256 workgroups) and 8x32 (Cin % 64 == 8)
    ("halo16", BF, 16, 120, 136, 48, 48, 3, 1, 1, False, HALO, K64_128x128, WG_64),
    ("halo8x32", BF, 8, 72, 136, 64, 96, 3, 1, 1, False, HALO, K64_128x128, wg_rows(128)),
    # halo-eligible by tile count but not tile-aligned (48 x 40): falls through to the 128 x 256 kernel
    ("halo_unaligned_48x40", BF, 20, 64, 136, 48, 40, 3, 1, 1, False, K64_128x256, K64_64x256, WG_64),
    # single-phase gather: 2x2 stride 2 from an odd input, pad 0 / 1 (taps * ceil(Cin / 64) = 8); the data gradients are 4-phase gathers
    ("gather1_pad0", BF, 2, 128, 136, 257, 257, 2, 2, 0, False, GATHER1, GATHER4, WG_64),
    ("gather1_pad1", BF, 2, 128, 136, 257, 257, 2, 2, 1, False, GATHER1, GATHER4, WG_64),
    # k64 plain tiles: ragged Cout <= 64 with a K tail; 128 x 128 with ragged channels
    ("k64_64x256", BF, 2, 72, 40, 32, 33, 3, 1, 1, False, K64_64x256, K64_128x128, WG_64),
    ("k64_128x128", F16, 2, 136, 200, 12, 20, 3, 1, 1, False, K64_128x128, K64_128x128, WG_64),
    # weight-gradient big tile (1 tap) with pixel splits
    ("wgrad_big_tile", BF, 4, 136, 200, 64, 64, 1, 1, 0, False, K64_128x128, K64_128x128, lambda d: WG_BIG(d) and SPLIT(d)),
    # headline geometry (sg2ada @ 256^2, reduced batch): G's 128 ch @ 256^2 and 256 ch @ 128^2 layers (halo, rows kernel 128-wide, pixel splits),
    # 512 ch @ 64^2 (128 x 128) and @ 8^2 (split K, rows kernel on the zero-padded 8-pixel rows)
    ("G_128ch_256", BF, 4, 128, 128, 256, 256, 3, 1, 1, False, HALO, HALO, lambda d: wg_rows(128)(d) and SPLIT(d)),
    ("G_256ch_128", BF, 2, 256, 256, 128, 128, 3, 1, 1, False, HALO, HALO, wg_rows(128)),
    ("G_512ch_64", BF, 2, 512, 512, 64, 64, 3, 1, 1, False, K64_128x128, K64_128x128, wg_rows(128)),
    ("G_512ch_8", BF, 4, 512, 512, 8, 8, 3, 1, 1, False, K64_128x128, K64_128x128, wg_rows(128)),
    # G's up-sampling layer 256 ch @ 128^2 -> 128 ch @ 257^2 (up2 + border); its data gradient is D-like: stride 2 from 257^2, 128 x 256 tiles
    ("G_up_128_to_257", BF, 2, 256, 128, 128, 128, 3, 2, 0, True, UP2, K64_128x256, wg_rows(128)),
    # D's conv1: 128 -> 256 ch, stride 2 from the 257-wide low-pass output
    ("D_conv1_257_s2", BF, 2, 128, 256, 257, 257, 3, 2, 0, False, K64_128x256, UP2, wg_rows(128)),
]

SPLIT_K_SHAPES = {"G_512ch_8"}          # forward and data gradient split K (checked on the launch record below)


def _slab_bytes(d, n, ih, iw, cin):
    """the bytes a conv_k64 launch logs when it writes raw fp32 slabs (split K): output term 4 * P * Cout, never read back"""
    return 2.0 * n * ih * iw * cin + 2.0 * d[3] * d[1] * cin + 4.0 * d[0] * d[1]


def _conv_case(dev, case, seed=0, dy_region=None):
    _, dtype, n, cin, cout, h, w, k, stride, pad, transpose, fwd_leaf, dx_leaf, dw_leaf = case
    gen = torch.Generator().manual_seed(seed)
    x = qint(gen, (n, cin, h, w))
    wt = qint(gen, (cin, cout, k, k) if transpose else (cout, cin, k, k))
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    yr = _ref_conv(xr, wr, stride, pad, transpose)
    dy = qint(gen, tuple(yr.shape))
    if dy_region is not None:
        keep = torch.zeros_like(dy)
        keep[dy_region] = 1
        dy = dy * keep
    gxr, gwr = torch.autograd.grad(yr, [xr, wr], dy)
    oh, ow = yr.shape[2], yr.shape[3]
    assert_range("forward", cin * k * k * 4)
    assert_range("data gradient", cout * k * k * 4)
    assert_range("weight gradient", n * max(oh * ow, h * w) * 4)

    xg = x.to(dev, dtype).contiguous(memory_format=CL).requires_grad_(True)
    wg = wt.to(dev, dtype).requires_grad_(True)
    fn = CG.conv_transpose2d if transpose else CG.conv2d
    tag = case[0]
    with expect_launch("conv_igemm", fwd_leaf, tag + " forward") as log:
        y = fn(xg, wg, stride=stride, padding=pad)
    if tag in SPLIT_K_SHAPES:
        assert any(d[6] == 1128128 and r["bytes"] == _slab_bytes(d, n, h, w, cin) for r in log if r["kind"] == "conv_igemm" for d in [r["dims"]]), \
            f"{tag}: forward did not split K: {[(r['dims'], r['bytes']) for r in log]}"
    assert_exact(y, yr.detach(), tag + " forward")
    with expect_launch("conv_igemm", dx_leaf, tag + " data gradient"), expect_launch("conv_wgrad", dw_leaf, tag + " weight gradient"):
        gx, gw = torch.autograd.grad(y, [xg, wg], dy.to(dev, dtype).contiguous(memory_format=CL))
    assert_exact(gx, gxr, tag + " dx")
    assert_exact(gw, gwr, tag + " dw")


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_leaf_exact(dev, case):
    """forward, dx and dw of one convolution leaf, each bit for bit against the fp64 reference rounded once, each launch's kernel asserted"""
    _conv_case(dev, case)


PROBE_CASES = [c for c in CONV_CASES if c[0] in ("thin_cout3", "halo8x32", "gather1_pad1", "up2_border", "k64_64x256", "wgrad_big_tile")]


@pytest.mark.parametrize("case", PROBE_CASES, ids=[c[0] for c in PROBE_CASES])
def test_wgrad_support_probes(dev, case):
    """weight gradient from a dy that is zero except on one region -- first / last row, first / last column, the last partial 16 x 16 tile,
    the last image, the last output-channel tail (the channels past the last multiple of 16) -- so that region alone produces dw"""
    _, dtype, n, cin, cout, h, w, k, stride, pad, transpose, *_ = case
    yh = (h - 1) * stride - 2 * pad + k if transpose else (h + 2 * pad - k) // stride + 1
    yw = (w - 1) * stride - 2 * pad + k if transpose else (w + 2 * pad - k) // stride + 1
    ctail = (cout // 16) * 16 if cout % 16 else cout - 8
    regions = [(slice(None), slice(None), 0), (slice(None), slice(None), yh - 1), (slice(None), slice(None), slice(None), 0),
               (slice(None), slice(None), slice(None), yw - 1), (slice(None), slice(None), slice((yh - 1) // 16 * 16, None), slice((yw - 1) // 16 * 16, None)),
               (n - 1,), (slice(None), slice(ctail, None))]
    for i, reg in enumerate(regions):
        _conv_case(dev, case, seed=100 + i, dy_region=reg)


def test_wgrad_empty_batch(dev):
    """sbg_conv2d_wgrad over no images (N = 0): the sum is empty, so `out` becomes zeros -- or stays as it is when accumulating -- the status
    is 0 and no weight-gradient kernel is launched"""
    lib = _lib.load()
    a = torch.zeros(64, dtype=torch.bfloat16, device=dev)          # never read; the entry point wants non-null 16-byte aligned operands
    p = _lib.WgradParams()
    p.a, p.b, p.workspace, p.dtype = a.data_ptr(), a.data_ptr(), None, _lib.SBG_BF16
    p.N, p.PH, p.PW, p.Ca, p.BH, p.BW, p.Cb = 0, 4, 4, 8, 4, 4, 8
    p.as_n, p.as_h, p.as_w = p.bs_n, p.bs_h, p.bs_w = 128, 32, 8
    p.stride, p.ntaps = 1, 1
    _lib.prof_enable(True); _lib.prof_fetch()
    for accumulate in (0, 1):
        out = torch.ones(1, 8, 8, device=dev)
        p.out, p.accumulate = out.data_ptr(), accumulate
        assert lib.sbg_conv2d_wgrad_workspace(p) == 0
        assert lib.sbg_conv2d_wgrad(p, _lib.stream_ptr(dev)) == 0
        torch.cuda.synchronize()
        assert bool((out == float(accumulate)).all()), (accumulate, out)
    _lib.prof_enable(False)
    assert not [r for r in _lib.prof_fetch() if r["kind"] in ("conv_wgrad", "wgrad_reduce")]


# ---------------------------------------------------------------------------------------------------------------- accumulate / split K / generic

def _packed(wt, dtype, dev):
    """[Cout, Cin, kh, kw] -> the [taps, Cout, Cin] operand of conv2d_gradfix._igemm and its tap list for padding (kh // 2, kw // 2)"""
    cout, cin, kh, kw = wt.shape
    wp = wt.permute(2, 3, 0, 1).reshape(kh * kw, cout, cin).to(dev, dtype).contiguous()
    taps = [(i - kh // 2, j - kw // 2, i * kw + j) for i in range(kh) for j in range(kw)]
    return wp, taps


# (id, n, cin, cout, h, w, k, stride, leaf of the launch)
ACCUM_CASES = [
    ("thin", 2, 16, 24, 20, 36, 3, 1, thin(2)),
    ("k64_64x256", 2, 72, 40, 20, 36, 3, 1, K64_64x256),
    ("k64_128x128", 2, 64, 136, 20, 36, 3, 1, K64_128x128),
    ("halo", 2, 64, 136, 128, 128, 3, 1, HALO),
    ("gather1", 2, 128, 136, 257, 257, 2, 2, GATHER1),
    ("k64_128x256", 20, 64, 136, 48, 40, 3, 1, K64_128x256),
    ("split_k", 4, 512, 136, 8, 8, 3, 1, K64_128x128),
    ("split_k_cout513", 2, 512, 513, 8, 8, 3, 1, K64_128x128),
]


@pytest.mark.parametrize("case", ACCUM_CASES, ids=[c[0] for c in ACCUM_CASES])
def test_accumulate_into_prefilled_fp32(dev, case):
    """conv2d_gradfix._igemm(accumulate=True) on a prefilled fp32 output: y = prefill + conv, exact (prefill values are multiples of 1/2).
    The split-K cases (plain fp32 sum: conv_ksplit_reduce_kernel adds the slabs to y) must log their slab launch (fp32, not read back)."""
    tag, n, cin, cout, h, w, k, stride, leaf = case
    gen = torch.Generator().manual_seed(7)
    x, wt = qint(gen, (n, cin, h, w)), qint(gen, (cout, cin, k, k))
    pad = k // 2 if k == 3 else 0
    ref = F.conv2d(x, wt, stride=stride, padding=pad)
    pre = qgrid(gen, tuple(ref.shape), -64, 64, 0.5)
    assert_range(tag, cin * k * k * 4 + 64, 1)
    oh, ow = ref.shape[2], ref.shape[3]
    xg = x.to(dev, torch.bfloat16).contiguous(memory_format=CL)
    wp, taps = _packed(wt, torch.bfloat16, dev)
    if k == 2:
        taps = [(i - pad, j - pad, i * 2 + j) for i in range(2) for j in range(2)]
    y = pre.to(dev, torch.float32).contiguous(memory_format=CL)
    with expect_launch("conv_igemm", leaf, tag) as log:
        CG._igemm(xg, wp, y, taps, stride, oh, ow, accumulate=True)
    if tag.startswith("split_k"):
        assert any(r["dims"][6] == 1128128 and r["bytes"] == _slab_bytes(r["dims"], n, h, w, cin) for r in log if r["kind"] == "conv_igemm"), \
            f"{tag}: no split-K slab launch: {[(r['dims'], r['bytes']) for r in log]}"
    assert_exact(y, pre + ref, tag)


@pytest.mark.parametrize("name", PLAN.LAUNCHABLE)
def test_launch_log_equals_the_plan(dev, name):
    """every launchable row of the plan table (conv_plan_cases.py), as a real call on zero operands: the launch log must equal, record for
    record in dims, flops and bytes, both what sbg_conv2d_igemm_plan says the call will launch and golden/conv_plan.json, the launches of the
    library before the plan became one function.  (The host-only half is tests/test_conv_plan_cpu.py.)"""
    import json
    import os
    lib = _lib.load()
    c = PLAN.CASES[name]
    x, wp, y, bias, store = PLAN.tensors(c, dev)
    p = PLAN.block(c, x=x.data_ptr(), w=wp.data_ptr(), y=store.data_ptr(), workspace=None, bias=bias.data_ptr())
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan.json")))[name]
    assert lib.sbg_conv2d_igemm_workspace(p) == want["workspace"]
    log = PLAN.launch_log(lib, p, dev)                  # (sets p.workspace)
    planned = [dict(dims=r["dims"], flops=r["flops"], bytes=r["bytes"]) for r in PLAN.plan(lib, p)]
    assert log == planned, (name, log, planned)
    assert log == want["launches"], (name, log, want["launches"])
    assert not bool(torch.isnan(store.float()).any()) and not bool(store.any())         # zero operands: zeros, whatever the epilogue


def test_generic_kernels_beyond_2GiB(dev):
    """an input of >= 2 GiB does not fit a buffer descriptor: the launch falls to the generic register-staged kernels of conv_igemm.hip
    (64 x 256 for Cout <= 64, 128 x 128 otherwise).  Exact check on row bands: the first, the last, and the band whose input rows straddle
    byte 2^31 of x."""
    n, cin, h, w = 1, 64, 4096, 4160
    assert 2 * cin * h * w > 2 ** 31
    gen = torch.Generator().manual_seed(11)
    torch.manual_seed(11)
    xg = torch.randint(1, 3, (n, h, w, cin), dtype=torch.int8, device=dev)
    xg *= torch.randint(0, 2, (n, h, w, cin), dtype=torch.int8, device=dev) * 2 - 1
    xg = xg.to(torch.bfloat16).permute(0, 3, 1, 2)          # channel-minor view [N, Cin, H, W]
    assert xg.stride(1) == 1
    row_2g = 2 ** 31 // (2 * cin * w)
    bands = [(0, 4), (row_2g - 2, row_2g + 3), (h - 4, h)]
    for cout, leaf in ((64, code(64256)), (72, code(128128))):       # codes below 1000000: BC * 1000 + BP of conv_igemm_kernel
        wt = qint(gen, (cout, cin, 3, 3))
        wp, taps = _packed(wt, torch.bfloat16, dev)
        y = torch.empty([n, cout, h, w], dtype=torch.bfloat16, device=dev, memory_format=CL)
        with expect_launch("conv_igemm", leaf, f"generic Cout {cout}"):
            CG._igemm(xg, wp, y, taps, 1, h, w)
        for r0, r1 in bands:
            xb = torch.zeros(n, cin, r1 - r0 + 2, w, dtype=torch.float64)           # input rows r0 - 1 .. r1, zero outside the image
            lo, hi = max(r0 - 1, 0), min(r1 + 1, h)
            xb[:, :, lo - (r0 - 1):hi - (r0 - 1)] = xg[:, :, lo:hi].to("cpu", torch.float64)
            ref = F.conv2d(F.pad(xb, (1, 1, 0, 0)), wt)
            assert_exact(y[:, :, r0:r1], ref, f"generic Cout {cout} rows {r0}:{r1}")
        del y
    del xg
    torch.cuda.empty_cache()


# ---------------------------------------------------------------------------------------------------------------- fused epilogue

# (id, n, cin, cout, h, w, k, stride, pad, leaf)
EPI_CASES = [
    ("thin", 2, 16, 40, 21, 35, 3, 1, 1, thin(4)),
    ("k64_64x256", 2, 72, 48, 20, 36, 3, 1, 1, K64_64x256),
    ("k64_128x128", 2, 64, 136, 20, 36, 3, 1, 1, K64_128x128),
    ("halo8x32", 2, 64, 136, 128, 128, 3, 1, 1, HALO),
    ("halo16", 16, 64, 136, 48, 48, 3, 1, 1, HALO),
    ("k64_128x256", 20, 64, 136, 48, 40, 3, 1, 1, K64_128x256),
    ("gather1", 2, 128, 136, 257, 257, 2, 2, 0, GATHER1),
    ("split_k_epi", 4, 512, 136, 8, 8, 3, 1, 1, K64_128x128),
]
EPI_TAILS = [  # (act, gain, clamp, per-sample noise, oscale, bias)
    ("linear", 1.0, -1.0, None, False, False),
    ("lrelu", 2.0, 60.0, True, True, True),
    ("lrelu", 0.5, -1.0, False, True, True),
    ("relu", 2.0, 60.0, True, False, True),
]


@pytest.mark.parametrize("case", EPI_CASES, ids=[c[0] for c in EPI_CASES])
def test_fused_epilogue_exact(dev, case):
    """y = clamp(act(conv * oscale[n, co] + noise + bias[co]) * gain) on every single-phase leaf that takes an epilogue: oscale in {1/4 .. 2},
    noise per sample and constant (multiples of 1/4), bias = multiple of 1/4 + 1/8 (no pre-activation is 0), lrelu slope 1/4, gain 2 / 1/2,
    clamp 60 (never hit exactly: every output is an odd multiple of a power of two below 1) -- bit for bit."""
    tag, n, cin, cout, h, w, k, stride, pad, leaf = case
    gen = torch.Generator().manual_seed(3)
    x, wt = qint(gen, (n, cin, h, w)), qint(gen, (cout, cin, k, k))
    conv = F.conv2d(x, wt, stride=stride, padding=pad)
    oh, ow = conv.shape[2], conv.shape[3]
    assert_range(tag, cin * k * k * 4 * 2 + 64, 7)
    xg, wg = x.to(dev, torch.bfloat16).contiguous(memory_format=CL), wt.to(dev, torch.bfloat16)
    for act, gain, clamp, per_sample, use_osc, use_bias in EPI_TAILS:
        osc = qpow2(gen, (n, cout)) if use_osc else None
        noise = None if per_sample is None else qgrid(gen, (n if per_sample else 1, 1, oh, ow), -4, 4, 0.25)
        bias = qgrid(gen, (cout,), -8, 8, 0.25) + 0.125 if use_bias else None
        v = conv * (osc[:, :, None, None] if osc is not None else 1)
        v = v + (noise if noise is not None else 0) + (bias[None, :, None, None] if bias is not None else 0)
        if act == "lrelu":
            v = torch.where(v > 0, v, v * 0.25)
        elif act == "relu":
            v = torch.where(v > 0, v, torch.zeros_like(v))          # +0, as the kernel writes it
        v = v * gain
        if clamp >= 0:
            assert not bool((v.abs() == clamp).any())
            v = v.clamp(-clamp, clamp)
        epi = CG.Epilogue(oscale=None if osc is None else osc.to(dev, torch.float32), noise=None if noise is None else noise.to(dev, torch.float32),
                          bias=None if bias is None else bias.to(dev, torch.float32), act=act, alpha=0.25, gain=gain, clamp=clamp)
        what = f"{tag} {act} gain {gain} clamp {clamp} noise {per_sample}"
        with expect_launch("conv_igemm", leaf, what) as log:
            y = CG._conv_forward(xg, wg, (stride, stride), (pad, pad), epi=epi)
        if tag.startswith("split_k"):
            assert any(r["dims"][6] == 1128128 and r["bytes"] == _slab_bytes(r["dims"], n, h, w, cin) for r in log if r["kind"] == "conv_igemm"), what
        assert_exact(y, v, what)


def test_fused_epilogue_bound_real_constants(dev):
    """Bound mode on the halo kernel with the real constants: lrelu alpha 0.2, gain sqrt(2), clamp 256, random demodulation-like oscale,
    real noise and bias, random bf16 operands.

    Derivation.  Each product of two bf16 values is exact in fp32; a sum of K of them in any order errs by at most (K - 1) u S, u = 2^-24,
    S = (|x| (*) |w|) (the same convolution of absolute values, fp64).  Then  * oscale, + noise, + bias  (3 roundings, each <= u of a
    magnitude <= |oscale| S + |noise| + |bias| =: M), lrelu (one rounding, slopes <= max(1, alpha) = 1) and * gain (one rounding), and
    alpha and gain themselves reach the kernel rounded to fp32 (relative u each): the fp32 value v before the output cast satisfies
    |v - ref| <= g (K + 6) u M with g = gain max(1, alpha); clamp is 1-Lipschitz.  The cast
    rounds once: |got - v| <= u_out |v| <= u_out (|ref| + |v - ref|).  So
        |got - ref| <= u_out |ref| + (1 + u_out) g (K + 6) u M.
    Teeth: the bound must reject the reference computed without input channels 0..7, and without the last input row."""
    torch.manual_seed(21)
    n, cin, cout, r = 2, 64, 136, 128
    x = torch.randn(n, cin, r, r).to(torch.bfloat16).double()
    wt = (torch.randn(cout, cin, 3, 3) / 24).to(torch.bfloat16).double()
    osc = torch.rand(n, cout, dtype=torch.float64) + 0.5
    noise = torch.randn(n, 1, r, r, dtype=torch.float64) * 0.3
    bias = torch.randn(cout, dtype=torch.float64) * 0.5
    alpha, gain, clamp = 0.2, float(np.sqrt(2)), 256.0
    osc, noise, bias = osc.float().double(), noise.float().double(), bias.float().double()      # what the kernel reads (fp32)

    def tail(xx):
        v = F.conv2d(xx, wt, padding=1) * osc[:, :, None, None] + noise + bias[None, :, None, None]
        return (torch.where(v > 0, v, v * alpha) * gain).clamp(-clamp, clamp)
    ref = tail(x)
    S = F.conv2d(x.abs(), wt.abs(), padding=1)
    K = cin * 9
    M = osc[:, :, None, None] * S + noise.abs() + bias.abs()[None, :, None, None]
    u_out = U_OUT[torch.bfloat16]
    bound = u_out * ref.abs() + (1 + u_out) * gain * max(1.0, alpha) * (K + 6) * U32 * M
    epi = CG.Epilogue(oscale=osc.to(dev, torch.float32), noise=noise.to(dev, torch.float32), bias=bias.to(dev, torch.float32),
                      act="lrelu", alpha=alpha, gain=gain, clamp=clamp)
    with expect_launch("conv_igemm", HALO, "bound-mode halo epilogue"):
        y = CG._conv_forward(x.to(dev, torch.bfloat16).contiguous(memory_format=CL), wt.to(dev, torch.bfloat16), (1, 1), (1, 1), epi=epi)
    got = y.cpu()
    assert within_bound(got, ref, bound), f"bound exceeded by {float(((got.double() - ref).abs() - bound).max()):.3e}"
    x_slab = x.clone(); x_slab[:, :8] = 0
    x_row = x.clone(); x_row[:, :, -1] = 0
    for name, bad in (("8-channel slab", x_slab), ("last row", x_row)):
        assert not within_bound(tail(bad), ref, bound), f"the bound does not reject the reference without the {name}"


def test_fp32_split_path_bound(dev):
    """Bound mode, fp32 operands: each operand is split into hi / mid / lo bf16 parts and six of the nine part products are summed in fp32.
    Derivation: |a - a_hi| <= 2^-9 |a|, |a_mid| <= 2^-9 |a| (1 + 2^-8), |a_lo| <= 2^-17 |a|, and the residual a - hi - mid - lo is 0 for
    normal fp32 inputs; the three dropped products (mid lo, lo mid, lo lo) together are <= 2^-25 |a b|.  The 6K kept products are exact and
    their fp32 sum errs by <= (6K - 1) u sum|products| <= (6K - 1) u (1 + 2^-7) S.  With u = 2^-24:  |got - ref| <= (6K + 1) u S.
    Forward, dx and dw (dw through the same split) of a 3x3 convolution; teeth: the bound rejects the reference without channels 0..7."""
    torch.manual_seed(22)
    n, cin, cout, r = 2, 40, 72, 24
    x = torch.randn(n, cin, r, r, dtype=torch.float64).float().double()
    wt = (torch.randn(cout, cin, 3, 3, dtype=torch.float64) / 20).float().double()
    dy = torch.randn(n, cout, r, r, dtype=torch.float64).float().double()
    xr, wr = x.clone().requires_grad_(True), wt.clone().requires_grad_(True)
    yr = F.conv2d(xr, wr, padding=1)
    gxr, gwr = torch.autograd.grad(yr, [xr, wr], dy)
    xa, wa = x.abs().requires_grad_(True), wt.abs().requires_grad_(True)
    Sy = F.conv2d(xa, wa, padding=1)
    Sx, Sw = torch.autograd.grad(Sy, [xa, wa], dy.abs())
    xg = x.to(dev, torch.float32).contiguous(memory_format=CL).requires_grad_(True)
    wg = wt.to(dev, torch.float32).requires_grad_(True)
    with expect_launch("conv_igemm", K64_128x128, "fp32 forward (six folded passes, split K)"):
        y = CG.conv2d(xg, wg, padding=1)
    gx, gw = torch.autograd.grad(y, [xg, wg], dy.to(dev, torch.float32).contiguous(memory_format=CL))
    for what, got, ref, S, K in (("y", y, yr.detach(), Sy.detach(), cin * 9), ("dx", gx, gxr, Sx, cout * 9), ("dw", gw, gwr, Sw, n * r * r)):
        bound = (6 * K + 1) * U32 * S
        got = got.detach().cpu()
        assert within_bound(got, ref, bound), f"fp32 {what}: bound exceeded by {float(((got.double() - ref).abs() - bound).max()):.3e}"
    x_slab = x.clone(); x_slab[:, :8] = 0
    assert not within_bound(F.conv2d(x_slab, wt, padding=1), yr.detach(), (6 * cin * 9 + 1) * U32 * Sy.detach())


def test_conv_bias_act_backward_exact(dev):
    """conv2d_bias_act backward: the activation slope comes from the STORED output (the reference bias_act convention: lrelu slope from
    y > 0, zero where the output was clamped) -- dx, dw and db bit for bit.  lrelu slope 1/4, gain 2, clamp 40 (never hit exactly)."""
    gen = torch.Generator().manual_seed(5)
    n, cin, cout, r = 2, 64, 136, 128
    x, wt = qint(gen, (n, cin, r, r)), qint(gen, (cout, cin, 3, 3))
    b = qgrid(gen, (cout,), -8, 8, 1.0) + 0.5
    xr, wr, br = x.clone().requires_grad_(True), wt.clone().requires_grad_(True), b.clone().requires_grad_(True)
    pre = F.conv2d(xr, wr, padding=1) + br[None, :, None, None]
    yr = (torch.where(pre > 0, pre, pre * 0.25) * 2.0).clamp(-40.0, 40.0)
    dy = qint(gen, tuple(yr.shape))
    gxr, gwr, gbr = torch.autograd.grad(yr, [xr, wr, br], dy)
    assert_range("conv_bias_act dw", n * r * r * 8, 1)
    xg = x.to(dev, torch.bfloat16).contiguous(memory_format=CL).requires_grad_(True)
    wg, bg = wt.to(dev, torch.bfloat16).requires_grad_(True), b.to(dev, torch.bfloat16).requires_grad_(True)
    with expect_launch("conv_igemm", HALO, "conv_bias_act forward"):
        y = conv_bias_act.conv2d_bias_act(xg, wg, bg, padding=1, act="lrelu", alpha=0.25, gain=2.0, clamp=40.0)
    assert_exact(y, yr.detach(), "conv_bias_act y")
    with expect_launch("conv_igemm", K64_64x256, "conv_bias_act dx"), expect_launch("conv_wgrad", wg_rows(128), "conv_bias_act dw"):
        gx, gw, gb = torch.autograd.grad(y, [xg, wg, bg], dy.to(dev, torch.bfloat16).contiguous(memory_format=CL))
    assert_exact(gx, gxr, "conv_bias_act dx")
    assert_exact(gw, gwr, "conv_bias_act dw")
    assert_exact(gb, gbr, "conv_bias_act db")


# ---------------------------------------------------------------------------------------------------------------- FIR leaves

def _f44(dev=None):
    f = UP.setup_filter([1, 3, 3, 1])           # outer([1, 3, 3, 1]) / 64: dyadic taps
    return f if dev is None else f.to(dev)


def _fir_ref(x, f, up, down, pad, gain):
    """fp64 upfirdn2d: zero-stuff, pad, convolve with the flipped filter, keep every down-th sample"""
    n, c, h, w = x.shape
    px0, px1, py0, py1 = pad
    if up > 1:
        z = torch.zeros(n, c, h * up, w * up, dtype=x.dtype)
        z[:, :, ::up, ::up] = x
        x = z
    x = F.pad(x, [max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
    x = x[:, :, max(-py0, 0): x.shape[2] - max(-py1, 0), max(-px0, 0): x.shape[3] - max(-px1, 0)]
    f = f if f.ndim == 2 else torch.outer(f, f)            # a separable [taps] filter is its outer product
    fk = (f.double() * gain).flip([0, 1])[None, None].repeat(c, 1, 1, 1)
    y = F.conv2d(x, fk, groups=c)
    return y[:, :, ::down, ::down]


# (id, dtype, n, c, h, w, up, down, pad, gain, channel-minor, leaf, filter)
FIR_CASES = [
    ("slide", BF, 2, 64, 40, 64, 1, 1, (1, 2, 1, 2), 1.0, True, fir(FIR_SLIDE), "44"),
    ("tile_outH_lt_16", F16, 2, 128, 9, 70, 1, 1, (1, 2, 1, 2), 1.0, True, fir(FIR_SLIDE), "44"),
    ("slide_edge", BF, 1, 64, 30, 66, 1, 1, (2, 2, 2, 2), 1.0, True, fir(FIR_SLIDE_EDGE), "44"),
    ("tile_edge", BF, 2, 64, 12, 99, 1, 1, (1, 1, 1, 1), 1.0, True, fir(FIR_SLIDE_EDGE), "44"),
    ("fixed44_c24", BF, 2, 24, 19, 27, 1, 1, (1, 2, 1, 2), 1.0, True, fir(FIR_FIXED44), "44"),
    ("generic_3x3", BF, 2, 16, 19, 27, 1, 1, (1, 1, 1, 1), 1.0, True, fir(FIR_GENERIC), "33"),
    ("vec8_up2", BF, 2, 16, 13, 11, 2, 1, (2, 1, 2, 1), 4.0, True, fir(FIR_VEC8, 2, 1), "44"),
    ("vec8_down2", BF, 2, 16, 26, 22, 1, 2, (1, 1, 1, 1), 1.0, True, fir(FIR_VEC8, 1, 2), "44"),
    ("scalar_nchw", BF, 2, 5, 13, 11, 2, 1, (2, 1, 2, 1), 4.0, False, fir(FIR_SCALAR, 2, 1), "44"),
    ("separable_fp32", torch.float32, 2, 8, 15, 9, 2, 1, (2, 1, 2, 1), 4.0, False, None, "4"),
    # headline: D's low-pass in front of the stride-2 conv1 (pad 2 -> 257 wide: strips + edge)
    ("D_lowpass_257", BF, 2, 128, 256, 256, 1, 1, (2, 2, 2, 2), 1.0, True, fir(FIR_SLIDE_EDGE), "44"),
]


@pytest.mark.parametrize("case", FIR_CASES, ids=[c[0] for c in FIR_CASES])
def test_fir_leaf_exact(dev, case):
    """one FIR kernel, forward and the gradient (the transposed FIR), bit for bit: inputs are integers in [-40, 40] \\ {0}, the taps of
    [1, 3, 3, 1] (or [1, 2, 1]) are dyadic, so every fp32 sum is exact and only the output cast rounds (nearest-even: sums like 1357/64 need
    more than 8 bits)."""
    tag, dtype, n, c, h, w, up, down, pad, gain, cl, leaf, fname = case
    gen = torch.Generator().manual_seed(9)
    x = qint(gen, (n, c, h, w), hi=40)
    f = {"44": _f44, "33": lambda: UP.setup_filter([1, 2, 1]), "4": lambda: UP.setup_filter([1, 3, 3, 1], separable=True)}[fname]()
    ref = _fir_ref(x, f, up, down, pad, gain)
    assert_range(tag, 40 * 64 * gain * 4, 6)
    xg = x.to(dev, dtype)
    xg = xg.contiguous(memory_format=CL) if cl else xg.contiguous()
    ctx = expect_launch("upfirdn2d", leaf, tag) if leaf is not None else expect_launch("upfirdn2d", lambda d: d[1] == 1 and d[6] == 100 + 10 * up + down, tag)
    with ctx:
        y = UP.upfirdn2d(xg, f.to(dev), up=up, down=down, padding=list(pad), gain=gain)
    assert_exact(y, ref, tag + " forward")
    if up == 1 and down == 1:           # gradient: the transposed FIR (same kernel family at the same sizes)
        dy = qint(gen, tuple(ref.shape), hi=40)
        xr = x.clone().requires_grad_(True)
        gr = torch.autograd.grad(_fir_ref(xr, f, 1, 1, pad, gain), xr, dy)[0]
        xg.requires_grad_(True)
        y = UP.upfirdn2d(xg, f.to(dev), padding=list(pad), gain=gain)
        gx = torch.autograd.grad(y, xg, dy.to(dev, dtype).contiguous(memory_format=CL if cl else torch.contiguous_format))[0]
        assert_exact(gx, gr, tag + " gradient")


# (n, c, input rows, input columns): G's up-sampling layer (128 ch, 257^2 -> 256^2), and an image below 16 output rows (13 x 73 -> 12 x 72)
FIR_TAIL_SHAPES = [(2, 128, 257, 257), (2, 64, 13, 73)]


@pytest.mark.parametrize("post,shape", [(post, shape) for shape in FIR_TAIL_SHAPES for post in (False, True)],
                         ids=["False", "True", "False-13x73", "True-13x73"])
def test_fir_forward_tail_exact(dev, post, shape):
    """the sliding-window FIR with the forward tail (pad 1, gain 4):
    y = clamp(lrelu(fir(t) * oscale + noise + bias) * gain) (* post) bit for bit (the transposed conv feeding it is the conv case
    G_up_128_to_257).  Dyadic oscale / noise / bias / post, lrelu slope 1/4, gain 2, clamp 60 + 2^-11."""
    gen = torch.Generator().manual_seed(13)
    n, c, ih, iw = shape
    t = qint(gen, (n, c, ih, iw), hi=40)
    f = _f44()
    filt = _fir_ref(t, f, 1, 1, (1, 1, 1, 1), 4.0)
    osc, noise = qpow2(gen, (n, c)), qgrid(gen, (n, 1, ih - 1, iw - 1), -4, 4, 0.25)
    bias = qgrid(gen, (c,), -8, 8, 0.25) + 0.125
    v = filt * osc[:, :, None, None] + noise + bias[None, :, None, None]
    v = (torch.where(v > 0, v, v * 0.25) * 2.0)
    clamp = 60.0 + 2.0 ** -11           # every output is a multiple of 2^-9: the clamp is never met exactly
    assert not bool((v.abs() == clamp).any())
    v = v.clamp(-clamp, clamp)
    ps = qpow2(gen, (n, c)) if post else None
    if post:
        v = v * ps[:, :, None, None]
    assert_range("fir tail", (160 * 2 + 16) * 2, 10)
    tg = t.to(dev, BF).contiguous(memory_format=CL)
    with expect_launch("upfirdn2d", fir(FIR_SLIDE), "fir forward tail"), torch.no_grad():
        y = UP.fir_bias_act(tg, f.to(dev), [1, 1, 1, 1], 4.0, osc.to(dev, torch.float32), noise.to(dev, torch.float32),
                            bias.to(dev, torch.float32), act="lrelu", alpha=0.25, act_gain=2.0, clamp=clamp,
                            post_scale=None if ps is None else ps.to(dev, torch.float32))
    assert_exact(y, v, f"fir forward tail post={post} {ih}x{iw}")


def test_fir_backward_dact_tail_exact(dev):
    """the sliding-window FIR with the backward tail (D: bias_act(conv0) -> low-pass pad 2 -> 257^2): the transposed low-pass of dy times the
    slope of the bias_act at its saved output y, and the bias gradient from the per-workgroup partial rows -- bit for bit.  The saved y is an
    lrelu (slope 1/2, gain 2, clamp 40) output with values on both sides of 0 and on the clamp rails; dy is +-1, so every bias-gradient
    partial sum is a multiple of 2^-6 below 2^17."""
    gen = torch.Generator().manual_seed(17)
    n, c, r = 1, 128, 256
    f = _f44()
    pre = qgrid(gen, (n, c, r, r), -30, 30, 1.0) + 0.5
    y_saved = (torch.where(pre > 0, pre, pre * 0.5) * 2.0).clamp(-40.0, 40.0)
    slope = torch.where(y_saved > 0, 2.0, 1.0) * (y_saved.abs() < 40.0)
    dy = qint(gen, (n, c, r + 1, r + 1), hi=1)
    cfg = (1, 1, 1, 1, 2, 2, 2, 2, False, 1.0)
    # gradient of upfirdn2d(x, f, pad 2) w.r.t. x, in fp64 through autograd
    xr = torch.zeros(n, c, r, r, dtype=torch.float64, requires_grad=True)
    g = torch.autograd.grad(_fir_ref(xr, f, 1, 1, (2, 2, 2, 2), 1.0), xr, dy)[0]
    ref = g * slope
    assert_range("dact", 2 * n * r * r, 6)
    with expect_launch("upfirdn2d", fir(FIR_SLIDE), "fir dact tail"):
        res = UP.fir_transposed_dact(dy.to(dev, BF).contiguous(memory_format=CL), f.to(dev), cfg, (r, r),
                                     y_saved.to(dev, BF).contiguous(memory_format=CL), "lrelu", 0.5, 2.0, 40.0)
    assert res is not None, "the backward tail did not take the launch"
    got, db = res
    assert_exact(got, ref, "fir dact gradient")
    assert_exact(db, ref.sum([0, 2, 3]), "fir dact bias gradient")


def _fir_probe_block(dtype, c, rows, cols, taps, exact, cl, n=2, up=1, in_stride=None):
    """a dense parameter block as ops/upfirdn2d.py fills it (no pointers: the two probe functions read sizes, strides and flags only)"""
    p = _lib.UpfirdnParams()
    ih, iw = rows + taps - 1, cols + taps - 1
    p.dtype, p.upx, p.upy, p.downx, p.downy, p.gain = dtype, up, up, 1, 1, 1.0
    p.inSize[:], p.outSize[:] = [iw, ih, c, n], [cols, rows, c, n]
    p.inStride[:] = [c, iw * c, 1, ih * iw * c] if cl else [1, iw, ih * iw, c * ih * iw]
    p.outStride[:] = [c, cols * c, 1, rows * cols * c] if cl else [1, cols, rows * cols, c * rows * cols]
    for k, v in (in_stride or {}).items():
        p.inStride[k] = v
    p.filterSize[:], p.filterStride[:], p.filter_exact16 = [taps, taps], [1, taps], exact
    return p


def test_fir_matrix_core_rule_pinned():
    """sbg_upfirdn2d_tail_supported() and sbg_upfirdn2d_dact_rows() over a table of parameter blocks: the Python layer asks them which launches
    the matrix-core FIR takes and the entry point fails a tail launch the kernel then declines, so their answers are pinned.  The expected
    values are those of the library before the acceptance rule became one function (recorded from that build, not derived from this one)."""
    lib = _lib.load()
    F32, H16, B16 = _lib.SBG_F32, _lib.SBG_F16, _lib.SBG_BF16
    # every (dtype, C, output rows, output columns, taps, filter_exact16, channel-minor) of the product below that the forward tail accepts,
    # and the dact_partial rows of those the backward tail accepts (16 rows at least); everything else: 0 and -1
    tail_yes = {(d, 64, rows, 16, 4, 1, True) for d in (H16, B16) for rows in (8, 15, 16)}
    dact_rows = {(H16, 64, 16, 16, 4, 1, True): 2, (B16, 64, 16, 16, 4, 1, True): 2}
    count = 0
    for key in itertools.product((F32, H16, B16), (64, 24), (7, 8, 15, 16), (15, 16), (3, 4), (0, 1), (True, False)):
        p = _fir_probe_block(*key)
        assert bool(lib.sbg_upfirdn2d_tail_supported(p)) == (key in tail_yes), key
        assert lib.sbg_upfirdn2d_dact_rows(p) == dact_rows.get(key, -1), key
        count += 1
    assert count == 384
    # beyond the product: (block, tail_supported, dact_rows).  The probe for the forward tail does not look at stride signs or at the
    # operand's extent (the launch does); up-sampling is no FIR launch; segment geometry of two real shapes
    ok = dict(dtype=B16, c=64, rows=16, cols=16, taps=4, exact=1, cl=True)
    for extra, tail, rows in [(dict(in_stride={0: -64}), 1, -1), (dict(in_stride={3: 1 << 30}), 1, -1), (dict(up=2), 0, -1),
                              (dict(n=4, c=128, rows=256, cols=257), 1, 1152), (dict(n=1, rows=64, cols=40), 1, 8)]:
        p = _fir_probe_block(**{**ok, **extra})
        assert (lib.sbg_upfirdn2d_tail_supported(p), lib.sbg_upfirdn2d_dact_rows(p)) == (tail, rows), extra
