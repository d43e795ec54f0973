"""The launch plan of the weight gradient (csrc/conv_wgrad.hip: wgrad_plan), pinned without a device through the one figure a host-only call
shows: the workspace size = pixel splits x taps x Ca x Cb x 4 bytes, 0 when the launch writes `out` itself, -1 for a refused block.  The
table reaches every branch of the plan -- thin (both strides), the rows kernel with 64 / 128-channel tiles at both strides, the 128 x 128
tile, the nine-tap groups, no split -- and every way a launch falls off a faster kernel: 32 x 32 channels, a row width that is no multiple
of 32, an operand of 2 GiB or more, a negative stride, a tap window too wide for the thin kernel.

The expected sizes in golden/wgrad_plan.json were recorded from the library as it was BEFORE the plan became one function, so they pin that
the refactor moved no launch to another kernel or split.  The empty batch (N = 0) has no recorded value: the old code divided by zero
there; a size of 0 is what the header's contract asks for."""
import ctypes
import json
import os

import pytest

from style_big_gan_amd import _lib

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wgrad_plan.json")

# name: (N, PH, PW, Ca, Cb, k, stride), then what departs from the dense k x k block
CASES = {
    "thin": ((2, 64, 64, 16, 16, 3, 1), {}),
    "thin_stride2": ((2, 32, 32, 32, 16, 3, 2), {}),
    "c32x32_not_thin": ((2, 64, 64, 32, 32, 3, 1), {}),
    "rows64": ((2, 32, 32, 64, 64, 3, 1), {}),
    "rows128": ((1, 64, 64, 128, 128, 3, 1), {}),
    "rows128_stride2": ((2, 32, 32, 256, 128, 3, 2), {}),
    "block8_padded_to_32_columns": ((4, 8, 32, 512, 512, 3, 1), {}),
    "pw_not_multiple_of_32": ((2, 32, 33, 72, 40, 3, 1), {}),
    "taps16": ((2, 24, 20, 72, 136, 4, 2), {}),
    "one_tap_big_tile": ((4, 64, 64, 136, 200, 1, 1), {}),
    "no_split": ((1, 4, 4, 64, 64, 3, 1), {}),
    "operand_2GiB_generic": ((64, 512, 512, 128, 128, 3, 1), {}),
    "rows64_shape_negative_as_h": ((2, 32, 32, 64, 64, 3, 1), dict(negate_as_h=True)),
    "thin_shape_window_too_wide": ((2, 64, 64, 16, 16, 3, 1), dict(taps=[(0, 0), (0, 3)])),
    "ca12_refused": ((2, 32, 32, 12, 64, 3, 1), {}),
}
EMPTY_BATCH = ((0, 8, 8, 64, 64, 3, 1), {})


def params(shape, negate_as_h=False, taps=None):
    """dense channel-minor bf16 operands, b = the a grid x stride + 2, taps (i - k//2, j - k//2) row-major; the pointers are never read"""
    N, PH, PW, Ca, Cb, k, stride = shape
    p = _lib.WgradParams()
    p.a, p.b, p.out, p.workspace = 0x1000, 0x2000, 0x3000, None
    p.dtype = _lib.SBG_BF16
    p.N, p.PH, p.PW, p.Ca = N, PH, PW, Ca
    p.BH, p.BW, p.Cb = PH * stride + 2, PW * stride + 2, Cb
    p.as_n, p.as_h, p.as_w = PH * PW * Ca, PW * Ca, Ca
    p.bs_n, p.bs_h, p.bs_w = p.BH * p.BW * Cb, p.BW * Cb, Cb
    if negate_as_h:
        p.as_h = -p.as_h
    p.stride = stride
    taps = taps or [(i - k // 2, j - k // 2) for i in range(k) for j in range(k)]
    p.ntaps = len(taps)
    for t, (dy, dx) in enumerate(taps):
        p.tap_dy[t], p.tap_dx[t] = dy, dx
    p.accumulate = 0
    return p


def workspace_bytes(case):
    """-> (bytes, the library's message when it refused)"""
    lib = _lib.load()
    n = lib.sbg_conv2d_wgrad_workspace(ctypes.byref(params(case[0], **case[1])))
    return n, (lib.sbg_last_error() or b"").decode() if n < 0 else ""


def test_golden_covers_the_table():
    golden = json.load(open(GOLDEN))
    assert sorted(golden) == sorted(CASES)
    assert all(golden[k]["shape"] == list(CASES[k][0]) for k in CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_workspace_matches_the_recorded_plan(name):
    want = json.load(open(GOLDEN))[name]
    n, msg = workspace_bytes(CASES[name])
    assert n == want["bytes"], (name, n, want)
    if want["bytes"] < 0:
        assert want["message"] in msg and "channel counts must be multiples of 8" in msg, msg


def test_empty_batch_needs_no_workspace():
    assert workspace_bytes(EMPTY_BATCH) == (0, "")
