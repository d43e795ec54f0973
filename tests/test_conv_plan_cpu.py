"""The launch plan of the forward / data-gradient convolution (csrc/conv_igemm.hip: conv_plan), pinned without a device through
sbg_conv2d_igemm_plan -- the plan printed out: one record per kernel launch the call would make -- and sbg_conv2d_igemm_workspace, the bytes
of the K split the plan chose.  The table is tests/conv_plan_cases.py: every kernel family and tile, every way off a faster kernel, the
K split taken and refused.  Pointers are dummy values; nothing is launched.

The expected records (dims, flops, bytes) and workspace sizes in golden/conv_plan.json were recorded from the library as it was BEFORE the plan
became one function and the K-split policy moved into it out of conv2d_gradfix._igemm (golden/make_golden_conv_plan.py: the launch log of
real calls on the GPU; the rows marked "read" are written from that commit's code), so they pin that the refactor moved no launch to
another kernel, tile or split.  Grid, block and LDS bytes are not in that log: they are asserted against a restatement of that commit's
launch_* functions (`geometry_of`) -- arithmetic, not a measurement.  Without a device the library counts 256 compute units, the MI355X's."""
import ctypes
import json
import os

import pytest

from style_big_gan_amd import _lib

import conv_plan_cases as C

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan.json")
CUS = 256


def golden():
    return json.load(open(GOLDEN))


def test_golden_covers_the_table():
    g = golden()
    assert sorted(g) == sorted(C.CASES)
    assert all(g[k]["shape"] == json.loads(json.dumps(C.CASES[k])) for k in C.CASES)
    assert all(g[k]["source"] == ("parent" if C.CASES[k].get("launch", True) else "read") for k in C.CASES)
    codes = {r["dims"][6] for row in g.values() for r in row["launches"]}
    assert codes >= {6000016, 6000032, 6000064, 9064256, 8128256, 4128256, 3128256, 1064256, 1128128, 1128256, 1256256, 64256, 128128}, codes


@pytest.mark.parametrize("name", list(C.CASES))
def test_plan_matches_the_recorded_launches(name):
    want = golden()[name]
    lib = _lib.load()
    p = C.block(C.CASES[name])
    got = C.plan(lib, p)
    assert got is not None, lib.sbg_last_error()
    assert [dict(dims=r["dims"], flops=r["flops"], bytes=r["bytes"]) for r in got] == want["launches"], (name, got, want["launches"])
    assert lib.sbg_conv2d_igemm_workspace(ctypes.byref(p)) == want["workspace"], name
    p.workspace = None                                  # without a workspace the call does not split; the size query still says what it would use
    assert lib.sbg_conv2d_igemm_workspace(ctypes.byref(p)) == want["workspace"], name
    assert all(r["grid_y"] == 1 for r in C.plan(lib, p) if r["dims"][6] // 1000000 != 6), name


def geometry_of(r, nbytes_ws, c):
    """(grid_x, grid_y, block, lds) of a planned launch from its logged record, restated from the launch_* functions the plan replaced"""
    pix, cout, cin, ntaps, stride, rows, code = r["dims"]
    fam, bc, bp = code // 1000000, code % 1000000 // 1000, code % 1000
    ksplit = nbytes_ws // (pix * cout * 4) if nbytes_ws else 1
    if fam == 6:                                        # thin: 16 x 16 pixel tiles of the largest phase grid per image, one grid row per phase
        g = C.geometry(c)
        grids = [(ph[2], ph[3]) for ph in g["phases"]] if "phases" in g else [(g["oh"], g["ow"])]
        maxtaps = max(len(ph[4]) for ph in g["phases"]) if "phases" in g else ntaps
        kpad = -(-maxtaps * cin // 32) * 32
        tcs = (code - 6000000) // 16
        return (c["n"] * -(-max(h for h, _ in grids) // 16) * -(-max(w for _, w in grids) // 16), len(grids), 256, 16 * tcs * (((kpad >> 1) | 4) << 1) * 2)
    if fam == 9:                                        # up2: 8 x 32 tiles of the common phase grid x 64-channel tiles
        return (pix // 4 // 256 * -(-cout // 64), 1, 512, 2 * 38 * 1024 + 4 * 16384 + 1024)
    if fam in (4, 8):                                   # persistent gather: 256-pixel tiles of the largest phase for every phase x 128-channel tiles
        g = C.geometry(c)
        pmax = max(c["n"] * ph[2] * ph[3] for ph in g["phases"]) if fam == 8 else pix
        return (min(-(-pmax // 256) * (4 if fam == 8 else 1) * -(-cout // 128), CUS), 1, 768, 3 * (128 * 128 + 256 * 128))
    if fam == 3:                                        # halo: 8 x 32 tiles where the grid allows, else 16 x 16
        g = C.geometry(c)
        th, tw = (8, 32) if g["ow"] % 32 == 0 and g["oh"] % 8 == 0 else (16, 16)
        return (min(pix // (th * tw) * -(-cout // 128), CUS), 1, 768, 4 * 128 * 128 + 2 * -(-(th + 2) * (tw + 2) // 8) * 1024 + 2 * 3072)
    tiles = -(-pix // bp) * -(-cout // bc)
    if fam == 1:
        return (tiles, ksplit, 512, (2 if bc == 256 else 3) * (bc * 128 + bp * 128))
    return (tiles, 1, 256, 2 * (4 * bc * 16 + 4 * bp * 16))


@pytest.mark.parametrize("name", list(C.CASES))
def test_launch_geometry(name):
    want = golden()[name]
    lib = _lib.load()
    got = C.plan(lib, C.block(C.CASES[name]))
    assert len(got) == len(want["launches"])
    for i, (r, w) in enumerate(zip(got, want["launches"])):
        ws = want["workspace"] if i == 0 else 0
        # the sub-launches of a call (border rectangles, single phases) are single grids of their own: their geometry follows from the record alone
        c = C.CASES[name] if len(got) == 1 or (i == 0 and w["dims"][6] == 9064256) else None
        assert (r["grid_x"], r["grid_y"], r["block"], r["lds"]) == geometry_of(w, ws, c), (name, i, r)
        assert r["lds"] <= 160 * 1024 and r["block"] <= 1024
        if w["dims"][6] // 1000000 in (3, 4, 8):
            assert r["grid_x"] <= CUS
    if want["workspace"]:
        assert got[0]["grid_y"] == want["workspace"] // (want["launches"][0]["dims"][0] * want["launches"][0]["dims"][1] * 4) >= 2


def test_no_pixels_no_launch():
    lib = _lib.load()
    p = C.block(C.EMPTY)
    assert C.plan(lib, p) == [] and lib.sbg_conv2d_igemm_workspace(ctypes.byref(p)) == 0


def test_refused_block():
    lib = _lib.load()
    p = C.block(C.CASES["k64_64x256"])
    p.Cin = 12
    assert C.plan(lib, p) is None and lib.sbg_conv2d_igemm_workspace(ctypes.byref(p)) == -1
    assert b"Cin must be a multiple of 8" in lib.sbg_last_error()
