"""Record tests/golden/conv_plan.json: what sbg_conv2d_igemm launched for every row of tests/conv_plan_cases.py BEFORE the forward
convolution had one launch plan.  Run on a GPU from a checkout of that commit (the one before conv_plan appeared in csrc/conv_igemm.hip), with
this file and tests/conv_plan_cases.py copied into it:

    python tests/golden/make_golden_conv_plan.py [out.json]

Rows marked "source": "parent" drive that commit's conv2d_gradfix._igemm / _igemm_phases on zero operands with the launch log on and store the
conv_igemm records (dims, flops, bytes) as logged.  A row's `raw` fields are set on the block _igemm built, just before the launch.  Stored
besides: `ksplit_block`, the ksplit that commit's _igemm put in the block (its own policy: fewer than 128 tiles, 16 K-steps, ...), asserted to be
one its library's plan_ksplit keeps (>= 2 and <= K-steps / 4), and `workspace`, the bytes of the split then used: ksplit_block slabs when the
library takes the split -- a dense y and a plain fp32 sum, or no accumulate, Cout % 8 == 0 and a 16-byte aligned y (sbg_conv_k64_dispatch of
that commit, restated in `library_splits`: the launch log shows the slab launch's fp32 output bytes but not the split).

Rows marked "source": "read" are not launched.  Negative strides cannot be (no tensor has them), operands of 2 GiB need no allocation for
a plan query, and a phase offset that is not a multiple of 8 elements would make the multi-phase gather kernel store 16-byte vectors at
8-byte aligned addresses.  Their records are written from that commit's code: launch_conv of conv_igemm.hip and launch_gather_ld of
conv_k64.hip (`read_records`)."""
import json
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import style_big_gan_amd  # noqa: E402,F401
from style_big_gan_amd import _lib  # noqa: E402
from style_big_gan_amd.torch_utils.ops import conv2d_gradfix as CG  # noqa: E402

import conv_plan_cases as C  # noqa: E402


class Proxy:
    """the library, with sbg_conv2d_igemm applying the row's `raw` fields to the block and keeping what _igemm had put in it"""

    def __init__(self, lib, raw, dev):
        self.lib, self.raw, self.dev, self.seen, self.keep = lib, raw, dev, None, None

    def __getattr__(self, name):
        return getattr(self.lib, name)

    def sbg_conv2d_igemm(self, p, stream):
        self.seen = dict(ksplit=p.ksplit, workspace=bool(p.workspace))
        if "ksplit" in self.raw:
            p.ksplit = self.raw["ksplit"]
            if p.ksplit > 1 and not p.workspace:
                self.keep = torch.empty([max(self.lib.sbg_conv2d_igemm_workspace(p) // 4, 4)], dtype=torch.float32, device=self.dev)
                p.workspace = self.keep.data_ptr()
        p.accumulate = self.raw.get("accumulate", p.accumulate)
        return self.lib.sbg_conv2d_igemm(p, stream)


def record(c, dev):
    g = C.geometry(c)
    x, wp, y, bias, store = C.tensors(c, dev)
    proxy = Proxy(_lib.load(), c.get("raw", {}), dev)
    real_load = _lib.load
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    _lib.prof_fetch()
    CG._lib.load = lambda: proxy
    try:
        if c["kind"] == "conv":
            epi = CG.Epilogue(bias=bias, act="lrelu", alpha=0.25, gain=2.0) if c.get("epi") else None
            CG._igemm(x, wp, y, g["taps"], c["stride"], g["oh"], g["ow"], y_off=g["y_off"], y_step=g["y_step"], accumulate=c.get("acc", False), epi=epi)
        else:
            CG._igemm_phases(x, wp, y, g["phases"], c["stride"])
        torch.cuda.synchronize()
    finally:
        CG._lib.load = real_load
        _lib.prof_enable(False)
    log = [dict(dims=list(r["dims"]), flops=r["flops"], bytes=r["bytes"]) for r in _lib.prof_fetch() if r["kind"] == "conv_igemm"]
    return log, proxy.seen["ksplit"]


def library_splits(c, p):
    """sbg_conv_k64_dispatch's conditions for taking a split the block asks for"""
    dense = p.ys_w == p.Cout and p.ys_h == p.OW * p.Cout and p.ys_n == p.OH * p.OW * p.Cout
    simple = p.ydtype == _lib.SBG_F32 and not c.get("epi")
    epi_ok = not p.accumulate and p.Cout % 8 == 0 and p.y % 16 == 0
    return dense and (simple or epi_ok) and p.Cout > 64


def read_records(c, p):
    """the one launch of a row that is not launched: the generic kernel (operands a buffer descriptor cannot address) or the multi-phase gather"""
    ys = 4.0 if p.ydtype == _lib.SBG_F32 else 2.0
    if p.nphase > 1:
        grids = [p.N * p.ph_oh[i] * p.ph_ow[i] for i in range(p.nphase)]
        macs, outpix, code = float(sum(g * p.ph_ntaps[i] for i, g in enumerate(grids))), float(sum(grids)), 4128256 + 1000000 * p.nphase
    else:
        outpix = float(p.N * p.OH * p.OW)
        macs, code = outpix * p.ntaps, (64256 if p.Cout <= 64 else 128128)
    nbytes = 2.0 * p.N * p.IH * p.IW * p.Cin + 2.0 * p.ntaps * p.Cout * p.Cin + ys * outpix * p.Cout * (2 if p.accumulate else 1)
    return [dict(dims=[int(outpix), p.Cout, p.Cin, p.ntaps, p.stride, p.OH, code], flops=2.0 * macs * p.Cout * p.Cin, bytes=nbytes)]


def main(out_path):
    dev = torch.device("cuda:0")
    golden = {}
    for name, c in C.CASES.items():
        p = C.block(c)
        row = dict(shape=c, source="parent" if c.get("launch", True) else "read", ksplit_block=0, workspace=0)
        if row["source"] == "read":
            row["launches"] = read_records(c, p)
        else:
            row["launches"], k = record(c, dev)
            k = c.get("raw", {}).get("ksplit", k)
            row["ksplit_block"] = k
            if k > 1:
                ksteps = p.ntaps * -(-p.Cin // 64)
                assert "ksplit" in c.get("raw", {}) or 2 <= k <= ksteps // 4, (name, k, ksteps)
                used = min(k, ksteps // 4) if library_splits(c, p) else 1
                row["workspace"] = used * p.N * p.OH * p.OW * p.Cout * 4 if used > 1 else 0
        golden[name] = row
        print(name, row["ksplit_block"], row["workspace"], [r["dims"] for r in row["launches"]], flush=True)
    with open(out_path, "w") as f:
        json.dump(golden, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "conv_plan.json"))
