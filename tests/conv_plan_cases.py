"""The table behind tests/test_conv_plan_cpu.py, the plan test of tests/test_kernel_paths_gpu.py and golden/make_golden_conv_plan.py: calls of
sbg_conv2d_igemm described the way conv2d_gradfix describes them -- `conv` = one launch of _igemm over a k x k window, `tconv` = the phases of a
stride-2 transposed convolution as _igemm_phases passes them -- plus what departs from that (`raw`: fields set on the finished block).

It reaches every kernel family and tile of the plan (csrc/conv_igemm.hip: conv_plan), every way a call falls off a faster kernel, and the K split
taken and refused.  Shapes are the smallest that reach their branch; most are the geometry of CONV_CASES / ACCUM_CASES / EPI_CASES."""
from style_big_gan_amd import _lib

DT = {"bf16": _lib.SBG_BF16, "f16": _lib.SBG_F16, "f32": _lib.SBG_F32}
ES = {"bf16": 2, "f16": 2, "f32": 4}


def conv(n, cin, cout, ih, iw, k, stride, pad, **kw):
    return dict(kind="conv", n=n, cin=cin, cout=cout, ih=ih, iw=iw, k=k, stride=stride, pad=pad, **kw)


def tconv(n, cin, cout, ih, iw, k, pad, opad=0, **kw):
    return dict(kind="tconv", n=n, cin=cin, cout=cout, ih=ih, iw=iw, k=k, stride=2, pad=pad, opad=opad, **kw)


# options: xdt / ydt (default bf16), acc (accumulate), epi (a fused bias + lrelu + gain tail), y_step / y_off / yfull (_igemm's strided output into a
# larger y), y_misalign (bytes), raw (block fields overridden: ksplit, accumulate, negate_xs_h, ph_yoff_shift), launch=False (a plan query only)
SPLIT = (4, 512, 136, 8, 8, 3, 1, 1)           # 4 tiles of 128 x 128, 72 K-steps: split 18
CASES = {
    # ---- every family and tile
    "thin_tc1": conv(2, 8, 3, 37, 45, 3, 1, 1),
    "thin_tc2_accumulate": conv(2, 16, 24, 20, 36, 3, 1, 1, ydt="f32", acc=True),
    "thin_tc4": conv(1, 24, 40, 70, 45, 3, 1, 1),
    "thin_phased": tconv(2, 32, 16, 24, 40, 3, 0, xdt="f16", ydt="f16"),
    "up2_border": tconv(2, 64, 136, 8, 32, 3, 0),
    "up2_no_border": tconv(2, 64, 136, 7, 31, 3, 0, opad=1),            # every phase grid exactly 8 x 32
    "gather_phases_4x4": tconv(2, 72, 136, 24, 20, 4, 1),
    "gather_phases_ragged": tconv(2, 64, 136, 24, 24, 3, 1),
    "one_launch_per_phase": tconv(1, 64, 136, 4, 4, 3, 0),              # 8 tiles < kPhaseMinTiles
    "halo16": conv(16, 120, 136, 48, 48, 3, 1, 1),
    "halo8x32": conv(8, 72, 136, 64, 96, 3, 1, 1),
    "k64_64x256": conv(2, 72, 40, 32, 33, 3, 1, 1),
    "k64_128x128_f16": conv(2, 136, 200, 12, 20, 3, 1, 1, xdt="f16", ydt="f16"),
    "k64_128x256_halo_eligible_48x40": conv(20, 64, 136, 48, 40, 3, 1, 1),
    "k64_256x256": conv(4, 72, 256, 257, 257, 3, 2, 0),
    "gather1_8_ksteps": conv(2, 128, 136, 257, 257, 2, 2, 0),
    "gather1_2_ksteps": conv(4, 128, 136, 128, 128, 1, 1, 0),
    "one_kstep_not_gather": conv(4, 64, 136, 128, 128, 1, 1, 0),
    "generic_64x256_2GiB": conv(1, 64, 64, 4096, 4160, 3, 1, 1, launch=False),
    "generic_128x128_2GiB": conv(1, 64, 72, 4096, 4160, 3, 1, 1, launch=False),
    "generic_128x128_negative_xs_h": conv(2, 64, 136, 20, 36, 3, 1, 1, raw=dict(negate_xs_h=True), launch=False),
    "generic_64x256_negative_xs_h": conv(2, 72, 40, 32, 33, 3, 1, 1, raw=dict(negate_xs_h=True), launch=False),
    # ---- every way off a faster kernel
    "thin_shape_kpad_over_640": conv(2, 64, 16, 20, 20, 4, 1, 1),
    "c64x64_not_thin": conv(2, 64, 64, 20, 36, 3, 1, 1),
    "thin_shape_caller_ksplit": conv(2, 16, 16, 20, 36, 3, 1, 1, raw=dict(ksplit=4)),
    "up2_shape_hm4": tconv(8, 64, 136, 4, 32, 3, 0),
    # (not launched: the gather kernel's 16-byte stores do not test the phase offsets, which conv2d_gradfix always makes multiples of 8 elements)
    "up2_shape_yoff_not_multiple_of_8": tconv(2, 64, 136, 8, 32, 3, 0, raw=dict(ph_yoff_shift=4), launch=False),
    "up2_shape_accumulate": tconv(2, 64, 136, 8, 32, 3, 0, ydt="f32", raw=dict(accumulate=1)),
    "halo_shape_few_tiles": conv(2, 64, 136, 20, 36, 3, 1, 1),
    "stride2_cout256_fewer_tiles_than_cus": conv(2, 72, 256, 257, 257, 3, 2, 0),
    # ---- the K split
    "split_plain_f32": conv(*SPLIT, ydt="f32"),
    "split_plain_f32_accumulate": conv(*SPLIT, ydt="f32", acc=True),
    "split_epilogue_bf16": conv(*SPLIT, epi=True),
    "split_cout513_f32": conv(2, 512, 513, 8, 8, 3, 1, 1, ydt="f32"),
    "nosplit_cout513_bf16": conv(2, 512, 513, 8, 8, 3, 1, 1),
    "nosplit_y_step": conv(*SPLIT, ydt="f32", y_step=(2, 2), yfull=(16, 16)),
    "nosplit_y_off": conv(*SPLIT, ydt="f32", y_off=(1, 0), yfull=(9, 8)),
    "nosplit_epilogue_y_not_16B_aligned": conv(*SPLIT, epi=True, y_misalign=8),
    "nosplit_128_tiles": conv(2, 128, 136, 64, 64, 3, 1, 1),
    "nosplit_9_ksteps": conv(4, 64, 136, 8, 8, 3, 1, 1),
    "nosplit_cout64": conv(4, 512, 64, 8, 8, 3, 1, 1),
    "nosplit_caller_ksplit_1": conv(*SPLIT, ydt="f32", raw=dict(ksplit=1)),
    "split_caller_cap_2": conv(*SPLIT, ydt="f32", raw=dict(ksplit=2)),
}
EMPTY = conv(0, 64, 136, 8, 8, 3, 1, 1)
LAUNCHABLE = [k for k, c in CASES.items() if c.get("launch", True)]


def geometry(c):
    """-> dict(oh, ow: the launch grid (phased: the whole output), yh, yw: the y tensor, taps | phases, y_off, y_step) as conv2d_gradfix derives them"""
    k, s, p = c["k"], c["stride"], c["pad"]
    if c["kind"] == "conv":
        oh, ow = (c["ih"] + 2 * p - k) // s + 1, (c["iw"] + 2 * p - k) // s + 1
        yh, yw = c.get("yfull", (oh, ow))
        return dict(oh=oh, ow=ow, yh=yh, yw=yw, taps=[(i - p, j - p, i * k + j) for i in range(k) for j in range(k)],
                    y_off=tuple(c.get("y_off", (0, 0))), y_step=tuple(c.get("y_step", (1, 1))))
    oh, ow = (c["ih"] - 1) * s - 2 * p + k + c["opad"], (c["iw"] - 1) * s - 2 * p + k + c["opad"]
    phases = []
    for a in range(s):
        for b in range(s):
            taps = [((a + p - i) // s, (b + p - j) // s, i * k + j) for i in range(k) if (a + p - i) % s == 0 for j in range(k) if (b + p - j) % s == 0]
            phases.append((a, b, (oh - a + s - 1) // s, (ow - b + s - 1) // s, taps))
    return dict(oh=oh, ow=ow, yh=oh, yw=ow, phases=phases, y_off=(0, 0), y_step=(s, s))


def block(c, x=0x1000, w=0x2000, y=0x3000, workspace=0x4000, bias=0x5000):
    """the parameter block of the case over dense channel-minor operands at the given addresses (dummy ones by default: a plan query reads none)"""
    g = geometry(c)
    n, cin, cout, ih, iw = c["n"], c["cin"], c["cout"], c["ih"], c["iw"]
    ydt = c.get("ydt", "bf16")
    p = _lib.ConvParams()
    ys = (g["yh"] * g["yw"] * cout, g["yw"] * cout, cout)               # y [n, yh, yw, cout]
    p.x, p.w, p.workspace = x, w, workspace
    p.y = y + c.get("y_misalign", 0) + (g["y_off"][0] * ys[1] + g["y_off"][1] * ys[2]) * ES[ydt]
    p.xdtype, p.ydtype = DT[c.get("xdt", "bf16")], DT[ydt]
    p.N, p.IH, p.IW, p.Cin, p.Cout = n, ih, iw, cin, cout
    p.xs_n, p.xs_h, p.xs_w = ih * iw * cin, iw * cin, cin
    p.ys_n, p.ys_h, p.ys_w = ys[0], ys[1] * g["y_step"][0], ys[2] * g["y_step"][1]
    p.ws_slab, p.ws_co = cout * cin, cin
    p.act, p.alpha, p.gain, p.clamp = 1, 0.0, 1.0, -1.0
    p.accumulate = int(c.get("acc", False))
    if c["kind"] == "conv":
        p.OH, p.OW, p.stride, taps = g["oh"], g["ow"], c["stride"], g["taps"]
    else:
        p.OH, p.OW, p.stride = max(ph[2] for ph in g["phases"]), max(ph[3] for ph in g["phases"]), 1
        for i, (a, b, goh, gow, t) in enumerate(g["phases"]):
            p.ph_ntaps[i], p.ph_oh[i], p.ph_ow[i], p.ph_yoff[i] = len(t), goh, gow, a * ys[1] + b * ys[2]
        p.nphase, taps = len(g["phases"]), [t for ph in g["phases"] for t in ph[4]]
    p.ntaps = len(taps)
    for i, (dy, dx, slab) in enumerate(taps):
        p.tap_dy[i], p.tap_dx[i], p.tap_slab[i] = dy, dx, slab
    if c.get("epi"):
        p.bias, p.act, p.alpha, p.gain = bias, 3, 0.25, 2.0
    raw = c.get("raw", {})
    p.ksplit = raw.get("ksplit", 0)
    p.accumulate = raw.get("accumulate", p.accumulate)
    if raw.get("negate_xs_h"):
        p.xs_h = -p.xs_h
    for i in range(p.nphase):
        p.ph_yoff[i] += raw.get("ph_yoff_shift", 0)
    return p


def tensors(c, dev):
    """zero operands of the case on `dev`: x [n, cin, ih, iw] and y [n, cout, yh, yw] channel-minor (y moved by y_misalign bytes), wp [slabs, cout, cin],
    the fp32 bias of the `epi` cases, and y's 16-byte aligned storage"""
    import torch
    g = geometry(c)
    td = {"bf16": torch.bfloat16, "f16": torch.float16, "f32": torch.float32}
    ydt = c.get("ydt", "bf16")
    x = torch.zeros([c["n"], c["cin"], c["ih"], c["iw"]], dtype=td[c.get("xdt", "bf16")], device=dev).contiguous(memory_format=torch.channels_last)
    wp = torch.zeros([c["k"] * c["k"], c["cout"], c["cin"]], dtype=x.dtype, device=dev)
    numel, shift = c["n"] * g["yh"] * g["yw"] * c["cout"], c.get("y_misalign", 0) // ES[ydt]
    store = torch.zeros([numel + 16], dtype=td[ydt], device=dev)
    y = store[shift:shift + numel].view(c["n"], g["yh"], g["yw"], c["cout"]).permute(0, 3, 1, 2)
    return x, wp, y, torch.zeros([c["cout"]], dtype=torch.float32, device=dev), store


def launch_log(lib, p, dev):
    """launches the block (with the workspace the library asks for) and returns the conv_igemm records of the launch log"""
    import torch
    nbytes = lib.sbg_conv2d_igemm_workspace(p)
    assert nbytes >= 0, lib.sbg_last_error()
    ws = torch.empty([max(nbytes // 4, 4)], dtype=torch.float32, device=dev)
    p.workspace = ws.data_ptr()
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    _lib.prof_fetch()
    try:
        _lib.check(lib.sbg_conv2d_igemm(p, _lib.stream_ptr(dev)), "sbg_conv2d_igemm")
        torch.cuda.synchronize()
    finally:
        _lib.prof_enable(False)
    return [dict(dims=list(r["dims"]), flops=r["flops"], bytes=r["bytes"]) for r in _lib.prof_fetch() if r["kind"] == "conv_igemm"]


def plan(lib, p):
    """sbg_conv2d_igemm_plan -> [dict(dims, flops, bytes, grid_x, grid_y, block, lds)], or None for a refused block"""
    out = (_lib.ConvLaunchInfo * 8)()
    n = lib.sbg_conv2d_igemm_plan(p, out, 8)
    if n < 0:
        return None
    assert n <= 5
    return [dict(dims=list(r.dims), flops=r.flops, bytes=r.bytes, grid_x=r.grid_x, grid_y=r.grid_y, block=r.block, lds=r.lds) for r in out[:n]]
