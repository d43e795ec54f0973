"""The streaming and reduction kernels of the G+D step (csrc/modulate.hip, bias_act.hip, weight_prep.hip, torgb.hip, fromrgb.hip) against
fp64 references, called through the C ABI so that every kernel form, split and tail is chosen on purpose; the launch log names the kernel
variant that served each launch (the codes are listed in include/sbg_hip.h).

Exact mode (most cases, helpers in exact_util.py): integer or dyadic operands, every product exact, every fp32 partial sum exact in any order
(each case asserts that precondition with `assert_range`), so the kernel's result must equal the fp64 reference rounded once, bit for bit.
Reductions are checked per pixel split / per workgroup block (the partial rows the kernel writes), not only through their total.

Saved 16-bit outputs carry values exactly on +-clamp, one 16-bit ulp inside +-clamp, 0 and -0; every kernel that reads one is also run with a
clamp that is not representable in the 16-bit type (0.7 and 0.71: one rounds down, the other up, in bf16 and f16 alike), where the rail test
must compare the stored value with the fp32 clamp as the reference does (bias_act.cu:141).

Bound mode (real constants, rsqrt, random fp32 data): element-wise bounds derived in each case's docstring; each such case shows that its
bound rejects the reference with one 8-channel slab or one border row removed.
"""
import math

import numpy as np
import pytest
import torch

import style_big_gan_amd  # noqa: F401
from style_big_gan_amd import _lib

from exact_util import U32, U_OUT, assert_exact, assert_range, expect_launch, qgrid, qint, qpow2, within_bound

pytestmark = pytest.mark.gpu

BF, F16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, F16, F32]
LINEAR, RELU, LRELU = 1, 2, 3
TRANSCENDENTAL = {"tanh": 4, "sigmoid": 5, "elu": 6, "selu": 7, "softplus": 8, "swish": 9}
TOL = {F32: 1e-5, BF: 2e-2, F16: 4e-3}
SWEEP8 = 2048 * 256 * 8             # elements one grid-stride sweep of a vec8 streaming kernel covers (sbg_stream_grid caps at 2048 workgroups)
NONREP_CLAMPS = (0.7, 0.71)         # bf16: 0.69921875 (down) / 0.7109375 (up); f16: 0.7001953 (up) / 0.7099609 (down)


def lib():
    return _lib.load()


def S():
    return _lib.stream_ptr()


_alive = []


def P(t):
    """device pointer of t; t stays referenced until the test has synchronised (a temporary freed while its kernel is queued could be handed
    to the next allocation)"""
    if t is not None:
        _alive.append(t)
    return _lib.ptr(t)


@pytest.fixture(autouse=True)
def _hold_operands():
    yield
    torch.cuda.synchronize()
    _alive.clear()


def dcode(dtype):
    return _lib.dtype_code(dtype)


def dev_t(t, dtype, dev):
    return t.to(dtype).to(dev)


def frac_bits(t):
    """smallest d with every element of the fp64 tensor t an integer multiple of 2^-d"""
    for d in range(0, 80):
        s = t * 2.0 ** d
        if bool((s == s.round()).all()):
            return d
    raise AssertionError("operand is not dyadic")


def exact_sum_range(what, terms, dim):
    """precondition for an exact fp32 sum of `terms` over `dim` in any order"""
    assert_range(what, float(terms.abs().sum(dim).max()), frac_bits(terms))


def unaligned(t, dtype, dev):
    """a copy of t on the device at a 2-byte (16-bit) / 4-byte (fp32) offset from a 16-B boundary: the scalar / generic kernels"""
    buf = torch.empty(t.numel() + 8, dtype=dtype, device=dev)
    v = buf[1:1 + t.numel()]
    v.copy_(t.reshape(-1).to(dtype))
    assert v.data_ptr() % 16 != 0
    return v


def rail_values(dtype, clamp):
    """+-clamp as stored, the largest 16-bit value below the fp32 clamp (f16 for fp32 tensors) and its negative, 0 and -0"""
    st = dtype if dtype != F32 else F16
    p = 8 if st == BF else 11                           # significand bits
    c32 = float(np.float32(clamp))
    stored = float(torch.tensor(c32, dtype=torch.float32).to(st))
    inside = stored
    if inside >= c32:
        e = math.floor(math.log2(inside))
        inside -= 2.0 ** (e - p if inside == 2.0 ** e else e - p + 1)
    return torch.tensor([stored, -stored, inside, -inside, 0.0, -0.0], dtype=torch.float64)


def where64(cond, a, b):
    return torch.where(cond, torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64))


def plant(gen, t, vals, frac=0.05):
    """t with a fraction of its elements replaced by values drawn from vals (sign of -0 kept)"""
    t = t.clone(memory_format=torch.contiguous_format)
    flat = t.view(-1)
    k = max(len(vals), int(flat.numel() * frac))
    idx = torch.randperm(flat.numel(), generator=gen)[:k]
    flat[idx] = vals[torch.arange(k) % len(vals)]
    return t


# ================================================================================================================ scale_nc / scale_shift_nc

def scale_ref(x, a, z, bnc, layout):
    """x: fp64 [N, HW, C] (layout 1) or [N, C, HW] (layout 0); a, bnc [N, C]; z [N or 1, HW]"""
    if layout == 1:
        y = x * a[:, None, :]
        if z is not None:
            y = y + z[:, :, None]
        if bnc is not None:
            y = y + bnc[:, None, :]
    else:
        y = x * a[:, :, None]
        if z is not None:
            y = y + z[:, None, :]
        if bnc is not None:
            y = y + bnc[:, :, None]
    return y


SCALE_CASES = [
    # (id, n, c, hw, layout, aligned, want vec8)
    ("cminor_vec8", 3, 40, 37 * 29, 1, True, True),
    ("cminor_odd_c", 2, 12, 101, 1, True, False),
    ("cminor_unaligned", 2, 24, 77, 1, False, False),
    ("planar", 2, 24, 9 * 13, 0, True, False),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", SCALE_CASES, ids=[c[0] for c in SCALE_CASES])
def test_scale_nc_exact(dev, case, dtype):
    tag, n, c, hw, layout, aligned, vec = case
    gen = torch.Generator().manual_seed(1)
    shape = (n, hw, c) if layout == 1 else (n, c, hw)
    x = qint(gen, shape)
    a = qpow2(gen, (n, c))
    z_all = qgrid(gen, (n, hw), -4, 4, 0.25)
    bnc = qgrid(gen, (n, c), -4, 4, 0.25)
    xg = dev_t(x, dtype, dev) if aligned else unaligned(x, dtype, dev)
    ag = a.to(dev, F32)
    for variant in ("plain", "z_per_sample", "z_shared", "shift"):
        y = torch.empty_like(xg) if aligned else unaligned(torch.zeros(x.shape), dtype, dev)
        with expect_launch("scale_nc", lambda d: d[3] == layout and d[4] == (1 if vec else 2), f"{tag} {variant}"):
            if variant == "shift":
                _lib.check(lib().sbg_scale_shift_nc(P(xg), P(ag), P(bnc.to(dev, F32)), P(y), dcode(dtype), layout, n, c, hw, S()), "scale_shift")
                ref = scale_ref(x, a, None, bnc, layout)
            else:
                z = None if variant == "plain" else (z_all if variant == "z_per_sample" else z_all[:1])
                zg = None if z is None else z.to(dev, F32)
                _lib.check(lib().sbg_scale_nc(P(xg), P(ag), P(zg), P(y), dcode(dtype), layout, n, c, hw, 0 if variant != "z_per_sample" else hw, S()),
                           "scale_nc")
                ref = scale_ref(x, a, z if z is None or z.shape[0] == n else z.expand(n, hw), None, layout)
        assert_exact(y.reshape(shape), ref, f"scale_nc {tag} {variant} {dtype}")


def test_scale_nc_two_sweeps_ragged(dev):
    """channel-minor bf16 tensor of 2 grid-stride sweeps of scale_nc_cminor8 plus a ragged remainder of 1439 vectors, with z and the shift"""
    gen = torch.Generator().manual_seed(2)
    n, c, hw = 3, 40, 70001
    nvec = n * c * hw // 8
    assert nvec > 2 * 2048 * 256 and (nvec - 2 * 2048 * 256) % 256 != 0
    x = qint(gen, (n, hw, c))
    a, z, bnc = qpow2(gen, (n, c)), qgrid(gen, (n, hw), -4, 4, 0.25), qgrid(gen, (n, c), -4, 4, 0.25)
    xg = dev_t(x, BF, dev)
    y = torch.empty_like(xg)
    with expect_launch("scale_nc", lambda d: d[4] == 1, "scale_nc two sweeps"):
        _lib.check(lib().sbg_scale_nc(P(xg), P(a.to(dev, F32)), P(z.to(dev, F32)), P(y), dcode(BF), 1, n, c, hw, hw, S()), "scale_nc")
    assert_exact(y, scale_ref(x, a, z, None, 1), "scale_nc two sweeps")
    with expect_launch("scale_nc", lambda d: d[4] == 1, "scale_shift_nc two sweeps"):
        _lib.check(lib().sbg_scale_shift_nc(P(xg), P(a.to(dev, F32)), P(bnc.to(dev, F32)), P(y), dcode(BF), 1, n, c, hw, S()), "scale_shift")
    assert_exact(y, scale_ref(x, a, None, bnc, 1), "scale_shift_nc two sweeps")


# ================================================================================================================ dot_hw / dot_hw_scale / moments_hw

def split_sums(t, nsplit, hw):
    """t: fp64 [N, HW, C] -> [nsplit, N, C] sums over the pixel splits sbg_dot_hw_splits describes"""
    pps = (hw + nsplit - 1) // nsplit
    return torch.stack([t[:, s * pps:min(hw, (s + 1) * pps)].sum(1) for s in range(nsplit)])


DOT_CASES = [
    # (id, dtype, n, c, hw, layout, aligned, form, ragged)   form 1 generic / 2 lane per channel vector / 3 serial
    ("lane_vec_c64_ragged", BF, 2, 64, 10003, 1, True, 2, True),
    ("lane_vec_c8", F16, 3, 8, 4099, 1, True, 2, True),
    ("lane_vec_c256_fp32", F32, 2, 256, 777, 1, True, 2, True),
    ("serial_c24", BF, 2, 24, 5003, 1, True, 3, True),
    ("serial_c520", F16, 2, 520, 301, 1, True, 3, True),
    ("generic_planar", BF, 2, 24, 999, 0, True, 1, False),
    ("generic_unaligned_memset", BF, 2, 64, 3001, 1, False, 1, False),
]


@pytest.mark.parametrize("case", DOT_CASES, ids=[c[0] for c in DOT_CASES])
def test_dot_hw_exact(dev, case):
    tag, dtype, n, c, hw, layout, aligned, form, ragged = case
    gen = torch.Generator().manual_seed(3)
    u, v = qint(gen, (n, hw, c)), qint(gen, (n, hw, c))
    if layout == 0:
        u_st, v_st = u.permute(0, 2, 1).contiguous(), v.permute(0, 2, 1).contiguous()
    else:
        u_st, v_st = u, v
    ns = lib().sbg_dot_hw_splits(layout, n, c, hw)
    pps = (hw + ns - 1) // ns
    if ragged:
        last = hw - (ns - 1) * pps
        assert ns > 1 and last != pps and (form != 2 or last % (256 // (c // 8)) != 0), (ns, pps)
    assert_range(tag, 4 * hw)
    ug = dev_t(u_st, dtype, dev) if aligned else unaligned(u_st, dtype, dev)
    vg = dev_t(v_st, dtype, dev) if aligned else unaligned(v_st, dtype, dev)
    for with_v in (True, False):
        part = torch.full((ns, n, c), float("nan"), device=dev)
        with expect_launch("dot_hw", lambda d: d[3] == layout and d[4] == form and d[5] == ns, f"{tag} v={with_v}"):
            _lib.check(lib().sbg_dot_hw(P(ug), P(vg) if with_v else None, P(part), dcode(dtype), layout, n, c, hw, S()), "dot_hw")
        prod = u * v if with_v else u
        if form == 1:
            ref = torch.zeros(ns, n, c, dtype=torch.float64)
            ref[0] = prod.sum(1)                                    # the generic kernel writes split 0; the host zeroed the others
        else:
            ref = split_sums(prod, ns, hw)
        assert_exact(part, ref, f"dot_hw {tag} v={with_v}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("c,hw", [(64, 10003), (8, 4099), (256, 1500)])
def test_dot_hw_scale_exact(dev, dtype, c, hw):
    """one pass: y = u * scale[n, c] (16-bit rounding once) and the per-split partials of sum u * v"""
    gen = torch.Generator().manual_seed(4)
    n = 2
    u, v, sc = qint(gen, (n, hw, c)), qint(gen, (n, hw, c)), qpow2(gen, (n, c), exps=(-3, -1, 0, 2))
    ns = lib().sbg_dot_hw_splits(1, n, c, hw)
    assert_range("dot_hw_scale", 4 * hw)
    ug, vg = dev_t(u, dtype, dev), dev_t(v, dtype, dev)
    y = torch.empty_like(ug)
    part = torch.full((ns, n, c), float("nan"), device=dev)
    with expect_launch("dot_hw", lambda d: d[3] == 3 and d[4] == 2 and d[5] == ns, "dot_hw_scale"):
        _lib.check(lib().sbg_dot_hw_scale(P(ug), P(vg), P(sc.to(dev, F32)), P(y), P(part), dcode(dtype), n, c, hw, S()), "dot_hw_scale")
    assert_exact(y, u * sc[:, None, :], f"dot_hw_scale y c={c}")
    assert_exact(part, split_sums(u * v, ns, hw), f"dot_hw_scale partials c={c}")


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("hw,vec", [(64 * 64 + 8, True), (33 * 31, False)])
def test_moments_hw_exact(dev, dtype, hw, vec):
    gen = torch.Generator().manual_seed(5)
    n, c = 3, 5
    x = qint(gen, (n, c, hw), hi=4)
    assert_range("moments", 16 * hw)
    r = torch.empty(2, n * c, device=dev)
    with expect_launch("dot_hw", lambda d: d[3] == 5 and d[4] == (1 if vec else 2), f"moments_hw vec={vec}"):
        _lib.check(lib().sbg_moments_hw(P(dev_t(x, dtype, dev)), P(r), dcode(dtype), n, c, hw, S()), "moments_hw")
    assert_exact(r, torch.stack([x.sum(2).reshape(-1), (x * x).sum(2).reshape(-1)]), f"moments_hw {dtype}")


# ================================================================================================================ modconv_bwd

ACTS = {"lrelu": (LRELU, 0.25, 2.0), "relu": (RELU, 0.0, 2.0), "linear": (LINEAR, 1.0, 2.0)}


def modconv_bwd_ref(dy, y, dcoef, noise, bias, ps, alpha, gain, clamp32):
    """fp64 statement of sbg_modconv_bwd(_prescaled) on [N, HW, C] tensors: d1 = (dy * ps) * slope(y) * [|y| < clamp], pre recovered from y"""
    g = dy * ps[:, None, :] if ps is not None else dy
    pos = y > 0
    live = (y > -clamp32) & (y < clamp32)
    d1 = torch.where(live, g * where64(pos, gain, gain * alpha), torch.zeros_like(g))
    inv_neg = 1.0 / (gain * alpha) if alpha > 0 else 0.0
    pre = y * where64(pos, 1.0 / gain, inv_neg)
    nz = noise[:, :, None] if noise is not None else 0.0
    b = bias[None, None, :] if bias is not None else 0.0
    t2 = d1 * (pre - nz - b)
    return d1, t2, (dy * y if ps is not None else None)


def run_modconv_bwd(dev, dtype, dy, y, dcoef, noise, bias, ps, act, alpha, gain, clamp, want_dn, what):
    n, hw, c = dy.shape
    ns = lib().sbg_dot_hw_splits(1, n, c, hw)
    dyg, yg = dev_t(dy, dtype, dev), dev_t(y, dtype, dev)
    d2 = torch.empty_like(dyg)
    part = torch.full((2, ns, n, c), float("nan"), device=dev)
    part3 = torch.full((ns, n, c), float("nan"), device=dev)
    dn = torch.full((n, hw), float("nan"), device=dev) if want_dn else None
    nsn = 0 if noise is None or noise.shape[0] == 1 else hw
    args = (P(dcoef.to(dev, F32)), P(None if noise is None else noise.to(dev, F32)), P(None if bias is None else bias.to(dev, F32)), P(d2), P(part))
    code = 4 if ps is not None else 2
    with expect_launch("dot_hw", lambda d: d[3] == code and d[4] == 2 and d[5] == ns, what):
        if ps is not None:
            _lib.check(lib().sbg_modconv_bwd_prescaled(P(dyg), P(yg), P(ps.to(dev, F32)), *args, P(part3), P(dn), dcode(dtype), n, c, hw, nsn,
                                                       act, alpha, gain, clamp, S()), what)
        else:
            _lib.check(lib().sbg_modconv_bwd(P(dyg), P(yg), *args, P(dn), dcode(dtype), n, c, hw, nsn, act, alpha, gain, clamp, S()), what)
    return ns, d2, part, part3, dn


def check_modconv_bwd_exact(dev, dtype, n, c, hw, act_name, noise_kind, want_dn, prescale, clamp, seed, y_range=8.0, y_step=0.25):
    act, alpha, gain = ACTS[act_name]
    gen = torch.Generator().manual_seed(seed)
    what = f"modconv_bwd {dtype} C={c} HW={hw} {act_name} noise={noise_kind} dnoise={want_dn} prescale={prescale} clamp={clamp}"
    dy = qint(gen, (n, hw, c), hi=1)
    y = qgrid(gen, (n, hw, c), -y_range, y_range, y_step)
    st = dtype if dtype != F32 else F16
    y = plant(gen, y, rail_values(dtype, clamp)).to(st).to(torch.float64)   # every saved value representable in the 16-bit type
    y[0, 0, 0] = -0.0
    dcoef = qpow2(gen, (n, c))
    noise = {"none": None, "shared": qgrid(gen, (1, hw), -4, 4, 0.25), "per_sample": qgrid(gen, (n, hw), -4, 4, 0.25)}[noise_kind]
    bias = qgrid(gen, (c,), -4, 4, 0.25) + 0.125
    ps = qpow2(gen, (n, c), exps=(-2, -1, 0)) if prescale else None
    c32 = float(np.float32(clamp))
    d1, t2, t3 = modconv_bwd_ref(dy, y, dcoef, None if noise is None else noise.expand(n, hw), bias, ps, alpha, gain, c32)
    ns, d2, part, part3, dn = run_modconv_bwd(dev, dtype, dy, y, dcoef, noise, bias, ps, act, alpha, gain, clamp, want_dn, what)
    for name, terms in (("bias sums", d1), ("demodulation sums", t2)) + ((("prescale sums", t3),) if prescale else ()):
        assert_range(what + " " + name, float(split_sums(terms.abs(), ns, hw).max()), frac_bits(terms))
    exact_sum_range(what + " dnoise", d1, 2)
    assert_exact(d2, d1 * dcoef[:, None, :], what + " d2")
    assert_exact(part[0], split_sums(d1, ns, hw), what + " bias sums")
    assert_exact(part[1], split_sums(t2, ns, hw), what + " demodulation sums")
    if prescale:
        assert_exact(part3, split_sums(t3, ns, hw), what + " prescale sums")
    if want_dn:
        assert_exact(dn, d1.sum(2), what + " dnoise")
    return d1


MODCONV_NOISE = ["none", "shared", "per_sample"]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("c", [8, 64, 512])
def test_modconv_bwd_exact(dev, dtype, c):
    """every activation, with and without prescale, cycling noise (none / shared / per sample) and dnoise (on / off); the image (37 x 29) splits
    into a ragged last split at every C; saved y on the grid 2^-2 in [-8, 8] with the rail values planted, clamp 8"""
    hw = 37 * 29
    i = 0
    for act_name in ACTS:
        for prescale in (False, True):
            check_modconv_bwd_exact(dev, dtype, 2, c, hw, act_name, MODCONV_NOISE[i % 3], (i // 3) % 2 == 0 or i == 5, prescale, 8.0, seed=10 + i)
            i += 1


@pytest.mark.parametrize("prescale", [False, True])
def test_modconv_bwd_exact_headline(dev, prescale):
    """G's 128-channel layer at 256^2, N = 2: all five results (d2, bias / demodulation / prescale sums per split, dnoise) bit for bit"""
    check_modconv_bwd_exact(dev, BF, 2, 128, 256 * 256, "lrelu", "per_sample", True, prescale, 8.0, seed=30)


@pytest.mark.parametrize("dtype", [BF, F16], ids=str)
@pytest.mark.parametrize("clamp", NONREP_CLAMPS)
def test_modconv_bwd_nonrepresentable_clamp(dev, dtype, clamp):
    """a clamp the 16-bit type cannot hold: the rail test compares the stored y with the fp32 clamp"""
    d1 = check_modconv_bwd_exact(dev, dtype, 2, 64, 31 * 17, "lrelu", "shared", True, False, clamp, seed=40, y_range=0.75, y_step=2.0 ** -6)
    assert bool((d1 != 0).any())


def test_modconv_bwd_bound_real_constants(dev):
    """alpha 0.2, gain sqrt 2, clamp 256; fp32 randn dy, noise, bias, dcoef; saved bf16 y (randn * 64, rail values planted).
    The kernel uses fl(gain), fl(gain) * fl(alpha) rounded, their fp32 reciprocals; per element with M = |pre| + |noise| + |b|:
      d1  = dy * slope: <= 3 U32 |d1| from the constants and the product;
      t   = (pre - noise - b): pre from y * fl(1 / slope) (<= 6 U32 |pre|) and two subtractions (<= 2 U32 M), then d1 * t (one more):
            <= 12 U32 |d1| M;
      sums over a split of P pixels in any order: <= (P - 1) U32 sum |term|.
    So |part[0] - ref| <= (P + 3) U32 sum |d1|,  |part[1] - ref| <= (P + 12) U32 sum |d1| M,  |dnoise - ref| <= (C + 3) U32 sum_c |d1|,
    d2 = fl16(fl(d1 * dcoef)): <= U_OUT |ref| + (1 + U_OUT) 5 U32 |ref|.  Rejection: the reference without the image's last row (the last
    split's sums) and without one 8-channel slab (dnoise)."""
    gen = torch.Generator().manual_seed(50)
    n, c, r = 2, 64, 64
    hw = r * r
    alpha, gain, clamp = 0.2, math.sqrt(2), 256.0
    dy = torch.randn(n, hw, c, generator=gen, dtype=torch.float64).to(BF).double()
    y = plant(gen, (torch.randn(n, hw, c, generator=gen, dtype=torch.float64) * 64).clamp(-256, 256), rail_values(BF, clamp)).to(BF).double()
    dcoef = (torch.rand(n, c, generator=gen, dtype=torch.float64) + 0.5).float().double()
    noise = torch.randn(n, hw, generator=gen, dtype=torch.float64).float().double()
    bias = torch.randn(c, generator=gen, dtype=torch.float64).float().double()
    d1, t2, _ = modconv_bwd_ref(dy, y, dcoef, noise, bias, None, alpha, gain, clamp)
    ns, d2, part, _, dn = run_modconv_bwd(dev, BF, dy, y, dcoef, noise, bias, None, LRELU, alpha, gain, clamp, True, "modconv_bwd bound")
    pps = (hw + ns - 1) // ns
    pre = torch.where(y > 0, y / gain, y / (gain * alpha))
    M = pre.abs() + noise.abs()[:, :, None] + bias.abs()[None, None, :]
    b0 = (pps + 3) * U32 * split_sums(d1.abs(), ns, hw)
    b1 = (pps + 12) * U32 * split_sums(d1.abs() * M, ns, hw)
    bn = (c + 3) * U32 * d1.abs().sum(2)
    ref_d2 = d1 * dcoef[:, None, :]
    bd2 = U_OUT[BF] * ref_d2.abs() + (1 + U_OUT[BF]) * 5 * U32 * ref_d2.abs()
    r0, r1 = split_sums(d1, ns, hw), split_sums(t2, ns, hw)
    assert within_bound(part[0].cpu(), r0, b0) and within_bound(part[1].cpu(), r1, b1), "modconv_bwd sums exceed the bound"
    assert within_bound(dn.cpu(), d1.sum(2), bn) and within_bound(d2.cpu().double(), ref_d2, bd2), "modconv_bwd dnoise / d2 exceed the bound"
    cut = d1.clone()
    cut[:, hw - r:] = 0
    cut2 = t2.clone()
    cut2[:, hw - r:] = 0
    assert not within_bound(part[0].cpu(), split_sums(cut, ns, hw), b0), "the bound does not reject the bias sums without the last row"
    assert not within_bound(part[1].cpu(), split_sums(cut2, ns, hw), b1), "the bound does not reject the demodulation sums without the last row"
    assert not within_bound(dn.cpu(), d1[:, :, 8:].sum(2), bn), "the bound does not reject dnoise without one 8-channel slab"


# ================================================================================================================ bias_act

def act_fwd64(name, x, alpha):
    if name == "linear":
        return x
    if name == "relu":
        return torch.where(x > 0, x, torch.zeros_like(x))
    if name == "lrelu":
        return torch.where(x > 0, x, x * alpha)
    if name == "tanh":
        return torch.tanh(x)
    if name == "sigmoid":
        return torch.sigmoid(x)
    if name == "elu":
        return torch.where(x >= 0, x, torch.expm1(x))
    if name == "selu":
        return torch.selu(x)
    if name == "softplus":
        return torch.nn.functional.softplus(x)
    if name == "swish":
        return x * torch.sigmoid(x)
    raise KeyError(name)


def act_grad64(name, x, xref, yy, alpha):
    """first derivative from the saved output yy = yref / gain (bias_act.cu:23-146) times the incoming x"""
    if name == "linear":
        return x
    if name == "relu":
        return torch.where(yy > 0, x, torch.zeros_like(x))
    if name == "lrelu":
        return torch.where(yy > 0, x, x * alpha)
    if name == "tanh":
        return x * (1 - yy * yy)
    if name == "sigmoid":
        return x * yy * (1 - yy)
    if name == "elu":
        return torch.where(yy >= 0, x, x * (yy + 1))
    if name == "selu":
        sc, al = 1.0507009873554804934193349852946, 1.6732632423543772848170429916717
        return torch.where(yy >= 0, x * sc, x * (yy + sc * al))
    if name == "softplus":
        return x * (1 - torch.exp(-yy))
    if name == "swish":
        c = torch.exp(xref)
        d = c + 1
        return torch.where(xref > 40, x, x * c * (xref + d) / (d * d))
    raise KeyError(name)


def bias_act_ref(name, grad, x, b_full, xref, yref, alpha, gain, clamp32):
    if grad == 0:
        y = act_fwd64(name, x + b_full, alpha) * gain
        if clamp32 >= 0:
            y = torch.where((y > -clamp32) & (y < clamp32), y, where64(y >= 0, clamp32, -clamp32))
        return y
    if grad == 2:
        return torch.zeros_like(x)
    xr = xref + b_full
    yy = yref / gain
    y = act_grad64(name, x, xr, yy, alpha) * gain
    if name == "swish":
        yref = act_fwd64("swish", xr, alpha) * gain
    if clamp32 >= 0:
        y = torch.where((yref > -clamp32) & (yref < clamp32), y, torch.zeros_like(y))
    return y


# (id, numel, sizeB, stepB, aligned, bias mode, vec)
BIAS_CASES = [
    ("no_bias", 8 * 301 + 5, 0, 0, True, 0, True),
    ("mode1_cminor", 64 * 97, 64, 1, True, 1, True),
    ("mode2_per_vector", 24 * 16 * 7 + 3, 24, 16, True, 2, True),
    ("mode3_generic", 20 * 9 * 11 + 6, 20, 9, True, 3, True),
    ("mode3_cminor_c12", 12 * 121, 12, 1, True, 3, True),
    ("scalar_unaligned", 16 * 77 + 7, 16, 77, False, 3, False),
    ("scalar_mode1_unaligned", 32 * 55, 32, 1, False, 1, False),
]


def run_bias_act(dev, dtype, name, grad, x, b, xref, yref, alpha, gain, clamp, sizeB, stepB, aligned, bmode, vec, what):
    put = (lambda t: dev_t(t, dtype, dev)) if aligned else (lambda t: unaligned(t, dtype, dev))
    xg = put(x)
    y = put(torch.zeros_like(x))
    bg = None if b is None else dev_t(b, dtype, dev)
    xr = None if xref is None else put(xref)
    yr = None if yref is None else put(yref)
    with expect_launch("bias_act", lambda d: d[1] == grad and d[4] == (1 if vec else 2) and d[5] == bmode, what):
        _lib.check(lib().sbg_bias_act(P(xg), P(bg), P(xr), P(yr), None, P(y), dcode(dtype), grad, {"linear": 1, "relu": 2, "lrelu": 3, **TRANSCENDENTAL}[name],
                                      alpha, gain, clamp, x.numel(), max(sizeB, 1), max(stepB, 1), S()), what)
    return y


def bias_full(b, numel, sizeB, stepB):
    if b is None:
        return torch.zeros(numel, dtype=torch.float64)
    return b[(torch.arange(numel) // stepB) % sizeB]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", BIAS_CASES, ids=[c[0] for c in BIAS_CASES])
def test_bias_act_exact(dev, case, dtype):
    """linear / relu / lrelu (slope 1/4, gain 2, clamp 8) at grad 0, 1 and 2, bit for bit: x on the grid 2^-2, bias offset by 2^-3 (no
    pre-activation is 0), the saved output yref with the rail values planted; the vec8 tail (numel % 8) and the scalar kernel"""
    tag, numel, sizeB, stepB, aligned, bmode, vec = case
    gen = torch.Generator().manual_seed(60)
    x = qgrid(gen, (numel,), -8, 8, 0.25)
    b = None if sizeB == 0 else qgrid(gen, (sizeB,), -2, 2, 0.25) + 0.125
    bf = bias_full(b, numel, sizeB, stepB)
    st = dtype if dtype != F32 else F16
    assert_range(tag, 2 * (8 + 2.125), 3)
    for name, (_, alpha, gain) in ACTS.items():
        for grad in (0, 1, 2):
            what = f"bias_act {tag} {name} grad {grad} {dtype}"
            if grad == 0:
                xref = yref = None
                ref = bias_act_ref(name, 0, x, bf, None, None, alpha, gain, 8.0)
            else:
                xref = qgrid(gen, (numel,), -8, 8, 0.25)
                yref = plant(gen, bias_act_ref(name, 0, xref, bf, None, None, alpha, gain, 8.0), rail_values(dtype, 8.0)).to(st).double()
                ref = bias_act_ref(name, grad, x, bf, xref, yref, alpha, gain, 8.0)
            y = run_bias_act(dev, dtype, name, grad, x, b, xref, yref, alpha, gain, 8.0, sizeB, stepB, aligned, bmode, vec, what)
            assert_exact(y, ref, what)


@pytest.mark.parametrize("name", ["linear", "relu", "lrelu"])
def test_bias_act_two_sweeps(dev, name):
    """bf16, channel-minor bias (mode 1), numel = 2 sweeps of the vec8 kernel + 1000 vectors + a 5-element tail, grad 0 and 1"""
    gen = torch.Generator().manual_seed(61)
    numel = 2 * SWEEP8 + 8 * 1000 + 5
    c = 16
    x = qgrid(gen, (numel,), -8, 8, 0.25)
    b = qgrid(gen, (c,), -2, 2, 0.25) + 0.125
    bf = bias_full(b, numel, c, 1)
    _, alpha, gain = ACTS[name]
    y = run_bias_act(dev, BF, name, 0, x, b, None, None, alpha, gain, 8.0, c, 1, True, 1, True, f"bias_act {name} two sweeps")
    assert_exact(y, bias_act_ref(name, 0, x, bf, None, None, alpha, gain, 8.0), f"bias_act {name} two sweeps")
    yref = plant(gen, bias_act_ref(name, 0, x, bf, None, None, alpha, gain, 8.0), rail_values(BF, 8.0)).to(BF).double()
    g = qint(gen, (numel,), hi=2)
    y = run_bias_act(dev, BF, name, 1, g, b, x, yref, alpha, gain, 8.0, c, 1, True, 1, True, f"bias_act {name} two sweeps grad 1")
    assert_exact(y, bias_act_ref(name, 1, g, bf, x, yref, alpha, gain, 8.0), f"bias_act {name} two sweeps grad 1")


@pytest.mark.parametrize("dtype", [BF, F16], ids=str)
@pytest.mark.parametrize("clamp", NONREP_CLAMPS)
def test_bias_act_nonrepresentable_clamp(dev, dtype, clamp):
    """grad 1 reads the saved 16-bit output: its rail test compares with the fp32 clamp (stored rails below it pass the gradient)"""
    gen = torch.Generator().manual_seed(62)
    numel = 8 * 999 + 3
    yref = plant(gen, qgrid(gen, (numel,), -0.75, 0.75, 2.0 ** -6), rail_values(dtype, clamp), frac=0.2).to(dtype).double()
    g = qint(gen, (numel,), hi=2)
    for name in ("linear", "lrelu"):
        _, alpha, gain = ACTS[name]
        y = run_bias_act(dev, dtype, name, 1, g, None, torch.zeros(numel, dtype=torch.float64), yref, alpha, gain, clamp, 0, 0, True, 0, True,
                         f"bias_act clamp {clamp}")
        assert_exact(y, bias_act_ref(name, 1, g, torch.zeros(numel, dtype=torch.float64), torch.zeros(numel, dtype=torch.float64), yref, alpha,
                                     gain, float(np.float32(clamp))), f"bias_act {name} clamp {clamp} {dtype}")


@pytest.mark.parametrize("name", list(TRANSCENDENTAL))
def test_bias_act_transcendental_indexing(dev, name):
    """the same indexing matrix (bias modes, tail, scalar kernel) for the transcendental activations against fp64 at the op tests' TOL"""
    gen = torch.Generator().manual_seed(63)
    for dtype in (F32, BF):
        for tag, numel, sizeB, stepB, aligned, bmode, vec in BIAS_CASES:
            x = torch.randn(numel, generator=gen, dtype=torch.float64).to(dtype).double() * 2
            b = None if sizeB == 0 else torch.randn(sizeB, generator=gen, dtype=torch.float64).to(dtype).double()
            bf = bias_full(b, numel, sizeB, stepB)
            for grad in (0, 1):
                what = f"bias_act {name} {tag} grad {grad} {dtype}"
                if grad == 0:
                    xref = yref = None
                else:
                    xref = torch.randn(numel, generator=gen, dtype=torch.float64).to(dtype).double()
                    yref = bias_act_ref(name, 0, xref, bf, None, None, 0.0, 1.0, -1.0).to(dtype).double()
                ref = bias_act_ref(name, grad, x, bf, xref, yref, 0.0, 1.0, -1.0)
                y = run_bias_act(dev, dtype, name, grad, x, b, xref, yref, 0.0, 1.0, -1.0, sizeB, stepB, aligned, bmode, vec, what)
                err = float((y.cpu().double() - ref).abs().max() / (ref.abs().max() + 1e-12))
                assert err <= TOL[dtype], f"{what}: rel err {err:.3e}"


# ================================================================================================================ weight preparation

def pack_ref(w64, gain, Bp, order_ab):
    """w64 [Cout, Cin, kh, kw]; order_ab: 'fwd' (rows Cout, cols Cin) or 'dgrad' (rows Cin, cols Cout) -> [taps, A, Bp] fp64, pads 0"""
    v = w64 * gain
    m = v.permute(2, 3, 0, 1) if order_ab == "fwd" else v.permute(2, 3, 1, 0)
    t = m.reshape(-1, m.shape[2], m.shape[3])
    out = torch.zeros(t.shape[0], t.shape[1], Bp, dtype=torch.float64)
    out[:, :, :t.shape[2]] = t
    return out


PACK_CASES = [
    # (id, cout, cin, k, channels_last, order, Bp, w2, transposing)
    ("fwd_contig_w2", 40, 72, 3, False, "fwd", 80, True, False),
    ("fwd_contig", 33, 70, 3, False, "fwd", 96, False, False),
    ("dgrad_channels_last_transposing", 72, 40, 3, True, "dgrad", 80, False, True),
    ("dgrad_channels_last_transposing_1x1", 130, 72, 1, True, "dgrad", 136, False, True),
    ("dgrad_contig", 40, 36, 3, False, "dgrad", 48, False, False),
    ("fwd_channels_last_w2", 24, 40, 3, True, "fwd", 40, True, False),
]


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
@pytest.mark.parametrize("case", PACK_CASES, ids=[c[0] for c in PACK_CASES])
def test_pack_weight_exact(dev, case, dtype):
    """out[t][a][b] = cast(w[a, b, t] * gain) with columns B..Bp exactly zero, w2 = sum_t (w * gain)^2 -- the parameter's own strides"""
    tag, cout, cin, k, cl, order, Bp, want_w2, transposing = case
    gen = torch.Generator().manual_seed(70)
    step = 2.0 ** -5 if want_w2 else 2.0 ** -12         # the fine grid exercises the 16-bit rounding (ties included); w2 needs exact squares
    w = qgrid(gen, (cout, cin, k, k), -2, 2, step)
    gain = 0.5
    wg = w.to(dev, F32)
    if cl:
        wg = wg.contiguous(memory_format=torch.channels_last)
    s = wg.stride()
    A, B, sA, sB = (cout, cin, s[0], s[1]) if order == "fwd" else (cin, cout, s[1], s[0])
    out = torch.full((k * k, A, Bp), float("nan"), device=dev).to(dtype)
    w2 = torch.full((A, B), float("nan"), device=dev) if want_w2 else None
    if want_w2:
        exact_sum_range(tag + " w2", ((w * gain) ** 2).reshape(cout, cin, -1), 2)
    with expect_launch("weight_prep", lambda d: d[3] == 0 and d[4] == (1 if transposing else 2), tag):
        _lib.check(lib().sbg_pack_weight(P(wg), P(out), dcode(dtype), A, B, k, k, sA, sB, s[2], s[3], Bp, gain, P(w2), S()), tag)
    ref = pack_ref(w, gain, Bp, order)
    assert_exact(out, ref, f"pack_weight {tag} {dtype}")
    assert bool((out[:, :, B:].float() == 0).all()) and not bool(torch.signbit(out[:, :, B:].float()).any()), f"{tag}: padding is not +0"
    if want_w2:
        sq = ((w * gain) ** 2).sum([2, 3])
        assert_exact(w2, sq if order == "fwd" else sq.t(), f"pack_weight {tag} w2")


@pytest.mark.parametrize("cl", [False, True], ids=["contiguous", "channels_last"])
@pytest.mark.parametrize("with_dw2", [False, True])
def test_unpack_wgrad_exact(dev, cl, with_dw2):
    """dw[a, b, t] = gain * dwp[t][a][b] (+ 2 gain^2 w[a, b, t] dw2[a][b]) into the parameter's own strides; dwp with a padded row stride"""
    gen = torch.Generator().manual_seed(71)
    cout, cin, k, gain = 40, 36, 3, 0.5
    Bp = 48
    dwp = qgrid(gen, (k * k, cout, Bp), -64, 64, 2.0 ** -4)
    w = qgrid(gen, (cout, cin, k, k), -2, 2, 2.0 ** -3)
    dw2 = qgrid(gen, (cout, cin), -4, 4, 2.0 ** -3) if with_dw2 else None
    dw = torch.full((cout, cin, k, k), float("nan"), device=dev)
    wg = w.to(dev, F32)
    if cl:
        dw = dw.contiguous(memory_format=torch.channels_last)
        wg = wg.contiguous(memory_format=torch.channels_last)
    s = dw.stride()
    assert s == wg.stride()
    with expect_launch("weight_prep", lambda d: d[3] == 1, "unpack_wgrad"):
        _lib.check(lib().sbg_unpack_wgrad(P(dwp.to(dev, F32)), cout * Bp, Bp, P(dw), P(wg), P(None if dw2 is None else dw2.to(dev, F32)), cout, cin, k, k,
                                          s[0], s[1], s[2], s[3], gain, S()), "unpack_wgrad")
    ref = gain * dwp[:, :, :cin].permute(1, 2, 0).reshape(cout, cin, k, k)
    if with_dw2:
        ref = ref + 2 * gain * gain * dw2[:, :, None, None] * w
    assert_exact(dw, ref, f"unpack_wgrad cl={cl} dw2={with_dw2}")


def split_values(gen, shape):
    """fp32 values: random bit patterns (normal range), ties (low 16 bits 0x8000), ties of the second part, and values near the bottom of the
    normal range whose second / third remainders are subnormal"""
    n = int(np.prod(shape))
    sign = torch.randint(0, 2, (n,), generator=gen, dtype=torch.int64) << 31
    expo = torch.randint(100, 150, (n,), generator=gen, dtype=torch.int64)
    expo[: n // 6] = torch.randint(1, 12, (n // 6,), generator=gen)                 # 2^-126 .. 2^-115: remainders fall below 2^-126
    mant = torch.randint(0, 1 << 23, (n,), generator=gen, dtype=torch.int64)
    bits = sign | (expo << 23) | mant
    k = n // 6
    bits[k:2 * k] = (bits[k:2 * k] & ~0xFFFF) | 0x8000                               # first part is a tie
    bits[2 * k:3 * k] = (bits[2 * k:3 * k] & ~0xFF) | 0x80                           # second part is (often) a tie
    return torch.from_numpy(bits.to(torch.int32).numpy().view(np.float32).copy()).reshape(shape)


def torch_parts(x):
    p0 = x.to(BF)
    r1 = x - p0.float()
    p1 = r1.to(BF)
    p2 = (r1 - p1.float()).to(BF)
    return [p0, p1, p2]


def assert_bits(got, want, what):
    g, w = got.cpu().contiguous().view(torch.int16), want.contiguous().view(torch.int16)
    bad = g != w
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} parts differ; first at {tuple(int(i) for i in bad.nonzero()[0])}"


def test_split_bf16_cat_exact(dev):
    """the three parts, laid side by side along C in the requested order, bit for bit against torch's RNE casts"""
    gen = torch.Generator().manual_seed(72)
    x = split_values(gen, (3, 20, 37))
    p1, p2 = (p.float() for p in torch_parts(x)[1:])
    assert bool((p2 != 0).any()) and bool(((p1 != 0) & (p1.abs() < 2.0 ** -126)).any()) and bool(((p2 != 0) & (p2.abs() < 2.0 ** -126)).any())
    for order in ((0, 1, 2), (2, 0, 1, 1, 0, 2)):
        y = torch.empty(3, len(order) * 20, 37, dtype=BF, device=dev)
        o = ctypes_int_array(order)
        with expect_launch("weight_prep", lambda d: d[3] == 4 and d[4] == len(order), "split_bf16_cat"):
            _lib.check(lib().sbg_split_bf16_cat(P(x.to(dev)), P(y), 3, 20, 37, len(order), o, S()), "split_bf16_cat")
        parts = torch_parts(x)
        assert_bits(y, torch.cat([parts[s] for s in order], 1), f"split_bf16_cat order {order}")


def ctypes_int_array(vals, kind="int"):
    import ctypes
    t = ctypes.c_int if kind == "int" else ctypes.c_int64
    return (t * len(vals))(*vals)


@pytest.mark.parametrize("cat", [0, 1, 2, 3])
def test_split_bf16_cat_nd_exact(dev, cat):
    """the split of a strided (permuted) 4-D view, written densely with the parts along dim `cat`"""
    gen = torch.Generator().manual_seed(73)
    base = split_values(gen, (24, 13, 3, 3)).to(dev)
    view = base.permute(2, 3, 0, 1)                                       # [kh, kw, cout, cin]
    order = (1, 0, 2)
    shape = list(view.shape)
    out_shape = list(shape)
    out_shape[cat] *= len(order)
    y = torch.empty(out_shape, dtype=BF, device=dev)
    with expect_launch("weight_prep", lambda d: d[3] == 5 and d[4] == len(order), "split_bf16_cat_nd"):
        _lib.check(lib().sbg_split_bf16_cat_nd(P(base), ctypes_int_array(shape, "i64"), ctypes_int_array(list(view.stride()), "i64"), cat, P(y),
                                               len(order), ctypes_int_array(order), S()), "split_bf16_cat_nd")
    parts = torch_parts(view.cpu().contiguous())
    assert_bits(y, torch.cat([parts[s] for s in order], cat), f"split_bf16_cat_nd cat={cat}")


# ================================================================================================================ demodulation coefficients

def test_demod_coefs_bound(dev):
    """d[n, o] = rsqrt(sum_i s^2 w2 + eps).  All terms are >= 0, so the fp32 sum (two roundings per term, any order) is within (I + 2) U32 of
    the exact sum relatively, + eps one more; rsqrt halves a relative error and adds its own (<= 2 ulp = 2^-22 allowed):
      |d - ref| <= ((I + 3) / 2 + 4) U32 d_ref.
    Backward against the kernel's own d, q = -0.5 g d^3 (3 roundings):  ds[n, i] = 2 s sum_o q w2 (one rounding per product, O - 1 additions,
    the final product)  ->  <= (O + 6) U32 2 |s| sum_o |q| w2;  dw2[o, i] = sum_n q s s  ->  <= (N + 6) U32 sum_n |q| s^2.
    Rejection: one 8-channel slab of i (forward) or of o (ds) removed."""
    gen = torch.Generator().manual_seed(80)
    n, o, i = 4, 72, 136
    s = (torch.randn(n, i, generator=gen, dtype=torch.float64) + 1).float().double()
    w2 = (torch.rand(o, i, generator=gen, dtype=torch.float64) * 0.05).float().double()
    g = torch.randn(n, o, generator=gen, dtype=torch.float64).float().double()
    eps = 1e-8
    d = torch.empty(n, o, device=dev)
    with expect_launch("weight_prep", lambda dd: dd[3] == 2, "demod_coefs"):
        _lib.check(lib().sbg_demod_coefs(P(s.to(dev, F32)), P(w2.to(dev, F32)), P(d), n, o, i, eps, S()), "demod_coefs")
    ref = 1 / torch.sqrt((s * s) @ w2.t() + float(np.float32(eps)))
    bound = ((i + 3) / 2 + 4) * U32 * ref
    assert within_bound(d.cpu(), ref, bound), f"demod_coefs: bound exceeded by {float(((d.cpu().double() - ref).abs() - bound).max()):.3e}"
    assert not within_bound(d.cpu(), 1 / torch.sqrt((s[:, 8:] ** 2) @ w2[:, 8:].t() + eps), bound)
    dd = d.cpu().double()
    ds = torch.empty(n, i, device=dev)
    dw2 = torch.empty(o, i, device=dev)
    with expect_launch("weight_prep", lambda x: x[3] == 3, "demod_coefs_bwd"):
        _lib.check(lib().sbg_demod_coefs_bwd(P(g.to(dev, F32)), P(d), P(s.to(dev, F32)), P(w2.to(dev, F32)), P(ds), P(dw2), n, o, i, S()), "demod_bwd")
    q = -0.5 * g * dd ** 3
    r_ds, r_dw2 = 2 * s * (q @ w2), q.t() @ (s * s)
    b_ds = (o + 6) * U32 * 2 * s.abs() * (q.abs() @ w2)
    b_dw2 = (n + 6) * U32 * (q.abs().t() @ (s * s))
    assert within_bound(ds.cpu(), r_ds, b_ds) and within_bound(dw2.cpu(), r_dw2, b_dw2), "demod_coefs_bwd: bound exceeded"
    assert not within_bound(ds.cpu(), 2 * s * (q[:, 8:] @ w2[8:]), b_ds), "the ds bound does not reject the sum without one 8-channel slab"


# ================================================================================================================ ToRGB

def torgb_fwd(dev, dtype, x, wmod, bias, clamp, want_code, what):
    n, hw, c = x.shape
    o = wmod.shape[1]
    y = torch.full((n, o, hw), float("nan"), device=dev)
    with expect_launch("torgb", lambda d: d[4] == 0 and d[5] == want_code, what):
        _lib.check(lib().sbg_torgb_fwd(P(dev_t(x, dtype, dev)), P(wmod.to(dev, F32)), P(None if bias is None else bias.to(dev, F32)), P(y), dcode(dtype),
                                       n, c, o, hw, clamp, S()), what)
    return y


def split3(w, dtype, scale):
    """the kernel's split of fp32 weights into three 16-bit parts (remainders scaled by 2^scale), returned as their fp64 values"""
    h = w.to(dtype).double()
    r1 = (w.double() - h) * 2.0 ** scale
    m = r1.float().to(dtype).double()
    r2 = (r1 - m) * 2.0 ** scale
    lo = r2.float().to(dtype).double()
    return h, m * 2.0 ** -scale, lo * 2.0 ** (-2 * scale)


def torgb_ref(x, wmod, bias, clamp):
    y = torch.einsum("npc,noc->nop", x, wmod)
    if bias is not None:
        y = y + bias[None, :, None]
    return y.clamp(-clamp, clamp) if clamp >= 0 else y


@pytest.mark.parametrize("c", [128, 256])
def test_torgb_fwd_mfma_bf16_exact(dev, c):
    """matrix-core forward, bf16: weights of 18 significant bits (|w| in [1/2, 1), grid 2^-18) so that all three bf16 parts are nonzero for most;
    x is +-1 on ~1/4 (C = 128) / ~1/8 (C = 256) of the channels, 0 elsewhere, so every sum stays below 2^24 grid steps"""
    gen = torch.Generator().manual_seed(90)
    n, o, hw = 2, 3, 32 * 48
    w = torch.zeros(n, o, c, dtype=torch.float64)
    todo = torch.ones(n, o, c, dtype=torch.bool)
    while bool(todo.any()):                             # draw until every weight has three nonzero parts
        k = int(todo.sum())
        w[todo] = torch.randint(1 << 17, 1 << 18, (k,), generator=gen).double() * 2.0 ** -18 * (torch.randint(0, 2, (k,), generator=gen) * 2 - 1)
        h, m, lo = split3(w.float(), BF, 0)
        todo = (m == 0) | (lo == 0)
    assert bool(((h + m + lo) == w).all())
    x = qint(gen, (n, hw, c), hi=1) * (torch.rand(n, hw, c, generator=gen, dtype=torch.float64) < (0.25 if c == 128 else 0.125))
    bias = qgrid(gen, (o,), -0.5, 0.5, 2.0 ** -18)
    nnz = float((x != 0).sum(2).max())
    assert_range(f"torgb C={c}", nnz * float(w.abs().max()) + float(bias.abs().max()), 18)
    for clamp in (-1.0, 8.0):
        y = torgb_fwd(dev, BF, x, w, bias, clamp, 1, f"torgb mfma bf16 C={c}")
        assert_exact(y, torgb_ref(x, w, bias, clamp), f"torgb mfma bf16 C={c} clamp={clamp}")


@pytest.mark.parametrize("dtype", [BF, F16], ids=str)
@pytest.mark.parametrize("c", [128, 256])
def test_torgb_fwd_mfma_split_one_hot(dev, dtype, c):
    """one nonzero x (+-1) per pixel: the output IS the weight, so the three-part split must reproduce every fp32 weight exactly.  Weights are
    random 24-bit fp32 values in [2^-12, 2^-1): for f16 the unscaled split would keep the second and third parts of every weight below ~2^-3 as
    f16 subnormals (quantum 2^-24: the split loses up to 2^-25 absolute); scaled by 2^11 and 2^22 the parts stay normal and the split is exact
    for 2^-14 <= |w| < 2^15.  For bf16 three parts cover 24 bits.  The test also shows it rejects a two-part split and, for f16, the unscaled one."""
    gen = torch.Generator().manual_seed(91)
    n, o, hw = 2, 3, 16 * 40
    e = torch.randint(-12, -1, (n, o, c), generator=gen).double()
    mant = 1 + torch.randint(0, 1 << 23, (n, o, c), generator=gen).double() * 2.0 ** -23
    w = (mant * torch.pow(2.0, e) * (torch.randint(0, 2, (n, o, c), generator=gen) * 2 - 1)).float().double()
    x = torch.zeros(n, hw, c, dtype=torch.float64)
    ch = torch.randint(0, c, (n, hw), generator=gen)
    x.scatter_(2, ch[:, :, None], qint(gen, (n, hw, 1), hi=1))
    y = torgb_fwd(dev, dtype, x, w, None, -1.0, 1, f"torgb mfma one-hot {dtype} C={c}")
    ref = torgb_ref(x, w, None, -1.0)
    assert_exact(y, ref, f"torgb mfma one-hot {dtype} C={c}")
    h, m, lo = split3(w.float(), dtype, 11 if dtype == F16 else 0)
    assert bool(((h + m + lo) == w).all())
    assert not torch.equal(torgb_ref(x, h + m, None, -1.0), ref), "a two-part split passes the one-hot test"
    if dtype == F16:
        hu, mu, lu = split3(w.float(), F16, 0)
        assert not torch.equal(torgb_ref(x, hu + mu + lu, None, -1.0), ref), "the unscaled f16 split passes the one-hot test"


def test_torgb_fwd_mfma_f16_bound(dev):
    """f16 forward on random data (x ~ randn in f16, weights log-uniform in [2^-12, 2^-1), bias randn).  The split is exact (one-hot test
    above), products of 16-bit parts are exact in fp32, so what remains is the fp32 accumulation of three accumulators over C terms and their
    combination (two power-of-two scalings, two additions) plus the bias:  |y - ref| <= (C + 4) U32 (sum_c |x w| + |b|).
    Rejection: the reference without one 8-channel slab of x."""
    gen = torch.Generator().manual_seed(92)
    n, o, c, hw = 2, 3, 128, 16 * 64
    e = torch.rand(n, o, c, generator=gen, dtype=torch.float64) * 11 - 12
    w = (torch.pow(2.0, e) * torch.sign(torch.randn(n, o, c, generator=gen, dtype=torch.float64))).float().double()
    x = torch.randn(n, hw, c, generator=gen, dtype=torch.float64).to(F16).double()
    b = torch.randn(o, generator=gen, dtype=torch.float64).float().double()
    y = torgb_fwd(dev, F16, x, w, b, -1.0, 1, "torgb mfma f16 bound")
    ref = torgb_ref(x, w, b, -1.0)
    bound = (c + 4) * U32 * (torch.einsum("npc,noc->nop", x.abs(), w.abs()) + b.abs()[None, :, None])
    assert within_bound(y.cpu(), ref, bound), f"torgb f16: bound exceeded by {float(((y.cpu().double() - ref).abs() - bound).max()):.3e}"
    xs = x.clone()
    xs[:, :, :8] = 0
    assert not within_bound(y.cpu(), torgb_ref(xs, w, b, -1.0), bound)


@pytest.mark.parametrize("dtype", [BF, F16], ids=str)
@pytest.mark.parametrize("c,o,hw,code", [(64, 3, 17 * 13, 2), (64, 4, 17 * 13, 3), (128, 1, 12 * 20 + 4, 2), (512, 2, 64, 2), (512, 4, 72, 3),
                                         (8, 4, 5 * 7, 3), (32, 3, 9 * 9, 2)])
def test_torgb_fwd_streaming_exact(dev, dtype, c, o, hw, code):
    """the streaming forward (NO = 3 for O <= 3, MAX_O for O = 4): lane sums by shuffles (C <= 64) or DPP rotates (C >= 128)"""
    gen = torch.Generator().manual_seed(93)
    n = 2
    w = qgrid(gen, (n, o, c), -2, 2, 2.0 ** -8)
    x = qint(gen, (n, hw, c), hi=2)
    b = qgrid(gen, (o,), -2, 2, 2.0 ** -8)
    assert_range("torgb streaming", 4 * c + 2, 8)
    y = torgb_fwd(dev, dtype, x, w, b, 64.0, code, f"torgb streaming C={c} O={o}")
    assert_exact(y, torgb_ref(x, w, b, 64.0), f"torgb streaming {dtype} C={c} O={o}")


@pytest.mark.parametrize("dtype", [BF, F16], ids=str)
@pytest.mark.parametrize("c,o", [(64, 3), (128, 4), (512, 1)])
def test_torgb_bwd_exact(dev, dtype, c, o):
    """dx = sum_o d1 wmod (16-bit, rounded once), per-block partials of d wmod = sum_p d1 x and db = sum_p d1 with blocks_per_n > 1; d1 = dy
    masked where the saved fp32 y sits on (or beyond) the rail, y planted with +-clamp and values just inside"""
    gen = torch.Generator().manual_seed(94)
    n, hw, clamp = 2, 64 * 64 + 37, 2.0
    nb = lib().sbg_torgb_bwd_blocks(n, c, hw)
    assert nb > 1
    x = qint(gen, (n, hw, c))
    w = qgrid(gen, (n, o, c), -2, 2, 2.0 ** -3)
    dy = qgrid(gen, (n, o, hw), -4, 4, 2.0 ** -2)
    y = plant(gen, qgrid(gen, (n, o, hw), -3, 3, 2.0 ** -4), torch.tensor([clamp, -clamp, clamp - 2.0 ** -20, -(clamp - 2.0 ** -20), 0.0, -0.0],
                                                                          dtype=torch.float64), frac=0.2)
    d1 = torch.where(y.abs() < clamp, dy, torch.zeros_like(dy))
    blk = (torch.arange(hw) // 256) % nb
    exact_sum_range("torgb dx", d1[:, :, None, :] * w[:, :, :, None], 1)
    assert_range("torgb dw", 8.0 * hw, 3)
    dx = torch.empty(n, hw, c, dtype=dtype, device=dev)
    part = torch.full((n, nb, o * c + o), float("nan"), device=dev)
    with expect_launch("torgb", lambda d: d[4] == 1, "torgb bwd"):
        _lib.check(lib().sbg_torgb_bwd(P(dev_t(x, dtype, dev)), P(w.to(dev, F32)), P(dy.to(dev, F32)), P(y.to(dev, F32)), P(dx), P(part), dcode(dtype),
                                       n, c, o, hw, clamp, S()), "torgb bwd")
    assert_exact(dx, torch.einsum("nop,noc->npc", d1, w), f"torgb bwd dx {dtype} C={c}")
    ref = torch.zeros(n, nb, o * c + o, dtype=torch.float64)
    for k in range(nb):
        sel = blk == k
        ref[:, k, :o * c] = torch.einsum("nop,npc->noc", d1[:, :, sel], x[:, sel]).reshape(n, -1)
        ref[:, k, o * c:] = d1[:, :, sel].sum(2)
    assert_exact(part, ref, f"torgb bwd partials {dtype} C={c}")


# ================================================================================================================ FromRGB

FROM_ACTS = {"lrelu": (LRELU, 0.25, 2.0), "relu": (RELU, 0.0, 2.0), "linear": (LINEAR, 0.0, 2.0)}


def fromrgb_fwd_ref(img, w, b, act, alpha, gain, clamp):
    """img [N, Ci, HW], w [Co, Ci] -> y [N, HW, Co]"""
    pre = torch.einsum("ncp,oc->npo", img, w) + (b[None, None, :] if b is not None else 0)
    z = {"lrelu": torch.where(pre > 0, pre, pre * alpha), "relu": pre.clamp(min=0), "linear": pre}[act] * gain
    return z.clamp(-clamp, clamp) if clamp >= 0 else z


def fromrgb_bwd_ref(img, w, dy, ys, act, alpha, gain, clamp32, nb):
    slope = where64(ys > 0, gain, {"lrelu": gain * alpha, "relu": 0.0, "linear": gain}[act])
    if clamp32 >= 0:
        slope = torch.where(ys.abs() < clamp32, slope, torch.zeros_like(slope))
    d1 = dy * slope
    n, hw, co = dy.shape
    ci = img.shape[1]
    blk = (torch.arange(hw) // 256) % nb
    part = torch.zeros(n, nb, co * ci + co, dtype=torch.float64)
    for k in range(nb):
        sel = blk == k
        part[:, k, :co * ci] = torch.einsum("npo,ncp->noc", d1[:, sel], img[:, :, sel]).reshape(n, -1)
        part[:, k, co * ci:] = d1[:, sel].sum(1)
    return d1, part, torch.einsum("npo,oc->ncp", d1, w)


def run_fromrgb(dev, dtype, img, w, b, dy, ys, act, alpha, gain, clamp, want_dimg, what):
    n, ci, hw = img.shape
    co = w.shape[0]
    actc = FROM_ACTS[act][0]
    y = torch.empty(n, hw, co, dtype=dtype, device=dev)
    with expect_launch("fromrgb", lambda d: d[4] == 0, what + " forward"):
        _lib.check(lib().sbg_fromrgb_fwd(P(img.to(dev, F32)), P(w.to(dev, F32)), P(None if b is None else b.to(dev, F32)), P(y), dcode(dtype), n, ci, co,
                                         hw, actc, alpha, gain, clamp, S()), what)
    if dy is None:
        return y, None, None, None
    nb = lib().sbg_fromrgb_bwd_blocks(n, hw)
    part = torch.full((n, nb, co * ci + co), float("nan"), device=dev)
    dimg = torch.full((n, ci, hw), float("nan"), device=dev) if want_dimg else None
    ci_code = 3 if ci == 3 else 4
    with expect_launch("fromrgb", lambda d: d[4] == 1 and d[5] == ci_code and d[6] == int(want_dimg), what + " backward"):
        _lib.check(lib().sbg_fromrgb_bwd(P(img.to(dev, F32)), P(w.to(dev, F32)), P(dev_t(dy, dtype, dev)), P(dev_t(ys, dtype, dev)), P(dimg), P(part),
                                         dcode(dtype), n, ci, co, hw, actc, alpha, gain, clamp, S()), what)
    return y, nb, part, dimg


@pytest.mark.parametrize("dtype", [BF, F16], ids=str)
@pytest.mark.parametrize("ci,co,act", [(3, 128, "lrelu"), (3, 32, "relu"), (1, 64, "linear"), (4, 8, "lrelu"), (2, 512, "lrelu")])
def test_fromrgb_exact(dev, dtype, ci, co, act):
    """forward (rounded once to 16 bits) and backward (dw / db per-block partials, dimg) bit for bit, CI = 3 and the generic instantiation,
    DIMG on and off; saved y planted with +-clamp, one ulp inside, 0 and -0 (clamp 8)"""
    gen = torch.Generator().manual_seed(100)
    n, hw, clamp = 2, 64 * 64 + 19, 8.0
    _, alpha, gain = FROM_ACTS[act]
    img = qgrid(gen, (n, ci, hw), -2, 2, 2.0 ** -4)
    w = qgrid(gen, (co, ci), -1, 1, 2.0 ** -3)
    b = qgrid(gen, (co,), -1, 1, 2.0 ** -3) + 2.0 ** -8
    dy = qint(gen, (n, hw, co), hi=1)
    ys = plant(gen, fromrgb_fwd_ref(img, w, b, act, alpha, gain, clamp), rail_values(dtype, clamp)).to(dtype).double()
    for want_dimg in (True, False):
        what = f"fromrgb {dtype} Ci={ci} Co={co} {act} dimg={want_dimg}"
        y, nb, part, dimg = run_fromrgb(dev, dtype, img, w, b, dy, ys, act, alpha, gain, clamp, want_dimg, what)
        assert nb > 1
        assert_exact(y, fromrgb_fwd_ref(img, w, b, act, alpha, gain, clamp), what + " y")
        d1, rpart, rdimg = fromrgb_bwd_ref(img, w, dy, ys, act, alpha, gain, clamp, nb)
        assert_range(what, 2.0 * 2 * 256 * 8, 5)
        assert_exact(part, rpart, what + " partials")
        if want_dimg:
            assert_exact(dimg, rdimg, what + " dimg")


@pytest.mark.parametrize("dtype", [BF, F16], ids=str)
@pytest.mark.parametrize("clamp", NONREP_CLAMPS)
def test_fromrgb_nonrepresentable_clamp(dev, dtype, clamp):
    """the backward's rail test compares the saved 16-bit y with the fp32 clamp, as the reference and the generic bias_act do: with clamp 0.7 in
    bf16 the stored rail 0.69921875 lies below the clamp and its gradient passes; with 0.71 the stored rail 0.7109375 is beyond it"""
    gen = torch.Generator().manual_seed(101)
    n, ci, co, hw = 2, 3, 64, 32 * 32
    img = qgrid(gen, (n, ci, hw), -1, 1, 2.0 ** -4)
    w = qgrid(gen, (co, ci), -1, 1, 2.0 ** -3)
    b = qgrid(gen, (co,), -0.5, 0.5, 2.0 ** -3) + 2.0 ** -8
    ys = plant(gen, fromrgb_fwd_ref(img, w, b, "lrelu", 0.25, 2.0, clamp), rail_values(dtype, clamp), frac=0.2).to(dtype).double()
    dy = qint(gen, (n, hw, co), hi=1)
    y, nb, part, dimg = run_fromrgb(dev, dtype, img, w, b, dy, ys, "lrelu", 0.25, 2.0, clamp, True, f"fromrgb clamp {clamp}")
    assert_exact(y, fromrgb_fwd_ref(img, w, b, "lrelu", 0.25, 2.0, float(np.float32(clamp))), f"fromrgb forward clamp {clamp} {dtype}")
    _, rpart, rdimg = fromrgb_bwd_ref(img, w, dy, ys, "lrelu", 0.25, 2.0, float(np.float32(clamp)), nb)
    assert_exact(part, rpart, f"fromrgb partials clamp {clamp} {dtype}")
    assert_exact(dimg, rdimg, f"fromrgb dimg clamp {clamp} {dtype}")


def test_fromrgb_bound_real_constants(dev):
    """alpha 0.2, gain sqrt 2, clamp 256, fp32 randn image / weights / bias, bf16 output and dy.  Forward, M = |b| + sum_c |img w|:
      pre: Ci FMAs (<= (Ci + 1) U32 M), lrelu x fl(alpha) and x fl(gain) (<= 4 U32 more, relative), a kink flip moves y by <= gain (1 + alpha)
      times the pre error; rounding to bf16 once: |y - ref| <= U_OUT |ref| + (1 + U_OUT) gain (1 + alpha) (Ci + 6) U32 M.
    Backward from the saved y: d1 = dy * fl(gain * alpha) (<= 3 U32 |d1|); a block's partial over its P pixels: <= (P + 3) U32 sum |d1 img|
    (dw) and (P + 3) U32 sum |d1| (db).  Rejection: the forward reference with image channel 2 dropped, the partials without the last row."""
    gen = torch.Generator().manual_seed(102)
    n, ci, co, r = 2, 3, 128, 64
    hw = r * r
    alpha, gain, clamp = 0.2, math.sqrt(2), 256.0
    img = torch.randn(n, ci, hw, generator=gen, dtype=torch.float64).float().double()
    w = (torch.randn(co, ci, generator=gen, dtype=torch.float64) * 40).float().double()
    b = torch.randn(co, generator=gen, dtype=torch.float64).float().double()
    dy = torch.randn(n, hw, co, generator=gen, dtype=torch.float64).to(BF).double()
    ref = fromrgb_fwd_ref(img, w, b, "lrelu", alpha, gain, clamp)
    assert bool((ref.abs() == clamp).any())
    ys = ref.to(BF).double()
    y, nb, part, _ = run_fromrgb(dev, BF, img, w, b, dy, ys, "lrelu", alpha, gain, clamp, False, "fromrgb bound")
    M = b.abs()[None, None, :] + torch.einsum("ncp,oc->npo", img.abs(), w.abs())
    bound = U_OUT[BF] * ref.abs() + (1 + U_OUT[BF]) * gain * (1 + alpha) * (ci + 6) * U32 * M
    assert within_bound(y.cpu(), ref, bound), f"fromrgb forward: bound exceeded by {float(((y.cpu().double() - ref).abs() - bound).max()):.3e}"
    img2 = img.clone()
    img2[:, 2] = 0
    assert not within_bound(y.cpu(), fromrgb_fwd_ref(img2, w, b, "lrelu", alpha, gain, clamp), bound)
    d1, rpart, _ = fromrgb_bwd_ref(img, w, dy, ys, "lrelu", alpha, gain, clamp, nb)
    pblk = int(math.ceil(hw / 256 / nb)) * 256
    absd = fromrgb_bwd_ref(img.abs(), w, dy.abs(), ys, "lrelu", alpha, gain, clamp, nb)[1].abs()
    pbound = (pblk + 3) * U32 * absd
    assert within_bound(part.cpu(), rpart, pbound), f"fromrgb partials: bound exceeded by {float(((part.cpu().double() - rpart).abs() - pbound).max()):.3e}"
    dy2 = dy.clone()
    dy2[:, hw - r:] = 0
    assert not within_bound(part.cpu(), fromrgb_bwd_ref(img, w, dy2, ys, "lrelu", alpha, gain, clamp, nb)[1], pbound)
