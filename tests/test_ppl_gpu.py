"""Perceptual path length on the device: the three HIP kernels of csrc/ppl.hip against exact or bounded references, the sampler end to end
against the reference's PPLSampler (tests/golden/ppl.npz), and compute_ppl at the sg2ada 256x256 widths.  The launch log (kind 'ppl',
dims[0] = variant) shows which kernel served each case."""
import contextlib
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: F401
from style_big_gan_amd import _lib
from style_big_gan_amd.metrics import metric_utils
from style_big_gan_amd.metrics import perceptual_path_length as ppl
from style_big_gan_amd.torch_utils.ops import ppl as ppl_ops
from style_big_gan_amd.torch_utils.ops import projector as proj_ops
from style_big_gan_amd.torch_utils.ops._exact_common import NT, block_sum_np, fma32, strided_sum_np
from golden_util import make_image_folder
import ppl_util

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
EPS = 1e-4


@contextlib.contextmanager
def launch_log():
    """collects the 'ppl' launches of the block: list of variant names"""
    _lib.prof_enable(True)
    _lib.prof_fetch()
    seen = []
    try:
        yield seen
        torch.cuda.synchronize()
    finally:
        recs = _lib.prof_fetch()
        _lib.prof_enable(False)
        seen.extend(_lib.PPL_VARIANTS[r["dims"][0]] for r in recs if r["kind"] == "ppl")


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------- image prep

@pytest.mark.parametrize("crop", [True, False])
@pytest.mark.parametrize("factor", [1, 2, 4])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("channels_last", [False, True])
def test_prep_exact(dev, crop, factor, C, channels_last):
    """dyadic inputs k / 64 in [-1, 1]: every box sum (<= 16 terms) is exact in fp32, so is the mean (factor^2 is a power of two) and m + 1;
    only (m + 1) * 127.5 rounds.  The kernel's result must equal the fp64 reference rounded once, bit for bit, in either memory format"""
    gen = torch.Generator().manual_seed(31 + factor + 10 * C)
    N, H = 4, 32
    x64 = torch.randint(-64, 65, [N, C, H, H], generator=gen).to(torch.float64) / 64
    ref = x64
    if crop:
        c = H // 8
        ref = ref[:, :, 3 * c:7 * c, 2 * c:6 * c]
    if factor > 1:
        ref = ref.reshape(N, C, ref.shape[2] // factor, factor, ref.shape[3] // factor, factor).mean([3, 5])
    ref = ((ref + 1) * 127.5).to(torch.float32)
    if C == 1:
        ref = ref.repeat([1, 3, 1, 1])
    x = x64.to(torch.float32).to(dev)
    if channels_last:
        x = x.contiguous(memory_format=torch.channels_last)
    with launch_log() as seen:
        out = ppl_ops.prep_images(x, crop=crop, factor=factor)
    assert seen == ["prep"]
    assert out.is_contiguous() and out.shape == ref.shape
    assert torch.equal(bits(out), bits(ref))


def test_prep_rejects_window_not_split_into_boxes(dev):
    x = torch.zeros([2, 3, 24, 24], device=dev)
    with pytest.raises(RuntimeError, match="boxes"):
        ppl_ops.prep_images(x, crop=True, factor=8)       # 12 x 12 window, 8 x 8 boxes


# ---------------------------------------------------------------------------------------------------------------- distance

@pytest.mark.parametrize("B,F", [(1, 1000), (2, 8192), (2, 8192 * 9 + 3), (3, 4099), (2, 8192 * 7 + 4)])
def test_distance_exact_and_reproducible(dev, B, F):
    """small-integer operands in [-3, 3]: every square and every partial sum is an integer below 2^24 (asserted), so the fp32 sum is exact in
    any order; the result must be that sum divided as the reference divides (fp32 sum / fp32(eps^2)), bit for bit.  F inside one chunk
    (8192 elements), across many chunks, and not a multiple of the vector width (scalar path)"""
    gen = torch.Generator().manual_seed(F)
    a = torch.randint(-3, 4, [2 * B, F], generator=gen).to(torch.float32)
    exact = (a[:B].to(torch.int64) - a[B:].to(torch.int64)).square().sum(1)
    assert int(exact.max()) < 2 ** 24
    ref = torch.from_numpy(exact.numpy().astype(np.float32) / np.float32(EPS ** 2))
    x = a.to(dev)
    with launch_log() as seen:
        d1 = ppl_ops.lpips_distance(x, EPS)
        d2 = ppl_ops.lpips_distance(x, EPS)
    assert seen == ["dist", "dist"]
    assert torch.equal(bits(d1), bits(ref)) and torch.equal(bits(d1), bits(d2))


def test_distance_same_on_every_run(dev):
    """real-valued features (not exact): two launches agree bit for bit (fixed-order reduction, no float atomics)"""
    x = torch.randn([4, 3 * 8192 * 5 + 17], generator=torch.Generator().manual_seed(5)).to(dev)
    d = [ppl_ops.lpips_distance(x, EPS) for _ in range(3)]
    assert torch.equal(bits(d[0]), bits(d[1])) and torch.equal(bits(d[0]), bits(d[2]))
    ref = (x[:2].double() - x[2:].double()).square().sum(1) / EPS ** 2
    assert torch.allclose(d[0].double(), ref, rtol=1e-5)


def _sqdist_np(a, b, div, fma_tail):
    """csrc/sqdist.h + csrc/merge.h in numpy float32 for rows a, b [B, F] (16-byte aligned rows when F % 4 == 0).  A chunk is 8192 features
    of a row.  Vector path (F % 4 == 0): lane t of 256 adds the squares of its float4 k = 0..7 at 4 (256 k + t), the four components in
    index order.  Scalar path: lane t adds the features 256 k + t, k = 0..31 -- by fmaf on the path-length side (fma_tail), as a rounded
    square otherwise.  block_sum adds the lanes; the chunk sums are added lane-strided, then block_sum; one division.  A feature behind
    the row's end is a zero here and skipped on the device: s + 0 and fmaf(0, 0, s) are s."""
    B, F = a.shape
    nchunk = -(-F // 8192)
    d = np.zeros([B, nchunk * 8192], dtype=np.float32)
    d[:, :F] = a - b
    acc = np.zeros([B, nchunk, NT], dtype=np.float32)
    if F % 4 == 0:
        d2 = (d * d).reshape(B, nchunk, 8, NT, 4)
        for k in range(8):
            for q in range(4):
                acc = acc + d2[:, :, k, :, q]
    else:
        d = d.reshape(B, nchunk, 32, NT)
        for k in range(32):
            acc = fma32(d[:, :, k], d[:, :, k], acc) if fma_tail else acc + d[:, :, k] * d[:, :, k]
    out = strided_sum_np(block_sum_np(acc)) / np.float32(div)
    assert out.dtype == np.float32
    return out


@pytest.mark.parametrize("B,F", [(2, 8192 * 3 + 4), (3, 4099), (2, 257 * 8192 + 3)])
def test_distance_float_order_is_the_numpy_restatement(dev, B, F):
    """random fp32 features: every sum rounds, so only the order of csrc/sqdist.h and of the shared merge kernel gives these bits.  The
    vector path, the scalar path (fmaf for the path length, rounded squares for the projector), and 258 partials per row: a lane of the
    merge adds two of them"""
    x = torch.randn([2 * B, F], generator=torch.Generator().manual_seed(F)) * 3
    xn = x.numpy()
    got = ppl_ops.lpips_distance(x.to(dev), EPS)
    assert torch.equal(bits(got), bits(torch.from_numpy(_sqdist_np(xn[:B], xn[B:], EPS ** 2, True))))
    t, s = x[:1].clone().to(dev), x[B:B + 1].clone().to(dev)
    got = proj_ops.sqdist(t, s).reshape(1)
    assert torch.equal(bits(got), bits(torch.from_numpy(_sqdist_np(xn[:1], xn[B:B + 1], 1.0, False))))


# ---------------------------------------------------------------------------------------------------------------- endpoints

@pytest.mark.parametrize("shape", [(4, 14, 512), (4, 3, 7)])
def test_lerp_endpoints_bit_equal_to_torch_lerp(dev, shape):
    """w space: bit-equal to torch.lerp on the device; t covers both of its branches (|w| < 0.5 and >= 0.5), and t + eps crosses 0.5 for
    one sample.  (4, 3, 7): rows not a multiple of the vector width (scalar path)"""
    gen = torch.Generator().manual_seed(11)
    B = shape[0]
    w0 = torch.randn(shape, generator=gen).to(dev)
    w1 = torch.randn(shape, generator=gen).to(dev)
    t = torch.tensor([0.1, 0.49995, 0.5, 0.9], dtype=torch.float32)[:B].to(dev)
    tb = t.reshape(B, 1, 1)
    ref = torch.cat([w0.lerp(w1, tb), w0.lerp(w1, tb + EPS)])
    with launch_log() as seen:
        out = ppl_ops.lerp_endpoints(w0, w1, t, EPS)
    assert seen == ["lerp"]
    assert torch.equal(bits(out), bits(ref))


@pytest.mark.parametrize("B,D", [(2, 512), (3, 16), (2, 100)])
def test_slerp_endpoints_within_ulp_bound(dev, B, D):
    """z space against the fp64 slerp of the same fp32 inputs (t and the fp32 value of t + eps).  Bound, in units of u = 2^-24 of the unit
    result: every norm / dot product is a sum of k = ceil(D / 64) + 6 terms (lane-strided, then a 6-level butterfly), relative error <= k u;
    the chain normalise a and b -> d -> acos -> c = b - d a -> normalise c -> a cos p + c sin p -> normalise has five such reductions plus a
    few ulp from acos / sin / cos and the divisions: |out - out64| <= (8 k + 16) u per element."""
    gen = torch.Generator().manual_seed(D)
    z0 = torch.randn([B, D], generator=gen)
    z1 = torch.randn([B, D], generator=gen)
    t = torch.rand([B], generator=gen)
    t1 = (t + EPS).to(torch.float32)
    ref = torch.cat([ppl_ops.slerp(z0.double(), z1.double(), t.double().unsqueeze(1)),
                     ppl_ops.slerp(z0.double(), z1.double(), t1.double().unsqueeze(1))])
    with launch_log() as seen:
        out = ppl_ops.slerp_endpoints(z0.to(dev), z1.to(dev), t.to(dev), EPS)
    assert seen == ["slerp"]
    k = -(-D // 64) + 6
    err = (out.double().cpu() - ref).abs().max().item()
    assert err <= (8 * k + 16) * U32, err


# ---------------------------------------------------------------------------------------------------------------- end to end

_G = ppl_util.fixture()
_CASES = _G.meta["cases"]


def _run_case(g, case, dev, shift_row=False, bf16=False):
    """the fixture case on the device: the package's generator with the fixture's weights, the stand-in LPIPS, the replayed draws; returns
    (per-pair dist [batches * 2], variants logged per batch)"""
    G = ppl_util.product_generator(g, case["G"], dev)
    sampler = ppl.PPLSampler(G=G, G_kwargs={}, epsilon=g.meta["epsilon"], space=case["space"], sampling=case["sampling"], crop=case["crop"],
                             vgg16=ppl_util.StandInLPIPS(g), vgg16_kwargs={}).eval().requires_grad_(False).to(dev)
    names = [n[len("G."):] for n, _ in sampler.named_buffers() if n.endswith(".noise_const")]
    assert sorted(names) == sorted(case["noise_names"])
    if bf16:        # control: the synthesis runs its configured bf16 blocks (force_fp32 dropped)
        synth = sampler.G.synthesis
        fwd = synth.forward
        synth.forward = lambda ws, force_fp32=False, **kw: fwd(ws, **kw).float()
    prep = ppl_ops.prep_images
    out, logs = [], []
    try:
        if shift_row:   # control: the crop window one row lower
            ppl.ppl_ops.prep_images = lambda img, crop, factor: prep(torch.roll(img, -1, dims=2), crop, factor)
        for bi in range(len(case["batches"])):
            draws = ppl_util.batch_draws(g, case, bi, names)
            draws = dict(draws, noise=[v.to(dev) for v in draws["noise"]])
            with launch_log() as seen, torch.no_grad():
                out.append(sampler(g.t(f"{case['key']}/b{bi}/c").to(dev), draws=draws).cpu())
            logs.append(seen)
    finally:
        ppl.ppl_ops.prep_images = prep
    return torch.cat(out), logs


def _ref(g, case):
    return torch.cat([g.t(f"{case['key']}/b{bi}/dist") for bi in range(len(case["batches"]))])


def _rel(d, ref):
    return ((d.double() - ref.double()).abs() / ref.double().abs()).max().item()


@pytest.mark.parametrize("case", _CASES, ids=[f"{c['G']}-{c['space']}-{c['sampling']}-{'crop' if c['crop'] else 'nocrop'}" for c in _CASES])
def test_sampler_end_to_end_matches_reference(dev, case):
    """fp32 synthesis through the HIP path (force_fp32), the three ppl kernels, the stand-in LPIPS: per-pair distances within
    ppl_util.REL_BOUND (2e-2; derivation there: independent fp32 rounding of the two endpoints' images, amplified by 1 / eps^2) of the
    reference's.  Two batches per case: the second batch's noise must reach every synthesis layer."""
    d, logs = _run_case(_G, case, dev)
    endpoint = "slerp" if case["space"] == "z" else "lerp"
    for seen in logs:
        assert seen == [endpoint, "prep", "dist"], seen
    rel = _rel(d, _ref(_G, case))
    assert rel < ppl_util.REL_BOUND, (d, _ref(_G, case), rel)


@pytest.mark.parametrize("control", ["bf16", "shift_row"])
def test_bound_rejects_bf16_synthesis_and_shifted_crop(dev, control):
    """the end-to-end bound is tight enough to see a bf16 synthesis (force_fp32 ignored) and a crop window one row off, at 16x16"""
    case = next(c for c in _CASES if c["G"] == "g16c0" and c["crop"])
    d, _ = _run_case(_G, case, dev, bf16=(control == "bf16"), shift_row=(control == "shift_row"))
    assert _rel(d, _ref(_G, case)) > ppl_util.REL_BOUND


# ---------------------------------------------------------------------------------------------------------------- headline width

def test_compute_ppl_sg2ada_256(dev, tmp_path):
    """compute_ppl (ppl_wend's parameters, num_samples 64, batch 2) on a randomly initialised generator at the sg2ada 256x256 widths
    (z = w = 512, 2 mapping layers, channel_base 32768, conv_clamp 256) with the stand-in LPIPS: finite and positive, and every iteration
    ran the three ppl kernels"""
    from style_big_gan_amd.train_parts.generators import generators
    torch.manual_seed(0)
    G = generators["sg2_classic"](z_dim=512, c_dim=0, w_dim=512, img_resolution=256, img_channels=3, mapping_kwargs=dict(num_layers=2),
                                  synthesis_kwargs=dict(channel_base=32768, num_fp16_res=4, block_kwargs=dict(conv_clamp=256))).eval()
    path = make_image_folder(str(tmp_path / "data"), n=4, res=16)
    opts = metric_utils.MetricOptions(G=G, dataset_kwargs=dict(path=path), num_gpus=1, rank=0, device=dev, cache=False,
                                      detector=ppl_util.StandInLPIPS(_G).to(dev))
    with launch_log() as seen:
        value = ppl.compute_ppl(opts, num_samples=64, epsilon=1e-4, space="w", sampling="end", crop=True, batch_size=2)
    assert np.isfinite(value) and value > 0
    assert seen == ["lerp", "prep", "dist"] * 32
