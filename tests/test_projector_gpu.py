"""Latent projector on the device: the HIP kernels of csrc/projector.hip against exact fp64 references (tests/projector_exact.py),
run-to-run identity, batch-1 generator gradients against the CPU oracle, project() end to end against the reference's own project()
(tests/golden/projector.npz), the launch budget of one projection step, and the CLI end to end.  The launch log (kind 'projector',
dims[0] = variant, one record per launch) shows which kernels ran."""
import contextlib
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: F401
from style_big_gan_amd import _lib, projector
from style_big_gan_amd.torch_utils.ops import projector as proj_ops
import ppl_util
import projector_exact as pe
import projector_util as pu

pytestmark = pytest.mark.gpu

U32 = 2.0 ** -24
SG2ADA_256 = [4, 8, 8, 16, 16, 32, 32, 64, 64, 128, 128, 256, 256]
SETS = {"sg2ada256": SG2ADA_256, "single4": [4], "single1024": [1024], "mix": [64, 4, 1024, 16, 8, 256, 32, 512]}


@contextlib.contextmanager
def launch_log():
    """collects every launch of the block: list of (kind, variant name or None)"""
    _lib.prof_enable(True)
    _lib.prof_fetch()
    seen = []
    try:
        yield seen
        torch.cuda.synchronize()
    finally:
        recs = _lib.prof_fetch()
        _lib.prof_enable(False)
        seen.extend((r["kind"], _lib.PROJ_VARIANTS[r["dims"][0]] if r["kind"] == "projector" else None) for r in recs)


def proj_counts(seen):
    out = {}
    for kind, v in seen:
        if kind == "projector":
            out[v] = out.get(v, 0) + 1
    return out


def bits(x):
    return x.detach().cpu().contiguous().view(torch.int32)


def exact_set(name, seed=11):
    """blocky buffers, and spiky ones at odd positions up to 256x256 (a single 4x4 is spiky): see projector_exact"""
    gen = torch.Generator().manual_seed(seed)
    sizes = SETS[name]
    if sizes == [4]:
        return [pe.spiky(gen, 4)]
    return [(pe.spiky if i % 2 == 1 and r <= 256 else pe.blocky)(gen, r) for i, r in enumerate(sizes)]


# ---------------------------------------------------------------------------------------------------------------- regulariser

@pytest.mark.parametrize("name", list(SETS))
def test_noise_reg_exact(dev, name):
    """every pooled value, product, product sum, mean and square is an fp32 value (asserted by pe.reference first), so the means and
    the gradients must equal the fp64 reference bit for bit, and reg the in-order fp32 sum of the exact squares"""
    bufs64 = exact_set(name)
    g = 0.75
    ref_means, ref_reg, ref_grads = pe.reference(bufs64, g=g)
    assert int((ref_means != 0).sum()) >= 1
    bufs = [b.float().to(dev).requires_grad_(True) for b in bufs64]
    with launch_log() as seen:
        means = proj_ops.noise_means(bufs)
    assert proj_counts(seen) == {"reg": 3 if max(SETS[name]) > 8 else 2}
    assert torch.equal(bits(means), bits(ref_means.float()))
    with launch_log() as seen:
        reg = proj_ops.noise_reg(bufs)
        (reg * g).backward()
    assert proj_counts(seen) == {"reg": 3 if max(SETS[name]) > 8 else 2, "reg_bwd": 1}
    assert float(reg) == ref_reg
    for b, r in zip(bufs, ref_grads):
        assert torch.equal(bits(b.grad), bits(r.float()))


def test_noise_reg_is_the_reference_formula_on_normal_noise(dev):
    """unit normals (not exact): the kernels against the reference's torch composition on the device, relative to the terms' scale"""
    gen = torch.Generator().manual_seed(12)
    bufs = [torch.randn([r, r], generator=gen).to(dev).requires_grad_(True) for r in SG2ADA_256]
    ref_bufs = [b.detach().clone().requires_grad_(True) for b in bufs]
    reg = proj_ops.noise_reg(bufs)
    reg.backward()
    ref = proj_ops.noise_reg_reference(ref_bufs)
    ref.backward()
    # each mean sums n^2 products of magnitude ~1 in another order: |d m| <= ~log2(n^2) u max|P|^2 ~ 20 * 6e-8 = 1.2e-6, against means of
    # ~1 / n (unit normals: the products are uncorrelated), so the squares and their sum move by <= ~2.4e-6 * n ~ 1e-4 relative at
    # n = 64 .. 256 in the worst case; the gradients inherit the same relative error through m
    assert abs(float(reg) - float(ref)) <= 1e-4 * float(ref)
    for b, r in zip(bufs, ref_bufs):
        assert float((b.grad - r.grad).abs().max()) <= 1e-4 * float(r.grad.abs().max())


def test_noise_kernels_are_deterministic(dev):
    gen = torch.Generator().manual_seed(13)
    bufs = [torch.randn([r, r], generator=gen).to(dev) for r in SETS["mix"]]
    runs = []
    for _ in range(2):
        bb = [b.clone().requires_grad_(True) for b in bufs]
        reg = proj_ops.noise_reg(bb)
        reg.backward()
        means = proj_ops.noise_means(bb)
        nb = [b.detach().clone() for b in bb]
        proj_ops.noise_normalize_(nb)
        runs.append([bits(reg), bits(means)] + [bits(b.grad) for b in bb] + [bits(b) for b in nb])
    assert all(torch.equal(a, b) for a, b in zip(*runs))


@pytest.mark.parametrize("bad", [[12], [2], [2048], [16, 6]])
def test_noise_reg_rejects_unsupported_sides(dev, bad):
    bufs = [torch.zeros([r, r], device=dev) for r in bad]
    with pytest.raises(RuntimeError, match="power of two"):
        proj_ops.noise_reg(bufs)
    with pytest.raises(RuntimeError, match="power of two"):
        proj_ops.noise_normalize_(bufs)


def test_noise_ops_reject_non_square_or_wrong_dtype(dev):
    with pytest.raises(RuntimeError, match="square float32"):
        proj_ops.noise_reg([torch.zeros([8, 16], device=dev)])
    with pytest.raises(RuntimeError, match="square float32"):
        proj_ops.noise_normalize_([torch.zeros([8, 8], device=dev, dtype=torch.float64)])


# ---------------------------------------------------------------------------------------------------------------- renormalisation

@pytest.mark.parametrize("name", list(SETS))
def test_noise_normalize_bound(dev, name):
    """buf = 1/2 + x - flip(x) with x blocky / spiky: the sum is exactly R^2 / 2, so the mean is 1/2, the centred values x - flip(x) are
    small integers, their squares and every order of their sum are exact (asserted), and v = mean(c^2) is the fp64 value.  Only rsqrt
    and the final product round.  HIP documents rsqrtf within 1 ulp (relative 2^-23); allowing 2 ulps for the hardware reciprocal
    square root, plus half an ulp (2^-24) for the product: |out - c / sqrt(v)| <= (2^-22 + 2^-24 + 2^-45) |c / sqrt(v)| per element"""
    bufs64 = [0.5 + x - x.flip(0) for x in exact_set(name, seed=14)]
    refs = []
    for b in bufs64:
        mean = b.mean()
        c = b - mean
        assert float(mean) == 0.5 and pe._exact32(c) and pe._any_order_exact(b) and pe._any_order_exact(c * c) and float((c * c).sum()) > 0
        refs.append(c / (c * c).mean().sqrt())
    bufs = [b.float().to(dev) for b in bufs64]
    with launch_log() as seen:
        proj_ops.noise_normalize_(bufs)
    assert proj_counts(seen) == {"normalize": 2}
    bound = 2.0 ** -22 + 2.0 ** -24 + 2.0 ** -45
    for b, r in zip(bufs, refs):
        err = (b.double().cpu() - r).abs()
        assert bool((err <= bound * r.abs()).all()), float((err / r.abs().clamp_min(1e-30)).max())


@pytest.mark.parametrize("side", [64, 128])
def test_noise_normalize_counts_every_wave_once(dev, side):
    """a +-1 checkerboard: the mean is exactly 0 and the sum of squares exactly R^2 in any order, so the scale is rsqrt(1).  At side 64
    each of the 16 waves of the second stage's 1024-wide workgroup contributes exactly one float4 per lane, at 128 four.  Every element
    must keep its sign and have one common magnitude within 1 ulp of 1 (2^-23: HIP documents rsqrtf within 1 ulp, and +-1 times the
    scale is exact); a dropped or double-counted wave scales by sqrt(16 / 15) or sqrt(16 / 17), ~3 % off"""
    i = torch.arange(side)
    board = (1.0 - 2.0 * ((i[:, None] + i[None, :]) % 2)).float()
    buf = board.to(dev)
    proj_ops.noise_normalize_([buf])
    out = buf.cpu()
    mags = out.abs().unique()
    assert mags.numel() == 1, mags
    assert abs(float(mags[0]) - 1.0) <= 2.0 ** -23, float(mags[0])
    assert torch.equal(out.sign(), board)


# ---------------------------------------------------------------------------------------------------------------- LPIPS distance

@pytest.mark.parametrize("F_", [1, 1000, 3 * 8192 + 5, 8 * 1024 * 1024 - 4, 8_016_000])
def test_sqdist_exact(dev, F_):
    """dyadic features k / 64 with |k| <= 16 on at most 4000 positions, zero elsewhere: every difference and square is exact, and the
    squares are multiples of 2^-12 whose sum stays below 2^24 * 2^-12 (asserted), so every summation order is exact.  The distance must
    equal the fp64 sum, and the gradient with a dyadic g, 2 g (s - t), the fp64 value"""
    gen = torch.Generator().manual_seed(15 + F_ % 97)
    t64 = torch.zeros([1, F_], dtype=torch.float64)
    s64 = torch.zeros([1, F_], dtype=torch.float64)
    nz = min(F_, 4000)
    idx = torch.randperm(F_, generator=gen)[:nz] if F_ <= 1 << 24 else torch.randint(0, F_, [nz], generator=gen)
    t64[0, idx] = torch.randint(-16, 17, [nz], generator=gen).double() / 64
    s64[0, idx] = torch.randint(-16, 17, [nz], generator=gen).double() / 64
    d2 = (t64 - s64).square()
    assert pe._exact32(t64 - s64) and pe._exact32(d2) and pe._any_order_exact(d2)
    ref = d2.sum()
    g = 0.375
    ref_ds = 2 * g * (s64 - t64)
    t, s = t64.float().to(dev), s64.float().to(dev).requires_grad_(True)
    with launch_log() as seen:
        d = proj_ops.sqdist(t, s)
        (d * g).backward()
    assert proj_counts(seen) == {"sqdist": 2, "sqdist_bwd": 1}
    assert float(d) == float(ref)
    assert torch.equal(bits(s.grad), bits(ref_ds.float()))
    d2nd = proj_ops.sqdist(t, s.detach())
    assert torch.equal(bits(d), bits(d2nd))


def test_sqdist_rejects_operands_on_different_devices(dev):
    """a host tensor next to a device one is an error before any kernel sees its pointer, in either position"""
    t, s = torch.zeros([1, 64]), torch.zeros([1, 64], device=dev)
    with pytest.raises(RuntimeError, match="same device"):
        proj_ops.sqdist(t, s)
    with pytest.raises(RuntimeError, match="same device"):
        proj_ops.sqdist(s, t)


def test_noise_ops_reject_buffers_on_different_devices(dev):
    for bufs in ([torch.zeros([8, 8], device=dev), torch.zeros([16, 16])], [torch.zeros([8, 8]), torch.zeros([16, 16], device=dev)]):
        with pytest.raises(RuntimeError, match="same device"):
            proj_ops.noise_reg(bufs)
        with pytest.raises(RuntimeError, match="same device"):
            proj_ops.noise_means(bufs)
        with pytest.raises(RuntimeError, match="same device"):
            proj_ops.noise_normalize_(bufs)


def test_sqdist_gradient_is_autograd_of_the_reference(dev):
    """the backward is the value autograd gives (t - s).square().sum() for s, bit for bit, on normal features"""
    gen = torch.Generator().manual_seed(16)
    t = torch.randn([1, 10000], generator=gen).to(dev)
    s = torch.randn([1, 10000], generator=gen).to(dev).requires_grad_(True)
    s2 = s.detach().clone().requires_grad_(True)
    (proj_ops.sqdist(t, s) * 3.0).backward()
    ((t - s2).square().sum() * 3.0).backward()
    assert torch.equal(bits(s.grad), bits(s2.grad))


# ---------------------------------------------------------------------------------------------------------------- generator gradients

@pytest.mark.parametrize("tag", ["g16", "g32"])
def test_batch1_gradients_match_the_oracle(dev, tag):
    """d <img, R> / d ws and / d noise_const at N = 1 with frozen weights, device generator against the CPU oracle on the same weights
    and buffers.  Both are fp32 with different op orders: each layer's outputs carry ~sqrt(K) u relative rounding (K = C * 9 terms per
    convolution, <= 144 here; u = 2^-24), the backward chain of ~2 L layers (L <= 5 resolutions) adds them, so the gradient's max error
    relative to its max is ~2 L sqrt(K) u ~ 10 * 12 * 6e-8 ~ 7e-6.  Bound: 1e-4 (a missing noise_strength factor or a
    dropped layer is off by O(1))."""
    g = pu.fixture()
    c = pu.case(g, tag)
    G = pu.product_generator(g, c, dev)
    O = pu.oracle_generator(g, c)
    noise = pu.draws(g, c)["noise"]
    nd, no = list(projector.noise_buffers(G).values()), list(projector.noise_buffers(O).values())
    for a, b, v in zip(nd, no, noise):
        a.copy_(v)
        b.copy_(v)
        a.requires_grad_(True)
        b.requires_grad_(True)
    gen = torch.Generator().manual_seed(17)
    ws = torch.randn([1, c["num_ws"], g.meta["w_dim"]], generator=gen)
    R = torch.randn([1, 3, c["res"], c["res"]], generator=gen)
    wd, wo = ws.to(dev).requires_grad_(True), ws.clone().requires_grad_(True)
    (G.synthesis(wd, noise_mode="const") * R.to(dev)).sum().backward()
    (O.synthesis(wo, noise_mode="const") * R).sum().backward()
    assert float((wd.grad.cpu() - wo.grad).abs().max()) <= 1e-4 * float(wo.grad.abs().max())
    for a, b in zip(nd, no):
        assert a.grad is not None and float(b.grad.abs().max()) > 0
        assert float((a.grad.cpu() - b.grad).abs().max()) <= 1e-4 * float(b.grad.abs().max())


# ---------------------------------------------------------------------------------------------------------------- project() end to end

@pytest.mark.parametrize("tag", ["g32", "g16", "g512"])
def test_project_reproduces_the_reference(dev, tag):
    g = pu.fixture()
    c = pu.case(g, tag)
    G = pu.product_generator(g, c, dev)
    assert list(projector.noise_buffers(G)) == c["noise_names"]
    w = projector.project(G, pu.target(g, c).to(dev), num_steps=c["num_steps"], w_avg_samples=g.meta["w_avg_samples"], device=dev,
                          vgg16=ppl_util.StandInLPIPS(g).to(dev), draws=pu.draws(g, c))
    ref = g.t(f"{tag}/w_out")
    assert w.device.type == "cuda" and w.shape == ref.shape
    err = float((w.cpu() - ref).abs().max() / ref.abs().max())
    assert err < pu.REL_BOUND, err


def test_projection_step_launch_budget(dev):
    """per step: at most 3 regulariser launches, 1 for its backward, 2 for the renormalisation, 2 + 1 for the distance; and no weight
    gradient at all (the weights are frozen)"""
    g = pu.fixture()
    c = pu.case(g, "g32")
    G = pu.product_generator(g, c, dev)
    steps = 3
    with launch_log() as seen:
        projector.project(G, pu.target(g, c).to(dev), num_steps=steps, w_avg_samples=8, device=dev, vgg16=ppl_util.StandInLPIPS(g).to(dev),
                          draws=pu.draws(g, c))
    counts = proj_counts(seen)
    assert counts == {"reg": 3 * steps, "reg_bwd": steps, "normalize": 2 * steps, "sqdist": 2 * steps, "sqdist_bwd": steps}, counts
    kinds = {k for k, _ in seen}
    assert "conv_wgrad" not in kinds and "wgrad_reduce" not in kinds


# ---------------------------------------------------------------------------------------------------------------- CLI

class ScriptedStandIn(torch.nn.Module):
    """the fixture's stand-in LPIPS network with the TorchScript vgg16.pt's call signature (resize_images, return_lpips)"""

    def __init__(self, base):
        super().__init__()
        for k, v in base.state_dict().items():
            self.register_buffer(k, v.clone())

    def _level(self, x, w, b, gw):
        x = torch.relu(torch.nn.functional.conv2d(x, w, b, padding=1))
        n = x / (x.square().sum(1, keepdim=True) + 1e-10).sqrt()
        return x, (n * gw.view(1, -1, 1, 1)).flatten(1) / float(x.shape[2] * x.shape[3]) ** 0.5

    def forward(self, img: torch.Tensor, resize_images: bool = False, return_lpips: bool = True) -> torch.Tensor:
        x, f1 = self._level(img / 127.5 - 1, self.w1, self.b1, self.g1)
        x, f2 = self._level(torch.nn.functional.avg_pool2d(x, 2), self.w2, self.b2, self.g2)
        return torch.cat([f1, f2], 1)


def test_cli_end_to_end(dev, tmp_path):
    import PIL.Image
    g = pu.fixture()
    c = pu.case(g, "g16")
    G = pu.product_generator(g, c, dev)
    snap = tmp_path / "network-snapshot-000000.pt"
    sd = {k: v.cpu() for k, v in G.state_dict().items()}
    torch.save({"G": sd, "G_ema": sd}, str(snap))
    det = torch.jit.script(ScriptedStandIn(ppl_util.StandInLPIPS(g)))
    det_path = str(tmp_path / "vgg16.pt")
    det.save(det_path)
    cfg = tmp_path / "cfg.yaml"
    cfg.write_text("gen:\n  generator: sg2_classic\ngens_args:\n  sg2_classic:\n    z_dim: 16\n    w_dim: 16\n"
                   "    mapping_kwargs:\n      num_layers: 2\n"
                   f"    synthesis_kwargs:\n      channel_base: {c['channel_base']}\n      channel_max: {c['channel_max']}\n"
                   "      num_fp16_res: 0\n      block_kwargs:\n        conv_clamp: 256\n")
    PIL.Image.fromarray(np.random.RandomState(18).randint(0, 256, [20, 24, 3], dtype=np.uint8)).save(str(tmp_path / "t.png"))
    out = tmp_path / "out"
    cmd = [sys.executable, "-m", "style_big_gan_amd.projector", f"exp.config_dir={tmp_path}", "exp.config=cfg.yaml",
           f"--snapshot={snap}", f"--target={tmp_path / 't.png'}", f"--outdir={out}", "--num-steps=3", f"--detector={det_path}"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "step    3/3" in r.stdout
    w = np.load(str(out / "projected_w.npz"))["w"]
    assert w.shape == (1, c["num_ws"], 16) and np.isfinite(w).all()
    assert PIL.Image.open(str(out / "proj.png")).size == (16, 16) and PIL.Image.open(str(out / "target.png")).size == (16, 16)
