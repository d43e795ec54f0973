"""Latent projector, host side: project() on the CPU restatement of the generator against the reference's own project()
(tests/golden/projector.npz), the op layer's CPU branches against the reference's formulas, the learning-rate and noise schedules,
and the CLI's argument parsing and target preparation.

The package's generator runs only on the device, so the CPU projection runs the CPU restatement of the same network
(oracle/networks.py, tests/projector_util.OracleGenerator); the projector's own arithmetic takes the op layer's CPU branch."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import projector
from style_big_gan_amd.torch_utils.ops import projector as proj_ops
import ppl_util
import projector_util as pu


@pytest.mark.parametrize("tag", ["g32", "g16", "g512"])
def test_project_reproduces_the_reference(tag):
    g = pu.fixture()
    c = pu.case(g, tag)
    G = pu.oracle_generator(g, c)
    assert list(projector.noise_buffers(G)) == c["noise_names"]
    w = projector.project(G, pu.target(g, c), num_steps=c["num_steps"], w_avg_samples=g.meta["w_avg_samples"], device=torch.device("cpu"),
                          vgg16=ppl_util.StandInLPIPS(g), draws=pu.draws(g, c))
    ref = g.t(f"{tag}/w_out")
    assert w.shape == ref.shape == (c["num_steps"], c["num_ws"], g.meta["w_dim"])
    assert float((w - ref).abs().max() / ref.abs().max()) < pu.REL_BOUND


def test_default_draws_follow_the_reference_call_order():
    """without `draws`, one randn_like per noise buffer and then one per step, from torch's global RNG: the recorded draws replay"""
    g = pu.fixture()
    c = pu.case(g, "g16")
    torch.manual_seed(c["draw_seed"])
    w = projector.project(pu.oracle_generator(g, c), pu.target(g, c), num_steps=c["num_steps"], w_avg_samples=g.meta["w_avg_samples"],
                          device=torch.device("cpu"), vgg16=ppl_util.StandInLPIPS(g))
    ref = g.t("g16/w_out")
    assert float((w - ref).abs().max() / ref.abs().max()) < pu.REL_BOUND


def test_project_leaves_the_caller_generator_alone():
    g = pu.fixture()
    c = pu.case(g, "g16")
    G = pu.oracle_generator(g, c)
    before = {k: v.clone() for k, v in G.state_dict().items()}
    projector.project(G, pu.target(g, c), num_steps=2, w_avg_samples=8, device=torch.device("cpu"), vgg16=ppl_util.StandInLPIPS(g),
                      draws=pu.draws(g, c))
    assert all(torch.equal(before[k], v) for k, v in G.state_dict().items())


def _random_bufs(seed, sizes):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn([r, r], generator=gen) for r in sizes]


SG2ADA_256 = [4, 8, 8, 16, 16, 32, 32, 64, 64, 128, 128, 256, 256]


def test_levels_match_the_reference_loop():
    assert sum(proj_ops.num_levels(r) for r in SG2ADA_256) == 43
    assert [proj_ops.num_levels(r) for r in (4, 8, 16, 32, 1024)] == [1, 1, 2, 3, 8]
    assert proj_ops.noise_means(_random_bufs(0, SG2ADA_256)).shape == (86,)


def test_cpu_noise_reg_is_the_reference_formula():
    bufs = [b.requires_grad_(True) for b in _random_bufs(1, [4, 16, 64])]
    reg = proj_ops.noise_reg(bufs)
    ref = 0.0
    for v in bufs:
        noise = v[None, None]
        while True:
            ref += (noise * torch.roll(noise, shifts=1, dims=3)).mean() ** 2
            ref += (noise * torch.roll(noise, shifts=1, dims=2)).mean() ** 2
            if noise.shape[2] <= 8:
                break
            noise = F.avg_pool2d(noise, kernel_size=2)
    assert torch.equal(reg, ref)
    m = proj_ops.noise_means(bufs)
    assert m.shape == (2 * (1 + 2 + 4),) and float((m.double() ** 2).sum()) == pytest.approx(float(reg), rel=1e-6)


def test_cpu_noise_reg_gradient_matches_the_closed_form():
    """d reg / d buf = sum_k G_k[y >> k, x >> k] / 4^k, G_k = 2 (m_x (P[j-1] + P[j+1]) + m_y (P[i-1] + P[i+1])) / n^2 -- the formula
    the device kernel implements -- checked on the reference's autograd in fp64"""
    bufs = [b.double().requires_grad_(True) for b in _random_bufs(2, [8, 32])]
    proj_ops.noise_reg(bufs).backward()
    for b in bufs:
        P, acc, k = b.detach(), torch.zeros_like(b), 0
        while True:
            n = P.shape[0]
            mx = (P * torch.roll(P, 1, 1)).mean()
            my = (P * torch.roll(P, 1, 0)).mean()
            G = 2 * (mx * (torch.roll(P, 1, 1) + torch.roll(P, -1, 1)) + my * (torch.roll(P, 1, 0) + torch.roll(P, -1, 0))) / n ** 2
            acc += G.repeat_interleave(2 ** k, 0).repeat_interleave(2 ** k, 1) / 4 ** k
            if n <= 8:
                break
            P = F.avg_pool2d(P[None, None], 2)[0, 0]
            k += 1
        assert torch.allclose(b.grad, acc, rtol=1e-12, atol=1e-15)


def test_no_noise_buffers_is_the_reference_behaviour():
    """a generator without noise_const buffers: the reference's loop leaves reg_loss = 0.0 and renormalises nothing"""
    assert proj_ops.noise_reg([]) == 0.0
    assert proj_ops.noise_means([]).shape == (0,)
    proj_ops.noise_normalize_([])


def test_cpu_noise_normalize_is_the_reference_formula():
    bufs = _random_bufs(3, [4, 32])
    ref = [b.clone() for b in bufs]
    proj_ops.noise_normalize_(bufs)
    for b, r in zip(bufs, ref):
        r -= r.mean()
        r *= r.square().mean().rsqrt()
        assert torch.equal(b, r)


def test_cpu_sqdist_is_the_reference_formula():
    gen = torch.Generator().manual_seed(4)
    t, s = torch.randn([1, 1000], generator=gen), torch.randn([1, 1000], generator=gen).requires_grad_(True)
    d = proj_ops.sqdist(t, s)
    assert torch.equal(d, (t - s).square().sum())
    with pytest.raises(RuntimeError, match="shapes differ"):
        proj_ops.sqdist(t, s[:, :10])


@pytest.mark.parametrize("num_steps", [10, 1000])
def test_schedules_match_the_reference(num_steps):
    """the reference's expressions (:82-88) for every step"""
    w_std = 0.7
    for step in range(num_steps):
        t = step / num_steps
        ref_scale = w_std * 0.05 * max(0.0, 1.0 - t / 0.75) ** 2
        lr_ramp = min(1.0, (1.0 - t) / 0.25)
        lr_ramp = 0.5 - 0.5 * np.cos(lr_ramp * np.pi)
        lr_ramp = lr_ramp * min(1.0, t / 0.05)
        assert projector.w_noise_scale(step, num_steps, w_std) == ref_scale
        assert projector.learning_rate(step, num_steps) == 0.1 * lr_ramp
    assert projector.learning_rate(0, num_steps) == 0.0
    assert projector.w_noise_scale(int(np.ceil(0.75 * num_steps)), num_steps, w_std) == 0.0


def test_cli_parses_config_overrides_and_options():
    rest, args = projector.parse_args(["exp.config_dir=/c", "exp.config=sg2ada.yaml", "--snapshot", "s.pt", "--target=t.png",
                                       "--outdir", "out", "--detector", "vgg16.pt", "gen.generator=sg2_classic"])
    assert rest == ["exp.config_dir=/c", "exp.config=sg2ada.yaml", "gen.generator=sg2_classic"]
    assert (args.snapshot, args.target, args.outdir, args.detector) == ("s.pt", "t.png", "out", "vgg16.pt")
    assert (args.num_steps, args.seed, args.save_video) == (1000, 303, False)
    _, args = projector.parse_args(["--snapshot=s", "--target=t", "--outdir=o", "--detector=d", "--num-steps", "7", "--seed=1", "--save-video"])
    assert (args.num_steps, args.seed, args.save_video) == (7, 1, True)
    with pytest.raises(SystemExit):
        projector.parse_args(["--snapshot=s", "--target=t", "--outdir=o", "--detector=d", "--bogus"])
    with pytest.raises(SystemExit):
        projector.parse_args(["--target=t", "--outdir=o", "--detector=d"])


@pytest.mark.parametrize("size", [(40, 24), (24, 40), (33, 33)])
def test_target_crop_and_resize_follow_pil(tmp_path, size):
    import PIL.Image
    rng = np.random.RandomState(5)
    path = str(tmp_path / "t.png")
    PIL.Image.fromarray(rng.randint(0, 256, [size[1], size[0], 3], dtype=np.uint8)).save(path)
    pil, arr = projector.load_target(path, 16)
    img = PIL.Image.open(path).convert("RGB")
    w, h = img.size
    s = min(w, h)
    ref = np.array(img.crop(((w - s) // 2, (h - s) // 2, (w + s) // 2, (h + s) // 2)).resize((16, 16), PIL.Image.LANCZOS), dtype=np.uint8)
    assert arr.shape == (16, 16, 3) and arr.dtype == np.uint8 and np.array_equal(arr, ref) and pil.size == (16, 16)


def test_cli_reads_generator_shape_from_the_snapshot_state():
    g = pu.fixture()
    state = g.state_dict("g32/G")
    assert projector.generator_common_kwargs(state) == dict(c_dim=0, img_resolution=32, img_channels=3)
    with pytest.raises(RuntimeError, match="no mapping/synthesis"):
        projector.generator_common_kwargs({"main.0.weight": torch.zeros(1)})


def test_detector_is_never_fetched():
    with pytest.raises(RuntimeError, match="nothing is fetched"):
        projector.resolve_detector("https://example.invalid/vgg16.pt", torch.device("cpu"))
    det, kw = projector.resolve_detector(lambda x: x, torch.device("cpu"))
    assert kw == {}


def test_save_video_without_imageio_is_a_clear_error(monkeypatch):
    monkeypatch.setitem(sys.modules, "imageio", None)
    from style_big_gan_amd import arguments
    monkeypatch.setattr(arguments, "load_config", lambda argv: None)
    with pytest.raises(RuntimeError, match="imageio"):
        projector.run_projection(["--snapshot=s", "--target=t", "--outdir=o", "--detector=d", "--save-video"])
