"""Image export on the device: the quantise-and-tile kernel and the latent-table kernel against the op layer's CPU branches bit for
bit, generate_images / generate_style_mix / save_image_snapshot on the HIP generator against the reference's images
(tests/golden/image_export.npz), and the two command-line tools end to end from a snapshot written by save_snapshot."""
import contextlib
import os
import subprocess
import sys

import numpy as np
import PIL.Image
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import _lib, arguments, generate, style_mixing
from style_big_gan_amd.torch_utils.ops import image_export
from style_big_gan_amd.train_parts import trainers as T
import image_export_util as iu
from test_image_export_cpu import check_images

pytestmark = pytest.mark.gpu

PLANAR4, MINOR4, PIXEL = 1, 2, 3        # dims[6] of a quantize_tile launch record


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


@contextlib.contextmanager
def launches():
    """-> list of (variant name, dims) of every image_export launch inside the block"""
    _lib.prof_enable(True)
    _lib.prof_fetch()
    seen = []
    try:
        yield seen
    finally:
        torch.cuda.synchronize()
        recs = _lib.prof_fetch()
        _lib.prof_enable(False)
        seen.extend((_lib.IMG_VARIANTS[r["dims"][0]], r["dims"]) for r in recs if r["kind"] == "image_export")


def _images(seed, shape, layout, dev):
    """fp32 images in [-1.3, 1.3] on the device with the asked memory layout, and the same values on the host"""
    N, C, H, W = shape
    x = torch.from_numpy((np.random.RandomState(seed).rand(N, C, H, W) * 2.6 - 1.3).astype(np.float32))
    if layout == "contiguous":
        d = x.to(dev)
    elif layout == "channels_last":
        d = x.to(dev).contiguous(memory_format=torch.channels_last)
    elif layout == "sliced":            # a window of a larger tensor: row and plane strides larger than the shape, base not 16-byte aligned
        big = torch.zeros([N, C, H + 3, W + 5], device=dev)
        d = big[:, :, 2:2 + H, 1:1 + W]
        d.copy_(x)
    elif layout == "sliced_aligned":    # a window whose rows stay 16-byte aligned
        big = torch.zeros([N, C, H + 3, W + 8], device=dev)
        d = big[:, :, 1:1 + H, 4:4 + W]
        d.copy_(x)
    assert torch.equal(d.cpu(), x)
    return d, x


@pytest.mark.parametrize("rule", ["grid", "clamp"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("W", [16, 13, 7])
@pytest.mark.parametrize("layout", ["contiguous", "channels_last", "sliced", "sliced_aligned"])
def test_quantize_tile_kernel_is_exact(dev, rule, C, W, layout):
    N, H, gw, gh, cell0 = 5, 6, 4, 2, 2
    d, x = _images(100 + W + C, (N, C, H, W), layout, dev)
    drange = [-1, 1] if rule == "grid" else None
    ref = image_export.tile(x, (gw, gh), rule, drange, canvas=torch.full([gh * H, gw * W, C], 201, dtype=torch.uint8), cell0=cell0)
    canvas = torch.full([gh * H, gw * W, C], 201, dtype=torch.uint8, device=dev)
    with launches() as seen:
        out = image_export.tile(d, (gw, gh), rule, drange, canvas=canvas, cell0=cell0)
    assert out is canvas and torch.equal(canvas.cpu(), ref)
    assert bool((canvas[:H, :2 * W] == 201).all()) and bool((canvas[H:, 3 * W:] == 201).all())     # cells 0, 1 and 7 keep the sentinel
    assert len(seen) == 1 and seen[0][0] == "quantize_tile" and seen[0][1][1:6] == (N, C, H, W, _lib.QUANT_RULES[rule])
    vec = W % 4 == 0 and layout != "sliced"
    want = PIXEL if not vec else MINOR4 if (layout == "channels_last" and C == 3) else PLANAR4
    assert seen[0][1][6] == want


@pytest.mark.parametrize("rule", ["grid", "clamp"])
@pytest.mark.parametrize("width", [264, 263])       # four pixels per work-item / one
def test_ties_out_of_range_and_non_finite(dev, rule, width):
    g = iu.fixture()
    x = g.t("grid/ties/x")[..., :width].contiguous()
    drange = [-1, 1] if rule == "grid" else None
    got = image_export.quantize(x.to(dev), rule, drange).cpu().numpy().reshape(-1)
    ref = (g.npz["grid/ties/png"] if rule == "grid" else g.npz["clamp/ties"]).reshape(-1)[:width]
    assert np.array_equal(got, ref)
    other = (g.npz["clamp/ties"] if rule == "grid" else g.npz["grid/ties/png"]).reshape(-1)[:width]
    assert not np.array_equal(got, other)
    nf = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0] * 2)[:8 if width % 4 == 0 else 7].reshape(1, 1, 1, -1)
    got = image_export.quantize(nf.to(dev), rule, drange).cpu()
    assert torch.equal(got, image_export.quantize(nf, rule, drange)) and got.reshape(-1)[:4].tolist() == [0, 255, 0, 128]


def test_quantize_at_the_snapshot_size(dev):
    """a batch_gpu chunk of the sg2ada grid (3 x 256 x 256) into the middle of a 30 x 16 canvas, both rules' fast paths at full size"""
    d, x = _images(9, (8, 3, 256, 256), "contiguous", dev)
    canvas = torch.zeros([16 * 256, 30 * 256, 3], dtype=torch.uint8, device=dev)
    image_export.tile(d, (30, 16), "grid", [-1, 1], canvas=canvas, cell0=237)
    ref = image_export.tile(x, (30, 16), "grid", [-1, 1], cell0=237)
    assert torch.equal(canvas.cpu(), ref)


def test_device_inputs_are_checked(dev):
    x = torch.zeros([2, 3, 4, 4], device=dev)
    with pytest.raises(RuntimeError, match="canvas on cpu"):
        image_export.tile(x, (2, 1), "clamp", canvas=torch.zeros([4, 8, 3], dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="float32"):
        image_export.quantize(x.half(), "clamp")
    with pytest.raises(RuntimeError, match="w_avg on cpu"):
        image_export.truncate_mix(torch.zeros([2, 3, 4], device=dev), torch.zeros(4), 1.0, [0], [0], [])
    lib = _lib.load()
    c = torch.zeros([4, 8, 3], dtype=torch.uint8, device=dev)
    args = (x.data_ptr(), c.data_ptr(), 2, 3, 4, 4, 48, 16, 4, 1)
    assert lib.sbg_img_quantize_tile(*args, 2, 1, 1, 1, 0.0, 1.0, None) != 0 and b"outside" in lib.sbg_last_error()       # cell 2 of a 2 x 1 grid
    assert lib.sbg_img_quantize_tile(*args, 2, 1, 0, 7, 0.0, 1.0, None) != 0 and b"unknown rule" in lib.sbg_last_error()


@pytest.mark.parametrize("D", [16, 18])     # float4 / scalar
@pytest.mark.parametrize("psi", [0.7, 1.0, -0.5])
def test_truncate_mix_kernel_is_exact(dev, D, psi):
    gen = torch.Generator().manual_seed(6)
    ws, w_avg = torch.randn([5, 8, D], generator=gen), torch.randn([D], generator=gen)
    rows, cols, styles = [4, 0, 2], [1, 1, 3, 0], [0, 2, 7]
    with launches() as seen:
        out = image_export.truncate_mix(ws.to(dev), w_avg.to(dev), psi, rows, cols, styles)
        table = image_export.truncate_mix(ws.to(dev), w_avg.to(dev), psi, range(5), [0], [])
    assert torch.equal(out.cpu(), image_export.truncate_mix(ws, w_avg, psi, rows, cols, styles))
    assert torch.equal(table.cpu(), w_avg + (ws - w_avg) * psi)
    assert [s[0] for s in seen] == ["truncate_mix"] * 2 and seen[0][1][1:5] == (12, 8, D, 1 if D % 4 == 0 else 2)


# ---------------------------------------------------------------------------------------------------------------- the tools on the HIP generator

@pytest.mark.parametrize("tag", ["plain", "trunc", "cond"])
def test_generate_images_on_the_device(dev, tmp_path, tag):
    g = iu.fixture()
    case = next(c for c in g.meta["gen"] if c["tag"] == tag)
    G = iu.product_generator(g, case["net"], dev)
    with launches() as seen:
        out = generate.generate_images(G, seeds=case["seeds"], truncation_psi=case["psi"], class_idx=case["class_idx"], outdir=str(tmp_path), device=dev)
    check_images(out, g.npz[f"gen/{tag}/uint8"], g.npz[f"gen/{tag}/float"])
    assert [s[0] for s in seen] == ["quantize_tile"] * len(case["seeds"])
    assert np.array_equal(np.array(PIL.Image.open(tmp_path / f"seed{case['seeds'][0]:04d}.png")), out[0])


def test_generate_from_projected_w_on_the_device(dev):
    g = iu.fixture()
    out = generate.generate_images(iu.product_generator(g, "g16", dev), projected_w=g.npz["proj/ws"], device=dev)
    check_images(out, g.npz["proj/uint8"], g.npz["proj/float"])


def test_style_mix_on_the_device(dev, tmp_path):
    g = iu.fixture()
    mix = g.meta["mix"]
    G = iu.product_generator(g, mix["net"], dev)
    kw = dict(col_styles=mix["styles"], truncation_psi=mix["psi"], device=dev)
    d = style_mixing.generate_style_mix(G, mix["rows"], mix["cols"], outdir=str(tmp_path), batch=4, **kw)
    keys = [tuple(k) for k in g.npz["mix/keys"].tolist()]
    assert list(d.keys()) == keys
    check_images(np.stack([d[k] for k in keys]), g.npz["mix/uint8"], g.npz["mix/float"])
    check_images(np.array(PIL.Image.open(tmp_path / "grid.png")), g.npz["mix/grid_png"], g.npz["mix/float"])
    assert sorted(os.listdir(tmp_path)) == mix["files"]
    # batched synthesis against the one-by-one form: the samples of a batch are independent at noise_mode='const'
    one = style_mixing.generate_style_mix(G, mix["rows"], mix["cols"], batch=1, **kw)
    whole = style_mixing.generate_style_mix(G, mix["rows"], mix["cols"], batch=64, **kw)
    for k in keys:
        assert np.array_equal(one[k], d[k]) and np.array_equal(whole[k], d[k]), k


SG2_YAML = ("exp:\n  trainer: sg2\ngen:\n  generator: sg2_classic\n  discriminator: sg2_classic\n  batch: 8\n  batch_gpu: 4\n  kimg: 1\n"
            "  disc_regs: [r1]\ndisc_regs_all:\n  r1:\n    r1_gamma: 0.01\nlosses_arch_args:\n  sg2:\n    style_mixing_prob: 0\n"
            "aug:\n  aug: noaug\ndata:\n  dataset: synthetic\n  resolution: 16\n"
            "gens_args:\n  sg2_classic:\n    z_dim: 16\n    w_dim: 16\n    mapping_kwargs:\n      num_layers: 2\n"
            "    synthesis_kwargs:\n      channel_base: 256\n      channel_max: 16\n      num_fp16_res: 0\n      block_kwargs:\n        conv_clamp: 256\n"
            "discs_args:\n  sg2_classic:\n    channel_base: 256\n    channel_max: 16\n    num_fp16_res: 0\n    architecture: orig\n"
            "    epilogue_kwargs:\n      mbstd_group_size: 4\n")


def _trainer(tmp_path):
    """an sg2 trainer at the fixture's generator shape, taken through the lifecycle up to the training loop, G and G_ema holding g16"""
    (tmp_path / "cfg.yaml").write_text(SG2_YAML)
    overrides = [f"exp.config_dir={tmp_path}", "exp.config=cfg.yaml", "exp.name=run", f"log.output={tmp_path / 'logs'}"]
    trainer = T.trainers["sg2"]().setup_arguments(arguments.load_config(overrides))
    for stage in ("setup_logs", "init_params", "setup_dataset", "setup_networks", "setup_augmentations"):
        getattr(trainer, stage)()
    state = iu.fixture().state_dict("g16/G")
    trainer.engine.G.load_state_dict(state)
    trainer.engine.G_ema.load_state_dict(state)
    return trainer, overrides


def test_trainer_image_snapshot_on_the_device(dev, tmp_path):
    g = iu.fixture()
    trainer, _ = _trainer(tmp_path)
    run = tmp_path / "logs" / "run"
    with launches() as seen:
        first = trainer.save_image_snapshot()
    assert first.endswith("fakes_init.png") and tuple(trainer.grid_size) == (32, 32)
    assert [s[0] for s in seen] == ["quantize_tile"] * 256          # 1024 cells in batch_gpu = 4 chunks, nothing else
    # the first snapshot, bit for bit: the device images quantised and tiled by the CPU branch
    with torch.no_grad():
        img = torch.cat([trainer.engine.G_ema(z, c, noise_mode="const") for z, c in zip(trainer.grid_z, trainer.grid_c)])
    ref = image_export.tile(img.float().cpu(), (32, 32), "grid", [-1, 1]).numpy()
    assert np.array_equal(np.array(PIL.Image.open(first)), ref)
    _, images, _ = T.setup_snapshot_image_grid(trainer.dataset)
    assert np.array_equal(np.array(PIL.Image.open(run / "reals.png"))[16:32, 48:64], images[32 + 3].transpose(1, 2, 0))
    # against the reference's images: the fixture's latents in every cell, cyclically
    seeds = next(c for c in g.meta["gen"] if c["tag"] == "plain")["seeds"]
    z = torch.cat([torch.from_numpy(np.random.RandomState(s).randn(1, 16)) for s in seeds]).float()
    pick = [i % len(seeds) for i in range(1024)]
    trainer.grid_z = z[pick].to(dev).split(trainer.batch_gpu)
    later = trainer.save_image_snapshot()
    assert later.endswith("fakes000000.png")
    f = g.npz["gen/plain/float"]
    expect = image_export.tile(torch.from_numpy(f[pick]), (32, 32), "grid", [-1, 1]).numpy()
    check_images(np.array(PIL.Image.open(later)), expect, f)


def test_cli_end_to_end_from_a_saved_snapshot(dev, tmp_path):
    g = iu.fixture()
    trainer, overrides = _trainer(tmp_path)
    snap = trainer.save_snapshot()
    assert os.path.isfile(snap)
    G = trainer.engine.G_ema
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))

    def run(module, *args):
        r = subprocess.run([sys.executable, "-m", module] + overrides + [f"--snapshot={snap}"] + list(args), cwd=ROOT, env=env, capture_output=True,
                           text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-2000:]
        return r.stdout

    out = tmp_path / "gen"
    run("style_big_gan_amd.generate", f"--outdir={out}", "--seeds=5,1234", "--trunc=0.7")
    ref = generate.generate_images(G, seeds=[5, 1234], truncation_psi=0.7, device=dev)
    assert sorted(os.listdir(out)) == ["seed0005.png", "seed1234.png"]
    assert np.array_equal(np.stack([np.array(PIL.Image.open(out / n)) for n in sorted(os.listdir(out))]), ref)
    check_images(ref, g.npz["gen/trunc/uint8"], g.npz["gen/trunc/float"])

    npz = tmp_path / "projected_w.npz"
    np.savez(str(npz), w=g.npz["proj/ws"][-1:])          # the projector's file: w [1, num_ws, w_dim]
    out = tmp_path / "proj"
    assert "Generating images from projected W" in run("style_big_gan_amd.generate", f"--outdir={out}", f"--projected-w={npz}")
    assert os.listdir(out) == ["proj00.png"]
    check_images(np.array(PIL.Image.open(out / "proj00.png"))[None], g.npz["proj/uint8"][-1:], g.npz["proj/float"][-1:])

    mix = g.meta["mix"]
    out = tmp_path / "mix"
    run("style_big_gan_amd.style_mixing", f"--outdir={out}", "--rows=" + ",".join(map(str, mix["rows"])), "--cols=" + ",".join(map(str, mix["cols"])),
        "--styles=0-2", f"--trunc={mix['psi']}")
    assert sorted(os.listdir(out)) == mix["files"]
    check_images(np.array(PIL.Image.open(out / "grid.png")), g.npz["mix/grid_png"], g.npz["mix/float"])
