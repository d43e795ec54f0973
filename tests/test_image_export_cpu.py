"""Image export, host side: the two quantisation rules' CPU branches, the snapshot grid set-up and writer, generate_images and
generate_style_mix on the CPU restatement of the generator, and the trainer's image snapshots -- all against what the reference
itself wrote (tests/golden/image_export.npz, from tests/golden/make_golden_image_export.py)."""
import glob
import os
import sys

import numpy as np
import PIL.Image
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import arguments, generate, starter, style_mixing
from style_big_gan_amd.torch_utils.ops import image_export
from style_big_gan_amd.train_parts import trainers as T
import image_export_util as iu

FLOAT_BATCHES = ["rgb", "grey", "ties"]


def _png_as_hwc(png):
    return png if png.ndim == 3 else png[:, :, None]


# ---------------------------------------------------------------------------------------------------------------- the two rules

@pytest.mark.parametrize("name", FLOAT_BATCHES)
def test_grid_rule_cpu_is_the_reference(name):
    g = iu.fixture()
    x = g.t(f"grid/{name}/x")
    canvas = image_export.tile(x, g.meta["grid"][name]["grid_size"], "grid", [-1, 1])
    assert canvas.dtype == torch.uint8 and np.array_equal(canvas.numpy(), _png_as_hwc(g.npz[f"grid/{name}/png"]))


@pytest.mark.parametrize("name", FLOAT_BATCHES)
def test_clamp_rule_cpu_is_the_reference(name):
    g = iu.fixture()
    q = image_export.quantize(g.t(f"grid/{name}/x"), "clamp")
    assert q.dtype == torch.uint8 and np.array_equal(q.numpy(), g.npz[f"clamp/{name}"])


def test_tie_vectors_tell_the_rules_apart():
    """swapping the rules on the tie vectors must change bytes: otherwise the fixture could not catch a kernel that uses the wrong one"""
    g = iu.fixture()
    x = g.t("grid/ties/x")
    assert np.array_equal(x.numpy(), iu.tie_vector())
    as_grid = image_export.quantize(x, "grid", [-1, 1]).numpy().reshape(-1)
    as_clamp = image_export.quantize(x, "clamp").numpy().reshape(-1)
    assert np.array_equal(as_grid, g.npz["grid/ties/png"].reshape(-1)) and np.array_equal(as_clamp, g.npz["clamp/ties"].reshape(-1))
    differ = int((as_grid[:255] != as_clamp[:255]).sum())
    print("ties: the rules differ on", differ, "of 255")
    assert differ >= 96         # every exact tie with an even k rounds down under `grid` and up under `clamp`
    v = (x.numpy().reshape(-1)[:255] - np.float32(-1)) * np.float32(127.5)
    assert int((v - np.floor(v) == 0.5).sum()) >= 96


def test_random_images_alone_do_not_tell_the_rules_apart():
    x = torch.from_numpy((np.random.RandomState(3).rand(4, 3, 32, 32) * 2 - 1).astype(np.float32))
    a, b = image_export.quantize(x, "grid", [-1, 1]), image_export.quantize(x, "clamp")
    assert float((a != b).float().mean()) < 1e-3


def test_non_finite_values_are_defined():
    x = torch.tensor([float("nan"), float("inf"), -float("inf"), 0.0]).reshape(1, 1, 1, 4)
    assert image_export.quantize(x, "grid", [-1, 1]).reshape(-1).tolist() == [0, 255, 0, 128]
    assert image_export.quantize(x, "clamp").reshape(-1).tolist() == [0, 255, 0, 128]


def test_tile_fills_a_run_of_cells_and_leaves_the_rest():
    x = torch.from_numpy((np.random.RandomState(4).rand(6, 3, 5, 8) * 2 - 1).astype(np.float32))
    whole = image_export.tile(x, (3, 2), "clamp")
    canvas = torch.full([10, 24, 3], 77, dtype=torch.uint8)
    assert image_export.tile(x[1:3], (3, 2), "clamp", canvas=canvas, cell0=1) is canvas
    assert torch.equal(canvas[:5, 8:], whole[:5, 8:]) and bool((canvas[:5, :8] == 77).all()) and bool((canvas[5:] == 77).all())
    image_export.tile(x[:1], (3, 2), "clamp", canvas=canvas, cell0=0)
    image_export.tile(x[3:], (3, 2), "clamp", canvas=canvas, cell0=3)
    assert torch.equal(canvas, whole)
    q = image_export.quantize(x, "clamp")
    assert q.shape == (6, 5, 8, 3) and torch.equal(q[4], whole[5:, 8:16])


def test_bad_inputs_raise():
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="unknown rule"):
        image_export.quantize(x, "round")
    with pytest.raises(RuntimeError, match="C = 1 or 3"):
        image_export.quantize(torch.zeros(2, 2, 4, 4), "clamp")
    with pytest.raises(RuntimeError, match="float32"):
        image_export.quantize(x.double(), "clamp")
    with pytest.raises(RuntimeError, match="drange"):
        image_export.quantize(x, "grid")
    with pytest.raises(RuntimeError, match="drange must be None"):
        image_export.quantize(x, "clamp", [-1, 1])
    with pytest.raises(RuntimeError, match="do not fit"):
        image_export.tile(x, (1, 1), "clamp")
    with pytest.raises(RuntimeError, match="canvas"):
        image_export.tile(x, (2, 1), "clamp", canvas=torch.zeros(4, 8, 1, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="indices"):
        image_export.truncate_mix(torch.zeros(2, 3, 4), torch.zeros(4), 1.0, [2], [0], [])
    with pytest.raises(IndexError):
        image_export.truncate_mix(torch.zeros(2, 3, 4), torch.zeros(4), 1.0, [0], [0], [3])


def test_truncate_mix_cpu_is_the_reference_formula():
    gen = torch.Generator().manual_seed(5)
    ws, w_avg = torch.randn([4, 6, 16], generator=gen), torch.randn([16], generator=gen)
    t = w_avg + (ws - w_avg) * 0.7
    assert torch.equal(image_export.truncate_mix(ws, w_avg, 0.7, range(4), [0], []), t)
    out = image_export.truncate_mix(ws, w_avg, 0.7, [3, 1], [0, 2, 3], [0, 1, 5])
    assert out.shape == (6, 6, 16)
    for r, row in enumerate([3, 1]):
        for c, col in enumerate([0, 2, 3]):
            w = t[row].clone()
            w[[0, 1, 5]] = t[col][[0, 1, 5]]
            assert torch.equal(out[r * 3 + c], w)
    assert not torch.equal(t, torch.lerp(w_avg, ws, 0.7))       # the mapping network's lerp rounds differently


# ---------------------------------------------------------------------------------------------------------------- snapshot grids

@pytest.mark.parametrize("name", ["labelled", "grey"])
def test_snapshot_grid_setup_and_writer_match_the_reference(tmp_path, name):
    g = iu.fixture()
    ds = iu.ToyDataset(**iu.TOY_SETS[name])
    grid_size, images, labels = T.setup_snapshot_image_grid(ds)
    assert list(grid_size) == g.meta["toy"][name]["grid_size"]
    assert ds.asked == g.npz[f"toy/{name}/indices"].tolist()
    assert images.dtype == np.uint8 and np.array_equal(images, ds.images[ds.asked]) and np.array_equal(labels, g.npz[f"toy/{name}/labels"])
    path = str(tmp_path / "reals.png")
    T.save_image_grid(images, path, drange=[0, 255], grid_size=grid_size)
    png = PIL.Image.open(path)
    assert png.mode == g.meta["toy"][name]["mode"] == ("RGB" if name == "labelled" else "L")
    assert np.array_equal(np.array(png), g.npz[f"toy/{name}/reals_png"])


@pytest.mark.parametrize("name", FLOAT_BATCHES)
def test_save_image_grid_on_float_images(tmp_path, name):
    g = iu.fixture()
    path = str(tmp_path / "f.png")
    T.save_image_grid(g.npz[f"grid/{name}/x"], path, drange=[-1, 1], grid_size=g.meta["grid"][name]["grid_size"])
    png = PIL.Image.open(path)
    assert png.mode == g.meta["grid"][name]["mode"] and np.array_equal(np.array(png), g.npz[f"grid/{name}/png"])


# ---------------------------------------------------------------------------------------------------------------- generate / style mixing

def check_images(got, ref_u8, ref_float):
    """another fp32 evaluation of the same generator: no byte off by more than one level, and at most flip_cap of them different"""
    got, ref_u8 = np.asarray(got), np.asarray(ref_u8)
    assert got.dtype == np.uint8 and got.shape == ref_u8.shape
    diff = np.abs(got.astype(np.int32) - ref_u8.astype(np.int32))
    share, cap = float((diff != 0).mean()), iu.flip_cap(ref_float)
    print(f"max level difference {int(diff.max())}, share of differing bytes {share:.5f} (cap {cap:.5f})")
    assert int(diff.max()) <= 1 and share <= cap


@pytest.mark.parametrize("key", ["gen/plain", "gen/trunc", "gen/cond", "proj", "mix"])
def test_flip_cap_is_sound_for_the_fixture(key):
    """the reference's float images moved by +-1e-4 max|img| (the most another fp32 evaluation may differ) and quantised again: bytes move
    by at most one level and no more than flip_cap of them move"""
    g = iu.fixture()
    f, u8 = g.npz[f"{key}/float"], g.npz[f"{key}/uint8"]
    assert np.array_equal(image_export.quantize(torch.from_numpy(f), "clamp").numpy(), u8)
    e = np.float32(1e-4 * np.abs(f).max())
    for moved in (f + e, f - e):
        check_images(image_export.quantize(torch.from_numpy(moved), "clamp").numpy(), u8, f)


@pytest.mark.parametrize("tag", ["plain", "trunc", "cond"])
def test_generate_images_reproduces_the_reference(tmp_path, tag):
    g = iu.fixture()
    case = next(c for c in g.meta["gen"] if c["tag"] == tag)
    G = iu.oracle_generator(g, case["net"])
    out = generate.generate_images(G, seeds=case["seeds"], truncation_psi=case["psi"], class_idx=case["class_idx"], outdir=str(tmp_path))
    check_images(out, g.npz[f"gen/{tag}/uint8"], g.npz[f"gen/{tag}/float"])
    assert sorted(os.listdir(tmp_path)) == sorted(f"seed{s:04d}.png" for s in case["seeds"])
    for s, img in zip(case["seeds"], out):
        png = PIL.Image.open(tmp_path / f"seed{s:04d}.png")
        assert png.mode == "RGB" and np.array_equal(np.array(png), img)


def test_generate_from_projected_w(tmp_path, capsys):
    g = iu.fixture()
    G = iu.oracle_generator(g, "g16")
    npz = str(tmp_path / "projected_w.npz")
    np.savez(npz, w=g.npz["proj/ws"])
    out = generate.generate_images(G, seeds=[1], projected_w=npz, outdir=str(tmp_path / "o"))
    assert "warn: --seeds is ignored when using --projected-w" in capsys.readouterr().out
    check_images(out, g.npz["proj/uint8"], g.npz["proj/float"])
    assert sorted(os.listdir(tmp_path / "o")) == ["proj00.png", "proj01.png"]
    assert np.array_equal(generate.generate_images(G, projected_w=g.npz["proj/ws"]), out)
    with pytest.raises(AssertionError):
        generate.generate_images(G, projected_w=g.npz["proj/ws"][:, :3])


def test_generate_failures_and_warnings(capsys):
    g = iu.fixture()
    with pytest.raises(ValueError, match="--seeds option is required"):
        generate.generate_images(iu.oracle_generator(g, "g16"))
    with pytest.raises(ValueError, match="Must specify class label"):
        generate.generate_images(iu.oracle_generator(g, "c16"), seeds=[0])
    generate.generate_images(iu.oracle_generator(g, "g16"), seeds=[0], class_idx=2)
    assert "warn: --class=lbl ignored when running on an unconditional network" in capsys.readouterr().out


def test_num_range():
    assert generate.num_range("1,2,5") == [1, 2, 5] and generate.num_range("3-6") == [3, 4, 5, 6] and generate.num_range("7") == [7]
    with pytest.raises(ValueError):
        generate.num_range("a-b")


def test_style_mix_reproduces_the_reference(tmp_path):
    g = iu.fixture()
    mix = g.meta["mix"]
    G = iu.oracle_generator(g, mix["net"])
    d = style_mixing.generate_style_mix(G, mix["rows"], mix["cols"], col_styles=mix["styles"], truncation_psi=mix["psi"], outdir=str(tmp_path), batch=4)
    keys = [tuple(k) for k in g.npz["mix/keys"].tolist()]
    assert list(d.keys()) == keys                 # same entries in the same order (the unmixed images in Python's set order, then the matrix)
    got = np.stack([d[k] for k in keys])
    check_images(got, g.npz["mix/uint8"], g.npz["mix/float"])
    assert sorted(os.listdir(tmp_path)) == mix["files"]
    grid = np.array(PIL.Image.open(tmp_path / "grid.png"))
    R = G.img_resolution
    assert grid.shape == g.npz["mix/grid_png"].shape and not grid[:R, :R].any()
    check_images(grid, g.npz["mix/grid_png"], g.npz["mix/float"])
    assert np.array_equal(grid[R:2 * R, 2 * R:3 * R], d[(mix["rows"][0], mix["cols"][1])]) and np.array_equal(grid[:R, R:2 * R], d[(mix["cols"][0],) * 2])
    one = style_mixing.generate_style_mix(G, mix["rows"], mix["cols"], col_styles=mix["styles"], truncation_psi=mix["psi"], batch=1)
    assert all(np.array_equal(one[k], d[k]) for k in keys)


def test_cli_parsing():
    rest, a = generate.parse_args(["exp.config=sg2ada.yaml", "--snapshot=s.pt", "--outdir", "o", "--seeds=0-2", "--trunc", "0.7", "--class=3",
                                   "--noise-mode=random"])
    assert rest == ["exp.config=sg2ada.yaml"] and (a.snapshot, a.outdir, a.seeds, a.truncation_psi, a.class_idx, a.noise_mode, a.projected_w) == \
        ("s.pt", "o", [0, 1, 2], 0.7, 3, "random", None)
    _, a = generate.parse_args(["--snapshot=s", "--outdir=o", "--projected-w=p.npz"])
    assert (a.seeds, a.truncation_psi, a.class_idx, a.noise_mode, a.projected_w) == (None, 1, None, "const", "p.npz")
    for bad in (["--snapshot=s", "--outdir=o"], ["--outdir=o", "--seeds=1"], ["--snapshot=s", "--outdir=o", "--seeds=1", "--bogus"],
                ["--snapshot=s", "--outdir=o", "--seeds=1", "--noise-mode=loud"]):
        with pytest.raises(SystemExit):
            generate.parse_args(bad)
    rest, a = style_mixing.parse_args(["a.b=1", "--snapshot=s", "--outdir=o", "--rows=85,100", "--cols=1-3"])
    assert rest == ["a.b=1"] and (a.row_seeds, a.col_seeds, a.col_styles, a.truncation_psi, a.noise_mode) == ([85, 100], [1, 2, 3], list(range(7)), 1, "const")
    _, a = style_mixing.parse_args(["--snapshot=s", "--outdir=o", "--rows=1", "--cols=2", "--styles=0-2", "--trunc=0.5", "--noise-mode=none"])
    assert (a.col_styles, a.truncation_psi, a.noise_mode) == ([0, 1, 2], 0.5, "none")
    with pytest.raises(SystemExit):
        style_mixing.parse_args(["--snapshot=s", "--outdir=o", "--rows=1"])


# ---------------------------------------------------------------------------------------------------------------- the trainer

DCGAN_LIKE = {
    "exp": {"trainer": "base"},
    "gen": {"kimg": 3200, "batch": 128, "loss_arch": "base", "loss": "bcew", "generator": "cnn32_dcgan", "discriminator": "cnn32_dcgan",
            "g_reg_interval": 0, "d_reg_interval": 0},
    "gens_args": {"cnn32_dcgan": {"z_dim": 100}},
    "optim_gen_args": {"adam": {"lr": 0.0002, "betas": [0.5, 0.9]}},
    "optim_disc_args": {"adam": {"lr": 0.0002, "betas": [0.5, 0.9]}},
    "ema": {"use_ema": False},
    "aug": {"aug": "noaug"},
}


def _argv(tmp_path, *more):
    with open(os.path.join(tmp_path, "dcgan.yaml"), "w") as fh:
        yaml.safe_dump(DCGAN_LIKE, fh)
    return ["exp.config_dir=" + str(tmp_path), "exp.config=dcgan.yaml", "exp.name=run", "log.output=" + str(tmp_path / "logs"), "gen.batch=16",
            "gen.batch_gpu=16", "data.dataset=synthetic", "data.resolution=32", "gen.kimg=1"] + list(more)


def test_a_run_writes_no_image_unless_asked(tmp_path):
    trainer = starter.main(_argv(tmp_path), max_iterations=2)
    assert trainer.image_snapshot_iterations is None and trainer.grid_size is None
    assert not glob.glob(str(tmp_path / "**" / "*.png"), recursive=True)


@pytest.mark.parametrize("cond", [False, True])
def test_trainer_image_snapshots(tmp_path, cond):
    config = arguments.load_config(_argv(tmp_path, *(["data.cond=true", "data.num_classes=5"] if cond else [])))
    trainer = T.trainers[config.exp.trainer]().setup_arguments(config)
    trainer.image_snapshot_iterations = 2
    starter.multiprocesses_main(0, trainer, str(tmp_path), max_iterations=2)
    run = tmp_path / "logs" / "run"
    assert sorted(os.listdir(run)) == ["fakes000000.png", "fakes_init.png", "reals.png"]
    assert tuple(trainer.grid_size) == (32, 32) and sum(len(z) for z in trainer.grid_z) == 1024 and trainer.grid_c[0].shape[1] == (5 if cond else 0)
    for name in os.listdir(run):
        png = PIL.Image.open(run / name)
        assert png.mode == "RGB" and png.size == (1024, 1024)
    assert trainer.engine.G.training                    # eval mode was only borrowed
    # reals.png holds the data set's own bytes, cell by cell; fakes are the grid rule of G's output for the kept latents
    ds = trainer.dataset
    _, images, labels = T.setup_snapshot_image_grid(ds)
    reals = np.array(PIL.Image.open(run / "reals.png"))
    assert np.array_equal(reals[32:64, 64:96], images[32 + 2].transpose(1, 2, 0))
    if cond:
        assert all(len(set(np.argmax(labels[y * 32:(y + 1) * 32], 1))) == 1 for y in range(32))      # one class per grid row
    G = trainer.engine.G.eval()
    with torch.no_grad():
        img = torch.cat([G(z, c, noise_mode="const") for z, c in zip(trainer.grid_z, trainer.grid_c)]).float().cpu()
    G.train()
    path = trainer.save_image_snapshot()
    assert path.endswith("fakes000000.png")
    ref = str(tmp_path / "ref.png")
    T.save_image_grid(img.numpy(), ref, drange=[-1, 1], grid_size=trainer.grid_size)
    assert np.array_equal(np.array(PIL.Image.open(path)), np.array(PIL.Image.open(ref)))


def test_synthetic_data_set_offers_what_the_grid_reads():
    ds = T.SyntheticDataset(32, 3, 4, seed=3)
    before = T.SyntheticDataset(32, 3, 4, seed=3).batch(2, "cpu")
    img, label = ds[7]
    assert img.dtype == np.uint8 and img.shape == (3, 32, 32) and label.dtype == np.float32 and label.shape == (4,) and label.sum() == 1
    assert np.array_equal(ds[7][0], img) and not np.array_equal(ds[8][0], img) and len(ds) > 0
    assert int(ds.get_details(7).raw_label) == int(np.argmax(label)) and ds.get_details(7).raw_label.flat[::-1].shape == (1,)
    after = ds.batch(2, "cpu")                          # indexing does not move the stream `batch` draws from
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])
    assert T.SyntheticDataset(32, 3, 0, seed=3)[0][1].shape == (0,)
