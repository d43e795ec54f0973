"""What the six snapshot tools share (tool_support.py): the seeded latents and the class label, every tool's options pinned to what its parser
returned before the shared option helpers, the PNG writer, and that no tool module imports another."""
import importlib
import types

import numpy as np
import PIL.Image
import pytest
import torch

from style_big_gan_amd import tool_support as TS

TOOLS = ("generate", "style_mixing", "projector", "calc_metrics", "nearest_neighbors", "avg_spectra")
OVERRIDES = ["exp.config_dir=d", "exp.config=c.yaml"]


class _G:
    z_dim = 24

    def __init__(self, c_dim):
        self.c_dim = c_dim


def test_seed_latents_draw_what_both_earlier_forms_drew():
    seeds = [3, 0, 11, 2 ** 31 - 1]
    z = TS.seed_latents(_G(0), seeds)
    assert z.dtype == np.float64 and z.shape == (4, 24)
    assert np.array_equal(z, np.concatenate([np.random.RandomState(s).randn(1, 24) for s in seeds]))
    assert np.array_equal(z, np.stack([np.random.RandomState(s).randn(24) for s in seeds]))


def test_class_label(capsys):
    with pytest.raises(ValueError) as e:
        TS.class_label(_G(5), None, "cpu")
    assert str(e.value) == "Must specify class label with --class when using a conditional network"
    capsys.readouterr()
    label = TS.class_label(_G(0), 3, "cpu")
    assert tuple(label.shape) == (1, 0) and capsys.readouterr().out == "warn: --class=lbl ignored when running on an unconditional network\n"
    assert tuple(TS.class_label(_G(0), None, "cpu").shape) == (1, 0) and capsys.readouterr().out == ""
    label = TS.class_label(_G(5), 3, "cpu")
    assert label.dtype == torch.float32 and label.tolist() == [[0, 0, 0, 1, 0]] and capsys.readouterr().out == ""


def _parse_cases(snap, det, against):
    """per tool: [(argv, overrides, vars(args)) minimal, the same fully specified], a rejected argv.  The dictionaries are what the tools'
    own parsers returned for these argv before their declarations moved into tool_support."""
    return {
        "generate": (
            [(["--snapshot=S", "--seeds=1", "--outdir=o"], [],
              dict(class_idx=None, noise_mode="const", outdir="o", projected_w=None, seeds=[1], snapshot="S", truncation_psi=1)),
             (OVERRIDES + ["--snapshot=S", "--seeds=0-2", "--trunc=0.7", "--class=3", "--noise-mode=random", "--projected-w=w.npz", "--outdir=o"], OVERRIDES,
              dict(class_idx=3, noise_mode="random", outdir="o", projected_w="w.npz", seeds=[0, 1, 2], snapshot="S", truncation_psi=0.7))],
            ["--snapshot=S", "--outdir=o"]),
        "style_mixing": (
            [(["--snapshot=S", "--rows=1,2", "--cols=3", "--outdir=o"], [],
              dict(col_seeds=[3], col_styles=[0, 1, 2, 3, 4, 5, 6], noise_mode="const", outdir="o", row_seeds=[1, 2], snapshot="S", truncation_psi=1)),
             (OVERRIDES + ["--snapshot=S", "--rows=1,2", "--cols=3-5", "--styles=0-3", "--trunc=0.5", "--noise-mode=none", "--outdir=o"], OVERRIDES,
              dict(col_seeds=[3, 4, 5], col_styles=[0, 1, 2, 3], noise_mode="none", outdir="o", row_seeds=[1, 2], snapshot="S", truncation_psi=0.5))],
            ["--snapshot=S", "--rows=1,2", "--outdir=o"]),
        "projector": (
            [(["--snapshot=S", "--target=t.png", "--outdir=o", "--detector=v.pt"], [],
              dict(detector="v.pt", num_steps=1000, outdir="o", save_video=False, seed=303, snapshot="S", target="t.png")),
             (OVERRIDES + ["--snapshot=S", "--target=t.png", "--outdir=o", "--detector=v.pt", "--num-steps=5", "--seed=7", "--save-video"], OVERRIDES,
              dict(detector="v.pt", num_steps=5, outdir="o", save_video=True, seed=7, snapshot="S", target="t.png"))],
            ["--snapshot=S", "--target=t.png", "--outdir=o", "--detector=v.pt", "--frobnicate"]),
        "calc_metrics": (
            [([f"--snapshot={snap}", f"--detector={det}"], [],
              dict(data=None, detector=det, device="auto", gpus=1, metrics=["fid50k_full"], mirror=None, snapshot=snap, verbose=1)),
             (OVERRIDES + [f"--snapshot={snap}", f"--detector={det}", "--metrics=fid50k_full,pr50k3_full", "--data=/d", "--mirror=1", "--gpus=2",
                           "--verbose=0", "--device=cpu"], OVERRIDES,
              dict(data="/d", detector=det, device="cpu", gpus=2, metrics=["fid50k_full", "pr50k3_full"], mirror=True, snapshot=snap, verbose=0))],
            [f"--snapshot={snap}.absent", f"--detector={det}"]),
        "nearest_neighbors": (
            [([f"--snapshot={snap}", "--outdir=o", "--seeds=0-1"], [],
              dict(batch=64, class_idx=None, data=None, detector=None, device="auto", k=5, mirror=None, noise_mode="const", num=None, outdir="o",
                   res=None, seeds=[0, 1], snapshot=snap, space="pixel", truncation_psi=1)),
             (OVERRIDES + [f"--snapshot={snap}", "--outdir=o", "--seeds=0-1", "--num=4", "--k=3", "--space=pixel", f"--detector={det}", "--res=8",
                           "--data=/d", "--mirror=0", "--trunc=0.7", "--class=3", "--noise-mode=random", "--device=cpu", "--batch=8"], OVERRIDES,
              dict(batch=8, class_idx=3, data="/d", detector=det, device="cpu", k=3, mirror=False, noise_mode="random", num=4, outdir="o", res=8,
                   seeds=[0, 1], snapshot=snap, space="pixel", truncation_psi=0.7))],
            [f"--snapshot={snap}", "--outdir=o", "--seeds=0-1", "--k=0"]),
        "avg_spectra": (
            [(["--outdir=o"], [],
              dict(against=None, batch=64, class_idx=None, data=None, db_range=None, device="auto", interp=1, noise_mode="const", num=16384,
                   outdir="o", snapshot=None, truncation_psi=1)),
             (OVERRIDES + ["--outdir=o", f"--snapshot={snap}", f"--against={against}", "--num=8", "--interp=2", "--trunc=0.7", "--class=3",
                           "--noise-mode=random", "--device=cpu", "--batch=4", "--db-range=-60,10"], OVERRIDES,
              dict(against=against, batch=4, class_idx=3, data=None, db_range=(-60.0, 10.0), device="cpu", interp=2, noise_mode="random", num=8,
                   outdir="o", snapshot=snap, truncation_psi=0.7))],
            ["--outdir=o", f"--against={against}"]),
    }


@pytest.mark.parametrize("tool", TOOLS)
def test_options_are_what_the_tool_parsed_before(tool, tmp_path):
    snap, det, against = (str(tmp_path / name) for name in ("snap.pt", "det.pt", "against.npz"))
    for path in (snap, det, against):
        open(path, "wb").close()
    mod = importlib.import_module(f"style_big_gan_amd.{tool}")
    accepted, rejected = _parse_cases(snap, det, against)[tool]
    for argv, overrides, options in accepted:
        got_overrides, args = mod.parse_args(argv)
        assert got_overrides == overrides and vars(args) == options, argv
        assert {k: type(v) for k, v in vars(args).items()} == {k: type(v) for k, v in options.items()}, argv     # 1 is not 1.0, 0 not False
    with pytest.raises(SystemExit):
        mod.parse_args(rejected)


@pytest.mark.parametrize("channels,mode", [(1, "L"), (3, "RGB")])
def test_save_png_round_trip(channels, mode, tmp_path):
    img = np.random.RandomState(channels).randint(0, 256, [5, 7, channels], dtype=np.uint8)
    TS.save_png(img, str(tmp_path / "a.png"))
    TS.save_png(img[:, ::-1], str(tmp_path / "b.png"))           # a view that is not contiguous
    with PIL.Image.open(str(tmp_path / "a.png")) as a, PIL.Image.open(str(tmp_path / "b.png")) as b:
        assert a.mode == b.mode == mode and a.size == (7, 5)
        assert np.array_equal(np.asarray(a).reshape(5, 7, channels), img) and np.array_equal(np.asarray(b).reshape(5, 7, channels), img[:, ::-1])


@pytest.mark.parametrize("tool", TOOLS)
def test_no_tool_imports_another(tool):
    """by what the imported module holds, not by its text: neither another tool module nor a name defined in one"""
    others = {f"style_big_gan_amd.{t}" for t in TOOLS if t != tool}
    mod = importlib.import_module(f"style_big_gan_amd.{tool}")
    held = {v.__name__ if isinstance(v, types.ModuleType) else getattr(v, "__module__", None) for v in vars(mod).values()}
    assert not held & others, held & others
