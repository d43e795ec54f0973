"""The network summary tool on the CPU, end to end on a cnn32_dcgan snapshot a capped `starter.main` run wrote: the files, the totals, the
independence of --batch, `load_discriminator`, a dead channel and the first non-finite layer."""
import json
import os
import sys

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E402,F401
from style_big_gan_amd import arguments, network_summary as NS, starter, tool_support  # noqa: E402
from test_image_export_cpu import DCGAN_LIKE  # noqa: E402
import run_log_util as ru  # noqa: E402


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """-> (config overrides, snapshot path, its state) of a six-iteration DCGAN run"""
    tmp = tmp_path_factory.mktemp("network_summary")
    with open(os.path.join(tmp, "dcgan.yaml"), "w") as fh:
        yaml.safe_dump(DCGAN_LIKE, fh)
    overrides = ["exp.config_dir=" + str(tmp), "exp.config=dcgan.yaml", "exp.name=run", "log.output=" + str(tmp / "logs"), "data.dataset=synthetic",
                 "data.resolution=32"] + ru.RUN_ARGS
    starter.main(overrides, max_iterations=6)
    snap = str(tmp / "logs" / "run" / "network-snapshot-000000.pt")
    return overrides, snap, torch.load(snap, map_location="cpu", weights_only=True), tmp


def _tool(run, outdir, *more, snapshot=None):
    overrides, snap, _, _ = run
    return NS.run_network_summary(overrides + [f"--snapshot={snapshot or snap}", f"--outdir={outdir}", "--device=cpu", "--seeds=0-7"] + list(more))


def _strict(text):
    def refuse(token):
        raise ValueError(f"not strict JSON: {token}")
    return json.loads(text, parse_constant=refuse)


@pytest.fixture(scope="module")
def batch3(run):
    out = str(run[3] / "out3")
    return out, _tool(run, out, "--batch=3")


def test_files_totals_and_columns(run, batch3):
    _, _, state, _ = run
    out, result = batch3
    assert sorted(os.listdir(out)) == ["exponents.png", "summary.json", "summary.npz", "summary.txt"]
    report = _strict(open(os.path.join(out, "summary.json")).read())
    assert report["options"]["seeds"] == list(range(8)) and report["options"]["batch"] == 3 and report["options"]["data"] is False
    nets = report["networks"]
    assert list(nets) == ["G", "D(fake)"] and nets["G"]["samples"] == nets["D(fake)"]["samples"] == 8
    for key, which in (("G", "G"), ("D(fake)", "D")):
        named = {k: v for k, v in state[which].items()}
        buffers = sum(v.numel() for k, v in named.items() if k.endswith(("running_mean", "running_var", "num_batches_tracked")))
        assert nets[key]["parameters"] == sum(v.numel() for v in named.values()) - buffers and nets[key]["buffers"] == buffers
        assert nets[key]["first_nonfinite"] is None
    g = {e["name"]: e for e in nets["G"]["entries"]}
    assert g["main.0"]["shape"] == [3, 512 * 2, 2, 2] and g["main.0"]["dtype"] == "float32" and g["main.0"]["memory_format"] == "contiguous"
    last = g["main.13"]["stats"]                                                # tanh: inside [-1, 1]
    assert last["n"] == 8 * 3 * 32 * 32 and 0 < last["absmax"] <= 1 and last["nonfinite"] == 0 and last["dead_channels"] == []
    assert last["fp16_headroom_bits"] == pytest.approx(np.log2(65504 / last["absmax"]))
    d = {e["name"]: e for e in nets["D(fake)"]["entries"]}
    assert d["linear"]["shape"] == [3, 1] and d["linear"]["stats"]["n"] == 8
    text = open(os.path.join(out, "summary.txt")).read()
    assert "Generator32_dcgan  Parameters  Buffers  Output shape" in text and "Discriminator32_dcgan" in text
    assert "fp16 bits  zero %  peak %  nonfinite  dead ch" in text and "D(fake): activation statistics over 8 samples" in text
    import PIL.Image
    rows = sum(1 for n in nets.values() for e in n["entries"] if e["stats"] is not None)
    assert PIL.Image.open(os.path.join(out, "exponents.png")).size == (64 * NS.CELL, rows * NS.CELL)
    # summary.npz derives the same numbers again
    arrays = np.load(os.path.join(out, "summary.npz"))
    key = [k for k in arrays.files if k.startswith("G.") and ".main.13." in k and k.endswith(".counts")][0]
    again = NS.act_stats.derive(arrays[key], arrays[key.replace(".counts", ".values")])
    again.pop("channels")
    assert again == last


def test_the_batch_size_does_not_change_a_bit(run, batch3):
    out8 = str(run[3] / "out8")
    _tool(run, out8, "--batch=8")
    a, b = np.load(os.path.join(batch3[0], "summary.npz")), np.load(os.path.join(out8, "summary.npz"))
    assert a.files == b.files and len(a.files) > 20
    for k in a.files:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape and (x.view(np.int64) == y.view(np.int64)).all(), k


def test_load_discriminator_is_strict_and_refuses_a_snapshot_without_d(run):
    overrides, snap, state, tmp = run
    config = arguments.load_config(overrides)
    G = tool_support.load_generator(config, snap, "cpu", announce=False)
    D = tool_support.load_discriminator(config, snap, G, "cpu")
    assert not D.training and not any(p.requires_grad for p in D.parameters())
    assert all(torch.equal(v, state["D"][k]) for k, v in D.state_dict().items())
    broken = dict(state, D={k: v for k, v in state["D"].items() if k != "linear.bias"})
    torch.save(broken, str(tmp / "network-snapshot-broken.pt"))
    with pytest.raises(RuntimeError, match="linear.bias"):
        tool_support.load_discriminator(config, str(tmp / "network-snapshot-broken.pt"), G, "cpu")
    torch.save({k: v for k, v in state.items() if k != "D"}, str(tmp / "network-snapshot-nod.pt"))
    with pytest.raises(RuntimeError, match="holds no discriminator"):
        tool_support.load_discriminator(config, str(tmp / "network-snapshot-nod.pt"), G, "cpu")
    with pytest.raises(RuntimeError, match="holds no discriminator"):
        _tool(run, str(tmp / "nod"), snapshot=str(tmp / "network-snapshot-nod.pt"))
    _tool(run, str(tmp / "gonly"), "--networks=G", snapshot=str(tmp / "network-snapshot-nod.pt"))          # G alone needs no D
    assert list(_strict(open(tmp / "gonly" / "summary.json").read())["networks"]) == ["G"]


def _edited(run, name, edit):
    _, _, state, tmp = run
    g = {k: v.clone() for k, v in state["G"].items()}
    edit(g)
    path = str(tmp / f"network-snapshot-{name}.pt")
    torch.save(dict(state, G=g), path)
    return path


def test_a_dead_channel_is_reported(run):
    def edit(g):
        g["main.3.weight"][:, 5] = 0                                            # ConvTranspose2d weight [in, out, k, k]; the layer has no bias
    out = str(run[3] / "dead")
    _tool(run, out, "--networks=G", snapshot=_edited(run, "dead", edit))
    entries = _strict(open(os.path.join(out, "summary.json")).read())["networks"]["G"]["entries"]
    dead = {e["name"]: e["stats"]["dead_channels"] for e in entries if e["stats"] is not None}
    assert dead["main.3"] == [5] and all(v == [] for k, v in dead.items() if k != "main.3")


def test_the_first_nonfinite_layer_is_named(run):
    def edit(g):
        g["main.6.weight"][0, 0, 0, 0] = float("inf")
    out = str(run[3] / "inf")
    _tool(run, out, snapshot=_edited(run, "inf", edit))
    nets = _strict(open(os.path.join(out, "summary.json")).read())["networks"]
    assert nets["G"]["first_nonfinite"] == "main.6" and nets["D(fake)"]["first_nonfinite"] == "main.0"
    by_name = {e["name"]: e["stats"] for e in nets["G"]["entries"]}
    assert by_name["main.3"]["nonfinite"] == 0 and by_name["main.6"]["nonfinite"] > 0
    assert "G: the first entry with a NaN or an infinity is main.6" in open(os.path.join(out, "summary.txt")).read()


def test_option_failures(run, capsys):
    for bad, message in ((["--networks=G,E"], "a list of G, D"), (["--batch=0"], "at least 1"), (["--frobnicate"], "unrecognised")):
        with pytest.raises(SystemExit):
            _tool(run, str(run[3] / "bad"), *bad)
        assert message in capsys.readouterr().err
