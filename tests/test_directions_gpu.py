"""The latent directions kernels on the device: `column_mean`, `gram` and `edit_table` equal the op's CPU path bit for bit (partial tiles, the
odd-row pad, chunk and group edges, mirrored tiles, the production width, a constant column, a column of subnormal numbers), the launch records,
the refusals, and the tool with --device=cuda: from a snapshot of this build, and against its own CPU run with the exact stand-in generator."""
import json
import os

import numpy as np
import PIL.Image
import pytest
import torch

import directions_util as du
from exact_util import expect_launch
from test_calc_metrics_cpu import _run
from style_big_gan_amd import _lib, arguments, directions as DR, tool_support
from style_big_gan_amd.torch_utils.ops import directions as ops

pytestmark = pytest.mark.gpu

SHAPES = [(1, 16, None), (2, 32, None), (3, 40, "constant"), (255, 32, None), (257, 96, "denormal"), (4097, 32, None), (130, 512, None), (600, 128, None)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _d(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x).copy()).to(dev)


@pytest.mark.parametrize("n,d,special", SHAPES)
def test_mean_and_gram_equal_the_cpu_path_bit_for_bit(dev, n, d, special):
    x = du.table(n, d, special)
    want_mean, want_plain, want_centred = du.cpu_results(n, d, special)
    xd = _d(x, dev)
    mean = ops.column_mean(xd)
    assert mean.dtype == torch.float64 and du.same_bits(mean.cpu().numpy(), want_mean)
    plain, centred = ops.gram(xd), ops.gram(xd, mean.to(torch.float32))
    for got, want in ((plain, want_plain), (centred, want_centred)):
        got = got.cpu().numpy()
        assert got.dtype == np.float64 and got.shape == (d, d)
        assert du.same_bits(got, got.T)                          # symmetric bit for bit
        assert du.same_bits(got, want)
    if special == "constant":
        c = centred.cpu().numpy()
        assert not c[1].any() and not c[:, 1].any() and c[0, 0] > 0
    if special == "denormal":
        assert 0 < np.abs(x[:, 2]).max() < 2.0 ** -126 and want_plain[2, 0] != 0      # subnormal inputs reach the products un-flushed
    again = ops.gram(xd, mean.to(torch.float32))
    assert torch.equal(again.view(torch.int64), centred.view(torch.int64))            # two launches, the same bits


@pytest.mark.parametrize("s,l,d,k,t", [(2, 3, 16, 2, 3), (3, 14, 512, 5, 5)])
def test_edit_table_equals_the_cpu_path_bit_for_bit(dev, s, l, d, k, t):
    rng = np.random.RandomState(s + d)
    ws, comps, scale = rng.randn(s, l, d).astype(np.float32), rng.randn(k, d).astype(np.float32), (rng.rand(k) + 0.5).astype(np.float32)
    sigmas, layers = DR.sigma_table(2.5, t), list(range(1, l, 2))
    host = [torch.from_numpy(v) for v in (ws, comps, scale, sigmas)]
    want = ops.edit_table(*host, layers).numpy()
    got = ops.edit_table(*[v.to(dev) for v in host], layers)
    assert got.device == dev and du.same_bits(got.cpu().numpy(), want)
    cells = got.cpu().numpy().reshape(s, k, t, l, d)
    assert all(np.array_equal(cells[:, i, t // 2], ws) for i in range(k)) and du.same_bits(cells[:, :, :, 0], np.broadcast_to(ws[:, None, None, 0], [s, k, t, d]))


def test_an_empty_edit_table(dev):
    z = lambda *shape: torch.zeros(shape, device=dev)
    for s, k, t in [(0, 2, 3), (2, 0, 3), (2, 2, 0)]:
        out = ops.edit_table(z(s, 3, 16), z(k, 16), z(k), z(t), [0])
        assert out.shape == (0, 3, 16) and out.dtype == torch.float32 and out.device == dev


def test_launch_records(dev):
    x = _d(du.table(4097, 32), dev)
    with expect_launch("directions", lambda r: r[:4] == (1, 4097, 32, 2), "gram") as log:
        ops.gram(x)
    recs = [r["dims"][:4] for r in log if r["kind"] == "directions"]
    assert recs == [(1, 4097, 32, 2), (2, 4097, 32, 2)]          # one gram, one merge: (variant, N, D, groups)
    with expect_launch("directions", lambda r: r[:4] == (0, 4097, 32, 5), "mean") as log:
        ops.column_mean(x)
    assert [r["dims"][:4] for r in log if r["kind"] == "directions"] == [(0, 4097, 32, 5), (2, 4097, 32, 5)]
    z = lambda *shape: torch.zeros(shape, device=dev)
    with expect_launch("directions", lambda r: r[:6] == (3, 2, 4, 5, 3, 16), "edit") as log:
        ops.edit_table(z(2, 3, 16), z(4, 16), z(4), z(5), [1])
    assert [_lib.DIRECTIONS_VARIANTS[r["dims"][0]] for r in log if r["kind"] == "directions"] == ["edit"]


def test_refusals_on_the_device(dev):
    x = torch.zeros([4, 8], device=dev)
    for fn in (ops.column_mean, ops.gram):
        for bad, message in [(x.double(), r"float64.*\(4, 8\)"), (x.t(), r"\(8, 4\)"), (x[:, ::2], r"\(4, 4\)"), (torch.zeros([1, 1025], device=dev), r"\(1, 1025\)"),
                             (x[:0], r"\(0, 8\)")]:
            with pytest.raises(RuntimeError, match=message):
                fn(bad)
    for mean, message in [(torch.zeros([8]), "cpu"), (torch.zeros([8], dtype=torch.float64, device=dev), "float64"), (torch.zeros([16], device=dev)[::2], r"\(8,\)")]:
        with pytest.raises(RuntimeError, match=message):
            ops.gram(x, mean)
    with pytest.raises(RuntimeError, match="cpu"):
        ops.edit_table(torch.zeros([2, 3, 8], device=dev), torch.zeros([2, 8]), torch.zeros([2], device=dev), torch.zeros([3], device=dev), [0])
    # the library's own checks, below the op layer's
    lib = _lib.load()
    out, ws = torch.full([8, 8], -7.0, dtype=torch.float64, device=dev), torch.zeros([4096], device=dev)
    for refused, message in [(lambda: lib.sbg_directions_gram(x.data_ptr(), None, out.data_ptr(), ws.data_ptr(), 4, 1025, _lib.stream_ptr(dev)), "[4, 1025]"),
                             (lambda: lib.sbg_directions_gram(x.data_ptr(), None, out.data_ptr(), ws.data_ptr(), 0, 8, _lib.stream_ptr(dev)), "[0, 8]"),
                             (lambda: lib.sbg_directions_gram(None, None, out.data_ptr(), ws.data_ptr(), 4, 8, _lib.stream_ptr(dev)), "null or misaligned"),
                             (lambda: lib.sbg_directions_mean(x.data_ptr(), out.data_ptr(), None, 4, 8, _lib.stream_ptr(dev)), "null or misaligned")]:
        status = refused()
        assert status == 1 and message in lib.sbg_last_error().decode(), message
    torch.cuda.synchronize()
    assert bool((out == -7).all())                               # a refused call launches nothing


def test_the_tool_from_a_snapshot_of_this_build(dev, tmp_path, capsys):
    _, overrides, snap, _ = _run(tmp_path)
    out = tmp_path / "out"
    result = DR.run_directions(overrides + [f"--snapshot={snap}", f"--outdir={out}", "--device=cuda", "--num=300", "--components=3", "--seeds=0,1", "--steps=3"])
    assert sorted(os.listdir(out)) == ["directions.json", "directions.npz", "seed0000.png", "seed0001.png"]
    stats = json.loads(open(out / "directions.json").read(), parse_constant=lambda name: pytest.fail(f"directions.json holds {name}"))
    assert stats == result["stats"] and (stats["method"], stats["num"], stats["w_dim"], stats["num_ws"]) == ("pca", 300, 16, 6)
    assert sum(c["explained"] for c in stats["components"]) <= 1 and 1 <= stats["effective_dim"] <= 16
    npz = np.load(out / "directions.npz")
    assert npz["components"].shape == (3, 16) and npz["eigenvalues"].shape == (16,) and npz["sigmas"].tolist() == [-2.0, 0.0, 2.0]
    G = tool_support.load_generator(arguments.load_config(overrides), snap, dev, announce=False)
    for seed in (0, 1):
        png = np.array(PIL.Image.open(out / f"seed{seed:04d}.png"))
        assert png.shape == (48, 48, 3)
        want = tool_support.generated_images(G, [seed], tool_support.class_label(G, None, dev), 1, "const", dev)[0].permute(1, 2, 0).cpu().numpy()
        for k in range(3):
            assert np.array_equal(png[16 * k:16 * k + 16, 16:32], want), (seed, k)
        assert not np.array_equal(png[:16, :16], png[:16, 32:])
    # sefa on the device: the conv affines of the ws indices 0..2
    res = DR.latent_directions(G, method="sefa", layers="0-2", components=3, device=dev)
    rows = torch.from_numpy(DR.sefa_rows(G, [0, 1, 2]))
    assert rows.shape == (48, 16) and du.same_bits(res["arrays"]["eigenvalues"], DR.eigen(ops.gram(rows).numpy(), 3)[1])
    with pytest.raises(ValueError, match="ToRGB"):
        DR.latent_directions(G, method="sefa", layers="5", components=3, device=dev)


def test_the_tool_on_the_device_equals_its_cpu_run(dev, tmp_path):
    """the stand-in generator is exact in fp32 on both devices, so every file is the same: the Gram matrix handed to eigh has the same bits"""
    runs = {}
    for name, device in (("cpu", torch.device("cpu")), ("cuda", dev)):
        G = du.ExactGenerator().to(device)
        runs[name] = DR.latent_directions(G, num=700, seed=2, components=5, layers="1-4", seeds=[0, 7], extent=1.5, steps=5, truncation_psi=0.5, batch=16,
                                          device=device, outdir=str(tmp_path / name))
    assert sorted(os.listdir(tmp_path / "cpu")) == sorted(os.listdir(tmp_path / "cuda")) == ["directions.json", "directions.npz", "seed0000.png", "seed0007.png"]
    a, b = np.load(tmp_path / "cpu" / "directions.npz"), np.load(tmp_path / "cuda" / "directions.npz")
    assert sorted(a.files) == sorted(b.files) and all(du.same_bits(a[k], b[k]) for k in a.files)
    assert open(tmp_path / "cpu" / "directions.json").read() == open(tmp_path / "cuda" / "directions.json").read()
    for name in ("seed0000.png", "seed0007.png"):
        assert open(tmp_path / "cpu" / name, "rb").read() == open(tmp_path / "cuda" / name, "rb").read()
        assert np.array_equal(runs["cpu"]["grids"][name], runs["cuda"]["grids"][name]) and runs["cpu"]["grids"][name].shape == (5 * 8, 5 * 8, 3)
    assert len(np.unique(runs["cuda"]["grids"]["seed0000.png"])) > 8
