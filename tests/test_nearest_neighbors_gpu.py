"""The nearest_neighbors tool on the device against its own CPU run (a mirrored 32 x 32 folder of 200 images, a stand-in generator whose
bytes are the same on both devices), the launches it makes, and the CLI with the package's generator."""
import json

import numpy as np
import PIL.Image
import pytest
import torch

import nearest_util as N
from golden_util import make_image_folder
from test_calc_metrics_cpu import _run
from style_big_gan_amd import _lib, nearest_neighbors as NN
from style_big_gan_amd.train_parts.datasets import ImageFolderDataset

pytestmark = pytest.mark.gpu


def _logged(fn):
    _lib.prof_enable(True)
    try:
        _lib.prof_fetch()
        out = fn()
        return out, [r for r in _lib.prof_fetch()]
    finally:
        _lib.prof_enable(False)


@pytest.mark.parametrize("res", [None, 16])
def test_device_run_equals_the_cpu_run(dev, tmp_path, res):
    dataset = ImageFolderDataset(path=make_image_folder(str(tmp_path / "data"), n=200, res=32), xflip=True)
    assert len(dataset) == 400
    G = N.BankGenerator(N.make_bank(dataset, 40))
    seeds, num, k, batch = [5, 1, 30, 8], 50, 5, 16
    kw = dict(seeds=seeds, num=num, k=k, res=res, batch=batch)
    want = NN.nearest_training_images(G, dataset, device=torch.device("cpu"), **kw)
    got, log = _logged(lambda: NN.nearest_training_images(G.to(dev), dataset, device=dev, **kw))
    assert got["mirrored"] and got["F"] == want["F"] == 3 * (res or 32) ** 2
    assert got["neighbors"] == want["neighbors"]                # d2, items, flips, files and rmse
    assert np.array_equal(got["canvas"], want["canvas"])
    assert np.array_equal(got["gen_to_train"], want["gen_to_train"]) and np.array_equal(got["train_to_train"], want["train_to_train"])
    assert got["stats"] == want["stats"]
    assert got["gen_to_train"].dtype == np.int64 and (got["gen_to_train"] == 0).any() and (got["train_to_train"] > 0).all()
    # every search ran on the kernels: two tile launches (as stored, mirrored) per query batch, none of them served elsewhere
    tiles = [r for r in log if r["kind"] == "nn_u8" and _lib.NN_VARIANTS[r["dims"][0]] in ("single", "split")]
    calls = len(seeds) + -(-num // batch) + -(-200 // batch)
    assert len(tiles) == 2 * calls, (len(tiles), calls)
    assert all(r["dims"][2] == 200 and r["dims"][3] == got["F"] for r in tiles)
    assert sorted({r["dims"][4] for r in tiles}) == [1, k]
    kinds = {r["kind"] for r in log}
    assert {"nn_u8", "resident", "image_export"} <= kinds and (("resample" in kinds) == (res is not None))


def test_cli_run_on_the_device(dev, tmp_path, capsys):
    """the package's generator: the listed d2 are those of the PNG's own cells, and every neighbour cell is the listed training image"""
    _, overrides, snap, data = _run(tmp_path, n_images=24)
    out = tmp_path / "out"
    result = NN.run_nearest_neighbors(overrides + [f"--snapshot={snap}", f"--outdir={out}", "--seeds=0-2", "--num=9", "--k=3", "--batch=4"])
    dataset = ImageFolderDataset(path=data, xflip=True)
    listing = json.load(open(out / "neighbors.json"))
    png = np.array(PIL.Image.open(out / "neighbors.png")).astype(np.int64)
    assert png.shape == (3 * 16, 4 * 16, 3)
    for r, seed in enumerate(range(3)):
        cells = png[r * 16:(r + 1) * 16].reshape(16, 4, 16, 3).transpose(1, 3, 0, 2)
        rows = listing["seeds"][str(seed)]
        d2, item = N.brute_force(cells[:1].astype(np.uint8), N.dataset_items(dataset), 3)
        assert [n["d2"] for n in rows] == d2[0].tolist() and [n["item"] for n in rows] == item[0].tolist()
        for t, n in enumerate(rows):
            assert np.array_equal(cells[1 + t], dataset[n["item"]][0]) and n["flip"] == int(n["item"] >= 24)
    npz = np.load(out / "nn_stats.npz")
    assert npz["gen_to_train"].shape == (9,) and np.array_equal(npz["train_to_train"], N.brute_train_to_train(dataset))
    assert json.load(open(out / "nn_stats.json")) == result["stats"]
