"""nearest_neighbors --space=vgg16 on the device against the same run on the CPU (the stand-in detector of the CPU test: exact features, so
both devices must agree in every bit), and the kernels that served it."""
import numpy as np
import pytest
import torch

import nearest_util as N
from golden_util import make_image_folder
from test_nearest_neighbors_feature_cpu import detector
from style_big_gan_amd import _lib, nearest_neighbors as NN
from style_big_gan_amd.train_parts.datasets import ImageFolderDataset

pytestmark = pytest.mark.gpu


def test_device_run_equals_the_cpu_run(dev, tmp_path):
    kw = dict(path=make_image_folder(str(tmp_path / "data"), n=200, res=32), xflip=True)
    dataset = ImageFolderDataset(**kw)
    assert len(dataset) == 400
    bank = N.make_bank(dataset, 40)
    seeds = list(range(16))
    run = lambda G, device: NN.nearest_training_images(G, dataset, seeds=seeds, num=40, k=5, batch=16, device=device, space="vgg16", detector=detector,
                                                       dataset_kwargs=kw)
    want = run(N.BankGenerator(bank), torch.device("cpu"))
    _lib.prof_enable(True)
    try:
        _lib.prof_fetch()
        got = run(N.BankGenerator(bank).to(dev), dev)
        torch.cuda.synchronize()
        log = _lib.prof_fetch()
    finally:
        _lib.prof_enable(False)
    assert got["F"] == want["F"] == 192 and got["mirrored"]
    for seed in seeds:
        a, b = got["neighbors"][seed], want["neighbors"][seed]
        assert [n["item"] for n in a] == [n["item"] for n in b] and [n["flip"] for n in a] == [n["flip"] for n in b], seed
        assert [np.float32(n["d2"]).view(np.uint32) for n in a] == [np.float32(n["d2"]).view(np.uint32) for n in b], seed
        assert a == b
    assert {0, 1} <= {n["flip"] for s in seeds for n in got["neighbors"][s]}
    assert np.array_equal(got["canvas"], want["canvas"])
    for name in ("gen_to_train", "train_to_train"):
        assert got[name].dtype == np.float32 and np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), name
    assert got["train_to_train"].shape == (200,) and got["stats"] == want["stats"]
    tiles = [r["dims"] for r in log if r["kind"] == "pr" and _lib.PR_VARIANTS[r["dims"][0]] in ("single", "split")]
    assert len(tiles) == 3 and all(d[6] == 3 for d in tiles), tiles                 # the seeds, the --num images, the baseline
    assert [(d[1], d[2], d[3], d[4]) for d in tiles] == [(16, 400, 192, 5), (40, 400, 192, 1), (200, 400, 192, 2)]
    assert not [r for r in log if r["kind"] == "nn_u8"]
