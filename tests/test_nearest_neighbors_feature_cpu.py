"""nearest_neighbors --space=vgg16 on the CPU, with a stand-in detector whose features are exact: uint8 [N, 3, H, W] ->
(images[:, :, ::H//8, ::W//8] - 128) flattened to float32 [N, 192].  It is integer-valued with |v| <= 128; 4 * 192 * 128^2 = 12.6 M < 2^24
and d2 <= 192 * 255^2 < 2^24, so every fp32 sum of the definition is exact and the feature-space search equals `nearest_util.brute_force`
over the subsampled items of the data set: the d2 as integers, the items in the same order."""
import json
import os
import zipfile

import numpy as np
import PIL.Image
import pytest
import torch

import nearest_util as N
from golden_util import make_image_folder
from test_calc_metrics_cpu import _cpu_generator, _run
from style_big_gan_amd import arguments, nearest_neighbors as NN
from style_big_gan_amd.metrics import metric_utils
from style_big_gan_amd.torch_utils.ops import image_export
from style_big_gan_amd.train_parts.datasets import ImageFolderDataset

CPU = torch.device("cpu")


def detector(images):
    """the stand-in: a callable takes the images alone"""
    assert images.dtype == torch.uint8 and images.shape[1] == 3
    H, W = images.shape[2:]
    return (images[:, :, ::H // 8, ::W // 8].to(torch.float32) - 128).flatten(1)


def reduce(img):
    """what the detector sees of a data set image, as bytes: uint8 [C, H, W] -> [3, 8, 8]"""
    img = np.repeat(img, 3, axis=0) if img.shape[0] == 1 else img
    return img[:, ::img.shape[1] // 8, ::img.shape[2] // 8]


class ScriptedDetector(torch.nn.Module):
    """the same features as a TorchScript file with the reference detectors' call signature"""

    def forward(self, images: torch.Tensor, return_features: bool = False):
        sh, sw = images.shape[2] // 8, images.shape[3] // 8
        return (images[:, :, ::sh, ::sw].to(torch.float32) - 128.0).flatten(1)


def _grey_folder(root, n=9, res=16, seed=5):
    rng = np.random.RandomState(seed)
    os.makedirs(root)
    for i in range(n):
        PIL.Image.fromarray(rng.randint(0, 256, [res, res], dtype=np.uint8), "L").save(os.path.join(root, f"img{i:03d}.png"))
    return root


def _data(tmp_path, kind):
    if kind == "grey":
        kw = dict(path=_grey_folder(str(tmp_path / "grey")), xflip=True)
    else:
        kw = dict(path=make_image_folder(str(tmp_path / "data"), n=23, res=16), xflip=kind == "mirrored")
    return ImageFolderDataset(**kw), kw


def _check_neighbors(result, G, dataset, seeds, k):
    """the tool's lists against the brute-force search over the subsampled dataset[i]; the canvas against the data set's images"""
    queries = N.seed_bytes(G, seeds)
    items = N.dataset_items(dataset, reduce)
    d2, item = N.brute_force(np.stack([reduce(x) for x in queries]), items, k)
    C, H, W = dataset.image_shape
    assert result["space"] == "vgg16" and result["F"] == 192 == items.shape[1] and result["k"] == k
    assert result["canvas"].shape == (len(seeds) * H, (k + 1) * W, C)
    for r, seed in enumerate(seeds):
        rows = result["neighbors"][seed]
        assert [set(n) for n in rows] == [{"item", "file", "flip", "d2", "dist"}] * k
        assert [n["item"] for n in rows] == item[r].tolist() and [n["d2"] for n in rows] == d2[r].tolist(), seed
        assert [n["flip"] for n in rows] == [int(dataset._xflip[i]) for i in item[r]]
        assert [n["file"] for n in rows] == [dataset._image_fnames[dataset._raw_idx[i]] for i in item[r]]
        assert all(n["dist"] == float(np.sqrt(np.float64(n["d2"]))) for n in rows)
        cells = result["canvas"][r * H:(r + 1) * H].reshape(H, k + 1, W, C).transpose(1, 3, 0, 2)          # [cell, C, H, W]
        assert np.array_equal(cells[0], queries[r])
        for t in range(k):                                      # full resolution, mirrored where the item is a mirrored one
            assert np.array_equal(cells[1 + t], dataset[int(item[r, t])][0]), (seed, t)
    return d2


@pytest.mark.parametrize("kind", ["mirrored", "plain", "grey"])
def test_feature_space_equals_brute_force(tmp_path, kind):
    dataset, kw = _data(tmp_path, kind)
    assert len(dataset) == dict(mirrored=46, plain=23, grey=18)[kind]
    G = N.BankGenerator(N.make_bank(dataset, 24))
    seeds = list(range(12))
    out = tmp_path / "out"
    result = NN.nearest_training_images(G, dataset, seeds=seeds, num=12, k=5, batch=5, device=CPU, outdir=str(out), space="vgg16", detector=detector,
                                        dataset_kwargs=kw)
    assert result["mirrored"] == (kind != "plain") and result["res"] == 16
    d2 = _check_neighbors(result, G, dataset, seeds, 5)
    if kind == "mirrored":                                      # the bank holds training images in both orientations
        assert {0, 1} <= {n["flip"] for s in seeds for n in result["neighbors"][s] if n["d2"] == 0}
    # files
    assert sorted(os.listdir(out)) == ["neighbors.json", "neighbors.png", "nn_stats.json", "nn_stats.npz"]
    listing = json.load(open(out / "neighbors.json"))
    assert set(listing) == {"space", "F", "k", "seeds"} and (listing["space"], listing["F"], listing["k"]) == ("vgg16", 192, 5)
    assert listing["seeds"] == {str(s): result["neighbors"][s] for s in seeds}
    png = np.array(PIL.Image.open(out / "neighbors.png"))
    assert np.array_equal(png.reshape(result["canvas"].shape), result["canvas"])
    # statistics: float32 d2; train_to_train per stored image, neither itself nor its mirrored twin
    base = N.brute_train_to_train(dataset, reduce)
    npz = np.load(out / "nn_stats.npz")
    assert sorted(npz.files) == ["gen_to_train", "train_to_train"] and npz["gen_to_train"].dtype == npz["train_to_train"].dtype == np.float32
    assert np.array_equal(npz["gen_to_train"], d2[:, 0]) and np.array_equal(npz["train_to_train"], base)
    assert base.shape == (len(np.unique(dataset._raw_idx)),) and (base > 0).all()
    stats = json.load(open(out / "nn_stats.json"))
    assert stats == result["stats"]
    assert set(stats) == {"space", "F", "res", "num", "stored_images", "mirrored", "gen_to_train", "train_to_train", "train_p01_d2", "fraction_below_train_p01"}
    for name, values in (("gen_to_train", d2[:, 0]), ("train_to_train", base)):
        dist = np.sqrt(values.astype(np.float64))
        q = np.quantile(dist, [0.01, 0.05, 0.25, 0.5, 0.75])
        want = dict(min=dist.min(), mean=dist.mean(), p01=q[0], p05=q[1], p25=q[2], p50=q[3], p75=q[4])
        assert set(stats[name]) == set(want) and all(abs(stats[name][key] - want[key]) < 1e-9 for key in want)
    p01 = np.quantile(base.astype(np.float64), 0.01)
    assert stats["train_p01_d2"] == p01 and stats["fraction_below_train_p01"] == float(np.mean(d2[:, 0] <= p01))
    assert (stats["space"], stats["num"], stats["stored_images"], stats["res"]) == ("vgg16", 12, len(base), 16)


def test_a_generator_that_returns_training_images_is_flagged(tmp_path):
    dataset, kw = _data(tmp_path, "mirrored")
    bank = np.stack([dataset[i][0] for i in range(0, 46, 3)])   # training images, mirrored ones among them
    result = NN.nearest_training_images(N.BankGenerator(bank), dataset, num=30, batch=7, device=CPU, space="vgg16", detector=detector, dataset_kwargs=kw)
    assert result["gen_to_train"].shape == (30,) and not result["gen_to_train"].any()
    assert result["stats"]["fraction_below_train_p01"] == 1 and result["stats"]["gen_to_train"]["mean"] == 0
    assert result["stats"]["train_to_train"]["min"] > 0


def test_refusals(tmp_path, capsys):
    dataset, kw = _data(tmp_path, "plain")
    G = N.BankGenerator(N.make_bank(dataset, 8))
    run = lambda **more: NN.nearest_training_images(G, dataset, seeds=[0], device=CPU, **dict(dict(k=2, space="vgg16", dataset_kwargs=kw), **more))
    with pytest.raises(ValueError, match="needs --detector"):
        run()
    with pytest.raises(ValueError, match="--res cannot be combined"):
        run(detector=detector, res=8)
    with pytest.raises(ValueError, match="must be one of pixel, vgg16"):
        run(detector=detector, space="lpips")
    with pytest.raises(ValueError, match="needs dataset_kwargs"):
        run(detector=detector, dataset_kwargs=None)
    with pytest.raises(ValueError, match="multiple of 8"):
        run(detector=lambda images: detector(images)[:, :190])
    with pytest.raises(ValueError, match="not all finite"):
        run(detector=lambda images: detector(images) * torch.where(torch.arange(192) == 7, float("nan"), 1.0))

    def nan_for_generated(images):                              # the data set's features are fine, one generated image's are not
        f = detector(images)
        return f if images.shape[0] > 1 else f * float("inf")
    with pytest.raises(ValueError, match="generated images are not all finite"):
        run(detector=nan_for_generated)
    with pytest.raises(ValueError, match="does not hold vgg16.pt"):
        run(detector=str(tmp_path))
    with pytest.raises(ValueError, match="holds 23 items"):
        run(detector=detector, k=24)
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    ok = [f"--snapshot={snap}", f"--outdir={tmp_path / 'out'}", "--seeds=1"]
    _, args = NN.parse_args(ok)
    assert args.space == "pixel" and args.detector is None
    _, args = NN.parse_args(ok + ["--space=vgg16", f"--detector={tmp_path}"])
    assert args.space == "vgg16" and args.detector == str(tmp_path)
    for bad, message in [(ok + ["--space=vgg16"], "needs --detector"), (ok + ["--space=vgg16", f"--detector={tmp_path}", "--res=8"], "--res cannot be combined"),
                         (ok + ["--space=vgg16", f"--detector={tmp_path / 'absent.pt'}"], "no such TorchScript file or directory"),
                         (ok + ["--space=lpips"], "invalid choice")]:
        with pytest.raises(SystemExit):
            NN.parse_args(bad)
        assert message in capsys.readouterr().err, bad


def test_a_stale_cache_file_is_recomputed(tmp_path):
    dataset, kw = _data(tmp_path, "mirrored")
    G = N.BankGenerator(N.make_bank(dataset, 24))
    det = tmp_path / "det" / "vgg16.pt"
    os.makedirs(det.parent)
    torch.jit.script(ScriptedDetector()).save(str(det))
    cache = tmp_path / "cache"
    run = lambda: NN.nearest_training_images(G, dataset, seeds=[0, 1, 2], k=3, device=CPU, space="vgg16", detector=str(det), dataset_kwargs=kw,
                                             cache_dir=str(cache))
    first = run()
    _check_neighbors(first, G, dataset, [0, 1, 2], 3)
    files = os.listdir(cache)
    assert len(files) == 1 and files[0].endswith(".npz")        # a detector file: the features are cached
    again = run()                                               # ... and the cache is used
    assert again["neighbors"] == first["neighbors"]
    stale = metric_utils.FeatureStats.load(str(cache / files[0]))
    assert stale.num_items == 46
    stale.all_features = [stale.get_all()[:40][::-1].copy()]    # the wrong row count (and rows that would give other neighbours)
    stale.num_items = 40
    stale.save(str(cache / files[0]))
    again = run()
    assert again["neighbors"] == first["neighbors"]
    assert metric_utils.FeatureStats.load(str(cache / files[0])).num_items == 40       # recomputed without the cache: the file is left alone
    # a callable is never cached
    NN.nearest_training_images(G, dataset, seeds=[0], k=3, device=CPU, space="vgg16", detector=detector, dataset_kwargs=kw, cache_dir=str(tmp_path / "none"))
    assert not os.path.exists(tmp_path / "none")


def test_cli_run_on_the_cpu(tmp_path, capsys, monkeypatch):
    """the whole tool from a snapshot the trainer wrote, with a TorchScript vgg16.pt; and --space=pixel against a run without the option"""
    _, overrides, snap, data = _run(tmp_path)
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", _cpu_generator)
    monkeypatch.setenv("SBG_CACHE_DIR", str(tmp_path / "cache"))
    det = tmp_path / "det"
    os.makedirs(det)
    torch.jit.script(ScriptedDetector()).save(str(det / "vgg16.pt"))
    common = overrides + [f"--snapshot={snap}", "--seeds=3,0,11", "--num=10", "--k=4", "--batch=4", "--device=cpu"]
    dataset = ImageFolderDataset(path=data, xflip=True)         # the run's config says mirror: true
    G = _cpu_generator(arguments.load_config(overrides), NN.snapshot_generator_state(snap), "cpu")
    items = N.dataset_items(dataset, reduce)

    def bytes_of(seeds):
        z = torch.from_numpy(np.concatenate([np.random.RandomState(s).randn(1, G.z_dim) for s in seeds]))
        return image_export.quantize_reference(G(z, torch.zeros([len(seeds), 0])).to(torch.float32), "clamp").permute(0, 3, 1, 2).numpy()

    for detector_arg in (det, det / "vgg16.pt"):                # a directory holding the file, and the file itself
        out = tmp_path / f"out_{detector_arg.name}"
        capsys.readouterr()
        result = NN.run_nearest_neighbors(common + [f"--outdir={out}", "--space=vgg16", f"--detector={detector_arg}"])
        assert sorted(os.listdir(out)) == ["neighbors.json", "neighbors.png", "nn_stats.json", "nn_stats.npz"]
        seeds = [3, 0, 11]
        queries = np.concatenate([bytes_of([s]) for s in seeds])
        d2, item = N.brute_force(np.stack([reduce(x) for x in queries]), items, 4)
        listing = json.load(open(out / "neighbors.json"))
        assert (listing["space"], listing["F"], listing["k"]) == ("vgg16", 192, 4) and list(listing["seeds"]) == ["3", "0", "11"]
        for r, seed in enumerate(seeds):
            rows = listing["seeds"][str(seed)]
            assert rows == result["neighbors"][seed]
            assert [n["item"] for n in rows] == item[r].tolist() and [n["d2"] for n in rows] == d2[r].tolist()
            assert [n["flip"] for n in rows] == [int(i >= 20) for i in item[r]]
            assert [n["file"] for n in rows] == [dataset._image_fnames[i % 20] for i in item[r]]
        png = np.array(PIL.Image.open(out / "neighbors.png"))
        assert png.shape == (3 * 16, 5 * 16, 3) and np.array_equal(png, result["canvas"])
        for r in range(3):
            cells = png[r * 16:(r + 1) * 16].reshape(16, 5, 16, 3).transpose(1, 3, 0, 2)
            assert np.array_equal(cells[0], queries[r])
            for t in range(4):
                assert np.array_equal(cells[1 + t], dataset[int(item[r, t])][0])
        gen = np.concatenate([N.brute_force(np.stack([reduce(x) for x in bytes_of(list(range(lo, min(lo + 4, 10))))]), items, 1)[0][:, 0]
                              for lo in range(0, 10, 4)])
        npz = np.load(out / "nn_stats.npz")
        assert npz["gen_to_train"].dtype == np.float32 and np.array_equal(npz["gen_to_train"], gen)
        assert np.array_equal(npz["train_to_train"], N.brute_train_to_train(dataset, reduce)) and npz["train_to_train"].shape == (20,)
        stats = json.load(open(out / "nn_stats.json"))
        assert stats == result["stats"] and json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == stats
        assert (stats["space"], stats["num"], stats["stored_images"], stats["mirrored"]) == ("vgg16", 10, 20, True)
    assert len(os.listdir(tmp_path / "cache" / "gan-metrics")) >= 1

    # --space=pixel writes exactly the bytes a run without the option writes, and no new keys
    NN.run_nearest_neighbors(common + [f"--outdir={tmp_path / 'plain'}"])
    NN.run_nearest_neighbors(common + [f"--outdir={tmp_path / 'pixel'}", "--space=pixel"])
    for name in ("neighbors.json", "neighbors.png", "nn_stats.json"):
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "pixel" / name).read_bytes(), name
    with zipfile.ZipFile(tmp_path / "plain" / "nn_stats.npz") as a, zipfile.ZipFile(tmp_path / "pixel" / "nn_stats.npz") as b:
        assert a.namelist() == b.namelist() == ["gen_to_train.npy", "train_to_train.npy"]      # the archive stamps its members with the time:
        assert all(a.read(member) == b.read(member) for member in a.namelist())                # the members' bytes are what is compared
    assert set(json.load(open(tmp_path / "pixel" / "neighbors.json"))) == {"F", "res", "k", "seeds"}
    assert "space" not in json.load(open(tmp_path / "pixel" / "nn_stats.json"))
