"""The nearest_neighbors tool on the CPU: option parsing and failures, `topk_reference` against the numpy oracle, the mirror equivalence
and `--res` against a brute-force search over `dataset[i]`, and the whole tool from a snapshot the trainer wrote."""
import json
import os

import numpy as np
import PIL.Image
import pytest
import torch

import nearest_util as N
import nn_u8_util as U
from golden_util import make_image_folder
from test_calc_metrics_cpu import _cpu_generator, _run
from style_big_gan_amd import arguments, nearest_neighbors as NN
from style_big_gan_amd.torch_utils.ops import image_export, nn_u8, resample_u8
from style_big_gan_amd.train_parts.datasets import ImageFolderDataset

CPU = torch.device("cpu")


def test_option_parsing_and_failures(tmp_path, capsys):
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    ok = [f"--snapshot={snap}", f"--outdir={tmp_path / 'out'}"]
    overrides, args = NN.parse_args(["exp.config=a.yaml"] + ok + ["--seeds=0-7"])
    assert overrides == ["exp.config=a.yaml"] and args.seeds == list(range(8)) and args.num is None and args.k == 5 and args.res is None
    assert args.mirror is None and args.truncation_psi == 1 and args.class_idx is None and args.noise_mode == "const" and args.device == "auto"
    assert args.batch == 64
    _, args = NN.parse_args(ok + ["--num=100", "--seeds=3,5", "--k=8", "--res=32", "--data=/d", "--mirror=0", "--trunc=0.5", "--class=2",
                                  "--noise-mode=random", "--device=cpu", "--batch=16"])
    assert (args.num, args.seeds, args.k, args.res, args.data, args.mirror) == (100, [3, 5], 8, 32, "/d", False)
    assert (args.truncation_psi, args.class_idx, args.noise_mode, args.device, args.batch) == (0.5, 2, "random", "cpu", 16)
    for bad, message in [(ok, "one of --seeds and --num"), (ok + ["--num=0"], "at least 1"), (ok + ["--seeds=1", "--k=0"], "between 1 and 8"),
                         (ok + ["--seeds=1", "--k=9"], "between 1 and 8"), (ok + ["--seeds=1", "--res=24"], "power of two"),
                         (ok + ["--seeds=1", "--res=2"], "power of two"), (ok + ["--seeds=1", "--batch=0"], "at least 1"),
                         ([f"--snapshot={tmp_path / 'absent.pt'}", "--outdir=o", "--seeds=1"], "no such file"),
                         ([f"--snapshot={snap}", "--seeds=1"], "--outdir"), (ok + ["--seeds=1", "--frobnicate"], "unrecognised")]:
        with pytest.raises(SystemExit):
            NN.parse_args(bad)
        assert message in capsys.readouterr().err, bad
    assert NN.check_res(None, 64) is None and NN.check_res(64, 64) is None and NN.check_res(16, 64) == 16
    for res in (2, 24, 128):
        with pytest.raises(ValueError, match="power of two"):
            NN.check_res(res, 64)


@pytest.mark.parametrize("Q,M,F,k", [(1, 1, 16, 1), (37, 130, 48, 5), (70, 260, 80, 8), (5, 9, 5000, 3), (3, 40, 7, 2)])
def test_topk_reference_equals_the_oracle(Q, M, F, k):
    queries, store, planted = U.make_case(Q, M, F, seed=Q + M + F)
    got = nn_u8.topk(torch.from_numpy(queries), torch.from_numpy(store), k)            # CPU tensors take topk_reference
    assert U.same(got, U.oracle_topk(queries, store, k))
    if M > k:
        exclude = np.random.RandomState(k).randint(-1, M + 1, size=Q).astype(np.int32)
        if planted:
            exclude[-1] = planted[0][0]
        got = nn_u8.topk_reference(torch.from_numpy(queries), torch.from_numpy(store), k, torch.from_numpy(exclude))
        assert U.same(got, U.oracle_topk(queries, store, k, exclude))


def test_topk_reference_flattens_and_refuses():
    rng = np.random.RandomState(1)
    q, s = torch.from_numpy(rng.randint(0, 256, [4, 3, 4, 4], dtype=np.uint8)), torch.from_numpy(rng.randint(0, 256, [12, 3, 4, 4], dtype=np.uint8))
    assert U.same(nn_u8.topk(q, s, 3), U.oracle_topk(q.numpy().reshape(4, -1), s.numpy().reshape(12, -1), 3))
    for args, message in [((q, s, 0), "k = 0 neighbours"), ((q, s, 9), "k = 9 neighbours"), ((q, s[:2], 3), "the store has 2 rows"),
                          ((q, s[:, :, :, ::2], 3), "must be dense"), ((q.float(), s, 3), "must be uint8"), ((q, s[:, :2].contiguous(), 3), "row length"),
                          ((q, s, 3, torch.zeros([4], dtype=torch.int64)), "exclude must be int32"),
                          ((q, s[:3], 3, torch.tensor([0, 5, 5, 5], dtype=torch.int32)), "one is excluded"), ((q.numpy(), s, 3), "torch tensor")]:
        with pytest.raises(RuntimeError, match=message):
            nn_u8.topk(*args)


def _dataset(tmp_path, n=23, res=16, xflip=True, **kw):
    return ImageFolderDataset(path=make_image_folder(str(tmp_path / "data"), n=n, res=res), xflip=xflip, **kw)


def _check_neighbors(result, G, dataset, seeds, k, reduce=None):
    """the tool's lists against the brute-force search over dataset[i]; the canvas against the data set's images"""
    queries = N.seed_bytes(G, seeds)
    items = N.dataset_items(dataset, reduce)
    q = queries if reduce is None else np.stack([reduce(x) for x in queries])
    d2, item = N.brute_force(q, items, k)
    F = items.shape[1]
    assert result["F"] == F
    C, H, W = dataset.image_shape
    assert result["canvas"].shape == (len(seeds) * H, (k + 1) * W, C)
    for r, seed in enumerate(seeds):
        rows = result["neighbors"][seed]
        assert [n["item"] for n in rows] == item[r].tolist() and [n["d2"] for n in rows] == d2[r].tolist(), seed
        assert [n["flip"] for n in rows] == [int(dataset._xflip[i]) for i in item[r]]
        assert [n["file"] for n in rows] == [dataset._image_fnames[dataset._raw_idx[i]] for i in item[r]]
        assert all(abs(n["rmse"] - (n["d2"] / F) ** 0.5) < 1e-12 for n in rows)
        cells = result["canvas"][r * H:(r + 1) * H].reshape(H, k + 1, W, C).transpose(1, 3, 0, 2)          # [cell, C, H, W]
        assert np.array_equal(cells[0], queries[r])
        for t in range(k):                                      # full resolution, mirrored where the mirrored copy matched
            assert np.array_equal(cells[1 + t], dataset[int(item[r, t])][0]), (seed, t)


def test_mirror_equivalence_against_brute_force(tmp_path):
    """the two searches (queries, queries.flip(3)) merged by (d2, flip, row) equal a brute-force search over dataset[i] in item order"""
    dataset = _dataset(tmp_path)
    assert len(dataset) == 46
    G = N.BankGenerator(N.make_bank(dataset, 24))
    seeds = list(range(12))
    result = NN.nearest_training_images(G, dataset, seeds=seeds, k=5, device=CPU)
    assert result["mirrored"] and result["res"] == 16
    _check_neighbors(result, G, dataset, seeds, 5)
    flips = [n["flip"] for s in seeds for n in result["neighbors"][s][:1]]
    assert 0 in flips and 1 in flips                            # the bank holds training images in both orientations
    assert any(result["neighbors"][s][0]["d2"] == 0 and result["neighbors"][s][0]["flip"] == 1 for s in seeds)
    # a subset in storage order, without the mirror: items are rows
    sub = ImageFolderDataset(path=dataset._path, xflip=False, max_size=9, random_seed=3)
    result = NN.nearest_training_images(G, sub, seeds=seeds[:4], k=8, device=CPU)
    assert not result["mirrored"]
    _check_neighbors(result, G, sub, seeds[:4], 8)
    with pytest.raises(ValueError, match="holds 9 stored images"):
        NN.nearest_training_images(G, sub, seeds=[0], k=8 + 2, device=CPU)
    with pytest.raises(ValueError, match="one of --seeds and --num"):
        NN.nearest_training_images(G, sub, device=CPU)
    with pytest.raises(ValueError, match="the generator makes"):
        NN.nearest_training_images(N.BankGenerator(np.zeros([2, 3, 8, 8], dtype=np.uint8)), sub, seeds=[0], device=CPU)


def _box(res):
    def reduce(img):
        return resample_u8.resize_reference(torch.from_numpy(np.ascontiguousarray(img.transpose(1, 2, 0))), res, res, "box").numpy().transpose(2, 0, 1)
    return reduce


def test_res_against_resize_reference(tmp_path):
    """--res compares box-reduced copies; every item is mirrored first and reduced then, which the tool's mirrored reduced query equals"""
    dataset = _dataset(tmp_path)
    G = N.BankGenerator(N.make_bank(dataset, 24))
    seeds = list(range(10))
    for res in (8, 4):
        result = NN.nearest_training_images(G, dataset, seeds=seeds, num=10, k=3, res=res, batch=4, device=CPU)
        assert result["res"] == res and result["F"] == 3 * res * res
        _check_neighbors(result, G, dataset, seeds, 3, _box(res))
        assert np.array_equal(result["train_to_train"], N.brute_train_to_train(dataset, _box(res)))
        assert np.array_equal(result["gen_to_train"], [result["neighbors"][s][0]["d2"] for s in seeds])
    with pytest.raises(ValueError, match="power of two"):
        NN.nearest_training_images(G, dataset, seeds=seeds, res=32, device=CPU)


def _stats_of(d2, F):
    rmse = np.sqrt(np.asarray(d2, dtype=np.float64) / F)
    q = np.quantile(rmse, [0.01, 0.05, 0.25, 0.5, 0.75])
    return dict(min=rmse.min(), mean=rmse.mean(), p01=q[0], p05=q[1], p25=q[2], p50=q[3], p75=q[4])


def test_cli_run_on_the_cpu(tmp_path, capsys, monkeypatch):
    """the whole tool from a snapshot the trainer wrote, the generator evaluated by the CPU restatement of the same network"""
    _, overrides, snap, data = _run(tmp_path)
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", _cpu_generator)
    out = tmp_path / "out"
    result = NN.run_nearest_neighbors(overrides + [f"--snapshot={snap}", f"--outdir={out}", "--seeds=3,0,11", "--num=10", "--k=4", "--batch=4",
                                                   "--device=cpu"])
    assert sorted(os.listdir(out)) == ["neighbors.json", "neighbors.png", "nn_stats.json", "nn_stats.npz"]
    dataset = ImageFolderDataset(path=data, xflip=True)         # the run's config says mirror: true
    assert len(dataset) == 40
    G = _cpu_generator(arguments.load_config(overrides), NN.snapshot_generator_state(snap), "cpu")
    items = N.dataset_items(dataset)
    F = items.shape[1]

    def bytes_of(seeds):
        z = torch.from_numpy(np.concatenate([np.random.RandomState(s).randn(1, G.z_dim) for s in seeds]))
        return image_export.quantize_reference(G(z, torch.zeros([len(seeds), 0])).to(torch.float32), "clamp").permute(0, 3, 1, 2).numpy()

    # --seeds: neighbors.json and the cells of neighbors.png
    seeds = [3, 0, 11]
    queries = np.concatenate([bytes_of([s]) for s in seeds])
    d2, item = N.brute_force(queries, items, 4)
    listing = json.load(open(out / "neighbors.json"))
    assert listing["F"] == F == 768 and listing["k"] == 4 and list(listing["seeds"]) == ["3", "0", "11"]
    for r, seed in enumerate(seeds):
        rows = listing["seeds"][str(seed)]
        assert rows == result["neighbors"][seed]
        assert [n["item"] for n in rows] == item[r].tolist() and [n["d2"] for n in rows] == d2[r].tolist()
        assert [n["flip"] for n in rows] == [int(i >= 20) for i in item[r]]
        assert [n["file"] for n in rows] == [dataset._image_fnames[i % 20] for i in item[r]]
        assert all(abs(n["rmse"] - (n["d2"] / F) ** 0.5) < 1e-12 for n in rows)
    png = np.array(PIL.Image.open(out / "neighbors.png"))
    assert png.shape == (3 * 16, 5 * 16, 3) and np.array_equal(png, result["canvas"])
    for r in range(3):
        cells = png[r * 16:(r + 1) * 16].reshape(16, 5, 16, 3).transpose(1, 3, 0, 2)
        assert np.array_equal(cells[0], queries[r])
        for t in range(4):
            assert np.array_equal(cells[1 + t], dataset[int(item[r, t])][0])

    # --num: nn_stats.npz and nn_stats.json
    gen = np.concatenate([N.brute_force(bytes_of(list(range(lo, min(lo + 4, 10)))), items, 1)[0][:, 0] for lo in range(0, 10, 4)])
    base = N.brute_train_to_train(dataset)
    npz = np.load(out / "nn_stats.npz")
    assert sorted(npz.files) == ["gen_to_train", "train_to_train"]
    assert npz["gen_to_train"].dtype == np.int64 and np.array_equal(npz["gen_to_train"], gen)
    assert npz["train_to_train"].dtype == np.int64 and np.array_equal(npz["train_to_train"], base) and base.shape == (20,)
    stats = json.load(open(out / "nn_stats.json"))
    assert stats == result["stats"] and json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == stats
    for name, d2 in (("gen_to_train", gen), ("train_to_train", base)):
        want = _stats_of(d2, F)
        assert set(stats[name]) == set(want) and all(abs(stats[name][key] - want[key]) < 1e-9 for key in want)
    p01 = np.quantile(base.astype(np.float64), 0.01)
    assert stats["fraction_below_train_p01"] == float(np.mean(gen <= p01)) and stats["train_p01_d2"] == p01
    assert (stats["num"], stats["stored_images"], stats["mirrored"], stats["res"]) == (10, 20, True, 16)

    # --data and --mirror override the run's config
    other = make_image_folder(str(tmp_path / "other"), n=6, res=16, seed=9)
    result = NN.run_nearest_neighbors(overrides + [f"--snapshot={snap}", f"--outdir={tmp_path / 'out2'}", "--seeds=1", "--k=6", f"--data={other}",
                                                   "--mirror=0", "--device=cpu"])
    assert sorted(n["item"] for n in result["neighbors"][1]) == list(range(6)) and not result["mirrored"]
    assert sorted(os.listdir(tmp_path / "out2")) == ["neighbors.json", "neighbors.png"]


def test_a_generator_that_returns_training_images_is_flagged(tmp_path, monkeypatch):
    _, overrides, snap, data = _run(tmp_path)
    dataset = ImageFolderDataset(path=data, xflip=True)
    bank = np.stack([dataset[i][0] for i in range(0, 40, 3)])   # training images, mirrored ones among them
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", lambda config, state, device: N.BankGenerator(bank).to(device))
    out = tmp_path / "out"
    result = NN.run_nearest_neighbors(overrides + [f"--snapshot={snap}", f"--outdir={out}", "--num=30", "--res=8", "--batch=7", "--device=cpu"])
    stats = json.load(open(out / "nn_stats.json"))
    assert stats["fraction_below_train_p01"] == 1 and stats["gen_to_train"]["min"] == 0 and stats["gen_to_train"]["mean"] == 0
    assert stats["train_to_train"]["min"] > 0 and stats["res"] == 8
    npz = np.load(out / "nn_stats.npz")
    assert npz["gen_to_train"].shape == (30,) and not npz["gen_to_train"].any() and np.array_equal(npz["gen_to_train"], result["gen_to_train"])
    assert sorted(os.listdir(out)) == ["nn_stats.json", "nn_stats.npz"]
