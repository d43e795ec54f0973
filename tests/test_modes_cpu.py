"""The mode coverage tool on the CPU: the integer centroid update against a scalar restatement, the rounding rule, ties, k-means++ seeding and
Lloyd iterations on a planted table, the bin statistics against closed formulas, the tool end to end on a data set of four modes with stand-in
generators, --from, the library's symbols and the shared reduction helpers."""
import importlib
import json
import math
import os
import types

import numpy as np
import PIL.Image
import pytest
import torch

import modes_util as mu
from nearest_util import BankGenerator
from style_big_gan_amd import _lib, modes as MD, nearest_neighbors, tool_support
from style_big_gan_amd.torch_utils.ops import kmeans_u8 as ops
from style_big_gan_amd.train_parts.datasets import ImageFolderDataset

CPU = torch.device("cpu")
_t = torch.from_numpy


# ---------------------------------------------------------------------------------------------------------------- update, assign

@pytest.mark.parametrize("n,k,f", mu.UPDATE_CASES)
def test_update_equals_the_scalar_restatement(n, k, f):
    points, labels, old = mu.update_case(n, k, f)
    got = ops.update(_t(points), _t(labels), _t(old))
    want = mu.scalar_update(points, labels, old)
    assert mu.same_update(got, want)
    assert int(got[1].sum()) == n
    if (n, k, f) == (5, 3, 16):
        assert want[1][1] == 0 and np.array_equal(got[0][1].numpy(), old[1]) and not got[2][1].any()


def test_the_mean_is_rounded_half_up():
    def centre(values):
        points = np.zeros([len(values), 16], dtype=np.uint8)
        points[:, 3] = values
        new, counts, sums = ops.update(_t(points), torch.zeros([len(values)], dtype=torch.int32), torch.full([1, 16], 9, dtype=torch.uint8))
        assert int(counts[0]) == len(values) and int(sums[0, 3]) == sum(values) and not new[0, :3].any()
        return int(new[0, 3])
    assert centre([0, 1]) == 1              # 1 of 2: 0.5 -> 1
    assert centre([1, 2]) == 2              # 3 of 2: 1.5 -> 2
    assert centre([254, 255]) == 255        # 509 of 2: 254.5 -> 255
    assert centre([1, 1, 2]) == 1 and centre([1, 2, 2]) == 2 and centre([255] * 7) == 255 and centre([0] * 5) == 0


def test_an_empty_cluster_keeps_its_old_row():
    points, labels, old = mu.table(40, 4, 32, empty=2)
    new, counts, sums = ops.update(_t(points), _t(labels), _t(old))
    assert int(counts[2]) == 0 and np.array_equal(new[2].numpy(), old[2]) and not sums[2].any()
    assert all(int(counts[c]) > 0 and not np.array_equal(new[c].numpy(), old[c]) for c in (0, 1, 3))


def test_assign_is_exact_and_ties_go_to_the_lower_centre():
    rng = np.random.RandomState(2)
    points = rng.randint(0, 256, [50, 32], dtype=np.uint8)
    cent = rng.randint(0, 256, [5, 32], dtype=np.uint8)
    cent[3] = cent[1]                                            # two identical centroids
    points[:10] = cent[1]
    label, d2 = ops.assign(_t(points), _t(cent))
    assert label.dtype == torch.int32 and d2.dtype == torch.int64 and label.shape == d2.shape == (50,)
    full = ((points.astype(np.int64)[:, None] - cent.astype(np.int64)[None]) ** 2).sum(2)
    assert np.array_equal(d2.numpy(), full.min(1)) and np.array_equal(label.numpy(), full.argmin(1))
    assert not (label == 3).any() and (label[:10] == 1).all() and not d2[:10].any()


def test_refusals():
    p, l, c = (_t(v) for v in mu.table(8, 3, 16))
    for args, message in [((p.float(), l, c), r"float32 \(8, 16\)"), ((p, l.long(), c), r"labels int64 \(8,\)"), ((p, l, c[:, :8].contiguous()), r"\(3, 8\)"),
                          ((p[:, ::2], l, c[:, ::2]), "dense"), ((p, l[:4], c), r"labels int32 \(4,\)"), ((p[:0], l[:0], c), r"\(0, 16\)"),
                          ((p, l, torch.zeros([257, 16], dtype=torch.uint8)), r"\(257, 16\)"), ((p.numpy(), l, c), "ndarray")]:
        with pytest.raises(RuntimeError, match=message):
            ops.update(*args)
    for bad in (-1, 3):
        worse = l.clone()
        worse[5] = bad
        with pytest.raises(RuntimeError, match=rf"labels lie in \[{min(bad, 0)}, {max(bad, 2)}\], outside \[0, 3\).*\(8, 16\)"):
            ops.update(p, worse, c)
    with pytest.raises(RuntimeError, match=r"uint8 \[N, F\]"):
        ops.assign(p.float(), c)
    with pytest.raises(RuntimeError, match="max_iter"):
        ops.lloyd(p, c, -1)


# ---------------------------------------------------------------------------------------------------------------- seed, lloyd

def test_seed_is_reproducible_and_picks_distinct_rows():
    points = _t(mu.table(300, 2, 48, seed=4)[0])
    a, b = ops.seed(points, 12, np.random.RandomState(3)), ops.seed(points, 12, np.random.RandomState(3))
    assert a.dtype == torch.uint8 and a.shape == (12, 48) and torch.equal(a, b)
    assert not torch.equal(a, ops.seed(points, 12, np.random.RandomState(4)))
    rows = [int(np.nonzero((points.numpy() == c[None]).all(1))[0][0]) for c in a.numpy()]
    assert len(set(rows)) == 12 and rows[0] == np.random.RandomState(3).randint(300)
    # the draw: r = (int(u 2^53) total) >> 53 against the int64 cumulative sum of the distances to the first centre
    rng = np.random.RandomState(3)
    first = int(rng.randint(300))
    best = ((points.numpy().astype(np.int64) - points.numpy().astype(np.int64)[first]) ** 2).sum(1)
    r = (int(rng.random_sample() * 2 ** 53) * int(best.sum())) >> 53
    assert rows[1] == int(np.nonzero(np.cumsum(best) > r)[0][0])


def test_seed_refuses_a_table_with_fewer_distinct_rows():
    points = _t(np.repeat(mu.table(3, 1, 16)[0], 5, axis=0))
    assert ops.seed(points, 3, np.random.RandomState(0)).unique(dim=0).shape[0] == 3
    with pytest.raises(RuntimeError, match=r"\(15, 16\) holds only 3 distinct rows, K = 4"):
        ops.seed(points, 4, np.random.RandomState(0))
    with pytest.raises(RuntimeError, match="K = 16 centres"):
        ops.seed(points, 16, np.random.RandomState(0))
    with pytest.raises(RuntimeError, match="RandomState"):
        ops.seed(points, 2, np.random.default_rng(0))


def test_seed_and_lloyd_on_the_planted_table():
    points, group = mu.planted_table()
    cent = ops.seed(_t(points), 4, np.random.RandomState(0))
    nearest_group = [int(group[np.nonzero((points == c[None]).all(1))[0][0]]) for c in cent.numpy()]
    assert sorted(nearest_group) == [0, 1, 2, 3]                 # one centre per group
    fit = ops.lloyd(_t(points), cent, 10)
    assert fit["converged"] and fit["iterations"] <= 3 and len(fit["inertia"]) == fit["iterations"]
    assert all(isinstance(v, int) for v in fit["inertia"]) and all(a >= b for a, b in zip(fit["inertia"], fit["inertia"][1:]))
    want = mu.rounded_means(points, group)
    assert np.array_equal(fit["centroids"].numpy(), want[nearest_group])
    assert np.array_equal(fit["labels"].numpy(), np.argsort(nearest_group)[group]) and fit["counts"].tolist() == [40] * 4
    assert fit["inertia"][-1] == int(fit["d2"].sum()) == int(((points.astype(np.int64) - want[group].astype(np.int64)) ** 2).sum())


def test_one_iteration_is_not_convergence():
    points, group = mu.planted_table()
    cent = ops.seed(_t(points), 4, np.random.RandomState(0))
    fit = ops.lloyd(_t(points), cent, 1)
    assert not fit["converged"] and fit["iterations"] == 1 and len(fit["inertia"]) == 2          # the iteration's assign and the final one
    assert not torch.equal(fit["centroids"], cent)               # a second iteration has a centre to move: a sampled row is not its group's mean
    labels, d2 = ops.assign(_t(points), fit["centroids"])
    assert torch.equal(labels, fit["labels"]) and torch.equal(d2, fit["d2"]) and fit["inertia"][1] == int(d2.sum())
    assert torch.equal(fit["counts"], torch.bincount(labels.long(), minlength=4))
    none = ops.lloyd(_t(points), cent, 0)
    assert none["iterations"] == 0 and torch.equal(none["centroids"], cent) and len(none["inertia"]) == 1


# ---------------------------------------------------------------------------------------------------------------- the statistics

def test_statistics_against_the_closed_formulas():
    ref, gen = [50, 30, 20], [20, 50, 130]                       # N_ref = 100, N_gen = 200
    s = MD.bin_statistics(ref, gen, 0.05)
    want_z = [mu.closed_z(a, 100, b, 200) for a, b in zip(ref, gen)]
    assert np.allclose(s["z"], want_z, rtol=0, atol=1e-12) and s["z"][0] > 0 > s["z"][2]
    # bin 0 by hand: p = 0.5, q = 0.1, pooled 70 / 300
    assert abs(want_z[0] - 0.4 / math.sqrt(7 / 30 * 23 / 30 * (1 / 100 + 1 / 200))) < 1e-12
    assert np.allclose(s["pvalue"], [math.erfc(abs(z) / math.sqrt(2)) for z in want_z], rtol=0, atol=1e-15)
    # bin 1: 0.3 against 0.25 is z = 0.05 / sqrt(4 / 15 * 11 / 15 * 0.015) = 0.92, no difference at 5 %
    assert abs(want_z[1] - 0.05 / math.sqrt(4 / 15 * 11 / 15 * 0.015)) < 1e-12 and s["different"].tolist() == [True, False, True]
    assert s["ndb"] == 2 and s["ndb_over_k"] == 2 / 3
    assert abs(s["js"] - mu.closed_js([0.5, 0.3, 0.2], [0.1, 0.25, 0.65])) < 1e-12 and 0 < s["js"] < 1


def test_statistics_edge_cases():
    same = MD.bin_statistics([10, 30, 60], [20, 60, 120], 0.05)  # equal histograms, different sizes
    assert same["ndb"] == 0 and same["js"] == 0 and not same["z"].any() and (same["pvalue"] == 1).all()
    apart = MD.bin_statistics([40, 60, 0], [0, 0, 50], 0.05)     # disjoint supports
    assert abs(apart["js"] - 1) < 1e-12 and apart["ndb"] == 3
    hollow = MD.bin_statistics([50, 0, 50], [30, 0, 70], 0.05)   # a bin that is empty in both sets
    assert hollow["z"][1] == 0 and hollow["pvalue"][1] == 1 and not hollow["different"][1]
    for bad in (([1, 2], [1, 2, 3]), ([0, 0], [1, 2]), ([1, 2], [0, 0])):
        with pytest.raises(ValueError, match="histograms"):
            MD.bin_statistics(*bad, 0.05)


def test_the_pvalue_at_the_five_percent_point():
    assert abs(math.erfc(1.959963984540054 / math.sqrt(2)) - 0.05) < 1e-12
    # counts whose z is a known number: N = 200 each, 120 against 80 -> z = 0.2 / sqrt(0.5 * 0.5 * 0.01) = 4
    s = MD.bin_statistics([120, 80], [80, 120], 0.05)
    assert abs(s["z"][0] - 4) < 1e-12 and abs(s["pvalue"][0] - math.erfc(4 / math.sqrt(2))) < 1e-18


def test_shown_bins():
    order, rows = MD.shown_bins([0.5, -3.0, 2.0, 0.5, -1.0, 0.0], 2)
    assert order.tolist() == [2, 0, 3, 5, 4, 1] and rows == [2, 0, 1, 4]
    assert MD.shown_bins([1.0, -1.0, 0.0], 6)[1] == [0, 2, 1] and MD.shown_bins([1.0, -1.0], 0)[1] == []


# ---------------------------------------------------------------------------------------------------------------- the tool

@pytest.fixture(scope="module")
def data(tmp_path_factory):
    images, mode = mu.mode_images()
    root = mu.write_folder(str(tmp_path_factory.mktemp("modes") / "data"), images)
    return images, mode, root


def _missing_mode_run(data, outdir, device=CPU, **kw):
    images, mode, root = data
    dataset = ImageFolderDataset(path=root)
    G = BankGenerator(images[mode != 2]).to(device)              # never produces mode 2
    return MD.mode_coverage(G, dataset, bins=4, res=8, holdout=0.25, show=2, examples=3, batch=50, outdir=outdir, device=device, **kw), dataset


def test_a_generator_that_never_produces_a_mode(data, tmp_path):
    images, mode, root = data
    out = tmp_path / "out"
    result, dataset = _missing_mode_run(data, str(out))
    assert sorted(os.listdir(out)) == ["modes.json", "modes.npz", "modes.png"]
    stats = json.loads(open(out / "modes.json").read(), parse_constant=lambda name: pytest.fail(f"modes.json holds {name}"))
    assert stats == result["stats"]
    assert (stats["N_ref"], stats["N_holdout"], stats["N_gen"]) == (180, 60, 180) and stats["converged"] and 1 <= stats["iterations"] <= 30
    assert len(stats["inertia"]) == stats["iterations"] and 0 < stats["rms"] < 4                 # the noise is uniform in [-4, 4]
    assert stats["options"]["bins"] == 4 and stats["options"]["res"] == 8 and stats["options"]["from_file"] is None
    npz = np.load(out / "modes.npz")
    assert sorted(npz.files) == sorted(MD.NPZ_KEYS)
    shapes = dict(centroids=(4, 192), ref_items=(180,), ref_labels=(180,), ref_d2=(180,), gen_labels=(180,), gen_d2=(180,), holdout_items=(60,),
                  holdout_labels=(60,), counts_ref=(4,), counts_gen=(4,), counts_holdout=(4,), z=(4,), pvalue=(4,), res=(), seed=())
    assert {k: npz[k].shape for k in npz.files} == shapes and npz["centroids"].dtype == np.uint8 and npz["ref_d2"].dtype == np.int64
    assert int(npz["res"]) == 8 and int(npz["seed"]) == 0
    P = np.random.RandomState(0).permutation(240)
    assert np.array_equal(npz["holdout_items"], P[:60]) and np.array_equal(npz["ref_items"], P[60:])
    # every bin is one mode
    bin_of_mode = [int(np.bincount(npz["ref_labels"][mode[npz["ref_items"]] == m], minlength=4).argmax()) for m in range(4)]
    assert sorted(bin_of_mode) == [0, 1, 2, 3] and np.array_equal(npz["ref_labels"], np.array(bin_of_mode)[mode[npz["ref_items"]]])
    assert np.array_equal(npz["holdout_labels"], np.array(bin_of_mode)[mode[npz["holdout_items"]]])
    assert np.array_equal(npz["counts_ref"], np.bincount(npz["ref_labels"], minlength=4)) and npz["counts_gen"].sum() == 180
    # the bin of mode 2 is missing, first in the list and the top row of the picture
    lost = bin_of_mode[2]
    first = stats["bins"][0]
    assert first["bin"] == lost and first["n_gen"] == 0 and first["missing"] and first["different"] and first["z"] > 3
    assert [b["missing"] for b in stats["bins"]] == [True, False, False, False]
    assert [b["z"] for b in stats["bins"]] == sorted((b["z"] for b in stats["bins"]), reverse=True)
    assert all(b["n_ref"] == npz["counts_ref"][b["bin"]] and b["n_holdout"] == npz["counts_holdout"][b["bin"]] and b["z"] == npz["z"][b["bin"]] and
               b["pvalue"] == npz["pvalue"][b["bin"]] for b in stats["bins"])
    assert stats["generated"]["ndb"] >= 1 and stats["generated"]["ndb_over_k"] == stats["generated"]["ndb"] / 4 and stats["generated"]["js"] > 0.05
    assert stats["holdout"]["ndb"] == 0 and stats["holdout"]["js"] < 0.05
    png = np.array(PIL.Image.open(out / "modes.png"))
    assert png.shape == (4 * 16, 7 * 16, 3) and np.array_equal(png, result["canvas"]) and result["rows"][0] == lost
    cells = png.reshape(4, 16, 7, 16, 3).transpose(0, 2, 4, 1, 3)                                # [row, cell, C, H, W]
    cent = npz["centroids"][lost].reshape(3, 8, 8)
    assert np.array_equal(cells[0, 0], cent.repeat(2, 1).repeat(2, 2))                           # pixel repetition
    assert np.abs(cent.astype(int) - np.array(mu.MODE_COLOURS[2])[:, None, None]).max() <= 1
    members = np.nonzero(npz["ref_labels"] == lost)[0]
    nearest = members[np.argsort(npz["ref_d2"][members], kind="stable")[:3]]
    for t in range(3):                                           # the nearest reference images at full resolution; no generated image: black
        assert np.array_equal(cells[0, 1 + t], dataset[int(npz["ref_items"][nearest[t]])][0])
        assert not cells[0, 4 + t].any()
    for row in range(1, 4):                                      # the other rows show generated images of their own mode
        m = bin_of_mode.index(result["rows"][row])
        assert all(np.abs(cells[row, c].astype(int).mean((1, 2)) - np.array(mu.MODE_COLOURS[m])).max() < 2 for c in range(7))


def test_a_generator_with_the_proportions_of_the_data(data, tmp_path):
    images, mode, root = data
    first, dataset = _missing_mode_run(data, None)
    G = mu.ListGenerator(images[first["arrays"]["ref_items"]], 180)
    result = MD.mode_coverage(G, dataset, bins=4, res=8, holdout=0.25, batch=64, device=CPU)
    assert result["stats"]["generated"]["ndb"] == 0 and result["stats"]["generated"]["js"] < 0.01
    assert np.array_equal(result["arrays"]["counts_gen"], result["arrays"]["counts_ref"])
    assert np.array_equal(result["arrays"]["gen_labels"], result["arrays"]["ref_labels"]) and np.array_equal(result["arrays"]["gen_d2"], result["arrays"]["ref_d2"])
    assert not any(b["missing"] or b["different"] for b in result["stats"]["bins"]) and all(b["z"] == 0 for b in result["stats"]["bins"])
    none = MD.mode_coverage(G, dataset, bins=4, res=8, holdout=0, num=20, show=1, examples=1, device=CPU)      # no baseline
    assert none["stats"]["holdout"] is None and none["stats"]["N_holdout"] == 0 and none["stats"]["N_ref"] == 240 and none["stats"]["N_gen"] == 20
    assert none["arrays"]["holdout_items"].shape == (0,) and not none["arrays"]["counts_holdout"].any()


def test_from_reuses_the_stored_bins(data, tmp_path):
    images, mode, root = data
    first, dataset = _missing_mode_run(data, str(tmp_path / "a"))
    again, _ = _missing_mode_run(data, str(tmp_path / "b"), from_file=str(tmp_path / "a" / "modes.npz"))
    assert again["stats"]["generated"] == first["stats"]["generated"] and again["stats"]["holdout"] == first["stats"]["holdout"]
    assert again["stats"]["bins"] == first["stats"]["bins"] and again["stats"]["rms"] == first["stats"]["rms"]
    assert again["stats"]["iterations"] is None and again["stats"]["inertia"] is None and again["stats"]["options"]["from_file"] == "modes.npz"
    a, b = np.load(tmp_path / "a" / "modes.npz"), np.load(tmp_path / "b" / "modes.npz")
    assert all(np.array_equal(a[k], b[k]) for k in MD.NPZ_KEYS)
    assert open(tmp_path / "a" / "modes.png", "rb").read() == open(tmp_path / "b" / "modes.png", "rb").read()
    G = BankGenerator(images[mode != 2])
    stored = str(tmp_path / "a" / "modes.npz")
    with pytest.raises(ValueError, match=r"at res 8 do not belong to images of 3 x 4 x 4"):
        MD.mode_coverage(G, dataset, res=4, holdout=0.25, from_file=stored, device=CPU)
    with pytest.raises(ValueError, match="--seed=0, this run has --seed=1"):
        MD.mode_coverage(G, dataset, res=8, holdout=0.25, seed=1, from_file=stored, device=CPU)
    with pytest.raises(ValueError, match="stored split"):
        MD.mode_coverage(G, dataset, res=8, holdout=0.5, from_file=stored, device=CPU)


def test_a_conditional_generator_takes_the_class_mix_of_the_data(tmp_path):
    images, mode = mu.mode_images(per_mode=30)
    keep = np.nonzero((mode != 1) | (np.arange(len(mode)) < 40))[0]              # 10 images of class 1, 30 of the others
    images, mode = images[keep], mode[keep]
    dataset = ImageFolderDataset(path=mu.write_folder(str(tmp_path / "data"), images, labels=mode), use_labels=True)
    bank = np.stack([mu.mode_images(per_mode=30, seed=8)[0][m::4] for m in range(4)])
    G = mu.ClassGenerator(bank)
    # without --class generated image p takes the label of reference item p mod N_ref: two rounds give the reference histogram twice
    result = MD.mode_coverage(G, dataset, bins=4, res=8, holdout=0, num=200, batch=32, device=CPU)
    arrays = result["arrays"]
    assert result["stats"]["N_ref"] == 100 and np.array_equal(arrays["counts_gen"], 2 * arrays["counts_ref"]) and sorted(arrays["counts_ref"]) == [10, 30, 30, 30]
    assert np.array_equal(arrays["gen_labels"], np.tile(arrays["ref_labels"], 2)) and result["stats"]["generated"] == dict(ndb=0, ndb_over_k=0.0, js=0.0)
    # with --class both sets are the items of that class
    one = MD.mode_coverage(G, dataset, bins=2, res=8, holdout=0.2, class_idx=1, num=12, device=CPU)
    assert (one["stats"]["N_ref"], one["stats"]["N_holdout"], one["stats"]["N_gen"]) == (8, 2, 12)
    assert sorted(np.concatenate([one["arrays"]["ref_items"], one["arrays"]["holdout_items"]]).tolist()) == np.nonzero(mode == 1)[0].tolist()
    cent = one["arrays"]["centroids"].reshape(2, 3, 64).astype(int)
    assert np.abs(cent - np.array(mu.MODE_COLOURS[1])[None, :, None]).max() <= 4
    with pytest.raises(ValueError, match="holds no image of this class"):
        MD.mode_coverage(G, ImageFolderDataset(path=dataset._path, use_labels=True, max_size=3), bins=1, res=8, class_idx=1, holdout=0, device=CPU)


def test_refusals_of_the_tool(data):
    images, mode, root = data
    dataset = ImageFolderDataset(path=root)
    G = BankGenerator(images[:8])
    for kw, message in [(dict(bins=257), "--bins=257"), (dict(bins=200, holdout=0.5), "120 images of the reference set"), (dict(res=32), "power of two"),
                        (dict(holdout=1.0), "--holdout"), (dict(alpha=0.0), "--alpha"), (dict(iters=0), "--iters"), (dict(num=0), "--num"), (dict(batch=0), "--batch")]:
        with pytest.raises(ValueError, match=message):
            MD.mode_coverage(G, dataset, **dict(dict(bins=4, res=8), **kw), device=CPU)
    with pytest.raises(ValueError, match="x-flips"):
        MD.mode_coverage(G, ImageFolderDataset(path=root, xflip=True), bins=4, res=8, device=CPU)
    with pytest.raises(ValueError, match="the generator makes"):
        MD.mode_coverage(BankGenerator(np.zeros([2, 3, 8, 8], dtype=np.uint8)), dataset, bins=4, res=8, device=CPU)


def test_cli_run_on_the_cpu(data, tmp_path, capsys, monkeypatch):
    from test_calc_metrics_cpu import _run
    images, mode, root = data
    _, overrides, snap, _ = _run(tmp_path)
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", lambda config, state, device: BankGenerator(images[mode != 2]).to(device))
    out = tmp_path / "out"
    result = MD.run_modes(overrides + [f"--snapshot={snap}", f"--outdir={out}", f"--data={root}", "--bins=4", "--res=8", "--holdout=0.25", "--show=2",
                                       "--examples=3", "--batch=50", "--device=cpu"])
    want, _ = _missing_mode_run(data, None)
    assert result["stats"] == want["stats"] and np.array_equal(result["canvas"], want["canvas"])
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed["generated"] == want["stats"]["generated"] and "bins" not in printed
    assert sorted(os.listdir(out)) == ["modes.json", "modes.npz", "modes.png"]


def test_option_parsing(tmp_path, capsys):
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    ok = [f"--snapshot={snap}", f"--outdir={tmp_path / 'out'}"]
    overrides, args = MD.parse_args(["exp.config=a.yaml"] + ok)
    assert overrides == ["exp.config=a.yaml"]
    assert (args.bins, args.res, args.num, args.holdout, args.alpha, args.seed, args.iters, args.show, args.examples) == (100, 32, None, 0.2, 0.05, 0, 30, 6, 4)
    assert (args.data, args.truncation_psi, args.class_idx, args.noise_mode, args.device, args.batch, args.from_file) == (None, 1, None, "const", "auto", 64, None)
    _, args = MD.parse_args(ok + ["--bins=256", "--res=none", "--num=7", "--holdout=0", "--alpha=0.01", "--seed=3", "--iters=5", "--show=0", "--examples=0",
                                  "--data=/d", "--trunc=0.5", "--class=2", "--noise-mode=random", "--device=cpu", "--batch=16", f"--from={snap}"])
    assert (args.bins, args.res, args.num, args.holdout, args.alpha, args.seed, args.iters, args.show, args.examples) == (256, None, 7, 0, 0.01, 3, 5, 0, 0)
    assert (args.data, args.truncation_psi, args.class_idx, args.noise_mode, args.device, args.batch, args.from_file) == ("/d", 0.5, 2, "random", "cpu", 16, str(snap))
    for bad, message in [(ok + ["--bins=257"], "between 1 and 256"), (ok + ["--bins=0"], "between 1 and 256"), (ok + ["--res=24"], "power of two"),
                         (ok + ["--num=0"], "at least 1"), (ok + ["--holdout=1"], "below 1"), (ok + ["--alpha=1"], "between 0 and 1"),
                         (ok + ["--iters=0"], "at least 1"), (ok + ["--show=-1"], "not be negative"), (ok + ["--batch=0"], "at least 1"),
                         (ok + [f"--from={tmp_path / 'absent.npz'}"], "no such file"), ([f"--snapshot={snap}"], "--outdir"), (ok + ["--frobnicate"], "unrecognised")]:
        with pytest.raises(SystemExit):
            MD.parse_args(bad)
        assert message in capsys.readouterr().err, bad


# ---------------------------------------------------------------------------------------------------------------- plumbing

def test_prototypes_are_in_the_binding_table():
    lib = _lib.load()
    assert _lib.KERNEL_KINDS[31] == "kmeans_u8" and _lib.KMEANS_VARIANTS == {0: "accumulate", 1: "finish"}
    assert len(lib.sbg_kmeans_u8_update.argtypes) == 11 and len(lib.sbg_kmeans_u8_update_workspace.argtypes) == 3
    assert lib.sbg_kmeans_u8_update_workspace.restype is _lib.ctypes.c_int64
    for n, f, k in [(0, 16, 1), (1, 24, 1), (1, 0, 1), (1, 16, 0), (1, 16, 257), ((1 << 24) + 1, 16, 1), (1, (3 << 20) + 16, 1)]:
        assert lib.sbg_kmeans_u8_update_workspace(n, f, k) == -1, (n, f, k)
    for n, f, k in [(1, 16, 1), (4099, 272, 7), (1 << 24, 16, 256), (50000, 3072, 100), (70000, 12288, 100)]:
        size = lib.sbg_kmeans_u8_update_workspace(n, f, k)
        assert size > 0 and size % (4 * k * (f + 1)) == 0 and size // (4 * k * (f + 1)) <= 512, (n, f, k)
    assert 0 < lib.sbg_kmeans_u8_update_workspace(1 << 17, 196608, 128) <= 1 << 30          # the bound of the largest --res=none run
    assert lib.sbg_kmeans_u8_update_workspace(8421505, 16, 2) >= 2 * 4 * 2 * 17             # more than 2^23 rows: more than one partial


def test_the_reduction_helpers_are_shared():
    for name in ("check_res", "reduce_images", "reduce_store"):
        assert getattr(nearest_neighbors, name) is getattr(tool_support, name) and getattr(MD, name) is getattr(tool_support, name)


def test_the_tool_imports_no_other_tool():
    from test_tool_support_cpu import TOOLS
    mod = importlib.import_module("style_big_gan_amd.modes")
    others = {f"style_big_gan_amd.{t}" for t in tuple(TOOLS) + ("diversity", "realism", "directions", "style_mixing", "generate")}
    held = {v.__name__ if isinstance(v, types.ModuleType) else getattr(v, "__module__", None) for v in vars(mod).values()}
    assert not held & others, held & others
