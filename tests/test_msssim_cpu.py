"""Pairwise MS-SSIM on the CPU (torch_utils/ops/msssim.py, diversity.py): the CPU path against the independent
restatement under the derived bounds, the exact cases, the levels and weights, every refusal, the invariance under the cut and the order
of a batch, and the tool end to end with a stand-in generator."""
import importlib
import json
import os
import types

import numpy as np
import PIL.Image
import pytest
import torch

import msssim_util as MU
from style_big_gan_amd import _lib, diversity as DV
from style_big_gan_amd.torch_utils.ops import msssim
from test_calc_metrics_cpu import _run


def test_window_levels_and_weights():
    g = msssim.window()
    k = np.arange(11, dtype=np.float64)
    e = np.exp(-(k - 5) ** 2 / 4.5)
    total = 0.0
    for v in e:
        total = total + v
    assert g.dtype == torch.float64 and np.array_equal(g.numpy(), e / total) and np.array_equal(g.numpy(), g.numpy()[::-1])
    assert abs(float(g.sum()) - 1) < 1e-15 and np.allclose(torch.outer(g, g).numpy(), MU.ref_window2d().numpy(), rtol=0, atol=1e-16)
    assert msssim.C1 == (0.01 * 255) ** 2 and msssim.C2 == (0.03 * 255) ** 2
    for s, num in [(16, 1), (32, 2), (64, 3), (128, 4), (256, 5), (1024, 5)]:
        sides, w = msssim.levels(s)
        assert sides == [s >> i for i in range(num)] and sides[-1] >= 16 and w.dtype == np.float64 and w.shape == (num,)
        pub = np.array(MU.PUBLISHED[:num], dtype=np.float64)
        if num == 5:
            assert np.array_equal(w, pub)                   # as published: they sum to 1.0001
        else:
            total = np.float64(0.0)
            for v in pub:
                total = total + v
            assert np.array_equal(w, pub / total) and abs(w.sum() - 1) < 1e-15
    assert msssim.levels(16)[1].tolist() == [1.0]
    for s in (8, 48, 0, 32768):
        with pytest.raises(ValueError, match=f"S={s} must be a power of two in \\[16, 16384\\]"):
            msssim.levels(s)


@pytest.mark.parametrize("S", [16, 32, 64, 256])
@pytest.mark.parametrize("kind", ["float", "bytes"])
def test_level_terms_against_the_restatement(kind, S):
    x, y = MU.random_pair(kind, 2, 3, S)
    got = msssim.level_terms(x, y)
    ref = MU.ref_level_terms(x, y)
    assert got.dtype == torch.float64 and tuple(got.shape) == (2, 3, 2)
    err = float((got - ref).abs().max())
    print(f"{kind} S={S}: max |term - restatement| {err:.3e}, bound {MU.TERM_ATOL:.0e}")
    assert err <= MU.TERM_ATOL


@pytest.mark.parametrize("C,S", [(3, 16), (1, 32), (3, 64), (3, 256)])
def test_pair_scores_against_the_restatement(C, S):
    x, y = MU.correlated_pair(3, C, S, seed=S + C)
    ref_scores, ref_terms = MU.ref_pair_scores(x, y)
    assert float(ref_terms.min()) >= 0.1, float(ref_terms.min())             # on the restatement alone: the power is not Lipschitz near 0
    scores, terms = msssim.pair_scores(x, y)
    assert scores.dtype == terms.dtype == torch.float64 and tuple(scores.shape) == (3,) and tuple(terms.shape) == (3, C, MU.ref_num_levels(S))
    err_t = float((terms - ref_terms).abs().max())
    err_s = float(((scores - ref_scores) / ref_scores).abs().max())
    print(f"C={C} S={S}: smallest term {float(ref_terms.min()):.3f}, max term error {err_t:.3e}, max relative score error {err_s:.3e}")
    assert err_t <= MU.TERM_ATOL and err_s <= MU.SCORE_RTOL
    assert 0 < float(scores.min()) and float(scores.max()) < 1


@pytest.mark.parametrize("C,S", [(1, 16), (3, 64), (3, 256)])
def test_identical_images_score_exactly_one(C, S):
    x = torch.from_numpy(MU.smooth_images(2, C, S, seed=3))
    noise, _ = MU.random_pair("float", 2, C, S)
    for v in (x, x.to(torch.float32), noise):
        scores, terms = msssim.pair_scores(v, v.clone())
        assert scores.tolist() == [1.0, 1.0] and bool((terms == 1.0).all())
        assert bool((msssim.level_terms(v, v.clone()) == 1.0).all())


def test_independent_random_bytes_reach_a_negative_mean_and_score_zero_there():
    x, y = MU.random_pair("bytes", 2, 3, 64)
    scores, terms = msssim.pair_scores(x, y)
    t = terms.numpy()
    assert tuple(t.shape) == (2, 3, 3) and (t[:, :, :2] < 0).any()            # a negative cs mean
    _, w = msssim.levels(64)
    per_channel = np.ones([2, 3])
    for i in range(3):
        per_channel = per_channel * np.maximum(t[:, :, i], 0.0) ** w[i]
    dead = (t <= 0).any(axis=2)
    assert dead.any() and (per_channel[dead] == 0).all() and (per_channel[~dead] > 0).all()
    assert np.array_equal(scores.numpy(), ((per_channel[:, 0] + per_channel[:, 1]) + per_channel[:, 2]) / 3.0)
    assert np.allclose(t, MU.ref_pair_scores(x, y)[1].numpy(), rtol=0, atol=MU.TERM_ATOL)


def test_down_is_the_exact_box_mean():
    x = torch.from_numpy(np.random.RandomState(1).randint(0, 256, [2, 3, 256, 256], dtype=np.uint8))
    ref = x.to(torch.float64)
    a = b = x
    for _ in range(4):                                      # exact for byte images at all five levels
        a, b, ref = msssim.down(a), msssim.down(b.to(torch.float32)), torch.nn.functional.avg_pool2d(ref, 2)
        assert a.dtype == torch.float32 and a.is_contiguous() and MU.same_bits(a, b) and torch.equal(a.to(torch.float64), ref)
    f = torch.from_numpy((np.random.RandomState(2).rand(1, 1, 4, 4) * 255).astype(np.float32))
    want = ((f[:, :, 0::2, 0::2] + f[:, :, 0::2, 1::2]) + (f[:, :, 1::2, 0::2] + f[:, :, 1::2, 1::2])) * 0.25
    assert MU.same_bits(msssim.down(f), want.contiguous())


def test_refusals():
    z = lambda *shape: torch.zeros(shape)
    for fn in (msssim.level_terms, msssim.pair_scores):
        for shape, message in [((1, 3, 48, 48), r"S=48 must be a power of two in \[16, 16384\]"), ((1, 3, 8, 8), r"S=8 must be a power of two"),
                               ((1, 2, 16, 16), r"expects 1 or 3 channels, got \(1, 2, 16, 16\)"), ((1, 3, 16, 32), r"square images \[N, C, S, S\]"),
                               ((3, 16, 16), r"square images")]:
            with pytest.raises(ValueError, match=message):
                fn(z(*shape), z(*shape))
        with pytest.raises(ValueError, match=r"x is torch.float32 \(2, 3, 16, 16\) on cpu, y is torch.float32 \(1, 3, 16, 16\) on cpu"):
            fn(z(2, 3, 16, 16), z(1, 3, 16, 16))
        with pytest.raises(ValueError, match=r"y is torch.float32 \(1, 3, 32, 32\)"):
            fn(z(1, 3, 16, 16), z(1, 3, 32, 32))
        with pytest.raises(ValueError, match=r"x is torch.uint8"):
            fn(z(1, 3, 16, 16).to(torch.uint8), z(1, 3, 16, 16))
        with pytest.raises(RuntimeError, match="uint8 or float32"):
            fn(z(1, 3, 16, 16).double(), z(1, 3, 16, 16).double())
        with pytest.raises(RuntimeError, match="must be a torch tensor"):
            fn(np.zeros([1, 3, 16, 16], dtype=np.float32), z(1, 3, 16, 16))
        with pytest.raises(ValueError, match="dense"):
            fn(z(1, 3, 16, 32)[:, :, :, ::2], z(1, 3, 16, 16))
    with pytest.raises(ValueError, match=r"S=6 must be a power of two in \[2, 16384\]"):
        msssim.down(z(1, 1, 6, 6))
    assert tuple(msssim.level_terms(z(0, 3, 16, 16), z(0, 3, 16, 16)).shape) == (0, 3, 2)


@pytest.mark.parametrize("kind", ["float", "bytes"])
def test_equal_bits_under_any_batch_cut_and_pair_order(kind):
    x, y = MU.random_pair(kind, 5, 3, 32)
    whole = msssim.level_terms(x, y)
    scores, terms = msssim.pair_scores(x, y)
    cut = torch.cat([msssim.level_terms(x[:2], y[:2]), msssim.level_terms(x[2:3], y[2:3]), msssim.level_terms(x[3:], y[3:])])
    assert MU.same_bits(whole, cut)
    order = torch.tensor([3, 0, 4, 2, 1])
    assert MU.same_bits(whole[order], msssim.level_terms(x[order].contiguous(), y[order].contiguous()))
    s2, t2 = msssim.pair_scores(x[order].contiguous(), y[order].contiguous())
    assert MU.same_bits(scores[order], s2) and MU.same_bits(terms[order], t2)
    each = [msssim.pair_scores(x[i:i + 1], y[i:i + 1]) for i in range(5)]
    assert MU.same_bits(scores, torch.cat([e[0] for e in each])) and MU.same_bits(terms, torch.cat([e[1] for e in each]))
    if kind == "bytes":                                     # bytes as uint8 and as fp32 are one input
        assert MU.same_bits(whole, msssim.level_terms(x.float(), y.float()))


def test_abi_symbols_resolve():
    lib = _lib.load()
    for name in ("sbg_msssim_workspace", "sbg_msssim_level", "sbg_msssim_down"):
        assert getattr(lib, name) is not None
    assert _lib.KERNEL_KINDS[29] == "msssim" and _lib.MSSSIM_VARIANTS == {0: "level", 1: "down", 2: "merge"}
    assert lib.sbg_msssim_workspace(1, 16) == 16 and lib.sbg_msssim_workspace(6, 64) == 6 * 2 * 8 * 8 and lib.sbg_msssim_workspace(3, 256) == 3 * 128 * 16
    for bc, s in [(0, 16), (1, 8), (1, 48), (1, 32768), (1 << 24, 256)]:
        assert lib.sbg_msssim_workspace(bc, s) == -1, (bc, s)


# ------------------------------------------------------------------------------------------------ the tool

def test_option_parsing_and_failures(tmp_path, capsys):
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    overrides, args = DV.parse_args(["exp.config=a.yaml", f"--outdir={tmp_path}", "--data=/d"])
    assert overrides == ["exp.config=a.yaml"] and vars(args) == dict(
        outdir=str(tmp_path), snapshot=None, data="/d", pairs=10000, seed=0, truncation_psi=1, class_idx=None, noise_mode="const", device="auto",
        batch=64, closest=8)
    _, args = DV.parse_args([f"--outdir={tmp_path}", f"--snapshot={snap}", "--pairs=100", "--seed=3", "--trunc=0.5", "--class=2", "--noise-mode=random",
                             "--device=cpu", "--batch=16", "--closest=0"])
    assert (args.pairs, args.seed, args.truncation_psi, args.class_idx, args.noise_mode, args.device, args.batch, args.closest, args.data) == \
        (100, 3, 0.5, 2, "random", "cpu", 16, 0, None)
    ok = [f"--outdir={tmp_path}", "--data=/d"]
    for bad, message in [(["--data=/d"], "--outdir"), ([f"--outdir={tmp_path}"], "at least one of --snapshot and --data"), (ok + ["--pairs=0"], "at least 1"),
                         (ok + ["--batch=0"], "at least 1"), (ok + ["--closest=-1"], "negative"), (ok + ["--seed=-1"], "negative"),
                         (ok + [f"--snapshot={tmp_path / 'absent.pt'}"], "no such file"), (ok + ["--frobnicate"], "unrecognised")]:
        with pytest.raises(SystemExit):
            DV.parse_args(bad)
        assert message in capsys.readouterr().err, bad


def test_the_tool_imports_no_other_tool():
    tools = ("generate", "style_mixing", "projector", "calc_metrics", "nearest_neighbors", "avg_spectra", "dataset_tool")
    others = {f"style_big_gan_amd.{t}" for t in tools}
    mod = importlib.import_module("style_big_gan_amd.diversity")
    held = {v.__name__ if isinstance(v, types.ModuleType) else getattr(v, "__module__", None) for v in vars(mod).values()}
    assert not held & others, held & others
    assert "diversity" in importlib.import_module("style_big_gan_amd.tool_support").__doc__


def _walk(order, classes, pairs):
    """the real-pair walk, restated"""
    out, pending = [], {}
    for i in order:
        if len(out) == pairs:
            break
        k = -1 if classes is None else int(classes[i])
        if k in pending:
            out.append((pending.pop(k), int(i), k))
        else:
            pending[k] = int(i)
    return out


def _bank():
    """24 smooth 32 x 32 images; the seeds 2, 3 and 8, 9 (pairs 1 and 4) hold one image each"""
    bank = MU.smooth_images(24, 3, 32, seed=5)
    bank[3], bank[9] = bank[2], bank[8]
    return bank


def test_tool_end_to_end_unconditional(tmp_path, monkeypatch, capsys):
    _, overrides, snap, _ = _run(tmp_path)
    bank = _bank()
    reals = MU.smooth_images(13, 3, 32, seed=9)
    data = MU.tool_dataset(tmp_path, reals)
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", lambda config, state, device: MU.ClassGenerator(bank).to(device))
    common = overrides + ["--device=cpu", "--batch=4", "--pairs=6"]

    out = tmp_path / "out"
    capsys.readouterr()
    result = DV.run_diversity(common + [f"--outdir={out}", f"--snapshot={snap}", f"--data={data}", "--closest=3"])
    assert sorted(os.listdir(out)) == ["closest_pairs.png", "diversity.json", "diversity_pairs.npz"]
    stats = json.load(open(out / "diversity.json"))
    assert stats == json.loads(json.dumps(result["stats"]))
    assert set(stats) == {"image_size", "channels", "level_sides", "weights", "options", "gen", "real", "closest_pairs", "fraction_above_real_p99"}
    assert (stats["image_size"], stats["channels"], stats["level_sides"]) == (32, 3, [32, 16]) and stats["weights"] == msssim.levels(32)[1].tolist()
    assert stats["options"] == dict(pairs=6, seed=0, trunc=1, class_idx=None, noise_mode="const", batch=4, closest=3)
    npz = np.load(out / "diversity_pairs.npz")
    assert sorted(npz.files) == ["gen_classes", "gen_scores", "gen_seeds", "gen_terms", "real_classes", "real_items", "real_scores", "real_terms"]

    # generated pair p is the images of the seeds 2p and 2p + 1
    want_scores, want_terms = msssim.pair_scores(torch.from_numpy(bank[0:12:2].copy()), torch.from_numpy(bank[1:12:2].copy()))
    assert np.array_equal(npz["gen_scores"], want_scores.numpy()) and np.array_equal(npz["gen_terms"], want_terms.numpy())
    assert npz["gen_seeds"].tolist() == [[2 * p, 2 * p + 1] for p in range(6)] and npz["gen_classes"].tolist() == [-1] * 6
    assert npz["gen_scores"][1] == 1.0 and npz["gen_scores"][4] == 1.0 and (np.delete(npz["gen_scores"], [1, 4]) < 1).all()

    # real pairs: consecutive items of the permutation, flips off
    order = np.random.RandomState(0).permutation(13)
    walk = _walk(order, None, 6)
    assert npz["real_items"].tolist() == [[a, b] for a, b, _ in walk] == [[int(order[2 * p]), int(order[2 * p + 1])] for p in range(6)]
    assert npz["real_classes"].tolist() == [-1] * 6
    real_scores, real_terms = msssim.pair_scores(torch.from_numpy(reals[npz["real_items"][:, 0]]), torch.from_numpy(reals[npz["real_items"][:, 1]]))
    assert np.array_equal(npz["real_scores"], real_scores.numpy()) and np.array_equal(npz["real_terms"], real_terms.numpy())

    # the summaries
    for name in ("gen", "real"):
        s, t = npz[f"{name}_scores"], npz[f"{name}_terms"]
        assert set(stats[name]) == {"msssim", "msssim_std", "p01", "p10", "p50", "p90", "p99", "levels", "num_pairs"}
        acc = 0.0
        for v in s:
            acc = acc + float(v)
        assert stats[name]["msssim"] == acc / 6 and stats[name]["msssim_std"] == float(np.std(s)) and stats[name]["num_pairs"] == 6
        assert [stats[name][k] for k in ("p01", "p10", "p50", "p90", "p99")] == np.quantile(s, [0.01, 0.1, 0.5, 0.9, 0.99]).tolist()
        assert set(stats[name]["levels"]) == {"32", "16"}
        assert abs(stats[name]["levels"]["16"] - t[:, :, 1].mean()) < 1e-15 and abs(stats[name]["levels"]["32"] - t[:, :, 0].mean()) < 1e-15
    assert stats["fraction_above_real_p99"] == float(np.mean(npz["gen_scores"] >= np.quantile(npz["real_scores"], 0.99)))
    assert stats["fraction_above_real_p99"] >= 2 / 6         # the two pairs of identical images always count
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["gen"]["msssim"] == stats["gen"]["msssim"] and line["fraction_above_real_p99"] == stats["fraction_above_real_p99"]

    # closest_pairs: descending by score, the tie of the pairs 1 and 4 to the lower pair
    third = int(np.argsort(-npz["gen_scores"], kind="stable")[2])
    assert stats["closest_pairs"] == [1, 4, third] and third not in (1, 4)
    png = np.array(PIL.Image.open(out / "closest_pairs.png"))
    assert png.shape == (96, 64, 3)
    for row, p in enumerate([1, 4, third]):
        assert np.array_equal(png[32 * row:32 * row + 32, :32], bank[2 * p].transpose(1, 2, 0))
        assert np.array_equal(png[32 * row:32 * row + 32, 32:], bank[2 * p + 1].transpose(1, 2, 0))

    # --seed changes the real pairs only; --pairs stops the walk; another batch size changes nothing
    again = tmp_path / "again"
    DV.run_diversity(overrides + ["--device=cpu", "--batch=5", "--pairs=6", "--seed=1", f"--outdir={again}", f"--snapshot={snap}", f"--data={data}", "--closest=0"])
    assert sorted(os.listdir(again)) == ["diversity.json", "diversity_pairs.npz"]                # no png with --closest=0
    npz1 = np.load(again / "diversity_pairs.npz")
    assert np.array_equal(npz1["gen_scores"], npz["gen_scores"]) and np.array_equal(npz1["gen_terms"], npz["gen_terms"])
    order1 = np.random.RandomState(1).permutation(13)
    assert npz1["real_items"].tolist() == [[int(order1[2 * p]), int(order1[2 * p + 1])] for p in range(6)] != npz["real_items"].tolist()
    assert "closest_pairs" not in json.load(open(again / "diversity.json"))

    # the data set alone, the generator alone
    alone = tmp_path / "alone"
    DV.run_diversity(overrides + ["--device=cpu", "--pairs=4", f"--outdir={alone}", f"--data={data}"])
    assert sorted(os.listdir(alone)) == ["diversity.json", "diversity_pairs.npz"]
    npz2 = np.load(alone / "diversity_pairs.npz")
    assert sorted(npz2.files) == ["real_classes", "real_items", "real_scores", "real_terms"]
    assert npz2["real_items"].tolist() == npz["real_items"][:4].tolist() and np.array_equal(npz2["real_scores"], npz["real_scores"][:4])
    assert set(json.load(open(alone / "diversity.json"))) == {"image_size", "channels", "level_sides", "weights", "options", "real"}
    gen_only = tmp_path / "gen_only"
    DV.run_diversity(common + [f"--outdir={gen_only}", f"--snapshot={snap}", "--pairs=12", "--batch=64"])      # --closest defaults to 8
    assert sorted(os.listdir(gen_only)) == ["closest_pairs.png", "diversity.json", "diversity_pairs.npz"]
    assert np.array(PIL.Image.open(gen_only / "closest_pairs.png")).shape == (8 * 32, 64, 3)
    capsys.readouterr()
    DV.run_diversity(common + [f"--outdir={gen_only}", f"--snapshot={snap}", "--class=1"])
    assert "warn: --class=lbl ignored" in capsys.readouterr().out


def test_tool_end_to_end_with_classes(tmp_path, monkeypatch):
    _, overrides, snap, _ = _run(tmp_path)
    bank = _bank()
    reals = MU.smooth_images(13, 3, 32, seed=9)
    labels = [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 0, 1]                       # 5, 5 and 3 items: the walk ends at 2 + 2 + 1 pairs
    data = MU.tool_dataset(tmp_path, reals, labels)
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", lambda config, state, device: MU.ClassGenerator(bank, c_dim=3, shift=5).to(device))
    common = overrides + ["--device=cpu", "--batch=4", "--pairs=6", f"--snapshot={snap}", f"--data={data}", "--closest=2"]

    cycle = tmp_path / "cycle"
    DV.run_diversity(common + [f"--outdir={cycle}"])
    npz = np.load(cycle / "diversity_pairs.npz")
    stats = json.load(open(cycle / "diversity.json"))
    assert npz["gen_classes"].tolist() == [0, 1, 2, 0, 1, 2]                 # pair p has class p mod c_dim
    first = [(2 * p + 5 * (p % 3)) % 24 for p in range(6)]
    want, _ = msssim.pair_scores(torch.from_numpy(bank[first]), torch.from_numpy(bank[[(i + 1) % 24 for i in first]]))
    assert np.array_equal(npz["gen_scores"], want.numpy())
    order = np.random.RandomState(0).permutation(13)
    walk = _walk(order, labels, 6)
    assert len(walk) == 5 and npz["real_items"].tolist() == [[a, b] for a, b, _ in walk] and npz["real_classes"].tolist() == [k for _, _, k in walk]
    assert all(labels[a] == labels[b] == k for a, b, k in walk)
    assert stats["real"]["num_pairs"] == 5 and set(stats["gen"]["per_class"]) == {"0", "1", "2"}
    assert set(stats["real"]["per_class"]) == {str(k) for k in set(npz["real_classes"].tolist())}
    for k in (0, 1, 2):
        sel = npz["gen_scores"][npz["gen_classes"] == k]
        assert stats["gen"]["per_class"][str(k)]["num_pairs"] == 2 and stats["gen"]["per_class"][str(k)]["msssim"] == (float(sel[0]) + float(sel[1])) / 2

    one = tmp_path / "one"
    DV.run_diversity(common + [f"--outdir={one}", "--class=1"])
    npz1 = np.load(one / "diversity_pairs.npz")
    assert npz1["gen_classes"].tolist() == [1] * 6 and "per_class" not in json.load(open(one / "diversity.json"))["gen"]
    want1, _ = msssim.pair_scores(torch.from_numpy(bank[[(2 * p + 5) % 24 for p in range(6)]]), torch.from_numpy(bank[[(2 * p + 6) % 24 for p in range(6)]]))
    assert np.array_equal(npz1["gen_scores"], want1.numpy()) and not np.array_equal(npz1["gen_scores"], npz["gen_scores"])
    assert npz1["real_items"].tolist() == npz["real_items"].tolist()        # --class moves the generated pairs only
    with pytest.raises(ValueError, match=r"--class=3: the network has the classes 0\.\.2"):
        DV.run_diversity(common + [f"--outdir={one}", "--class=3"])


def test_tool_function_refusals():
    G = MU.ClassGenerator(_bank())
    for kw, message in [(dict(pairs=0), "--pairs=0"), (dict(batch=0), "--batch=0"), (dict(closest=-1), "--closest=-1")]:
        with pytest.raises(ValueError, match=message):
            DV.pairwise_diversity(G, None, **kw)
    with pytest.raises(ValueError, match="at least one of --snapshot and --data"):
        DV.pairwise_diversity(None, None)
    with pytest.raises(ValueError, match=r"S=8 must be a power of two"):
        DV.pairwise_diversity(MU.ClassGenerator(np.zeros([2, 3, 8, 8], dtype=np.uint8)), None, pairs=1)
    with pytest.raises(ValueError, match="1 or 3 channels only"):
        DV.pairwise_diversity(MU.ClassGenerator(np.zeros([2, 2, 16, 16], dtype=np.uint8)), None, pairs=1)
    assert DV.closest_order([0.5, 1.0, 0.25, 1.0, 0.75], 3).tolist() == [1, 3, 4]
    items, classes = DV.real_pairs(7, np.array([0, 0, 1, 1, 0, 0, 2]), 10, seed=4)
    order = np.random.RandomState(4).permutation(7)
    assert [tuple(p) + (k,) for p, k in zip(items.tolist(), classes.tolist())] == _walk(order, [0, 0, 1, 1, 0, 0, 2], 10)
