"""The realism score without a device: the op's torch path against the numpy oracle of knn_realism_util bit for bit (exact integer features,
pruned radii, exclusions, ties, duplicates), its invariants and refusals, the C prototypes and the workspace formula, `scores.realism_scores`
(pruning, its ties, the leave-one-out baseline) and the tool end to end with the exact stand-in detector of the feature-space search tests."""
import importlib
import json
import os
import re
import types

import numpy as np
import PIL.Image
import pytest
import torch

import knn_manifold_util as ku
import knn_realism_util as ru
import nearest_util as N
from test_knn_workspace_cpu import SHAPES, expected
from test_nearest_neighbors_feature_cpu import ScriptedDetector, _data, detector, reduce
from test_calc_metrics_cpu import _cpu_generator, _run
from style_big_gan_amd import _lib, realism as RL, nearest_neighbors, tool_support
from style_big_gan_amd.metrics import scores
from style_big_gan_amd.torch_utils.ops import knn_manifold

CPU = torch.device("cpu")
EXACT = [(37, 130, 40, 3, 11), (300, 260, 72, 7, 0), (300, 5000, 40, 7, 77)]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x))


def _op(probes, manifold, radius, exclude=None):
    score, index = knn_manifold.realism(_t(probes), _t(manifold), _t(radius), _t(exclude))
    assert score.dtype == torch.float32 and index.dtype == torch.int32 and score.shape == index.shape == (len(probes),)
    return score.numpy(), index.numpy()


@pytest.mark.parametrize("excluded", [False, True])
@pytest.mark.parametrize("pruned", [False, True])
@pytest.mark.parametrize("R,C,F,k,offset", EXACT)
def test_cpu_path_equals_the_oracle_bit_for_bit(R, C, F, k, offset, pruned, excluded):
    case = ku.exact_case(R, C, F, k, offset)
    want_score, want_index, radius, exclude = ru.exact_realism(R, C, F, k, offset, pruned, excluded)
    score, index = _op(case["probes"], case["manifold"], radius, exclude)
    ties = ru.tied(case["probes"], case["manifold"], radius, exclude)
    print(f"inf {np.mean(np.isinf(want_score)):.2f}, tied {ties.mean():.2f}, score >= 1 {np.mean(want_score >= 1):.2f}")
    assert np.array_equal(ru.f32_bits(score), ru.f32_bits(want_score)) and np.array_equal(index, want_index)
    assert np.isinf(want_score).any() and ties.any()           # the case exercises both rules
    if excluded:
        assert (index != exclude).all()


def test_all_radii_negative_gives_zero_and_minus_one():
    case = ku.exact_case(37, 130, 40, 3, 11)
    score, index = _op(case["probes"], case["manifold"], np.full([130], -1, dtype=np.float16))
    assert not score.any() and (index == -1).all()
    # ... and so does a probe whose only kept ball is the one it excludes
    radius = np.full([130], -1, dtype=np.float16)
    radius[4] = 2
    score, index = _op(case["probes"], case["manifold"], radius, np.full([37], 4, dtype=np.int32))
    assert not score.any() and (index == -1).all()


def test_an_exact_tie_goes_to_the_lower_index():
    manifold = np.zeros([6, 8], dtype=np.float16)
    manifold[:, 0] = [3, -3, 4, -4, 3, 6]                       # at distances 3, 3, 4, 4, 3, 6 of the origin
    radius = np.array([1.5, 3, 2, 4, 3, 6], dtype=np.float16)   # ratios 0.5, 1, 0.5, 1, 1, 1: a four-way tie at indices 1, 3, 4, 5
    probes = np.zeros([2, 8], dtype=np.float16)
    score, index = _op(probes, manifold, radius)
    assert score.tolist() == [1.0, 1.0] and index.tolist() == [1, 1]
    score, index = _op(probes, manifold, radius, np.array([1, 3], dtype=np.int32))
    assert score.tolist() == [1.0, 1.0] and index.tolist() == [3, 1]
    radius[1] = -1
    assert _op(probes, manifold, radius)[1].tolist() == [3, 3]


def test_a_duplicate_row_scores_infinity_also_at_radius_zero():
    case = ku.exact_case(37, 130, 40, 3, 11)
    manifold, probes = case["manifold"], case["probes"]
    assert case["radius_all"][0] == 0 and np.array_equal(probes[0], manifold[0])       # four copies of point 0: radius 0 at k = 3
    score, index = _op(probes, manifold, case["radius_all"])
    assert np.isinf(score[0]) and score[0] > 0 and index[0] == 0
    radius = np.zeros([130], dtype=np.float16)                  # every radius 0: +inf on a copy, 0 everywhere else
    score, index = _op(probes, manifold, radius)
    d = ku.distances(probes, manifold)[0]
    copy = (d == 0).any(axis=1)
    assert copy.any() and not copy.all()
    assert np.isinf(score[copy]).all() and not score[~copy].any()
    assert np.array_equal(index[copy], (d == 0).argmax(axis=1)[copy]) and not index[~copy].any()


@pytest.mark.parametrize("R,C,F,k,offset", EXACT)
def test_score_at_least_one_is_membership(R, C, F, k, offset):
    case = ku.exact_case(R, C, F, k, offset)
    for radius in (case["radius_all"], ru.half_pruned(case["radius_all"])):
        score, _ = _op(case["probes"], case["manifold"], radius)
        inside = knn_manifold.in_manifold(_t(case["probes"]), _t(case["manifold"]), _t(radius)).numpy()
        assert np.array_equal(score >= 1, inside) and 0 < inside.mean() < 1


def test_any_cut_into_batches_gives_the_same_bits(monkeypatch):
    R, C, F, k, offset = EXACT[1]
    case = ku.exact_case(R, C, F, k, offset)
    want_score, want_index, radius, exclude = ru.exact_realism(R, C, F, k, offset, True, True)
    for cuts in ([0, 300], [0, 1, 128, 129, 300], [0, 37, 299, 300]):
        parts = [_op(case["probes"][a:b], case["manifold"], radius, exclude[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        assert np.array_equal(ru.f32_bits(np.concatenate([p[0] for p in parts])), ru.f32_bits(want_score))
        assert np.array_equal(np.concatenate([p[1] for p in parts]), want_index)
    monkeypatch.setattr(knn_manifold, "_CPU_ROWS", 7)           # the op's own row blocks
    score, index = _op(case["probes"], case["manifold"], radius, exclude)
    assert np.array_equal(ru.f32_bits(score), ru.f32_bits(want_score)) and np.array_equal(index, want_index)


def test_refusals():
    x, m = torch.zeros([5, 16], dtype=torch.float16), torch.zeros([9, 16], dtype=torch.float16)
    r = torch.ones([9], dtype=torch.float16)
    for args, message in [((x[0], m, r), r"expects \[R, F\] and \[C, F\]"), ((x[:, :8], m, r), r"expects \[R, F\] and \[C, F\]"),
                          ((x, m, r[:8]), "one radius per manifold point"), ((x, m, r[None]), "one radius per manifold point"),
                          ((x, m, r, torch.zeros([5], dtype=torch.int64)), "exclude must be int32"),
                          ((x, m, r, torch.zeros([4], dtype=torch.int32)), "one excluded manifold index per probe"),
                          ((x, m[:0], r[:0]), "the manifold has 0 points"),
                          ((x.to("meta"), m, r), "different devices"), ((x, m, r.to("meta")), "one radius per manifold point"),
                          ((x, m, r, torch.zeros([5], dtype=torch.int32, device="meta")), "one excluded manifold index per probe")]:
        with pytest.raises(RuntimeError, match=message):
            knn_manifold.realism(*args)
    score, index = knn_manifold.realism(x[:0], m, r)            # no probes: empty outputs
    assert score.shape == index.shape == (0,) and score.dtype == torch.float32 and index.dtype == torch.int32


def test_prototypes_are_in_the_header_and_the_binding_table():
    header = re.sub(r"\s+", " ", open(os.path.join(ROOT, "include", "sbg_hip.h")).read())
    assert "int64_t sbg_knn_realism_workspace(int P, int C);" in header
    assert ("int sbg_knn_realism(const void* probes, const void* manifold, const void* radius, int P, int C, int64_t F, const int32_t* exclude, "
            "float* score, int32_t* index, void* workspace, sbg_stream_t stream);") in header
    lib = _lib.load()
    assert lib.sbg_knn_realism_workspace.restype is not None and len(lib.sbg_knn_realism_workspace.argtypes) == 2
    assert len(lib.sbg_knn_realism.argtypes) == 11
    assert _lib.PR_VARIANTS == {0: "single", 1: "split", 2: "merge", 3: "norms"}


@pytest.mark.parametrize("P,C", SHAPES)
def test_workspace_formula(P, C):
    lib = _lib.load()
    assert lib.sbg_knn_realism_workspace(P, C) == expected(P, C, 4, lambda runs: 8 * P * runs)          # one 64-bit key per (run, row)


def test_workspace_refusals():
    lib = _lib.load()
    big = (1 << 24) + 1
    for P, C in [(0, 100), (100, 0), (-1, 100), (big, 100), (100, big)]:
        assert lib.sbg_knn_realism_workspace(P, C) == -1
    assert lib.sbg_knn_realism_workspace(1 << 24, 1 << 24) > 0


# ---------------------------------------------------------------------------------------------------------------- scores.realism_scores

def test_realism_scores_prunes_the_larger_radius_half():
    real, gen = ku.realistic_features(61, 40, 72, seed=3)
    score, item, kept = scores.realism_scores(_t(real), _t(gen), nhood_size=3, keep=0.5, row_batch_size=16)
    radius = ku.kth_radius(real, real, 3)
    want_kept = ru.prune(radius, 0.5)
    assert np.array_equal(ku.bits(kept.numpy()), ku.bits(want_kept))
    assert (want_kept >= 0).sum() == 31                          # ceil(0.5 * 61)
    assert radius[want_kept >= 0].astype(np.float32).max() <= radius[want_kept < 0].astype(np.float32).min()
    want_score, want_index = ru.realism(gen, real, want_kept)
    assert np.array_equal(ru.f32_bits(score.numpy()), ru.f32_bits(want_score)) and np.array_equal(item.numpy(), want_index)
    assert (want_kept[item.numpy()] >= 0).all()
    # keep = 1 prunes nothing; other values are refused
    assert np.array_equal(ku.bits(scores.realism_scores(_t(real), _t(gen), 3, keep=1.0)[2].numpy()), ku.bits(radius))
    for keep in (0, 1.5, -0.5):
        with pytest.raises(ValueError, match="keep"):
            scores.realism_scores(_t(real), _t(gen), 3, keep=keep)


def test_pruning_ties_go_to_the_lower_index():
    radius = torch.tensor([2, 1, 2, 1, 2, 3, 2], dtype=torch.float16)
    assert scores.pruned_radii(radius, 0.5).tolist() == [2, 1, 2, 1, -1, -1, -1]      # ceil(3.5) = 4 kept: both 1s, then the first two 2s
    assert scores.pruned_radii(radius, 1 / 7).tolist() == [-1, 1, -1, -1, -1, -1, -1]
    assert np.array_equal(ru.prune(radius.numpy(), 0.5), scores.pruned_radii(radius, 0.5).numpy())
    case = ku.exact_case(300, 260, 72, 7, 0)                    # integer features: many equal radii
    r = case["radius_all"]
    kept = scores.pruned_radii(_t(r), 0.5).numpy()
    assert len(np.unique(r)) < len(r) // 2 and np.array_equal(ku.bits(kept), ku.bits(ru.prune(r, 0.5)))
    edge = r[kept >= 0].astype(np.float32).max()
    at_edge = np.nonzero(r.astype(np.float32) == edge)[0]
    assert (kept[at_edge] >= 0).any() and (kept[at_edge] < 0).any()                 # the cut falls inside a run of equal radii ...
    assert at_edge[kept[at_edge] >= 0].max() < at_edge[kept[at_edge] < 0].min()      # ... and keeps its lower indices


def test_leave_one_out_excludes_exactly_the_own_ball():
    case = ku.exact_case(300, 260, 72, 7, 0)                    # duplicate points: a copy elsewhere still counts
    real, probes = case["manifold"], case["probes"]
    out = scores.realism_scores(_t(real), _t(probes), nhood_size=7, keep=0.5, row_batch_size=100, leave_one_out=True)
    assert len(out) == 5
    kept = ru.prune(ku.kth_radius(real, real, 7), 0.5)
    assert np.array_equal(ku.bits(out[2].numpy()), ku.bits(kept))
    want_score, want_index = ru.realism(real, real, kept, np.arange(260, dtype=np.int32))
    assert np.array_equal(ru.f32_bits(out[3].numpy()), ru.f32_bits(want_score)) and np.array_equal(out[4].numpy(), want_index)
    assert (out[4].numpy() != np.arange(260)).all()
    with_own, _ = ru.realism(real, real, kept)                  # with its own ball, a kept point scores +inf at once
    assert np.isinf(with_own[kept >= 0]).all() and not np.isinf(want_score[kept >= 0]).all()
    assert np.isinf(want_score).any()                           # the copies of point 0 find one another


# ---------------------------------------------------------------------------------------------------------------- the tool

def _brute_tool(dataset, queries, k, keep):
    """the tool's numbers by brute force over the subsampled bytes (integer d2, exact in fp32)"""
    items = N.dataset_items(dataset, reduce).astype(np.float16) - 128
    q = np.stack([reduce(x) for x in queries]).reshape(len(queries), -1).astype(np.float16) - 128
    radius = ru.prune(ku.kth_radius(items, items, k), keep)
    return ru.realism(q, items, radius) + (radius,) + ru.realism(items, items, radius, np.arange(len(items), dtype=np.int32))


def test_the_tool_end_to_end(tmp_path):
    dataset, kw = _data(tmp_path, "plain")
    G = N.BankGenerator(N.make_bank(dataset, 24))
    seeds = list(range(40))
    out = tmp_path / "out"
    result = RL.realism_ranking(G, dataset, seeds, k=3, keep=0.5, show=5, batch=7, device=CPU, outdir=str(out), detector=detector, dataset_kwargs=kw)
    queries = N.seed_bytes(G, seeds)
    score, item, radius, real_score, real_item = _brute_tool(dataset, queries, 3, 0.5)
    assert sorted(os.listdir(out)) == ["realism.json", "realism.npz", "realism.png"]
    npz = np.load(out / "realism.npz")
    assert sorted(npz.files) == ["item", "radius", "real_item", "real_score", "score", "seeds"]
    assert npz["seeds"].tolist() == seeds and npz["score"].dtype == npz["real_score"].dtype == np.float32 and npz["radius"].dtype == np.float16
    assert np.array_equal(ru.f32_bits(npz["score"]), ru.f32_bits(score)) and np.array_equal(npz["item"], item)
    assert np.array_equal(ru.f32_bits(npz["real_score"]), ru.f32_bits(real_score)) and np.array_equal(npz["real_item"], real_item)
    assert np.array_equal(ku.bits(npz["radius"]), ku.bits(radius)) and (radius >= 0).sum() == 12
    # strict JSON: the bank's exact copies of kept training images score +inf and are counted, the statistics are clipped
    text = open(out / "realism.json").read()
    stats = json.loads(text, parse_constant=lambda name: pytest.fail(f"realism.json holds {name}"))
    assert stats == result["stats"] and json.dumps(stats, allow_nan=False)
    assert set(stats) == {"k", "keep", "F", "manifold_points", "kept_points", "num", "generated", "real", "fraction_below_real_p01"}
    assert (stats["k"], stats["keep"], stats["F"], stats["manifold_points"], stats["kept_points"], stats["num"]) == (3, 0.5, 192, 23, 12, 40)
    copies = int(sum(any(np.array_equal(reduce(qi), reduce(dataset[j][0])) for j in np.nonzero(radius >= 0)[0]) for qi in queries))
    assert stats["generated"]["num_infinite"] == copies == int(np.isinf(score).sum()) and copies > 0
    assert stats["real"]["num_infinite"] == 0
    for name, values in (("generated", score), ("real", real_score)):
        clipped = np.minimum(values.astype(np.float64), 65504.0)
        q = np.quantile(clipped, [0.01, 0.10, 0.50, 0.90, 0.99])
        want = dict(min=clipped.min(), p01=q[0], p10=q[1], p50=q[2], p90=q[3], p99=q[4], fraction_realistic=np.mean(values >= 1),
                    num_infinite=np.isinf(values).sum())
        assert set(stats[name]) == set(want) and all(stats[name][key] == want[key] for key in want), name
    assert stats["generated"]["p99"] == RL.SCORE_CLIP == 65504.0
    p01 = np.quantile(np.minimum(real_score.astype(np.float64), 65504.0), 0.01)
    assert stats["fraction_below_real_p01"] == float(np.mean(np.minimum(score.astype(np.float64), 65504.0) <= p01))
    # the picture: the 5 highest descending, the 5 lowest ascending, ties (the +inf copies; equal images of one bank entry) to the lower seed
    best = sorted(range(40), key=lambda i: (-float(score[i]), seeds[i]))[:5]
    worst = sorted(range(40), key=lambda i: (float(score[i]), seeds[i]))[:5]
    assert result["shown"] == dict(best=best, worst=worst) and copies >= 2 and best[:2] == sorted(best[:2])
    png = np.array(PIL.Image.open(out / "realism.png"))
    assert png.shape == (2 * 16, 5 * 16, 3) and np.array_equal(png, result["canvas"])
    for row, picks in enumerate((best, worst)):
        cells = png[row * 16:(row + 1) * 16].reshape(16, 5, 16, 3).transpose(1, 3, 0, 2)
        assert np.array_equal(cells, queries[picks]), row
    # the batch size changes nothing, and seeds need not be 0 .. n - 1
    again = RL.realism_ranking(G, dataset, seeds, k=3, keep=0.5, show=5, batch=40, device=CPU, detector=detector, dataset_kwargs=kw)
    assert again["stats"] == result["stats"] and np.array_equal(again["canvas"], result["canvas"]) and again["shown"] == result["shown"]
    some = RL.realism_ranking(G, dataset, [31, 4, 17], show=8, batch=2, device=CPU, detector=detector, dataset_kwargs=kw)
    assert np.array_equal(ru.f32_bits(some["arrays"]["score"]), ru.f32_bits(score[[31, 4, 17]])) and some["canvas"].shape == (32, 3 * 16, 3)
    assert some["arrays"]["seeds"].tolist() == [31, 4, 17]


def test_the_tool_validates_its_options(tmp_path, capsys):
    dataset, kw = _data(tmp_path, "plain")
    G = N.BankGenerator(N.make_bank(dataset, 8))
    run = lambda **more: RL.realism_ranking(G, dataset, [0, 1], device=CPU, **dict(dict(detector=detector, dataset_kwargs=kw), **more))
    for more, message in [(dict(k=0), "--k=0"), (dict(k=8), "--k=8"), (dict(keep=0), "--keep=0"), (dict(keep=1.01), "--keep=1.01"),
                          (dict(show=-1), "--show=-1"), (dict(batch=0), "--batch=0"), (dict(detector=None), "--detector is required"),
                          (dict(dataset_kwargs=None), "dataset_kwargs are required"), (dict(detector=str(tmp_path)), "does not hold vgg16.pt"),
                          (dict(detector=lambda images: detector(images)[:, :190]), "--detector: the detector returns features of shape")]:
        with pytest.raises(ValueError, match=message):
            run(**more)
    with pytest.raises(ValueError, match="no seeds"):
        RL.realism_ranking(G, dataset, [], device=CPU, detector=detector, dataset_kwargs=kw)
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    ok = [f"--snapshot={snap}", f"--outdir={tmp_path / 'out'}", f"--detector={tmp_path}"]
    overrides, args = RL.parse_args(["exp.config=a.yaml"] + ok + ["--num=5"])
    assert overrides == ["exp.config=a.yaml"] and args.seeds == [0, 1, 2, 3, 4] and (args.k, args.keep, args.show, args.batch) == (3, 0.5, 8, 64)
    assert RL.parse_args(ok + ["--seeds=3-6", "--k=5", "--keep=0.25", "--show=0"])[1].seeds == [3, 4, 5, 6]
    for bad, message in [(ok, "exactly one of --seeds and --num"), (ok + ["--seeds=0-3", "--num=4"], "exactly one of --seeds and --num"),
                         (ok + ["--num=0"], "--num must be at least 1"), (ok + ["--num=4", "--k=0"], "--k=0: must be between 1 and 7"),
                         (ok + ["--num=4", "--k=8"], "--k=8"), (ok + ["--num=4", "--keep=0"], "--keep=0"), (ok + ["--num=4", "--keep=1.5"], "--keep=1.5"),
                         (ok + ["--num=4", "--show=-2"], "--show=-2"), (ok + ["--num=4", "--batch=0"], "--batch=0"),
                         (ok[:2] + ["--num=4"], "--detector"), (ok[:2] + [f"--detector={tmp_path / 'absent.pt'}", "--num=4"], "not downloaded"),
                         (ok + ["--num=4", "--frobnicate"], "unrecognised")]:
        with pytest.raises(SystemExit):
            RL.parse_args(bad)
        assert message in capsys.readouterr().err, bad


def test_the_tool_imports_no_other_tool_and_shares_the_feature_helpers():
    from test_tool_support_cpu import TOOLS
    mod = importlib.import_module("style_big_gan_amd.realism")
    others = {f"style_big_gan_amd.{t}" for t in TOOLS if t != "realism"}
    held = {v.__name__ if isinstance(v, types.ModuleType) else getattr(v, "__module__", None) for v in vars(mod).values()}
    assert not held & others, held & others
    assert nearest_neighbors.checked_features is tool_support.checked_features is RL.checked_features
    assert nearest_neighbors.dataset_features is tool_support.dataset_features is RL.dataset_features
    assert tool_support.checked_features.__module__ == "style_big_gan_amd.tool_support"


def test_cli_run_on_the_cpu(tmp_path, capsys, monkeypatch):
    """the whole tool from a snapshot the trainer wrote, with a TorchScript vgg16.pt in a directory; the manifold is the unmirrored data set"""
    _, overrides, snap, data = _run(tmp_path)
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", _cpu_generator)
    monkeypatch.setenv("SBG_CACHE_DIR", str(tmp_path / "cache"))
    det = tmp_path / "det"
    os.makedirs(det)
    torch.jit.script(ScriptedDetector()).save(str(det / "vgg16.pt"))
    out = tmp_path / "out"
    capsys.readouterr()
    result = RL.run_realism(overrides + [f"--snapshot={snap}", f"--detector={det}", f"--outdir={out}", "--num=10", "--show=3", "--batch=4", "--device=cpu"])
    stats = json.load(open(out / "realism.json"))
    assert stats == result["stats"] and json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == stats
    assert (stats["manifold_points"], stats["kept_points"], stats["num"], stats["F"]) == (20, 10, 10, 192)      # the run's config says mirror: true
    npz = np.load(out / "realism.npz")
    assert npz["seeds"].tolist() == list(range(10)) and npz["real_score"].shape == (20,) and np.array_equal(npz["score"], result["arrays"]["score"])
    assert np.array(PIL.Image.open(out / "realism.png")).shape == (32, 48, 3)
    assert len(os.listdir(tmp_path / "cache" / "gan-metrics")) >= 1                # a detector file: the data set's features are cached
