"""The realism pass of the fused k-NN kernels (csrc/knn_manifold.hip, mode 4) on the device: bit-exact against the numpy oracle of
knn_realism_util on integer features (one candidate, ragged tiles, K tails, split + merge, several tiles per workgroup; plain, with half the
balls pruned, with exclusions), its launch records, invariants, realistic values inside the margin of one fp16 ulp of d, determinism, the
library's refusals, `scores.realism_scores` against the CPU path and the tool on both devices."""
import numpy as np
import pytest
import torch

import knn_manifold_util as ku
import knn_realism_util as ru
import nearest_util as N
from golden_util import make_image_folder
from test_nearest_neighbors_feature_cpu import detector
from test_prdc_gpu import REALISTIC
from style_big_gan_amd import realism as RL
from style_big_gan_amd.metrics import scores
from style_big_gan_amd.torch_utils.ops import knn_manifold
from style_big_gan_amd.train_parts.datasets import ImageFolderDataset

pytestmark = pytest.mark.gpu

# (R, C, F, k, offset): one candidate, fewer columns than a tile, two runs with a ragged last tile, a K tail, three ragged query tiles, the
# metric's width, 40 runs merged
EXACT = [(1, 1, 40, 0, 0), (37, 8, 40, 7, 0), (37, 130, 40, 3, 11), (37, 130, 72, 0, 64), (300, 260, 72, 7, 0), (300, 260, 4096, 3, 0),
         (300, 5000, 40, 7, 77)]
VARIANTS = {"plain": (False, False), "pruned": (True, False), "exclude": (False, True)}
MULTI_TILE = (37, 200000, 40, 3)
REALISM = 4                 # dims[6] of a realism launch record


def _dev(x, dev):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(dev)


def _run(dev, probes, manifold, radius, exclude=None):
    score, index = knn_manifold.realism(_dev(probes, dev), _dev(manifold, dev), _dev(radius, dev), _dev(exclude, dev))
    assert score.dtype == torch.float32 and index.dtype == torch.int32 and score.shape == index.shape == (len(probes),)
    return ku.to_np(score), ku.to_np(index)


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("R,C,F,k,offset", EXACT)
def test_exact_integer_features_match_the_oracle_bit_for_bit(dev, R, C, F, k, offset, variant):
    case = ku.exact_case(R, C, F, k, offset)
    want_score, want_index, radius, exclude = ru.exact_realism(R, C, F, k, offset, *VARIANTS[variant])
    with ku.pr_launches() as seen:
        score, index = _run(dev, case["probes"], case["manifold"], radius, exclude)
    print(f"inf {np.mean(np.isinf(want_score)):.2f}, score >= 1 {np.mean(want_score >= 1):.2f}, none {np.mean(want_index < 0):.2f}, "
          f"tied {ru.tied(case['probes'], case['manifold'], radius, exclude).mean():.2f}")
    assert np.array_equal(ru.f32_bits(score), ru.f32_bits(want_score))
    assert np.array_equal(index, want_index)
    # the launch records: norms of both operands, the tile kernel, and a merge when the columns are split
    assert [v for v, _ in seen] == (["norms", "norms", "single"] if C <= 128 else ["norms", "norms", "split", "merge"])
    for v, d in seen:
        if v != "norms":
            assert d[1:4] == (R, C, F) and d[6] == REALISM


def test_exact_integer_features_over_several_tiles_per_workgroup(dev):
    R, C, F, k = MULTI_TILE
    ctiles, runs, tiles_per_run = ku.plan(R, C)
    assert tiles_per_run >= 3 and runs * tiles_per_run >= ctiles > (runs - 1) * tiles_per_run
    case = ku.multi_tile_case(R, C, F, k)
    exclude = ru.exclude_for(R, C)
    for radius, ex in ((case["radius"], None), (ru.half_pruned(case["radius"]), exclude)):
        want_score, want_index = ru.realism(case["probes"], case["manifold"], radius, ex)
        with ku.pr_launches() as seen:
            score, index = _run(dev, case["probes"], case["manifold"], radius, ex)
        print(f"inf {np.mean(np.isinf(want_score)):.2f}, score >= 1 {np.mean(want_score >= 1):.2f}, winners in {len(np.unique(want_index // 128 // tiles_per_run))} runs")
        assert np.array_equal(ru.f32_bits(score), ru.f32_bits(want_score)) and np.array_equal(index, want_index)
        assert len(np.unique(want_index // 128 // tiles_per_run)) > 3 and (want_index // 128 % tiles_per_run != 0).any()
        tile_launches = [(v, d) for v, d in seen if v in ("single", "split")]
        assert [v for v, _ in tile_launches] == ["split"]
        for _, d in tile_launches:                               # the launch took the plan this test is about: several tiles per run
            assert d[1:4] == (R, C, F) and d[5] == runs and -(-ctiles // d[5]) >= 3 and d[6] == REALISM
        assert [d[6] for v, d in seen if v == "merge"] == [REALISM]


@pytest.mark.parametrize("R,C,F,k,offset", [EXACT[1], EXACT[4], EXACT[6]])
def test_invariants(dev, R, C, F, k, offset):
    case = ku.exact_case(R, C, F, k, offset)
    probes, manifold = case["probes"], case["manifold"]
    d = ku.distances(probes, manifold)[0].astype(np.float32)
    for radius in (case["radius_all"], ru.half_pruned(case["radius_all"])):
        score, index = _run(dev, probes, manifold, radius)
        inside = knn_manifold.in_manifold(_dev(probes, dev), _dev(manifold, dev), _dev(radius, dev))
        assert np.array_equal(score >= 1, ku.to_np(inside))
        assert (index >= 0).all() and (radius[index] >= 0).all()
        at = d[np.arange(R), index]
        with np.errstate(divide="ignore", invalid="ignore"):
            want = np.where(at == 0, np.float32(np.inf), radius[index].astype(np.float32) / at).astype(np.float32)
        assert np.array_equal(ru.f32_bits(score), ru.f32_bits(want))
    score, index = _run(dev, probes, manifold, np.full([C], -1, dtype=np.float16))
    assert not score.any() and (index == -1).all()


@pytest.mark.parametrize("n_real,n_gen,F,seed", REALISTIC)
def test_realistic_values(dev, n_real, n_gen, F, seed):
    case = ru.realistic_case(n_real, n_gen, F, seed)
    score, index = _run(dev, case["gen"], case["real"], case["radius"])
    rel, equal, ok = ru.within_margin(score, index, case["score"], case["index"], case["q"])
    print(f"scores {case['score'].min():.3f}..{case['score'].max():.3f}, >= 1 {np.mean(case['score'] >= 1):.3f}; device: max relative difference "
          f"{rel:.3e} (bound {ru.REL:.3e}), equal in bits {equal:.4f}, indices equal {np.mean(index == case['index']):.4f}")
    assert rel <= ru.REL
    assert equal >= 0.99
    assert ok.all()


def test_two_launches_give_the_same_bits(dev):
    # single; split + merge with one tile per run; split + merge with four tiles per run
    for R, C, F in [(37, 8, 40), (300, 5000, 40), (37, 200000, 40)]:
        real, gen = ku.realistic_features(C, R, F, seed=5)
        m, p = _dev(real, dev), _dev(gen, dev)
        radius = scores.pruned_radii(knn_manifold.kth_radius(m, m, min(3, C - 1)), 0.5)
        (s1, i1), (s2, i2) = (knn_manifold.realism(p, m, radius) for _ in range(2))
        assert torch.equal(s1.view(torch.int32), s2.view(torch.int32)) and torch.equal(i1, i2)
        assert bool((i1 >= 0).all()) and bool((radius[i1.long()] >= 0).all())


def test_library_refusals_carry_a_code_and_a_message(dev):
    """the entry point itself, below the op layer's own checks: SBG_ERR_INVALID (1) and a message in sbg_last_error()"""
    from style_big_gan_amd import _lib
    lib = _lib.load()
    x = torch.zeros([16, 40], dtype=torch.float16, device=dev)
    r = torch.ones([16], dtype=torch.float16, device=dev)
    score = torch.full([16], -7.0, dtype=torch.float32, device=dev)
    index = torch.full([16], -9, dtype=torch.int32, device=dev)
    ws = torch.zeros([4096], dtype=torch.float32, device=dev)
    stream = _lib.stream_ptr(dev)

    def call(P=16, F=40, probes=x.data_ptr(), manifold=x.data_ptr(), radius=r.data_ptr(), s=score.data_ptr(), i=index.data_ptr(), w=ws.data_ptr()):
        return lib.sbg_knn_realism(probes, manifold, radius, P, 16, F, None, s, i, w, stream)

    calls = [(lambda: call(probes=None), "null pointer"), (lambda: call(manifold=None), "null pointer"), (lambda: call(radius=None), "null pointer"),
             (lambda: call(s=None), "null pointer"), (lambda: call(i=None), "null pointer"), (lambda: call(w=None), "null pointer"),
             (lambda: call(F=36), "multiple of 8"), (lambda: call(P=15, probes=x.view(-1)[4:].data_ptr()), "16-byte aligned"),
             (lambda: call(P=0), "bad sizes"), (lambda: call(P=-3), "bad sizes")]
    for refused, message in calls:
        status = refused()
        assert status == 1 and message in lib.sbg_last_error().decode(), message
        with pytest.raises(RuntimeError, match=message):
            _lib.check(status, "sbg_knn_realism")
    torch.cuda.synchronize()
    assert bool((score == -7).all()) and bool((index == -9).all())               # a refused call launches nothing
    assert lib.sbg_knn_realism_workspace(300, 5000) == 1200 + 20000 + 8 * 300 * 40
    assert lib.sbg_knn_realism_workspace(300, 100) == 1200 + 400
    assert lib.sbg_knn_realism_workspace(0, 16) == -1
    with pytest.raises(RuntimeError, match="float16"):
        knn_manifold.realism(x.float(), x.float(), r.float())
    with pytest.raises(RuntimeError, match="float16"):
        knn_manifold.realism(x, x, r.float())
    with pytest.raises(RuntimeError, match="exclude must be int32"):
        knn_manifold.realism(x, x, r, torch.zeros([16], dtype=torch.int64, device=dev))
    with pytest.raises(RuntimeError, match="one excluded manifold index per probe"):
        knn_manifold.realism(x, x, r, torch.zeros([16], dtype=torch.int32))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        knn_manifold.realism(x[:, :36], x[:, :36], r)
    assert call() == 0                                           # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert bool(torch.isinf(score).all()) and bool((index == 0).all())           # sixteen zero rows: every probe is a copy of row 0


@pytest.mark.parametrize("n_real,n_gen,F,seed", [REALISTIC[0], REALISTIC[2]])
def test_realism_scores_against_the_cpu_path(dev, n_real, n_gen, F, seed):
    real, gen = ku.realistic_features(n_real, n_gen, F, seed)
    want = scores.realism_scores(torch.from_numpy(real), torch.from_numpy(gen), 3, 0.5, 128, leave_one_out=True)
    with ku.pr_launches() as seen:
        got = scores.realism_scores(_dev(real, dev), _dev(gen, dev), 3, 0.5, 128, leave_one_out=True)
    assert [d[6] for v, d in seen if v in ("single", "split")].count(REALISM) == -(-n_gen // 128) + -(-n_real // 128)
    want, got = [ku.to_np(t) for t in want], [ku.to_np(t) for t in got]
    kept = want[2]
    print(f"radii equal in bits {np.mean(ku.bits(got[2]) == ku.bits(kept)):.4f}, kept sets equal {np.array_equal(got[2] >= 0, kept >= 0)}")
    for name, probes, (s, i), (ws, wi), ex in (("generated", gen, got[0:2], want[0:2], None), ("real", real, got[3:5], want[3:5], np.arange(n_real))):
        rel, equal, ok = ru.within_margin(s, i, ws, wi, ru.ratios(probes, real, kept, ex))
        print(f"{name}: max relative difference {rel:.3e} (bound {ru.REL:.3e}), equal in bits {equal:.4f}, indices equal {np.mean(i == wi):.4f}")
        assert rel <= ru.REL and equal >= 0.99 and ok.all()
    assert (got[4] != np.arange(n_real)).all()


def test_the_tool_writes_the_same_files_on_both_devices(dev, tmp_path):
    kw = dict(path=make_image_folder(str(tmp_path / "data"), n=200, res=16), xflip=False)
    dataset = ImageFolderDataset(**kw)
    bank = N.make_bank(dataset, 40)
    seeds = list(range(48))
    run = lambda G, device, out: RL.realism_ranking(G, dataset, seeds, k=3, keep=0.5, show=6, batch=20, device=device, outdir=str(tmp_path / out),
                                                    detector=detector, dataset_kwargs=kw)
    want = run(N.BankGenerator(bank), torch.device("cpu"), "cpu")
    with ku.pr_launches() as seen:
        got = run(N.BankGenerator(bank).to(dev), dev, "cuda")
    assert [d[6] for v, d in seen if v in ("single", "split")].count(REALISM) == 1 + 3        # the baseline, then three batches of seeds
    assert got["stats"] == want["stats"] and got["shown"] == want["shown"]
    assert want["stats"]["generated"]["num_infinite"] > 0 and 0 < want["stats"]["generated"]["fraction_realistic"] < 1
    for name in ("realism.json", "realism.png"):
        assert (tmp_path / "cuda" / name).read_bytes() == (tmp_path / "cpu" / name).read_bytes(), name
    a, b = np.load(tmp_path / "cuda" / "realism.npz"), np.load(tmp_path / "cpu" / "realism.npz")
    assert sorted(a.files) == sorted(b.files) == ["item", "radius", "real_item", "real_score", "score", "seeds"]
    for name in a.files:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name].view(np.uint8), b[name].view(np.uint8)), name
