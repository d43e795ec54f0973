"""The MS-SSIM kernels (csrc/msssim.hip) on the device: the same bits as the op layer's CPU arithmetic (the value graph and the order of the
float64 sums are the definition), the full five levels against the independent restatement, the exact score of
identical images, the invariance under the cut of a batch, the launch records, and the tool on both devices.  The shapes (N, C, S) are the
smallest at which a map with fewer entries than lanes, a ragged map, an odd image-channel count and several 16 x 32 tiles both ways with
ragged last tiles can go wrong."""
import json

import numpy as np
import pytest
import torch

import msssim_util as MU
from exact_util import expect_launch
from style_big_gan_amd import diversity as DV
from style_big_gan_amd.torch_utils.ops import msssim
from test_calc_metrics_cpu import _run

pytestmark = pytest.mark.gpu

_cpu_results = {}


def _cpu(kind, shape):
    """the CPU path's results of a case, computed once"""
    if (kind, shape) not in _cpu_results:
        x, y = MU.random_pair(kind, *shape)
        _cpu_results[kind, shape] = (msssim.level_terms(x, y), msssim.down(x), *msssim.pair_scores(x, y))
    return _cpu_results[kind, shape]


@pytest.mark.parametrize("shape", MU.GPU_SHAPES)
@pytest.mark.parametrize("kind", ["float", "bytes"])
def test_device_equals_cpu_path_bit_for_bit(dev, kind, shape):
    x, y = MU.random_pair(kind, *shape, device=dev)
    assert x.dtype == (torch.uint8 if kind == "bytes" else torch.float32)
    want_terms, want_down, want_scores, want_pair_terms = _cpu(kind, shape)
    got = msssim.level_terms(x, y)
    assert got.device == x.device and got.dtype == torch.float64 and MU.same_bits(got, want_terms)
    down = msssim.down(x)
    assert down.device == x.device and down.dtype == torch.float32 and MU.same_bits(down, want_down)
    scores, terms = msssim.pair_scores(x, y)
    assert MU.same_bits(scores, want_scores) and MU.same_bits(terms, want_pair_terms)
    if kind == "bytes":                                     # bytes as uint8 and as fp32 are one input
        assert MU.same_bits(msssim.level_terms(x.float(), y.float()), want_terms) and MU.same_bits(msssim.down(x.float()), want_down)


def test_five_levels_against_the_restatement(dev):
    x, y = MU.correlated_pair(2, 3, 256, seed=4)
    ref_scores, ref_terms = MU.ref_pair_scores(x, y)
    assert float(ref_terms.min()) >= 0.1
    scores, terms = msssim.pair_scores(x.to(dev), y.to(dev))
    assert tuple(terms.shape) == (2, 3, 5)
    err_t = float((terms - ref_terms).abs().max())
    err_s = float(((scores - ref_scores) / ref_scores).abs().max())
    print(f"S=256: max term error {err_t:.3e} (bound {MU.TERM_ATOL:.0e}), max relative score error {err_s:.3e} (bound {MU.SCORE_RTOL:.0e})")
    assert err_t <= MU.TERM_ATOL and err_s <= MU.SCORE_RTOL
    got = msssim.level_terms(x.to(dev), y.to(dev))          # the 246 x 246 map: 8 x 16 tiles
    assert float((got.cpu() - MU.ref_level_terms(x, y)).abs().max()) <= MU.TERM_ATOL


@pytest.mark.parametrize("C,S", [(1, 16), (3, 64), (3, 256)])
def test_identical_images_score_exactly_one(dev, C, S):
    x = torch.from_numpy(MU.smooth_images(2, C, S, seed=3)).to(dev)
    noise, _ = MU.random_pair("float", 2, C, S, device=dev)
    for v in (x, noise):
        scores, terms = msssim.pair_scores(v, v.clone())
        assert scores.tolist() == [1.0, 1.0] and bool((terms == 1.0).all())
        assert bool((msssim.level_terms(v, v.clone()) == 1.0).all())


@pytest.mark.parametrize("shape", [(5, 3, 32), (3, 1, 64)])
def test_batch_invariance(dev, shape):
    x, y = MU.random_pair("float", *shape, device=dev)
    whole = msssim.level_terms(x, y)
    scores, terms = msssim.pair_scores(x, y)
    each_terms = torch.cat([msssim.level_terms(x[i:i + 1], y[i:i + 1]) for i in range(shape[0])])
    each = [msssim.pair_scores(x[i:i + 1], y[i:i + 1]) for i in range(shape[0])]
    assert MU.same_bits(whole, each_terms)
    assert MU.same_bits(scores, torch.cat([e[0] for e in each])) and MU.same_bits(terms, torch.cat([e[1] for e in each]))
    order = torch.arange(shape[0] - 1, -1, -1, device=dev)
    assert MU.same_bits(whole[order], msssim.level_terms(x[order].contiguous(), y[order].contiguous()))


def test_launch_records(dev):
    """a level call is one level and one merge record, dims (variant, BC, S); a pair_scores call walks the sides"""
    x, y = MU.random_pair("bytes", 2, 3, 64, device=dev)
    with expect_launch("msssim", lambda d: d[:3] == (0, 6, 64), "the level kernel") as log:
        with expect_launch("msssim", lambda d: d[:3] == (2, 6, 64), "the merge of its partials"):
            msssim.level_terms(x, y)
    assert [r["dims"][:3] for r in log if r["kind"] == "msssim"] == [(0, 6, 64), (2, 6, 64)]
    with expect_launch("msssim", lambda d: d[:3] == (1, 6, 64), "down") as log:
        msssim.down(x)
    assert [r["dims"][:3] for r in log if r["kind"] == "msssim"] == [(1, 6, 64)]
    with expect_launch("msssim", lambda d: d[:3] == (0, 6, 16), "the coarsest level") as log:
        msssim.pair_scores(x, y)
    assert [r["dims"][:3] for r in log if r["kind"] == "msssim"] == [(0, 6, 64), (2, 6, 64), (1, 6, 64), (1, 6, 64), (0, 6, 32), (2, 6, 32), (1, 6, 32),
                                                                    (1, 6, 32), (0, 6, 16), (2, 6, 16)]


def test_refusals_on_the_device(dev):
    z = lambda *shape: torch.zeros(shape, device=dev)
    with pytest.raises(ValueError, match="S=48"):
        msssim.level_terms(z(1, 3, 48, 48), z(1, 3, 48, 48))
    with pytest.raises(ValueError, match="on cpu"):
        msssim.level_terms(z(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    assert tuple(msssim.level_terms(z(0, 3, 16, 16), z(0, 3, 16, 16)).shape) == (0, 3, 2)


def test_tool_from_a_snapshot_of_this_build(dev, tmp_path):
    """the real generator of a 16 x 16 run: the three files, and the scores of the bytes of the seeds 2p and 2p + 1"""
    import os
    from style_big_gan_amd import arguments, tool_support as TS
    _, overrides, snap, data = _run(tmp_path)
    out = tmp_path / "out"
    DV.run_diversity(overrides + ["--device=cuda", "--pairs=5", "--batch=3", "--closest=2", f"--snapshot={snap}", f"--data={data}", f"--outdir={out}"])
    assert sorted(os.listdir(out)) == ["closest_pairs.png", "diversity.json", "diversity_pairs.npz"]
    npz = np.load(out / "diversity_pairs.npz")
    G = TS.load_generator(arguments.load_config(overrides), snap, dev, announce=False)
    label = TS.class_label(G, None, dev)
    img = torch.cat([TS.generated_images(G, seeds, label, 1, "const", dev) for seeds in (list(range(0, 6)), list(range(6, 10)))])
    scores, terms = msssim.pair_scores(img[0::2].contiguous(), img[1::2].contiguous())
    assert np.array_equal(npz["gen_scores"], scores.numpy()) and np.array_equal(npz["gen_terms"], terms.numpy()) and tuple(terms.shape) == (5, 3, 1)
    assert npz["real_scores"].shape == (5,) and (npz["real_scores"] <= 1 + 1e-12).all() and (npz["gen_scores"] >= 0).all()
    stats = json.load(open(out / "diversity.json"))
    assert stats["image_size"] == 16 and stats["gen"]["num_pairs"] == stats["real"]["num_pairs"] == 5 and 0 <= stats["fraction_above_real_p99"] <= 1


def test_tool_on_the_device_equals_the_cpu_run(dev, tmp_path, monkeypatch):
    _, overrides, snap, _ = _run(tmp_path)
    bank = MU.smooth_images(24, 3, 32, seed=5)
    bank[3] = bank[2]
    reals = MU.smooth_images(13, 3, 32, seed=9)
    labels = [0, 1, 2, 0, 1, 2, 0, 1, 2, 0, 1, 0, 1]
    data = MU.tool_dataset(tmp_path, reals, labels)
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", lambda config, state, device: MU.ClassGenerator(bank, c_dim=3, shift=5).to(device))
    for device in ("cuda", "cpu"):
        DV.run_diversity(overrides + [f"--device={device}", "--batch=4", "--pairs=6", f"--snapshot={snap}", f"--data={data}", "--closest=3",
                                      f"--outdir={tmp_path / device}"])
    a, b = np.load(tmp_path / "cuda" / "diversity_pairs.npz"), np.load(tmp_path / "cpu" / "diversity_pairs.npz")
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 8
    for name in a.files:
        assert a[name].dtype == b[name].dtype and np.array_equal(a[name], b[name]), name
    assert json.load(open(tmp_path / "cuda" / "diversity.json"))["gen"]["num_pairs"] == 6
    assert open(tmp_path / "cuda" / "diversity.json").read() == open(tmp_path / "cpu" / "diversity.json").read()
    assert open(tmp_path / "cuda" / "closest_pairs.png", "rb").read() == open(tmp_path / "cpu" / "closest_pairs.png", "rb").read()
