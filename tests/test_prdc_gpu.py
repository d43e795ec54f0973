"""The probe pass of the fused k-NN kernels (csrc/knn_manifold.hip, mode 2) and the density / coverage metric on the device: bit-exact
against the numpy oracle on integer features (one tile, ragged tiles, K tails, split + merge, several tiles per workgroup), every ball
holding every probe, refusals, realistic values inside the deciding margin, determinism, and the metric end to end."""
import json
import os

import numpy as np
import pytest
import torch

import knn_manifold_util as ku
import knn_probe_util as pu
from golden_util import make_image_folder
from test_calc_metrics_cpu import _detectors, _run
from style_big_gan_amd import calc_metrics
from style_big_gan_amd.metrics import metric_utils, scores
from style_big_gan_amd.torch_utils.ops import knn_manifold

pytestmark = pytest.mark.gpu

# (R, C, F, k, offset): one tile, ragged tiles, K tails of the 64-deep step, the metric's width, 40 column runs merged
EXACT = [(1, 1, 40, 0, 0), (37, 8, 40, 7, 0), (37, 130, 40, 3, 11), (37, 130, 72, 0, 64), (300, 260, 72, 7, 0), (300, 260, 4096, 3, 0),
         (37, 5000, 40, 3, 4100), (300, 5000, 40, 7, 77)]
MULTI_TILE = [(37, 200000, 40, 3), (2100, 13000, 40, 7), (33000, 300, 40, 3)]
REALISTIC = [(300, 260, 72, 0), (200, 136, 72, 1), (300, 260, 4096, 2), (200, 136, 4096, 3)]
PROBE = 2                   # dims[6] of a probe launch record


def _dev(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x)).to(dev)


@pytest.mark.parametrize("R,C,F,k,offset", EXACT)
def test_exact_integer_features_match_the_oracle_bit_for_bit(dev, R, C, F, k, offset):
    case = ku.exact_case(R, C, F, k, offset)
    want_count, want_nearest = pu.exact_probe(R, C, F, k, offset)
    probes, manifold, radius = (_dev(case[key], dev) for key in ("probes", "manifold", "radius_all"))
    with ku.pr_launches() as seen:
        count, nearest = knn_manifold.probe(probes, manifold, radius)
    assert count.dtype == torch.int32 and nearest.dtype == torch.float16 and count.shape == nearest.shape == (R,)
    print(f"count {want_count.min()}..{want_count.max()}, {len(np.unique(want_count))} values, zeros {np.mean(want_count == 0):.2f}")
    assert np.array_equal(ku.to_np(count), want_count)
    assert np.array_equal(ku.bits(ku.to_np(nearest)), ku.bits(want_nearest))
    assert torch.equal(count > 0, knn_manifold.in_manifold(probes, manifold, radius))
    assert torch.equal(nearest.view(torch.int16), knn_manifold.kth_radius(probes, manifold, 0).view(torch.int16))
    assert [v for v, _ in seen] == (["norms", "norms", "single"] if C <= 128 else ["norms", "norms", "split", "merge"])
    for v, d in seen:
        if v != "norms":
            assert d[1:4] == (R, C, F) and d[6] == PROBE


# radius 65504 everywhere: every ball holds every probe.  Padded columns of a ragged tile counted, partial counts narrower than 32 bits
# (C = 200 000) or a merge that skips a run would all show.
@pytest.mark.parametrize("case", [("exact", 37, 130, 40, 3, 11), ("exact", 300, 260, 72, 7, 0), ("exact", 300, 5000, 40, 7, 77), ("multi", 37, 200000, 40, 3)])
def test_every_ball_holds_every_probe(dev, case):
    data = ku.exact_case(*case[1:]) if case[0] == "exact" else ku.multi_tile_case(*case[1:])
    C = case[2]
    count, _ = knn_manifold.probe(_dev(data["probes"], dev), _dev(data["manifold"], dev), torch.full([C], 65504.0, dtype=torch.float16, device=dev))
    assert torch.equal(count, torch.full_like(count, C))


@pytest.mark.parametrize("R,C,F,k", MULTI_TILE)
def test_exact_integer_features_over_several_tiles_per_workgroup(dev, R, C, F, k):
    ctiles, runs, tiles_per_run = ku.plan(R, C)
    assert tiles_per_run >= 3 and runs * tiles_per_run >= ctiles > (runs - 1) * tiles_per_run
    case = ku.multi_tile_case(R, C, F, k)
    want_count, want_nearest = pu.multi_tile_probe(R, C, F, k)
    with ku.pr_launches() as seen:
        count, nearest = knn_manifold.probe(_dev(case["probes"], dev), _dev(case["manifold"], dev), _dev(case["radius"], dev))
    print(f"count {want_count.min()}..{want_count.max()}, zeros {np.mean(want_count == 0):.2f}")
    assert np.array_equal(ku.to_np(count), want_count)
    assert np.array_equal(ku.bits(ku.to_np(nearest)), ku.bits(want_nearest))
    assert want_count.max() >= 4 and 0.1 < np.mean(want_count == 0) < 0.9
    tile_launches = [(v, d) for v, d in seen if v in ("single", "split")]
    assert [v for v, _ in tile_launches] == (["single"] if runs == 1 else ["split"])
    for _, d in tile_launches:                                   # the launch took the plan this test is about: several tiles per run
        assert d[1:4] == (R, C, F) and d[5] == runs and -(-ctiles // d[5]) >= 3 and d[6] == PROBE
    assert [d[6] for v, d in seen if v == "merge"] == ([] if runs == 1 else [PROBE])


def test_library_refusals_carry_a_code_and_a_message(dev):
    """the entry point itself, below the op layer's own checks: SBG_ERR_INVALID (1) and a message in sbg_last_error()"""
    from style_big_gan_amd import _lib
    lib = _lib.load()
    x = torch.zeros([16, 40], dtype=torch.float16, device=dev)
    r = torch.ones([16], dtype=torch.float16, device=dev)
    count = torch.full([16], -7, dtype=torch.int32, device=dev)
    nearest = torch.full([16], 3.0, dtype=torch.float16, device=dev)
    ws = torch.zeros([4096], dtype=torch.float32, device=dev)
    stream = _lib.stream_ptr(dev)

    def probe(P=16, F=40, probes=x, radius=r.data_ptr(), c=count.data_ptr(), n=nearest.data_ptr()):
        return lib.sbg_knn_probe(probes.data_ptr(), x.data_ptr(), radius, P, 16, F, c, n, ws.data_ptr(), stream)

    calls = [(lambda: probe(c=None), "null pointer"), (lambda: probe(n=None), "null pointer"), (lambda: probe(radius=None), "null pointer"),
             (lambda: probe(F=36), "multiple of 8"), (lambda: probe(P=15, probes=x.view(-1)[4:]), "16-byte aligned"), (lambda: probe(P=0), "bad sizes")]
    for call, message in calls:
        status = call()
        assert status == 1 and message in lib.sbg_last_error().decode(), message
        with pytest.raises(RuntimeError, match=message):
            _lib.check(status, "sbg_knn_probe")
    torch.cuda.synchronize()
    assert bool((count == -7).all()) and bool((nearest == 3.0).all())            # a refused call launches nothing
    # the workspace: P + C floats of norms (each rounded up to 16 bytes), then one {int32, float} pair per (run, row) when the columns are split
    assert lib.sbg_knn_probe_workspace(300, 5000) == 1200 + 20000 + 8 * 300 * 40
    assert lib.sbg_knn_probe_workspace(300, 100) == 1200 + 400
    assert lib.sbg_knn_probe_workspace(0, 16) == -1
    with pytest.raises(RuntimeError, match="float16"):
        knn_manifold.probe(x.float(), x.float(), r.float())
    with pytest.raises(RuntimeError, match="float16"):
        knn_manifold.probe(x, x, r.float())
    assert probe() == 0                                          # the same call with nothing wrong runs


@pytest.mark.parametrize("n_real,n_gen,F,seed", REALISTIC)
def test_realistic_values(dev, n_real, n_gen, F, seed):
    real, gen = ku.realistic_features(n_real, n_gen, F, seed)
    k = 5
    radius = {id(real): ku.kth_radius(real, real, k), id(gen): ku.kth_radius(gen, gen, k)}
    near_total = pairs = 0
    for manifold, probes in [(real, gen), (gen, real)]:
        want_count, want_nearest = pu.probe(probes, manifold, radius[id(manifold)])
        count, nearest = knn_manifold.probe(_dev(probes, dev), _dev(manifold, dev), _dev(radius[id(manifold)], dev))
        near = pu.near_pairs(probes, manifold, radius[id(manifold)]).sum(axis=1)
        off = np.abs(ku.to_np(count).astype(np.int64) - want_count)
        ulps = np.abs(ku.bits(ku.to_np(nearest)).astype(np.int64) - ku.bits(want_nearest).astype(np.int64))
        print(f"count: differs on {int((off > 0).sum())} probes, near pairs {int(near.sum())} of {near.size * len(manifold)}; "
              f"nearest: max ulp {ulps.max()}, equal {np.mean(ulps == 0):.4f}")
        assert (off <= near).all()
        assert ulps.max() <= 1 and np.mean(ulps == 0) >= 0.99
        near_total += int(near.sum())
        pairs += len(probes) * len(manifold)
    undecided = pu.undecided_cover(real, gen, radius[id(real)])
    print(f"near pairs {near_total / pairs:.5f}, coverage-undecided reals {undecided.mean():.4f}")
    assert near_total <= 0.005 * pairs and undecided.mean() <= 0.05         # the conditions: the margins excuse little


def test_two_launches_give_the_same_bits(dev):
    # single; split + merge with one tile per run; split + merge with four tiles per run
    for R, C, F in [(37, 8, 40), (300, 5000, 40), (37, 200000, 40)]:
        real, gen = ku.realistic_features(C, R, F, seed=5)
        m, p = _dev(real, dev), _dev(gen, dev)
        radius = knn_manifold.kth_radius(m, m, min(5, C - 1))
        (c1, n1), (c2, n2) = (knn_manifold.probe(p, m, radius) for _ in range(2))
        assert torch.equal(c1, c2) and torch.equal(n1.view(torch.int16), n2.view(torch.int16))


@pytest.mark.parametrize("n_real,n_gen,F,seed", [REALISTIC[0], REALISTIC[2]])
def test_prdc_fused_against_the_cpu_path(dev, n_real, n_gen, F, seed):
    real, gen = ku.realistic_features(n_real, n_gen, F, seed)
    k = 5
    want = scores.prdc_fused(torch.from_numpy(real), torch.from_numpy(gen), k, 128)
    with ku.pr_launches() as seen:
        got = scores.prdc_fused(_dev(real, dev), _dev(gen, dev), k, 128)
    assert [d[6] for v, d in seen if v in ("single", "split")].count(PROBE) == 3 + 3        # 260 and 300 probe rows in batches of 128
    # the two differ only where fp32 summation order decides a comparison: inside the margin of knn_probe_util.NEAR
    r_real, r_gen = ku.kth_radius(real, real, k), ku.kth_radius(gen, gen, k)
    near_a, near_b = pu.near_pairs(gen, real, r_real), pu.near_pairs(real, gen, r_gen)
    undecided = pu.undecided_cover(real, gen, r_real)
    bounds = [near_a.any(axis=1).sum() / n_gen + 1e-7, near_b.any(axis=1).sum() / n_real + 1e-7,       # 1e-7: the fp32 quotients' own rounding
              near_a.sum() / (k * n_gen) + 1e-12, undecided.sum() / n_real + 1e-12]
    print(f"device {got} cpu {want} bounds {[float(b) for b in bounds]}")
    for value, ref, bound in zip(got, want, bounds):
        assert abs(value - ref) <= bound


class _Projection:
    """callable stand-in detector: uint8 images -> 24 features"""
    __name__ = "projection24"

    def __init__(self):
        self.w = torch.randn(48, 24, generator=torch.Generator().manual_seed(5))

    def __call__(self, images):
        x = torch.nn.functional.adaptive_avg_pool2d(images.float() / 255.0, 4).flatten(1)
        return x @ self.w.to(x.device)


def test_compute_prdc_runs_the_kernels(dev, tmp_path):
    from style_big_gan_amd.train_parts.generators import generators
    path = make_image_folder(str(tmp_path / "data"), n=24, res=32)
    torch.manual_seed(9)
    G = generators["cnn32_dcgan"](z_dim=8, c_dim=0, img_resolution=32).eval().to(dev)
    G.c_dim = 0
    opts = metric_utils.MetricOptions(G=G, dataset_kwargs=dict(path=path, use_labels=False), num_gpus=1, rank=0, device=dev, detector=_Projection(),
                                      cache=False)
    with ku.pr_launches() as seen:
        precision, recall, density, coverage = scores.compute_prdc(opts, max_real=None, num_gen=32, nhood_size=5, row_batch_size=16)
    assert 0.0 <= precision <= 1.0 and 0.0 <= recall <= 1.0 and 0.0 <= coverage <= 1.0 and 0.0 <= density < float("inf")
    # 24 reals and 32 generated images in row batches of 16: 2 + 2 radius launches, then 2 + 2 probe launches, each on one tile
    assert [d[6] for v, d in seen if v == "single"] == [0, 0, 0, 0, PROBE, PROBE, PROBE, PROBE]


def test_cli_run_on_the_device(dev, tmp_path, capsys, monkeypatch):
    _, overrides, snap, _ = _run(tmp_path, n_images=24)
    det = _detectors(str(tmp_path / "det"))
    prdc = scores.compute_prdc
    monkeypatch.setattr(scores, "compute_prdc", lambda opts, max_real, num_gen, nhood_size, row_batch_size, **kw:
                        prdc(opts, max_real=max_real, num_gen=32, nhood_size=nhood_size, row_batch_size=16, **kw))
    with open(os.path.join(os.path.dirname(snap), "training_options.json"), "w") as f:       # a run directory: the jsonl is appended there
        json.dump({}, f)
    argv = overrides + [f"--snapshot={snap}", f"--detector={det}", "--metrics=prdc50k5_full", "--device=cuda", "--verbose=0"]
    capsys.readouterr()
    with ku.pr_launches() as seen:
        results = calc_metrics.run_calc_metrics(argv)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert json.loads(open(os.path.join(os.path.dirname(snap), "metric-prdc50k5_full.jsonl")).read()) == line
    assert line["metric"] == "prdc50k5_full" and line["results"] == dict(results["prdc50k5_full"].results)
    assert set(line["results"]) == {f"prdc50k5_full_{name}" for name in ("precision", "recall", "density", "coverage")}
    assert all(0 <= line["results"][f"prdc50k5_full_{name}"] <= 1 for name in ("precision", "recall", "coverage"))
    assert np.isfinite(line["results"]["prdc50k5_full_density"]) and line["results"]["prdc50k5_full_density"] >= 0
    assert [d[6] for v, d in seen if v == "single"].count(PROBE) == 4 and not [v for v, _ in seen if v in ("split", "merge")]
