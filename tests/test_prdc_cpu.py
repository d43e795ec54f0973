"""Density / coverage next to precision / recall (Naeem et al., ICML 2020) on the CPU: the probe op's torch path against the numpy oracle,
`prdc_fused` on hand-checkable sets and against a brute-force evaluation, two gloo ranks, and the `prdc50k5_full` registry entry end to end."""
import json
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import knn_manifold_util as ku
import knn_probe_util as pu
from golden_util import make_image_folder
from style_big_gan_amd import calc_metrics
from style_big_gan_amd.metrics import metric_main, scores
from style_big_gan_amd.torch_utils.ops import knn_manifold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"prdc50k5_full_precision", "prdc50k5_full_recall", "prdc50k5_full_density", "prdc50k5_full_coverage"}
FEATURES = (300, 260, 72, 0)        # ku.realistic_features arguments of the metric tests


@pytest.mark.parametrize("R,C,F,k,offset", [(37, 130, 40, 3, 11), (300, 260, 72, 7, 0)])
def test_probe_matches_the_oracle(R, C, F, k, offset):
    case = ku.exact_case(R, C, F, k, offset)
    probes, manifold, radius = (torch.from_numpy(case[key].copy()) for key in ("probes", "manifold", "radius_all"))
    want_count, want_nearest = pu.exact_probe(R, C, F, k, offset)
    count, nearest = knn_manifold.probe(probes, manifold, radius)
    assert count.dtype == torch.int32 and nearest.dtype == torch.float16 and count.shape == nearest.shape == (R,)
    assert np.array_equal(count.numpy(), want_count)
    assert np.array_equal(ku.bits(nearest.numpy()), ku.bits(want_nearest))
    assert torch.equal(count > 0, knn_manifold.in_manifold(probes, manifold, radius))
    assert torch.equal(nearest.view(torch.int16), knn_manifold.kth_radius(probes, manifold, 0).view(torch.int16))
    assert len(np.unique(want_count)) >= 4 and (want_count == 0).any()         # a flag instead of a count cannot pass
    empty = knn_manifold.probe(probes[:0], manifold, radius)
    assert empty[0].shape == empty[1].shape == (0,) and empty[0].dtype == torch.int32 and empty[1].dtype == torch.float16
    with pytest.raises(RuntimeError, match="one radius per manifold point"):
        knn_manifold.probe(probes, manifold, radius[:-1])


def test_prdc_on_hand_checkable_sets():
    k = 5
    real = torch.from_numpy(ku.realistic_features(*FEATURES)[0])
    precision, recall, density, coverage = scores.prdc_fused(real, real.clone(), k, 64)
    # every ball holds its centre and its k neighbours, so the counts sum to at least k + 1 per ball
    assert precision == recall == coverage == 1.0 and density >= (k + 1) / k
    assert scores.prdc_fused(real, real + 1000, k, 64) == (0.0, 0.0, 0.0, 0.0)


def test_prdc_against_brute_force_and_precision_recall_fused():
    k = 5
    real, gen = ku.realistic_features(*FEATURES)
    want = pu.prdc(real, gen, k)
    got = scores.prdc_fused(torch.from_numpy(real), torch.from_numpy(gen), k, 64)
    print(f"prdc {got} oracle {want}")
    assert all(isinstance(v, float) for v in got) and got == want
    assert got[:2] == scores.precision_recall_fused(torch.from_numpy(real), torch.from_numpy(gen), k, 64)
    assert 0 < got[0] < 1 and 0 < got[1] < 1 and got[2] > 0 and 0 < got[3] < 1       # the features decide something
    assert got == scores.prdc_fused(torch.from_numpy(real), torch.from_numpy(gen), k, 10000)       # the row batches do not matter


def _prdc_worker(rank, world, init_file, results):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import style_big_gan_amd  # noqa: F401
    from style_big_gan_amd.metrics import scores as sc
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        real, gen = (torch.from_numpy(x) for x in ku.realistic_features(*FEATURES))
        results[rank] = (sc.prdc_fused(real, gen, 5, 64, num_gpus=world, rank=rank), sc.prdc_fused(real[:299], gen[:255], 5, 64, num_gpus=world, rank=rank))
    finally:
        dist.destroy_process_group()


def test_prdc_fused_world2_gloo():
    """two ranks share the radius rows and the probe rows (all of them, then 299 and 255: neither divides by 2); every rank returns the
    one-rank numbers"""
    real, gen = (torch.from_numpy(x) for x in ku.realistic_features(*FEATURES))
    solo = (scores.prdc_fused(real, gen, 5, 64), scores.prdc_fused(real[:299], gen[:255], 5, 64))
    world = 2
    with tempfile.TemporaryDirectory() as d:
        mgr = mp.Manager()
        results = mgr.dict()
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_prdc_worker, args=(r, world, os.path.join(d, "rdzv"), results)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=180)
        for p in procs:
            assert p.exitcode == 0, f"worker exit code {p.exitcode}"
        assert dict(results) == {0: solo, 1: solo}


class _Projection:
    """callable stand-in detector: uint8 images -> 24 features"""
    __name__ = "projection24"

    def __init__(self):
        self.w = torch.randn(48, 24, generator=torch.Generator().manual_seed(5))

    def __call__(self, images):
        x = torch.nn.functional.adaptive_avg_pool2d(images.float() / 255.0, 4).flatten(1)
        return x @ self.w.to(x.device)


def _toy_generator():
    from style_big_gan_amd.train_parts.generators import generators
    torch.manual_seed(9)
    G = generators["cnn32_dcgan"](z_dim=8, c_dim=0, img_resolution=32).eval()
    G.c_dim = 0
    return G


def test_registry_and_cli_parse(tmp_path):
    assert metric_main.is_valid_metric("prdc50k5_full") and "prdc50k5_full" in metric_main.list_valid_metrics()
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    _, args = calc_metrics.parse_args([f"--snapshot={snap}", f"--detector={tmp_path}", "--metrics=fid50k_full,prdc50k5_full"])
    assert args.metrics == ["fid50k_full", "prdc50k5_full"]


def test_calc_metrics_on_the_cpu_writes_the_four_numbers(tmp_path, capsys, monkeypatch):
    path = make_image_folder(str(tmp_path / "data"), n=24, res=32)
    seen = dict()
    prdc = scores.compute_prdc

    def small(opts, max_real, num_gen, nhood_size, row_batch_size, **kw):      # the registry's arguments, then 32 generated images instead of 50 000
        seen.update(max_real=max_real, num_gen=num_gen, nhood_size=nhood_size, row_batch_size=row_batch_size, xflip=opts.dataset_kwargs.get("xflip"))
        return prdc(opts, max_real=max_real, num_gen=32, nhood_size=nhood_size, row_batch_size=16, **kw)

    monkeypatch.setattr(scores, "compute_prdc", small)
    run_dir = tmp_path / "run"
    run_dir.mkdir()
    capsys.readouterr()
    out = calc_metrics.calc_metrics(_toy_generator(), ["prdc50k5_full"], dict(path=path, use_labels=False, xflip=True), _Projection(), device="cpu",
                                    run_dir=str(run_dir), snapshot=str(run_dir / "network-snapshot-000000.pt"))
    assert seen == dict(max_real=200000, num_gen=50000, nhood_size=5, row_batch_size=10000, xflip=False)
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert json.loads(open(run_dir / "metric-prdc50k5_full.jsonl").read()) == line
    results = line["results"]
    assert line["metric"] == "prdc50k5_full" and set(results) == KEYS and results == dict(out["prdc50k5_full"].results)
    assert all(0.0 <= results[f"prdc50k5_full_{name}"] <= 1.0 for name in ("precision", "recall", "coverage"))
    assert results["prdc50k5_full_density"] >= 0.0 and np.isfinite(results["prdc50k5_full_density"])
