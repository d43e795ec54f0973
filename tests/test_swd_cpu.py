"""The sliced Wasserstein distance metric (swd16k) on the CPU: the op layer's CPU arithmetic against the independent restatement
(tests/swd_util.py) under a derived bound, the registered metric, its invariances and refusals, and the detector-free plumbing of the
trainer and of calc_metrics."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import swd_util as U
from swd_cases import TinyG, byte_sets, derived_bound, level_descriptors, small_tables
from golden_util import make_image_folder
from style_big_gan_amd import calc_metrics
from style_big_gan_amd.metrics import metric_main, metric_utils, scores

def test_cpu_path_matches_the_restatement_under_the_derived_bound():
    real, fake = byte_sets()
    tables = small_tables(3, 24, 32, 3, 8, 32)
    ref, ref_desc = U.score(real, fake, tables["centres"], tables["dirs"], 2, 16)
    dr, df = level_descriptors(real, tables), level_descriptors(fake, tables)
    for i, res in enumerate((32, 16)):
        got = scores.sliced_wasserstein(dr[i], df[i], tables["dirs"], 2, 16, what=f"level {res}")
        bound = derived_bound([ref_desc[res]], 147)
        print(f"level {res}: score {got!r}, restatement {ref[res]!r}, |difference| {abs(got - ref[res]):.3e}, bound {bound:.3e}")
        assert ref[res] > 1.0 and bound < 1e-2 * ref[res]        # the bound is far below the number it guards
        assert abs(got - ref[res]) <= bound


def test_identical_sets_score_exactly_zero():
    real, _ = byte_sets(1, n=6)
    tables = small_tables(0, 6, 32, 3, 8, 32)
    d = level_descriptors(real, tables)
    for i in range(2):
        assert scores.sliced_wasserstein(d[i], d[i].clone(), tables["dirs"], 2, 16) == 0.0


def test_descriptors_do_not_depend_on_the_batch_size_or_the_rank_shares():
    real, fake = byte_sets(2, n=7)
    tables = small_tables(5, 7, 32, 3, 8, 32)
    one = level_descriptors(real, tables, batch=7)
    for batch in (1, 3):
        assert all(torch.equal(a, b) for a, b in zip(one, level_descriptors(real, tables, batch=batch)))
    # two ranks fill the rows of their image shares into zeros and add: the one-rank matrices
    parts = []
    for rank in range(2):
        lo, hi = scores._rank_share(7, 2, rank)
        acc = scores.SwdDescriptors(7, 32, 3, tables["centres"], "cpu")
        acc.add(lo, torch.from_numpy(real[lo:hi]))
        parts.append(acc.desc)
    assert all(torch.equal(a, p0 + p1) for a, p0, p1 in zip(one, *parts))
    # two ranks take contiguous shares of the directions; rank 0 adds the distances in direction order
    df = level_descriptors(fake, tables)
    solo = scores.sliced_wasserstein(one[0], df[0], tables["dirs"], 2, 16)
    shares = [scores.swd_direction_distances(one[0], df[0], tables["dirs"], *scores._rank_share(32, 2, rank), dir_chunk=5) for rank in range(2)]
    assert [len(s) for s in shares] == [16, 16]
    assert scores.swd_score(torch.cat(shares), one[0].shape[0], 2, 16) == solo and solo > 0


ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _world2_worker(rank, world, init_file, results):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import style_big_gan_amd  # noqa: F401
    from style_big_gan_amd.metrics import scores as sc
    from swd_cases import byte_sets as sets, small_tables as tables_of
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        real, fake = sets(2, n=7)
        tables = tables_of(5, 7, 32, 3, 8, 33)
        lo, hi = sc._rank_share(7, world, rank)
        desc = []
        for images in (real, fake):
            acc = sc.SwdDescriptors(7, 32, 3, tables["centres"], "cpu")
            acc.add(lo, torch.from_numpy(images[lo:hi]))
            desc.append(acc.exchange(world))
        results[rank] = [sc.sliced_wasserstein(desc[0][i], desc[1][i], tables["dirs"], 3, 11, num_gpus=world, rank=rank) for i in range(2)]
    finally:
        dist.destroy_process_group()


def test_two_gloo_ranks_return_the_one_rank_scores():
    """7 images and 33 directions (neither divides by 2): the ranks fill their image shares, exchange the rows, take contiguous direction
    shares and gather the distances; every rank returns the one-rank numbers"""
    real, fake = byte_sets(2, n=7)
    tables = small_tables(5, 7, 32, 3, 8, 33)
    dr, df = level_descriptors(real, tables), level_descriptors(fake, tables)
    solo = [scores.sliced_wasserstein(dr[i], df[i], tables["dirs"], 3, 11) for i in range(2)]
    world = 2
    with tempfile.TemporaryDirectory() as d:
        mgr = mp.Manager()
        results = mgr.dict()
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_world2_worker, args=(r, world, os.path.join(d, "rdzv"), results)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=180)
        for p in procs:
            assert p.exitcode == 0, f"worker exit code {p.exitcode}"
        assert dict(results) == {0: solo, 1: solo} and all(v > 0 for v in solo)


def test_constant_channel_and_odd_resolutions_are_refused(tmp_path):
    real, fake = byte_sets(4, n=4)
    fake[:, 1] = 77
    tables = small_tables(0, 4, 32, 3, 8, 32)
    dr, df = level_descriptors(real, tables), level_descriptors(fake, tables)
    with pytest.raises(ValueError, match=r"generated set, level 32.*channel 1"):
        scores.sliced_wasserstein(dr[0], df[0], tables["dirs"], 2, 16, what="level 32")
    for bad in (48, 8, 0):
        with pytest.raises(ValueError, match=str(bad)):
            scores.swd_resolutions(bad)
    assert scores.swd_resolutions(16) == [16] and scores.swd_resolutions(128) == [128, 64, 32, 16]
    data = make_image_folder(str(tmp_path / "d48"), n=4, res=48)
    with pytest.raises(ValueError, match="resolution 48"):
        metric_main.calc_metric("swd16k", G=TinyG(48), dataset_kwargs=dict(path=data), device=torch.device("cpu"), cache=False)


def test_swd16k_is_registered_and_independent_of_the_batch_size(tmp_path):
    assert metric_main.is_valid_metric("swd16k") and not metric_main.needs_detector("swd16k")
    assert all(metric_main.needs_detector(m) for m in metric_main.list_valid_metrics() if not m.startswith("swd"))
    data = make_image_folder(str(tmp_path / "two"), n=2, res=32)
    kw = dict(G=TinyG(32), dataset_kwargs=dict(path=data, xflip=True), device=torch.device("cpu"), cache=False)
    result = metric_main.calc_metric("swd16k", **kw)
    r = result.results
    assert set(r) == {"swd16k_32", "swd16k_16", "swd16k_avg"}
    assert all(np.isfinite(v) and v > 0 for v in r.values()) and r["swd16k_avg"] == (r["swd16k_32"] + r["swd16k_16"]) / 2
    # the same numbers from other batch sizes, and nothing but the seed decides them
    data = make_image_folder(str(tmp_path / "five"), n=5, res=32)
    o = metric_utils.MetricOptions(G=TinyG(32), dataset_kwargs=dict(path=data, xflip=False, max_size=None), device=torch.device("cpu"), cache=False)
    small = dict(nhoods_per_image=8, dir_repeats=2, dirs_per_repeat=8, data_loader_kwargs=dict(num_workers=0))
    a = scores.compute_swd(o, 16384, batch_size=64, **small)
    assert scores.compute_swd(o, 16384, batch_size=2, batch_gen=1, **small) == a
    assert scores.compute_swd(o, 16384, batch_size=3, batch_gen=3, **small) == a
    assert scores.compute_swd(o, 16384, seed=1, **small) != a
    assert scores.compute_swd(o, 2, **small) != a               # num_images caps the sets


def _trainer_argv(tmp_path, data, metrics):
    import yaml
    cfg = {"exp": {"trainer": "base"},
           "gen": {"kimg": 1, "batch": 8, "batch_gpu": 8, "loss_arch": "base", "loss": "bcew", "generator": "cnn32_dcgan", "discriminator": "cnn32_dcgan",
                   "g_reg_interval": 0, "d_reg_interval": 0},
           "gens_args": {"cnn32_dcgan": {"z_dim": 16}}, "ema": {"use_ema": False}, "aug": {"aug": "noaug"},
           "log": {"output": str(tmp_path / "logs"), "metrics": list(metrics)},
           "data": {"dataset": "image_folder", "dataset_path": data}, "dataloaders_args": {"basic": {"num_workers": 0}}}
    with open(tmp_path / "run.yaml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    return ["exp.config_dir=" + str(tmp_path), "exp.config=run.yaml", "exp.name=m"]


def test_trainer_accepts_swd16k_without_a_detector(tmp_path, monkeypatch):
    if torch.cuda.is_available():
        pytest.skip("plumbing test is for the CPU container")
    from style_big_gan_amd import starter
    data = make_image_folder(str(tmp_path / "data"), n=8, res=32)
    t = starter.main(_trainer_argv(tmp_path, data, ["swd16k"]), max_iterations=0)
    assert t.metrics == ["swd16k"] and t.metric_detector is None
    with pytest.raises(ValueError, match=r"log\.metrics=\['swd16k', 'fid50k_full'\] needs log\.metric_detector=<local TorchScript file or directory holding "
                                         r"inception-2015-12-05\.pt / vgg16\.pt> \(detectors are not downloaded in this build\); log\.metrics=\[\] turns them off"):
        starter.main(_trainer_argv(tmp_path, data, ["swd16k", "fid50k_full"]), max_iterations=0)
    with pytest.raises(ValueError, match="no local feature detector"):       # asked of the trainer directly, a detector metric still needs one
        t.evaluate_metrics(metrics=["fid50k_full"])
    for stage in ("setup_logs", "init_params", "setup_dataset", "setup_networks", "setup_augmentations"):
        getattr(t, stage)()
    full = scores.compute_swd
    monkeypatch.setattr(scores, "compute_swd", lambda opts, num_images, **kw: full(opts, num_images, nhoods_per_image=4, dir_repeats=1, dirs_per_repeat=4, **kw))
    out = t.evaluate_metrics()          # no detector anywhere: the configured metric runs on the trainer's generator and data set
    assert set(out) == {"swd16k_32", "swd16k_16", "swd16k_avg"} and all(np.isfinite(v) for v in out.values())


def test_calc_metrics_needs_a_detector_only_for_detector_metrics(tmp_path, capsys):
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    det = tmp_path / "det"
    det.mkdir()
    _, args = calc_metrics.parse_args([f"--snapshot={snap}", "--metrics=swd16k"])
    assert args.metrics == ["swd16k"] and args.detector is None
    _, args = calc_metrics.parse_args([f"--snapshot={snap}", "--metrics=swd16k", f"--detector={det}"])
    assert args.detector == str(det)
    for argv in ([f"--snapshot={snap}"], [f"--snapshot={snap}", "--metrics=swd16k,fid50k_full"]):
        with pytest.raises(SystemExit):
            calc_metrics.parse_args(argv)
        assert "the following arguments are required: --detector" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        calc_metrics.parse_args([f"--snapshot={snap}", "--metrics=swd16k", f"--detector={tmp_path / 'absent'}"])
    assert "not downloaded" in capsys.readouterr().err
    # the function: no detector for swd16k, the old refusal for a metric that needs one
    data = make_image_folder(str(tmp_path / "data"), n=2, res=32)
    G = TinyG(32)
    with pytest.raises(ValueError, match="not downloaded"):
        calc_metrics.calc_metrics(G, ["swd16k", "fid50k_full"], dict(path=data), None, device="cpu")
    out = calc_metrics.calc_metrics(G, ["swd16k"], dict(path=data), None, device="cpu")
    assert set(out["swd16k"].results) == {"swd16k_32", "swd16k_16", "swd16k_avg"}
    assert '"metric": "swd16k"' in capsys.readouterr().out
