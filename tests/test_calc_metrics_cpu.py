"""The calc_metrics tool on the CPU: option parsing and failures, one full run from a snapshot the trainer wrote, the data set options it
derives from the run's config, and precision_recall_fused across two gloo ranks."""
import json
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import projector_util
from golden_util import Golden, make_image_folder
from style_big_gan_amd import arguments, calc_metrics
from style_big_gan_amd.metrics import scores
from style_big_gan_amd.train_parts import trainers as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SG2_YAML = ("exp:\n  trainer: sg2\ngen:\n  generator: sg2_classic\n  discriminator: sg2_classic\n  batch: 8\n  batch_gpu: 4\n  kimg: 1\n"
            "  disc_regs: [r1]\ndisc_regs_all:\n  r1:\n    r1_gamma: 0.01\nlosses_arch_args:\n  sg2:\n    style_mixing_prob: 0\n"
            "aug:\n  aug: noaug\ndata:\n  dataset: image_folder\n  dataset_path: {path}\n  mirror: true\nlog:\n  metrics: []\n"
            "dataloaders_args:\n  basic:\n    num_workers: 0\n"
            "gens_args:\n  sg2_classic:\n    z_dim: 16\n    w_dim: 16\n    mapping_kwargs:\n      num_layers: 2\n"
            "    synthesis_kwargs:\n      channel_base: 256\n      channel_max: 16\n      num_fp16_res: 0\n      block_kwargs:\n        conv_clamp: 256\n"
            "discs_args:\n  sg2_classic:\n    channel_base: 256\n    channel_max: 16\n    num_fp16_res: 0\n    architecture: orig\n"
            "    epilogue_kwargs:\n      mbstd_group_size: 4\n")


class _ScriptedDetector(torch.nn.Module):
    """TorchScript stand-in with the reference detectors' call surface: 16-d features with return_features=True"""

    def __init__(self):
        super().__init__()
        g = torch.Generator().manual_seed(5)
        self.register_buffer("w", torch.randn(48, 16, generator=g) / 48 ** 0.5)
        self.register_buffer("head", torch.randn(16, 4, generator=g))

    def forward(self, images: torch.Tensor, return_features: bool = False, no_output_bias: bool = False) -> torch.Tensor:
        x = torch.nn.functional.adaptive_avg_pool2d(images.float() / 255.0, 4).flatten(1) @ self.w
        if return_features:
            return x
        return torch.softmax(x @ self.head + (0.0 if no_output_bias else 1.0), dim=1)


def _detectors(root):
    os.makedirs(root, exist_ok=True)
    for name in ("inception-2015-12-05.pt", "vgg16.pt"):
        torch.jit.script(_ScriptedDetector()).save(os.path.join(root, name))
    return root


def _run(tmp_path, n_images=20):
    """config overrides of an sg2 run on a generated image folder, and a snapshot its trainer wrote (without training_options.json)"""
    data = make_image_folder(str(tmp_path / "data"), n=n_images, res=16)
    (tmp_path / "cfg.yaml").write_text(SG2_YAML.format(path=data))
    overrides = [f"exp.config_dir={tmp_path}", "exp.config=cfg.yaml", "exp.name=run", f"log.output={tmp_path / 'logs'}"]
    trainer = T.trainers["sg2"]().setup_arguments(arguments.load_config(overrides))
    for stage in ("setup_logs", "init_params", "setup_dataset", "setup_networks", "setup_augmentations"):
        getattr(trainer, stage)()
    snap_dir = tmp_path / "snaps"
    snap_dir.mkdir()
    snap = str(snap_dir / "network-snapshot-000000.pt")
    state = trainer.engine.G_ema if trainer.engine.G_ema is not None else trainer.engine.G
    torch.save({"G_ema": {k: v.detach().cpu() for k, v in state.state_dict().items()}}, snap)
    return trainer, overrides, snap, data


def test_option_parsing_and_failures(tmp_path, capsys):
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    det = _detectors(str(tmp_path / "det"))
    ok = [f"--snapshot={snap}", f"--detector={det}"]
    overrides, args = calc_metrics.parse_args(["exp.config=a.yaml"] + ok)
    assert overrides == ["exp.config=a.yaml"] and args.metrics == ["fid50k_full"] and args.gpus == 1 and args.mirror is None and args.device == "auto"
    _, args = calc_metrics.parse_args(ok + ["--metrics=fid50k_full,pr50k3_full", "--mirror=0", "--gpus=16", "--device=cpu", "--data=/d", "--verbose=0"])
    assert args.metrics == ["fid50k_full", "pr50k3_full"] and args.mirror is False and args.gpus == 16 and args.data == "/d" and args.verbose == 0
    assert calc_metrics.parse_args(ok + ["--metrics=none"])[1].metrics == []
    for bad, message in [(ok + ["--metrics=fid50k_full,fid_of_nothing"], "pr50k3_full"),         # the valid names are listed
                         (ok + ["--gpus=0"], "at least 1"), (ok + ["--gpus=17"], "at most 16"),
                         ([f"--snapshot={tmp_path / 'absent.pt'}", f"--detector={det}"], "no such file"),
                         ([f"--snapshot={snap}", f"--detector={tmp_path / 'absent'}"], "not downloaded"),
                         ([f"--snapshot={snap}"], "--detector"), (ok + ["--frobnicate"], "unrecognised")]:
        with pytest.raises(SystemExit):
            calc_metrics.parse_args(bad)
        assert message in capsys.readouterr().err, bad
    with pytest.raises(ValueError, match="vgg16.pt"):            # the path-length metrics keep the trainer's checks
        calc_metrics.check_metrics(["ppl_wend"], None, os.path.join(det, "inception-2015-12-05.pt"))
    with pytest.raises(ValueError, match="mapping and synthesis"):
        calc_metrics.check_metrics(["ppl_wend"], torch.nn.Linear(2, 2), det)


def test_dataset_kwargs_follow_the_config_and_the_overrides(tmp_path):
    trainer, overrides, snap, data = _run(tmp_path)
    config = arguments.load_config(overrides)
    assert T.training_set_kwargs_from_config(config, seed=config.gen.seed) == trainer.training_set_kwargs       # what the trainer built before
    assert trainer.training_set_kwargs == dict(trainer.training_set_kwargs, path=data, resolution=16, use_labels=False, max_size=20, xflip=True)
    G = trainer.engine.G
    kw = calc_metrics.dataset_kwargs_for(config, G)
    assert kw == trainer.training_set_kwargs
    other = make_image_folder(str(tmp_path / "other"), n=9, res=16)
    kw = calc_metrics.dataset_kwargs_for(config, G, data=other, mirror=False)
    assert kw["path"] == other and kw["max_size"] == 9 and not kw.get("xflip") and kw["use_labels"] is False
    assert calc_metrics.dataset_kwargs_for(config, G, mirror=True)["xflip"] is True

    class Conditional:
        c_dim = 4
    assert calc_metrics.dataset_kwargs_for(config, Conditional())["use_labels"] is True         # the labels follow the network


class _CpuGenerator(projector_util.OracleGenerator):
    """the package's generator runs only on the device: the CPU run evaluates the snapshot's weights with the CPU restatement of the same
    network (oracle/networks.py), at the shape of SG2_YAML"""

    def forward(self, z, c, noise_mode="const", **kw):
        return self.synthesis(self.mapping(z, c), noise_mode=noise_mode)


def _cpu_generator(config, state, device):
    assert config.gen.generator == "sg2_classic" and torch.device(device).type == "cpu"
    m = dict(z_dim=16, w_dim=16, img_resolution=16, channel_base=256, channel_max=16, mapping_layers=2, conv_clamp=256)
    return _CpuGenerator(m, state).eval().requires_grad_(False)


def test_cli_run_on_the_cpu(tmp_path, capsys, monkeypatch):
    _, overrides, snap, data = _run(tmp_path)
    det = _detectors(str(tmp_path / "det"))
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", _cpu_generator)
    fid, pr = scores.compute_fid, scores.compute_pr
    monkeypatch.setattr(scores, "compute_fid", lambda opts, max_real, num_gen, **kw: fid(opts, max_real=max_real, num_gen=24, **kw))
    monkeypatch.setattr(scores, "compute_pr", lambda opts, max_real, num_gen, nhood_size, row_batch_size, col_batch_size, **kw:
                        pr(opts, max_real=max_real, num_gen=24, nhood_size=nhood_size, row_batch_size=8, col_batch_size=8, **kw))
    argv = overrides + [f"--snapshot={snap}", f"--detector={det}", "--metrics=fid50k_full,pr50k3_full", "--device=cpu", "--verbose=0"]
    capsys.readouterr()
    results = calc_metrics.run_calc_metrics(argv)
    lines = [json.loads(line) for line in capsys.readouterr().out.strip().splitlines()]
    assert [line["metric"] for line in lines] == ["fid50k_full", "pr50k3_full"]
    assert np.isfinite(lines[0]["results"]["fid50k_full"]) and lines[0]["results"]["fid50k_full"] == results["fid50k_full"].results.fid50k_full
    assert set(lines[1]["results"]) == {"pr50k3_full_precision", "pr50k3_full_recall"} and 0 <= lines[1]["results"]["pr50k3_full_recall"] <= 1
    assert lines[0]["snapshot_pkl"] == snap and lines[0]["num_gpus"] == 1
    snap_dir = os.path.dirname(snap)
    assert sorted(os.listdir(snap_dir)) == ["network-snapshot-000000.pt"]            # no training_options.json: nothing is appended
    with open(os.path.join(snap_dir, "training_options.json"), "w") as f:
        json.dump({}, f)
    for _ in range(2):
        calc_metrics.run_calc_metrics(argv[:-3] + ["--metrics=fid50k_full", "--device=cpu", "--verbose=0"])
    assert sorted(os.listdir(snap_dir)) == ["metric-fid50k_full.jsonl", "network-snapshot-000000.pt", "training_options.json"]
    recs = [json.loads(line) for line in open(os.path.join(snap_dir, "metric-fid50k_full.jsonl"))]
    assert len(recs) == 2 and recs[0]["snapshot_pkl"] == "network-snapshot-000000.pt"          # appended, relative to the run dir


def _pr_worker(rank, world, init_file, results):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import style_big_gan_amd  # noqa: F401
    from style_big_gan_amd.metrics import scores as sc
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        g = Golden("metrics")
        real, gen = g.t("real")[:301].to(torch.float16), g.t("gen")[:255].to(torch.float16)
        results[rank] = sc.precision_recall_fused(real, gen, 3, 64, num_gpus=world, rank=rank)
    finally:
        dist.destroy_process_group()


def test_precision_recall_fused_world2_gloo():
    """two ranks share the manifold rows and the probe rows (301 and 255: neither divides by 2); every rank returns the one-rank numbers"""
    g = Golden("metrics")
    real, gen = g.t("real")[:301].to(torch.float16), g.t("gen")[:255].to(torch.float16)
    solo = scores.precision_recall_fused(real, gen, 3, 64)
    assert 0 < solo[0] < 1 and 0 < solo[1] < 1
    world = 2
    with tempfile.TemporaryDirectory() as d:
        mgr = mp.Manager()
        results = mgr.dict()
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_pr_worker, args=(r, world, os.path.join(d, "rdzv"), results)) for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=180)
        for p in procs:
            assert p.exitcode == 0, f"worker exit code {p.exitcode}"
        assert dict(results) == {0: solo, 1: solo}
