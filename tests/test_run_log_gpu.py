"""The training run log on the device: a tiny sg2 run of six iterations writes four ticks -- status lines, stats.jsonl with the gradient
health of every phase from the fused kernel and the phases' device times, image and network snapshots -- and a resumed trainer continues
the tick count."""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import _lib, starter
import run_log_util as ru

pytestmark = pytest.mark.gpu

SG2_YAML = ("exp:\n  trainer: sg2\ngen:\n  generator: sg2_classic\n  discriminator: sg2_classic\n"
            "  disc_regs: [r1]\ndisc_regs_all:\n  r1:\n    r1_gamma: 0.01\nlosses_arch_args:\n  sg2:\n    style_mixing_prob: 0\n"
            "aug:\n  aug: noaug\ndata:\n  dataset: synthetic\n  resolution: 32\n"
            "gens_args:\n  sg2_classic:\n    z_dim: 16\n    w_dim: 16\n    mapping_kwargs:\n      num_layers: 2\n"
            "    synthesis_kwargs:\n      channel_base: 512\n      channel_max: 16\n      num_fp16_res: 0\n      block_kwargs:\n        conv_clamp: 256\n"
            "discs_args:\n  sg2_classic:\n    channel_base: 512\n    channel_max: 16\n    num_fp16_res: 0\n    architecture: orig\n"
            "    epilogue_kwargs:\n      mbstd_group_size: 4\n")


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """one run shared by the tests below -> (argv, run directory, trainer, grad_finish launch variants seen during the run)"""
    tmp = tmp_path_factory.mktemp("run_log")
    (tmp / "cfg.yaml").write_text(SG2_YAML)
    argv = [f"exp.config_dir={tmp}", "exp.config=cfg.yaml", "exp.name=run", f"log.output={tmp / 'logs'}"] + ru.RUN_ARGS
    _lib.prof_enable(True)
    try:
        _lib.prof_fetch()
        trainer = starter.main(argv, max_iterations=6)
        seen = [_lib.GRAD_FINISH_VARIANTS[r["dims"][0]] for r in _lib.prof_fetch() if r["kind"] == "grad_finish"]
    finally:
        _lib.prof_enable(False)
    return argv, str(tmp / "logs" / "run"), trainer, seen


def test_ticks_files_and_statistics(run):
    _, run_dir, trainer, _ = run
    assert [p.name for p in trainer.engine.phases] == ["Gmain", "Greg", "Dmain", "Dreg"] and trainer.cur_tick == 4
    stats = ru.check_run_dir(run_dir, phases=["Gmain", "Dmain"], timed=True)
    assert stats[0]["Grad/Dreg/norm"]["num"] == 1 and "Grad/Dreg/norm" in stats[2] and not any(k.startswith("Grad/Greg") for k in stats[3])
    assert stats[1]["Resources/peak_gpu_mem_gb"]["mean"] > 0


def test_the_health_comes_from_the_kernel(run):
    """six iterations run Gmain and Dmain six times and Dreg twice; Gmain finishes two reducers (mapping, synthesis): one sweep per bucket
    and one merge per reducer and phase, and the reducers hold the record on the device"""
    _, _, trainer, seen = run
    reducers = trainer.engine.dp_modules
    buckets = {k: len(r._buckets) for k, r in reducers.items()}
    finishes = {"G_mapping": 6, "G_synthesis": 6, "D": 8}
    assert seen.count("merge") == sum(finishes.values())
    assert seen.count("sweep") == sum(finishes[k] * buckets[k] for k in finishes)
    for r in reducers.values():
        assert r.last_health.is_cuda and r.last_health.dtype == torch.float64 and r.last_health.shape == (3,)


def test_resume_continues_the_tick_count(run):
    argv, run_dir, _, _ = run
    resumed = starter.main([a for a in argv if a != "log.run_log=on"] + ["log.run_log=off", f"trans.resume={os.path.join(run_dir, 'network-snapshot-000000.pt')}"],
                           max_iterations=0)
    assert resumed.cur_tick == 4 and resumed.engine.cur_nimg == 48 and resumed.engine.batch_idx == 6
    assert len(ru.status_lines(run_dir)) == 4          # log.run_log=off: nothing was appended
