"""The training run log, host side: the tick rule, the status line, stats.jsonl with the gradient health from the torch path of
GradReducer.finish(), snapshots, `log.run_log = auto | on | off`, format_time, and a two-rank gloo run."""
import json
import os
import sys

import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import starter
from style_big_gan_amd.train_parts import trainers as T
from test_image_export_cpu import DCGAN_LIKE
import run_log_util as ru


def _argv(tmp, *more):
    with open(os.path.join(tmp, "dcgan.yaml"), "w") as fh:
        yaml.safe_dump(DCGAN_LIKE, fh)
    return ["exp.config_dir=" + str(tmp), "exp.config=dcgan.yaml", "exp.name=run", "log.output=" + str(tmp / "logs"), "data.dataset=synthetic",
            "data.resolution=32", "gen.batch=8", "gen.batch_gpu=8", "gen.kimg=1", "log.metrics=[]"] + list(more)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("run_log")
    argv = _argv(tmp, *[a for a in ru.RUN_ARGS if a not in ("gen.batch=8", "gen.batch_gpu=8", "gen.kimg=1", "log.metrics=[]")])
    trainer = starter.main(argv, max_iterations=6)
    return argv, str(tmp / "logs" / "run"), trainer


def test_ticks_files_and_statistics(run, capsys):
    _, run_dir, trainer = run
    assert trainer.run_log and trainer.cur_tick == 4 and trainer.engine.batch_idx == 6
    on_gpu = trainer.engine.device.type == "cuda"
    ru.check_run_dir(run_dir, phases=["Gboth", "Dboth"], timed=on_gpu)
    text = open(os.path.join(run_dir, "log.txt")).read()
    for needle in ("Training options:", f"Output directory:   {run_dir}", "Training data:      synthetic", "Training duration:  1 kimg", "Number of GPUs:     1",
                   "Number of images:   4096", "Image resolution:   32", "Conditional model:  False", "Dataset x-flips:    False",
                   "Exporting sample images...", "Training for 1 kimg..."):
        assert needle in text, needle
    state = torch.load(os.path.join(run_dir, "network-snapshot-000000.pt"), weights_only=True)
    assert state["progress"] == {"cur_nimg": 48, "batch_idx": 6, "cur_tick": 4}


def test_resume_continues_the_tick_count_and_appends(run):
    argv, run_dir, _ = run
    resumed = starter.main(argv + [f"trans.resume={os.path.join(run_dir, 'network-snapshot-000000.pt')}", "gen.kimg=0.056"], max_iterations=None)
    assert resumed.cur_tick == 5 and resumed.engine.batch_idx == 7           # one more iteration reaches 56 images: the closing tick, numbered 4
    lines = ru.status_lines(run_dir)
    assert len(lines) == 5 and int(ru.STATUS.match(lines[4]).group(1)) == 4 and len(ru.stats_lines(run_dir)) == 5


def test_a_capped_run_without_the_key_logs_nothing(tmp_path, capsys):
    trainer = starter.main(_argv(tmp_path), max_iterations=2)
    assert not trainer.run_log and trainer.run_log_mode == "auto" and not trainer.engine.time_phases and not trainer.engine.report_grad_health
    assert not os.path.exists(tmp_path / "logs")
    assert "tick " not in capsys.readouterr().out
    trainer.save_snapshot(run_dir=str(tmp_path / "snap"))
    assert json.load(open(tmp_path / "snap" / "training_options.json"))["start_options"] == {"cur_nimg": 16, "batch_idx": 2}


def test_run_log_off_without_a_cap_logs_nothing(tmp_path, capsys):
    trainer = starter.main(_argv(tmp_path, "log.run_log=off", "gen.kimg=0.016"))
    assert trainer.engine.batch_idx == 2 and not trainer.run_log and not os.path.exists(tmp_path / "logs")
    assert "tick " not in capsys.readouterr().out
    with pytest.raises(ValueError, match="run_log"):
        starter.main(_argv(tmp_path, "log.run_log=sometimes"), max_iterations=0)


def test_auto_without_a_cap_is_on(tmp_path):
    """a real run: no key, no cap.  gen.kimg=0.008 is one iteration: the tick after the first iteration is also the closing one"""
    trainer = starter.main(_argv(tmp_path, "gen.kimg=0.008", "log.kimg_per_tick=0.5"))
    run_dir = str(tmp_path / "logs" / "run")
    assert trainer.run_log and trainer.cur_tick == 1 and len(ru.status_lines(run_dir)) == 1 and len(ru.stats_lines(run_dir)) == 1
    assert sorted(os.listdir(run_dir)) == ru.RUN_FILES


def test_format_time():
    assert [T.format_time(s) for s in (59, 60, 3599, 3600, 86399, 86400)] == ["59s", "1m 00s", "59m 59s", "1h 00m 00s", "23h 59m 59s", "1d 00h 00m"]
    assert T.format_time(59.4) == "59s" and T.format_time(59.6) == "1m 00s" and T.format_time(0) == "0s" and T.format_time(90061) == "1d 01h 01m"


def _rank_worker(rank, argv, tmp, results):
    sys.path.insert(0, ROOT)
    import style_big_gan_amd  # noqa: F401
    from style_big_gan_amd import arguments, starter
    from style_big_gan_amd.train_parts import trainers as T
    trainer = T.trainers["base"]().setup_arguments(arguments.load_config(argv))
    try:
        starter.multiprocesses_main(rank, trainer, tmp, 3)
        stats = trainer.stats.as_dict()
        results[rank] = {k: (v["num"], v["mean"]) for k, v in stats.items() if k.startswith("Grad/")}
    finally:
        torch.distributed.destroy_process_group()


def test_two_ranks_over_gloo(tmp_path):
    if torch.cuda.is_available():
        pytest.skip("plumbing test is for the CPU container")
    argv = _argv(tmp_path, "perf.gpus=2", "gen.batch=8", "log.run_log=on", "log.kimg_per_tick=0.016", "log.snap=50")
    results = torch.multiprocessing.get_context("spawn").Manager().dict()
    torch.multiprocessing.spawn(_rank_worker, args=(argv, str(tmp_path), results), nprocs=2)
    assert set(results.keys()) == {0, 1} and results[0] == results[1] and len(results[0]) == 6
    for name, (num, mean) in results[0].items():
        assert num == 4 and (mean == 0 if name.endswith("nonfinite") else mean > 0), (name, num, mean)       # the closing tick: iterations 2 and 3 on two ranks
    run_dir = str(tmp_path / "logs" / "run")
    assert sorted(os.listdir(run_dir)) == ru.RUN_FILES
    stats = ru.stats_lines(run_dir)
    assert [s["Progress/tick"]["mean"] for s in stats] == [0, 1] and [s["Progress/tick"]["num"] for s in stats] == [1, 1]
    assert stats[1]["Grad/Gboth/norm"]["num"] == 4 and len(ru.status_lines(run_dir)) == 2        # iterations 2 and 3, two ranks each
