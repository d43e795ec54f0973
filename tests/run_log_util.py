"""What the run-log tests share: the status line's field pattern and the checks on a run directory written by a six-iteration run with
gen.batch=8, log.kimg_per_tick=0.016 (two iterations per tick), log.snap=2 -- ticks after iterations 1, 3, 5 and 6."""
import json
import math
import os
import re

STATUS = re.compile(r"^tick (\d+) +kimg (\d+\.\d) +time (\S+(?: \S+){0,2}) +time left (\S+(?: \S+){0,2}) +sec/tick (\d+\.\d) +sec/kimg (\d+\.\d\d) +"
                    r"maintenance (\d+\.\d) +cpumem (\d+\.\d\d) +gpumem (\d+\.\d\d) +augment (\d+\.\d{3})$")

RUN_ARGS = ["gen.batch=8", "gen.batch_gpu=8", "gen.kimg=1", "log.kimg_per_tick=0.016", "log.snap=2", "log.metrics=[]", "log.run_log=on"]
RUN_FILES = ["fakes000000.png", "fakes_init.png", "log.txt", "network-snapshot-000000.pt", "reals.png", "stats.jsonl", "training_options.json"]


def status_lines(run_dir):
    with open(os.path.join(run_dir, "log.txt")) as fh:
        return [ln.rstrip("\n") for ln in fh if ln.startswith("tick ")]


def stats_lines(run_dir):
    with open(os.path.join(run_dir, "stats.jsonl")) as fh:
        return [json.loads(ln) for ln in fh]


def check_run_dir(run_dir, phases, timed):
    """the files, four ticks numbered 0..3 in both logs, and the statistics of the second tick (iterations 2 and 3)"""
    assert sorted(os.listdir(run_dir)) == RUN_FILES
    lines = status_lines(run_dir)
    assert len(lines) == 4
    for i, ln in enumerate(lines):
        m = STATUS.match(ln)
        assert m is not None and int(m.group(1)) == i, ln
        assert len(ln.split(" time ")[0]) == len("tick 0     kimg 0.0     ")         # the reference's column widths: <5d and <8.1f
    stats = stats_lines(run_dir)
    assert len(stats) == 4
    assert [s["Progress/tick"]["mean"] for s in stats] == [0, 1, 2, 3] and all(s["timestamp"] > 0 for s in stats)
    assert [round(s["Progress/kimg"]["mean"] * 1000) for s in stats] == [8, 24, 40, 48]
    second = stats[1]
    for ph in phases:
        for what in ("norm", "absmax", "nonfinite"):
            assert second[f"Grad/{ph}/{what}"]["num"] == 2, (ph, what, second[f"Grad/{ph}/{what}"])
        norm, absmax = second[f"Grad/{ph}/norm"]["mean"], second[f"Grad/{ph}/absmax"]["mean"]
        assert math.isfinite(norm) and norm > 0 and math.isfinite(absmax) and 0 < absmax <= norm
        assert second[f"Grad/{ph}/nonfinite"]["mean"] == 0
        if timed:
            assert second[f"Timing/{ph}"]["num"] == 1 and second[f"Timing/{ph}"]["mean"] > 0
        else:
            assert f"Timing/{ph}" not in second
    for name in ("Timing/total_sec", "Timing/sec_per_tick", "Timing/sec_per_kimg", "Timing/maintenance_sec", "Timing/total_hours", "Timing/total_days",
                 "Resources/cpu_mem_gb", "Resources/peak_gpu_mem_gb", "Progress/augment"):
        assert second[name]["num"] == 1, name
    assert second["Resources/cpu_mem_gb"]["mean"] > 0
    with open(os.path.join(run_dir, "training_options.json")) as fh:
        assert json.load(fh)["start_options"] == {"cur_nimg": 48, "batch_idx": 6, "cur_tick": 4}
    return stats
