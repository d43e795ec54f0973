"""Which layer takes the largest steps, which one went non-finite?  A table from a run's ``layers.jsonl``.

With ``log.layer_health=on`` the run log appends one line per tick to ``layers.jsonl`` in the run directory (README, "The run log"; DESIGN
section 30): per phase and parameter the gradient's per-element rms and largest magnitude over the tick's steps, how many gradient elements
were not finite before ``nan_to_num`` erased them and in how many steps, the weight's rms and largest magnitude after the tick's last step,
and ``update_ratio`` = rms over the steps of ``|delta w|`` against ``|w|``.  This tool prints one tick and phase of that file as a table.  Host
code only: it reads the file and nothing else.

    python -m style_big_gan_amd.layer_health RUN_DIR [--tick=-1] [--phase=Gmain] [--sort=update_ratio|grad_rms|nonfinite] [--top=20]

``--tick`` is the tick's number as logged, or a negative index from the end of the file (-1: the latest).  Parameters without a number in the
sort column (a phase whose optimizer the update pass does not restate has no ``update_ratio``) come last.
"""
import argparse
import json
import os
import sys

SORT_KEYS = ("update_ratio", "grad_rms", "nonfinite")
COLUMNS = (("numel", "numel"), ("grad_rms", "grad rms"), ("grad_absmax", "grad absmax"), ("nonfinite", "nonfinite"), ("steps_with_nonfinite", "bad steps"),
           ("weight_rms", "weight rms"), ("weight_absmax", "weight absmax"), ("update_ratio", "update ratio"))


def _refuse(token):
    raise ValueError(f"layers.jsonl is strict JSON: {token} is not a value")


def read_lines(run_dir):
    """-> the parsed lines of RUN_DIR/layers.jsonl (RUN_DIR may also be the file itself)"""
    path = run_dir if os.path.isfile(run_dir) else os.path.join(run_dir, "layers.jsonl")
    if not os.path.isfile(path):
        raise ValueError(f"{path}: no such file (layers.jsonl is written by a run with log.layer_health=on)")
    with open(path) as fh:
        return [json.loads(ln, parse_constant=_refuse) for ln in fh if ln.strip()]


def pick_tick(lines, tick):
    if not lines:
        raise ValueError("layers.jsonl holds no tick yet")
    if tick < 0:
        if -tick > len(lines):
            raise ValueError(f"--tick={tick}: the file holds {len(lines)} ticks")
        return lines[tick]
    found = [ln for ln in lines if ln["tick"] == tick]
    if not found:
        raise ValueError(f"--tick={tick}: the file holds the ticks {[ln['tick'] for ln in lines]}")
    return found[-1]            # a resumed run may log a tick number again: the latest stands


def _cell(v):
    if v is None:
        return "-"
    return str(v) if isinstance(v, int) else f"{v:.4g}"


def table(line, phase, sort="update_ratio", top=20):
    """-> the lines of the table of one parsed tick and phase"""
    if phase not in line["phases"]:
        raise ValueError(f"--phase={phase}: tick {line['tick']} holds the phases {sorted(line['phases'])}")
    if sort not in SORT_KEYS:
        raise ValueError(f"--sort={sort}: use one of {', '.join(SORT_KEYS)}")
    ph = line["phases"][phase]
    rows = sorted(ph["params"].items(), key=lambda kv: (kv[1][sort] is None, -(kv[1][sort] or 0), kv[0]))
    rows = rows[:top] if top > 0 else rows
    head = ["parameter"] + [title for _, title in COLUMNS]
    body = [[name] + [_cell(d[key]) for key, _ in COLUMNS] for name, d in rows]
    widths = [max(len(r[i]) for r in [head] + body) for i in range(len(head))]
    fmt = lambda r: "  ".join([r[0].ljust(widths[0])] + [c.rjust(w) for c, w in zip(r[1:], widths[1:])])
    out = [f"tick {line['tick']}  kimg {line['kimg']:.1f}  phase {phase}  steps {ph['steps']}  parameters {len(ph['params'])}  sorted by {sort}", "",
           fmt(head), fmt(["-" * w for w in widths])] + [fmt(r) for r in body]
    bad = ph.get("nonfinite_params", [])
    out += ["", f"parameters with non-finite gradient elements: {', '.join(bad) if bad else 'none'}"]
    return out


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m style_big_gan_amd.layer_health", description=__doc__.split("\n\n")[0])
    ap.add_argument("run_dir", metavar="RUN_DIR")
    ap.add_argument("--tick", type=int, default=-1)
    ap.add_argument("--phase", default="Gmain")
    ap.add_argument("--sort", default="update_ratio", choices=SORT_KEYS)
    ap.add_argument("--top", type=int, default=20)
    a = ap.parse_args(argv)
    try:
        lines = table(pick_tick(read_lines(a.run_dir), a.tick), a.phase, a.sort, a.top)
    except ValueError as err:
        print(f"layer_health: {err}", file=sys.stderr)
        return 2
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
