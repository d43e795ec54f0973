"""Per-layer gradient and update health, host side: the numpy value graph of the two passes against a plain restatement of their definitions,
the segment table of a GradReducer, the update formula against a real torch.optim.Adam step, `log.layer_health = off | on`, layers.jsonl and
the reader."""
import math
import os
import sys

import numpy as np
import pytest
import torch
import yaml

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import layer_health as reader
from style_big_gan_amd import starter
from style_big_gan_amd.parallel import GradReducer
from style_big_gan_amd.torch_utils.ops import layer_health as lh
from test_image_export_cpu import DCGAN_LIKE
import layer_health_util as lu

F = {name: i for i, name in enumerate(lh.FIELDS)}


def _close(a, b, n):
    """two float64 sums of the same n non-negative terms"""
    return abs(a - b) <= n * lu.U * max(abs(a), abs(b))


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_grads_cpu_against_the_definition(scale):
    x, offs = lu.sprinkled(lu.LENGTHS + [0], seed=1)
    lengths = lu.LENGTHS + [0]
    flat = torch.from_numpy(x.copy())
    views = [flat[o:o + n] for o, n in zip(offs, lengths)]
    running = lh.new_running(len(views), "cpu")
    lh.grads_cpu(views, scale, running)
    assert np.array_equal(flat.numpy().view(np.int32), x.view(np.int32))        # read-only
    run = running.numpy().copy()
    for row, o, n in zip(run, offs, lengths):
        count, sumsq, absmax = lu.grads_plain(x[o:o + n], scale)
        assert row[F["steps"]] == 1 and row[F["nonfinite"]] == count and row[F["steps_with_nonfinite"]] == (count > 0)
        assert row[F["grad_absmax"]] == absmax
        assert _close(row[F["grad_sumsq"]], sumsq, n), (n, row[F["grad_sumsq"]], sumsq)
        assert not row[F["weight_sumsq"]:].any()
    assert not run[-1, 1:].any()            # n == 0: a step of zeros
    lh.grads_cpu(views, scale, running)     # a second fold: sums add, the maximum stays
    again = running.numpy()
    assert np.array_equal(again[:, :4], 2 * run[:, :4]) and np.array_equal(again[:, F["grad_absmax"]], run[:, F["grad_absmax"]])


def test_updates_cpu_against_the_definition():
    rng = np.random.RandomState(2)
    lr, eps, (bc1, bc2) = 0.002, 1e-8, lh.bias_corrections(0.9, 0.99, 3)
    triples = []
    for shape in ([5], [4097], [3 * 4096 + 1], [0]):
        w, m = (torch.from_numpy(rng.randn(*shape).astype(np.float32)) for _ in range(2))
        v = torch.from_numpy((rng.randn(*shape) ** 2 * 1e-3).astype(np.float32))
        triples.append((w, m, v))
    cl = [torch.from_numpy(rng.randn(8, 4, 3, 3).astype(np.float32)).contiguous(memory_format=torch.channels_last) for _ in range(3)]
    triples.append((cl[0], cl[1], cl[2].square()))
    running = lh.new_running(len(triples), "cpu")
    running[:, F["weight_sumsq"]] = 7.0         # "last" fields are overwritten
    lh.updates_cpu(triples, lr, eps, bc1, bc2, running)
    for row, (w, m, v) in zip(running.numpy(), triples):
        n = w.numel()
        wsq, wmax, dsq = lu.updates_plain(*(t.numpy().reshape(-1) for t in (w, m, v)), lr, eps, bc1, bc2)
        assert row[F["weight_absmax"]] == wmax and row[F["steps"]] == 0
        assert _close(row[F["weight_sumsq"]], wsq, n) and _close(row[F["update_sumsq"]], dsq, n)


class _Net(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(4, 8, 3)
        self.conv.weight.data = self.conv.weight.data.contiguous(memory_format=torch.channels_last)
        self.gain = torch.nn.Parameter(torch.ones([]))
        self.fc = torch.nn.Linear(5, 3)


@pytest.mark.parametrize("bucket_bytes", [32 << 20, 128])
def test_segments_of_a_reducer(bucket_bytes):
    net = _Net()
    red = GradReducer(net, bucket_bytes=bucket_bytes)
    segs = lh.segments(red)
    named = list(net.named_parameters())
    assert [(s.name, s.n) for s in segs] == [(name, p.numel()) for name, p in reversed(named)]         # bucket order: reverse registration
    assert len(red._buckets) == (1 if bucket_bytes > 128 else 3)      # 128 bytes: [fc.bias, fc.weight, conv.bias], [conv.weight], [gain]
    for a, b in zip(segs, segs[1:]):
        if a.bucket == b.bucket:
            assert b.ptr == a.ptr + 4 * a.n and b.offset == a.offset + a.n          # back to back: 4-byte aligned only
    for s in segs:
        assert s.param.grad.data_ptr() == s.ptr and s.ptr == red._buckets[s.bucket].flat.data_ptr() + 4 * s.offset
    # a channels_last weight is read in memory order: what lies in the bucket is the (o, kh, kw, i) order of its gradient
    w = dict(named)["conv.weight"]
    assert not w.is_contiguous() and w.grad.stride() == w.stride()
    w.grad.copy_(torch.arange(w.numel(), dtype=torch.float32).reshape(w.shape))
    s = next(s for s in segs if s.name == "conv.weight")
    seg = red._buckets[s.bucket].flat[s.offset:s.offset + s.n]
    assert torch.equal(seg, w.grad.permute(0, 2, 3, 1).reshape(-1)) and torch.equal(lh.memory_order(w.grad), seg)
    assert lh.memory_order(w.grad).data_ptr() == s.ptr
    with pytest.raises(RuntimeError, match="not dense"):
        lh.memory_order(torch.zeros(4, 4)[:, :2])


def test_reducer_measures_before_it_sanitises():
    """the switch on a CPU reducer: finish() folds every parameter's gradient into health_running and still sanitises the buckets"""
    net = _Net()
    red = GradReducer(net)
    red.layer_health = True
    for p in net.parameters():
        p.grad.fill_(2.0)
    net.fc.bias.grad[1] = float("nan")
    net.gain.grad.fill_(float("-inf"))
    red.finish()
    rows = dict(zip([s.name for s in lh.segments(red)], lh.derive(red.health_running, [s.n for s in lh.segments(red)], with_updates=False)))
    assert rows["fc.bias"]["nonfinite"] == 1 and rows["gain"]["nonfinite"] == 1 and rows["conv.weight"]["nonfinite"] == 0
    assert rows["gain"]["grad_absmax"] == 1e5 and rows["conv.weight"]["grad_rms"] == 2.0 and rows["fc.bias"]["grad_rms"] == math.sqrt(8 / 3)
    assert rows["fc.weight"]["update_ratio"] is None and rows["fc.weight"]["weight_rms"] is None
    assert all(bool(torch.isfinite(b.flat).all()) for b in red._buckets)
    off = GradReducer(_Net())
    off.finish()
    assert off.health_running is None


def test_update_formula_against_a_real_adam_step():
    """two stock Adam steps; before the second the weight is set to 0, so that w_after = -delta of step t = 2.  Gradients of ordinary size,
    so that eps = 1e-8 is far below sqrt(v): the fp32 update then carries under ten roundings of 2^-24 against the float64 restatement."""
    torch.manual_seed(3)
    w = torch.nn.Parameter(torch.randn(6, 4, 3, 3).contiguous(memory_format=torch.channels_last))
    opt = torch.optim.Adam([w], lr=0.0025, betas=(0.9, 0.99), eps=1e-8)
    for t in (1, 2):
        with torch.no_grad():
            w.zero_()
        w.grad = torch.randn_like(w) + 0.1
        opt.step()
    st = opt.state[w]
    assert int(st["step"]) == 2
    running = lh.new_running(1, "cpu")
    lh.updates_cpu([(w.detach(), st["exp_avg"], st["exp_avg_sq"])], 0.0025, 1e-8, *lh.bias_corrections(0.9, 0.99, 2), running)
    delta = math.sqrt(float(running[0, F["update_sumsq"]]))
    moved = float(w.detach().double().square().sum().sqrt())
    assert moved > 0 and abs(delta - moved) <= 1e-6 * moved, (delta, moved)
    assert float(running[0, F["weight_sumsq"]]) == pytest.approx(moved ** 2, rel=1e-12)


def test_derive():
    run = np.zeros([3, 8])
    run[0] = [2, 1, 3, 8.0, 5.0, 16.0, 3.0, 0.02]
    run[1] = [2, 0, 0, 0.0, 0.0, 0.0, 0.0, 0.0]
    a, b, c = lh.derive(run, [4, 4, 4])
    assert a == dict(numel=4, grad_rms=1.0, grad_absmax=5.0, nonfinite=3, steps_with_nonfinite=1, weight_rms=2.0, weight_absmax=3.0,
                     update_ratio=math.sqrt(0.01) / 4.0)
    assert b["update_ratio"] is None and b["weight_rms"] == 0.0 and b["grad_rms"] == 0.0      # a weight norm of 0
    assert c["grad_rms"] is None and c["weight_rms"] is None and c["nonfinite"] == 0           # no step in the tick
    assert lh.derive(run, [4, 4, 4], with_updates=False)[0]["update_ratio"] is None


def test_the_abi():
    from style_big_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "sbg_hip.h")).read()
    declared = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()
    for name in ("sbg_layer_health_grads", "sbg_layer_health_updates", "sbg_layer_health_fold"):
        assert f" {name}(" in header and name in declared and hasattr(lib, name)
    assert "SBG_K_LAYER_HEALTH = 35" in header and _lib.KERNEL_KINDS[35] == "layer_health"
    assert _lib.LAYER_HEALTH_VARIANTS == {0: "grads", 1: "updates", 2: "fold"}
    assert f"#define SBG_LAYER_HEALTH_CHUNK {lh.CHUNK}" in header and f"#define SBG_LAYER_HEALTH_FIELDS {len(lh.FIELDS)}" in header
    assert lh.CHUNK == 4096 and lh.FIELDS == ("steps", "steps_with_nonfinite", "nonfinite", "grad_sumsq", "grad_absmax", "weight_sumsq",
                                              "weight_absmax", "update_sumsq")


def _argv(tmp, *more):
    with open(os.path.join(tmp, "dcgan.yaml"), "w") as fh:
        yaml.safe_dump(DCGAN_LIKE, fh)
    return ["exp.config_dir=" + str(tmp), "exp.config=dcgan.yaml", "exp.name=run", "log.output=" + str(tmp / "logs"), "data.dataset=synthetic",
            "data.resolution=32", "gen.batch=8", "gen.batch_gpu=8", "gen.kimg=1", "log.metrics=[]", "log.snap=0", "log.kimg_per_tick=0.016"] + list(more)


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """three iterations, ticks after the first and the third; the generator's optimizer runs amsgrad, which the update pass does not restate"""
    tmp = tmp_path_factory.mktemp("layer_health")
    trainer = starter.main(_argv(tmp, "log.run_log=on", "log.layer_health=on", "optim_gen_args.adam.amsgrad=true"), max_iterations=3)
    return str(tmp / "logs" / "run"), trainer


def test_a_run_writes_strict_lines(run):
    run_dir, trainer = run
    eng = trainer.engine
    text = open(os.path.join(run_dir, "layers.jsonl")).read().splitlines()
    lines = [lu.parse_strict(ln) for ln in text]
    assert len(lines) == 2 == trainer.cur_tick
    names = {"Gboth": [n for n, _ in eng.G.named_parameters()], "Dboth": [n for n, _ in eng.D.named_parameters()]}
    for tick, (line, steps) in enumerate(zip(lines, (1, 2))):
        lu.check_line(line, tick, names)
        assert line["phases"]["Gboth"]["steps"] == steps and line["phases"]["Dboth"]["steps"] == steps
    # the first tick closes after one iteration: the per-parameter sums add up to the phase's norm in stats.jsonl
    import run_log_util as ru
    stats = ru.stats_lines(run_dir)[0]
    for ph, module in (("Gboth", eng.G), ("Dboth", eng.D)):
        params = lines[0]["phases"][ph]["params"]
        n = sum(p.numel() for p in module.parameters())
        total = math.sqrt(sum(d["grad_rms"] ** 2 * d["numel"] for d in params.values()))
        assert abs(total - stats[f"Grad/{ph}/norm"]["mean"]) <= n * lu.U * total, ph
        assert sum(d["nonfinite"] for d in params.values()) == stats[f"Grad/{ph}/nonfinite"]["mean"] == 0
        assert lines[0]["phases"][ph]["nonfinite_params"] == []
        assert sum(d["numel"] for d in params.values()) == n


def test_unsupported_optimizer_settings_give_null_update_fields(run):
    run_dir, trainer = run
    assert set(trainer.engine.layer_health_unsupported) == {"Gboth"}
    last = lu.read_layers(os.path.join(run_dir, "layers.jsonl"))[-1]["phases"]
    for d in last["Gboth"]["params"].values():
        assert d["update_ratio"] is None and d["weight_rms"] is None and d["weight_absmax"] is None and d["grad_rms"] > 0
    for name, d in last["Dboth"]["params"].items():
        assert d["weight_rms"] >= 0 and d["grad_rms"] >= 0
        assert d["update_ratio"] is None or 0 < d["update_ratio"] < float("inf"), name
    assert any(d["update_ratio"] for d in last["Dboth"]["params"].values())
    log = open(os.path.join(run_dir, "log.txt")).read()
    assert log.count("Gboth: no update fields") == 1 and "Dboth: no update fields" not in log


def test_the_step_count_is_the_optimizers(run):
    _, trainer = run
    eng = trainer.engine
    for ph in eng.phases:
        p = next(iter(ph.module.parameters()))
        assert eng._layer_health_t[id(ph.opt)] == int(ph.opt.state[p]["step"]) == 3


def test_on_without_the_run_log_is_refused(tmp_path):
    with pytest.raises(ValueError, match=r"log\.layer_health=on.*log\.run_log"):
        starter.main(_argv(tmp_path, "log.run_log=off", "log.layer_health=on"), max_iterations=1)
    with pytest.raises(ValueError, match=r"log\.layer_health=on.*log\.run_log"):
        starter.main(_argv(tmp_path, "log.layer_health=on"), max_iterations=1)           # auto with a cap keeps no run log
    with pytest.raises(ValueError, match="layer_health"):
        starter.main(_argv(tmp_path, "log.layer_health=sometimes"), max_iterations=0)
    assert not os.path.exists(tmp_path / "logs")
    trainer = starter.main(_argv(tmp_path, "log.run_log=on"), max_iterations=1)          # off by default: no file, nothing switched on
    assert not trainer.layer_health and not trainer.engine.layer_health and not any(r.layer_health for r in trainer.engine.dp_modules.values())
    assert "layers.jsonl" not in os.listdir(tmp_path / "logs" / "run")


def test_the_reader(run, capsys):
    run_dir, _ = run
    assert reader.main([run_dir, "--phase=Dboth", "--sort=grad_rms", "--top=3"]) == 0
    out = capsys.readouterr().out.splitlines()
    assert out[0].startswith("tick 1 ") and "phase Dboth" in out[0] and "steps 2" in out[0]
    body = out[4:7]
    assert len(body) == 3 and [float(ln.split()[2]) for ln in body] == sorted((float(ln.split()[2]) for ln in body), reverse=True)
    assert out[-1] == "parameters with non-finite gradient elements: none"
    assert reader.main([run_dir, "--tick=0", "--phase=Gboth", "--top=0"]) == 0          # no update_ratio anywhere: every row, dashes in the column
    assert capsys.readouterr().out.count(" -") >= 3
    assert reader.main([run_dir, "--phase=Gmain"]) == 2 and "holds the phases" in capsys.readouterr().err
    assert reader.main([run_dir, "--tick=7", "--phase=Dboth"]) == 2
    with pytest.raises(ValueError, match="strict JSON"):
        reader._refuse("NaN")
