"""Per-layer gradient and update health on the device (csrc/layer_health.hip): both passes and the fold against the numpy value graph bit
for bit, the gradient pass against grad_finish over the same buffer, and a tiny sg2 run that writes layers.jsonl."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import _lib, starter
from style_big_gan_amd.torch_utils.ops import grad_finish
from style_big_gan_amd.torch_utils.ops import layer_health as lh
import layer_health_util as lu
import run_log_util as ru

pytestmark = pytest.mark.gpu

DEV = "cuda"
F = {name: i for i, name in enumerate(lh.FIELDS)}
N = sum(lu.LENGTHS)


def _bits(t):
    return t.detach().cpu().contiguous().numpy().view(np.int64 if t.dtype == torch.float64 else np.int32)


@pytest.fixture(scope="module")
def buffers():
    """two buffers of the nine segments laid back to back, on the host and on the device, and the segments' offsets"""
    xa, offs = lu.sprinkled(lu.LENGTHS, seed=11)
    xb, _ = lu.sprinkled(lu.LENGTHS, seed=12)
    assert sorted(set(int(o) % 4 for o in offs)) == [0, 1, 2, 3]
    return xa, xb, torch.from_numpy(xa).to(DEV), torch.from_numpy(xb).to(DEV), offs


def _views(x, offs):
    flat = torch.from_numpy(x.copy())
    return [flat[o:o + n] for o, n in zip(offs, lu.LENGTHS)]


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_gradient_pass_bit_for_bit_and_read_only(buffers, scale):
    xa, _, da, _, offs = buffers
    table = lh.buffer_table(da, lu.LENGTHS)
    assert table.records == sum(-(-n // 4096) for n in lu.LENGTHS) and table.total_n == N
    running = lh.grads(table, scale, lh.new_running(len(lu.LENGTHS), DEV))
    want = lh.grads_cpu(_views(xa, offs), scale, lh.new_running(len(lu.LENGTHS), "cpu"))
    assert np.array_equal(_bits(running), _bits(want))
    assert want[:, F["nonfinite"]].sum() > 20 and want[:, F["steps"]].eq(1).all()
    assert np.array_equal(_bits(da), xa.view(np.int32))                 # after the pass the buffer's bits are unchanged


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_gradient_pass_against_grad_finish(buffers, scale):
    _, _, da, _, _ = buffers
    run = lh.grads(lh.buffer_table(da, lu.LENGTHS), scale, lh.new_running(len(lu.LENGTHS), DEV)).cpu().numpy()
    swept = da.clone()
    partials = torch.zeros([grad_finish.records(N), 3], dtype=torch.float64, device=DEV)
    grad_finish.sweep(swept, scale, partials)
    count, sumsq, absmax = grad_finish.merge(partials).cpu().tolist()
    print(f"scale {scale}: count {run[:, F['nonfinite']].sum()} / {count}, absmax {run[:, F['grad_absmax']].max()} / {absmax}, "
          f"sumsq {run[:, F['grad_sumsq']].sum()!r} / {sumsq!r}")
    assert run[:, F["nonfinite"]].sum() == count
    assert run[:, F["grad_absmax"]].max() == absmax
    assert abs(run[:, F["grad_sumsq"]].sum() - sumsq) <= N * lu.U * sumsq


def test_two_calls_fold_as_defined(buffers):
    xa, xb, da, db, offs = buffers
    P = len(lu.LENGTHS)
    running = lh.new_running(P, DEV)
    first = lh.grads(lh.buffer_table(da, lu.LENGTHS), 1.0, running).cpu().numpy().copy()
    lh.grads(lh.buffer_table(db, lu.LENGTHS), 0.5, running)
    alone = lh.grads(lh.buffer_table(db, lu.LENGTHS), 0.5, lh.new_running(P, DEV)).cpu().numpy()
    both = running.cpu().numpy()
    for f in ("steps", "steps_with_nonfinite", "nonfinite", "grad_sumsq"):
        assert np.array_equal(both[:, F[f]], first[:, F[f]] + alone[:, F[f]]), f          # sums add (one float64 addition per field)
    assert np.array_equal(both[:, F["grad_absmax"]], np.maximum(first[:, F["grad_absmax"]], alone[:, F["grad_absmax"]]))
    assert not both[:, F["weight_sumsq"]:].any()
    want = lh.new_running(P, "cpu")
    lh.grads_cpu(_views(xa, offs), 1.0, want)
    lh.grads_cpu(_views(xb, offs), 0.5, want)
    assert np.array_equal(_bits(running), _bits(want))


def _triples(seed):
    rng = np.random.RandomState(seed)
    out = []
    for shape in ([5], [4097]):
        out.append(tuple(torch.from_numpy(a.astype(np.float32)) for a in (rng.randn(*shape), rng.randn(*shape) * 0.1, rng.randn(*shape) ** 2 * 1e-2)))
    cl = [torch.from_numpy(a.astype(np.float32)).contiguous(memory_format=torch.channels_last)
          for a in (rng.randn(8, 4, 3, 3), rng.randn(8, 4, 3, 3) * 0.1, rng.randn(8, 4, 3, 3) ** 2 * 1e-2)]
    out.append(tuple(cl))
    out[0][2][0] = 0.0          # v == 0 with m == 0: 0 / (0 + eps)
    out[0][1][0] = 0.0
    return out


def test_update_pass_bit_for_bit():
    P = 3
    lr, eps = 0.0025 * 16 / 17, 1e-8
    host_a, host_b = _triples(21), _triples(22)
    dev_a, dev_b = ([tuple(t.to(DEV) for t in tr) for tr in host] for host in (host_a, host_b))
    assert not dev_a[2][0].is_contiguous() and dev_a[2][0].is_contiguous(memory_format=torch.channels_last)
    before = [_bits(t) for tr in dev_a for t in tr]
    running, want = lh.new_running(P, DEV), lh.new_running(P, "cpu")
    bc = lh.bias_corrections(0.0, 0.99 ** (16 / 17), 3)
    lh.updates(lh.update_table(dev_a), lr, eps, *bc, running)
    lh.updates_cpu(host_a, lr, eps, *bc, want)
    assert np.array_equal(_bits(running), _bits(want))
    assert all(np.array_equal(a, _bits(t)) for a, t in zip(before, (t for tr in dev_a for t in tr)))
    first = want.numpy().copy()
    bc = lh.bias_corrections(0.9, 0.999, 4)
    lh.updates(lh.update_table(dev_b), lr, eps, *bc, running)
    lh.updates_cpu(host_b, lr, eps, *bc, want)
    assert np.array_equal(_bits(running), _bits(want))
    alone = lh.updates_cpu(host_b, lr, eps, *bc, lh.new_running(P, "cpu")).numpy()
    both = running.cpu().numpy()
    assert np.array_equal(both[:, F["weight_sumsq"]], alone[:, F["weight_sumsq"]]) and np.array_equal(both[:, F["weight_absmax"]], alone[:, F["weight_absmax"]])
    assert np.array_equal(both[:, F["update_sumsq"]], first[:, F["update_sumsq"]] + alone[:, F["update_sumsq"]])        # "last" overwritten, the sum added
    assert not both[:, :F["weight_sumsq"]].any() and both[:, F["update_sumsq"]].min() > 0


def test_inputs_that_are_not_dense_fp32_are_errors():
    with pytest.raises(RuntimeError):
        lh.buffer_table(torch.zeros(8, dtype=torch.float16, device=DEV), [8])
    with pytest.raises(RuntimeError):
        lh.buffer_table(torch.zeros(8), [8])
    with pytest.raises(RuntimeError):
        lh.buffer_table(torch.zeros(8, device=DEV), [9])
    w = torch.zeros(4, 4, device=DEV)
    with pytest.raises(RuntimeError, match="not dense"):
        lh.update_table([(w[:, :2], w[:, :2], w[:, :2])])
    with pytest.raises(RuntimeError, match="layout"):
        lh.update_table([(w, w.t(), w)])
    table = lh.buffer_table(torch.zeros(8, device=DEV), [3, 5])
    with pytest.raises(RuntimeError):
        lh.grads(table, 1.0, lh.new_running(3, DEV))
    with pytest.raises(RuntimeError):
        lh.grads(table, 1.0, lh.new_running(2, "cpu"))
    with pytest.raises(RuntimeError):
        lh.updates(table, 1e-3, 1e-8, 1.0, 1.0, lh.new_running(2, DEV))


SG2_YAML = ("exp:\n  trainer: sg2\ngen:\n  generator: sg2_classic\n  discriminator: sg2_classic\n"
            "  disc_regs: [r1]\ndisc_regs_all:\n  r1:\n    r1_gamma: 0.01\nlosses_arch_args:\n  sg2:\n    style_mixing_prob: 0\n"
            "aug:\n  aug: noaug\ndata:\n  dataset: synthetic\n  resolution: 32\n"
            "gens_args:\n  sg2_classic:\n    z_dim: 16\n    w_dim: 16\n    mapping_kwargs:\n      num_layers: 2\n"
            "    synthesis_kwargs:\n      channel_base: 512\n      channel_max: 16\n      num_fp16_res: 0\n      block_kwargs:\n        conv_clamp: 256\n"
            "discs_args:\n  sg2_classic:\n    channel_base: 512\n    channel_max: 16\n    num_fp16_res: 0\n    architecture: orig\n"
            "    epilogue_kwargs:\n      mbstd_group_size: 4\n")
RUN_ARGS = ["gen.batch=8", "gen.batch_gpu=8", "gen.kimg=1", "log.kimg_per_tick=0.016", "log.snap=0", "log.metrics=[]", "log.run_log=on"]


def _launches(argv, iterations):
    _lib.prof_enable(True)
    try:
        _lib.prof_fetch()
        trainer = starter.main(argv, max_iterations=iterations)
        seen = [(_lib.LAYER_HEALTH_VARIANTS[r["dims"][0]], r["dims"]) for r in _lib.prof_fetch() if r["kind"] == "layer_health"]
    finally:
        _lib.prof_enable(False)
    return trainer, seen


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    """three iterations of a tiny sg2 run with the option on -> (run directory, trainer, the layer_health launches of the run)"""
    tmp = tmp_path_factory.mktemp("layer_health")
    (tmp / "cfg.yaml").write_text(SG2_YAML)
    argv = [f"exp.config_dir={tmp}", "exp.config=cfg.yaml", "exp.name=run", f"log.output={tmp / 'logs'}"] + RUN_ARGS
    trainer, seen = _launches(argv + ["log.layer_health=on"], 3)
    return argv, str(tmp / "logs" / "run"), trainer, seen


def test_a_training_run_writes_layers_jsonl(run):
    _, run_dir, trainer, _ = run
    eng = trainer.engine
    assert [p.name for p in eng.phases if not p.idle] == ["Gmain", "Dmain", "Dreg"] and not eng.layer_health_unsupported
    lines = lu.read_layers(os.path.join(run_dir, "layers.jsonl"))
    stats = ru.stats_lines(run_dir)
    assert len(lines) == len(stats) == trainer.cur_tick == 2          # one line per tick: after the first iteration and after the third
    g, d = [n for n, _ in eng.G.named_parameters()], [n for n, _ in eng.D.named_parameters()]
    for tick, line in enumerate(lines):
        lu.check_line(line, tick, {"Gmain": g, "Dmain": d, "Dreg": d})
    assert [lines[0]["phases"][ph]["steps"] for ph in ("Gmain", "Dmain", "Dreg")] == [1, 1, 1]
    assert [lines[1]["phases"][ph]["steps"] for ph in ("Gmain", "Dmain", "Dreg")] == [2, 2, 0]
    assert all(v["grad_rms"] is None for v in lines[1]["phases"]["Dreg"]["params"].values())
    for ph, module in (("Gmain", eng.G), ("Dmain", eng.D), ("Dreg", eng.D)):      # tick 0 closes after exactly one iteration
        params = lines[0]["phases"][ph]["params"]
        n = sum(p.numel() for p in module.parameters())
        assert sum(v["numel"] for v in params.values()) == n
        total = math.sqrt(sum(v["grad_rms"] ** 2 * v["numel"] for v in params.values()))
        norm = stats[0][f"Grad/{ph}/norm"]["mean"]
        print(f"{ph}: n {n}, sqrt of the summed grad_sumsq {total!r}, Grad/{ph}/norm {norm!r}")
        assert norm > 0 and abs(total - norm) <= n * lu.U * norm
        assert sum(v["nonfinite"] for v in params.values()) == stats[0][f"Grad/{ph}/nonfinite"]["mean"]
        ratios = [v["update_ratio"] for v in params.values() if v["update_ratio"] is not None]
        assert len(ratios) >= len(params) // 2 and all(0 < r < float("inf") for r in ratios)
        assert all(v["weight_rms"] >= 0 and v["weight_absmax"] >= 0 for v in params.values())


def test_launches_with_the_option_on_and_off(run):
    """on: one gradient pass and one fold per reducer and phase (Gmain finishes the mapping and the synthesis reducer), one update pass and
    one fold per optimizer step; three iterations run Gmain and Dmain three times and Dreg once.  off: no launch of the kind."""
    argv, _, trainer, seen = run
    kinds = [k for k, _ in seen]
    finishes, opt_steps = 3 * 2 + 3 + 1, 3 + 3 + 1
    assert kinds.count("grads") == finishes and kinds.count("updates") == opt_steps
    assert [dims[3] for k, dims in seen if k == "fold"].count(0) == finishes and [dims[3] for k, dims in seen if k == "fold"].count(1) == opt_steps
    assert all(len(r._buckets) == 1 for r in trainer.engine.dp_modules.values())
    off, seen_off = _launches([a.replace("exp.name=run", "exp.name=plain") for a in argv], 1)
    assert seen_off == [] and not off.engine.layer_health
    assert "layers.jsonl" not in os.listdir(os.path.join(os.path.dirname(run[1]), "plain"))
