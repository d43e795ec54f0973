"""CPU: bench.py's own rank launcher (`python bench.py --gpus N` without torchrun) -- the counterpart of the reference's
starter.py:26-30 (one process per GPU).  The ranks rendezvous over gloo here (SBG_DIST_BACKEND=gloo), count themselves with an
all-reduce and rank 0 prints the JSON; with the RCCL backend and fewer devices than ranks the launcher must fail loudly instead
of printing a one-GPU number."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def _env(**kw):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT", "MASTER_ADDR")}
    env.update(kw)
    return env


def test_launcher_starts_n_ranks_over_gloo():
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rendezvous-only"], env=_env(SBG_DIST_BACKEND="gloo"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, "exactly one JSON line (rank 0's)"
    rec = json.loads(lines[0])
    assert rec == dict(ranks_seen=2, n_gpus=2, backend="gloo")


def test_launcher_refuses_more_ranks_than_devices():
    import torch
    if torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("needs a machine with fewer than two devices")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2"], env=_env(SBG_DIST_BACKEND="nccl"), capture_output=True, text=True, timeout=300)
    assert r.returncode != 0
    assert "2 ranks need 2 devices" in r.stderr
    assert not [l for l in r.stdout.splitlines() if l.startswith("{")], "no value may be printed"


def test_launcher_fails_when_a_rank_fails():
    # WORLD_SIZE is what the ranks check --gpus against: a launcher environment that disagrees makes every rank exit non-zero
    r = subprocess.run([sys.executable, BENCH, "--gpus", "2", "--rendezvous-only"], env=_env(SBG_DIST_BACKEND="gloo", WORLD_SIZE="3", RANK="0"),
                       capture_output=True, text=True, timeout=300)
    assert r.returncode != 0 and "WORLD_SIZE=3 but --gpus 2" in r.stderr
    sys.path.insert(0, ROOT)
    import bench
    old = dict(os.environ)
    try:
        os.environ["SBG_DIST_BACKEND"] = "gloo"
        assert bench.launch_ranks(2, ["--gpus", "2", "--workload", "no_such_workload"]) != 0      # argparse rejects it in every child
    finally:
        os.environ.clear(); os.environ.update(old)


def test_host_cores_is_bounded_by_affinity():
    sys.path.insert(0, ROOT)
    import bench
    n = bench.host_cores()
    assert 1 <= n <= len(os.sched_getaffinity(0))


def test_dump_outputs_writes_the_gradients_of_the_last_step(tmp_path, monkeypatch):
    """--dump-outputs: one float32 file per gradient reducer holding what the step computed -- zeros before any step, after one step
    the gradients autograd left on the parameters -- and, above DUMP_MAX_ELEMS values, a sample that is the same in every run"""
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    import bench
    from style_big_gan_amd.train_parts import trainers
    eng = trainers.StepEngine("cpu", generator="cnn32_dcgan", discriminator="cnn32_dcgan", gen_kwargs=dict(z_dim=8, c_dim=0, img_resolution=32),
                              disc_kwargs=dict(), loss_arch="base", loss="wasserstein", gen_regs=[], dis_regs=[("grad_pen", dict(alpha=10.))],
                              optim_gen=("adam", dict(lr=1e-3, betas=[0.5, 0.9])), optim_disc=("adam", dict(lr=1e-3, betas=[0.5, 0.9])),
                              g_reg_interval=0, d_reg_interval=0, batch=4, batch_gpu=2, ema_kimg=0.01, seed=3)
    names = sorted(eng.dp_modules)
    assert names == ["D", "G"]
    n_params = {k: sum(p.numel() for p in eng.dp_modules[k].module.parameters()) for k in names}
    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", max(n_params.values()))
    bench.dump_outputs(eng, str(tmp_path / "before"))
    for k in names:
        assert not np.load(tmp_path / "before" / f"grad_{k}.npy").any(), "a not-stepped engine holds no gradient"

    torch.manual_seed(50)
    eng.train_iteration(torch.rand(4, 3, 32, 32) * 2 - 1, None)
    bench.dump_outputs(eng, str(tmp_path / "after"))
    grads = {}
    for k in names:
        got = np.load(tmp_path / "after" / f"grad_{k}.npy")
        ref = np.concatenate([p.grad.detach().reshape(-1).numpy() for p in eng.dp_modules[k].module.parameters()])
        assert got.dtype == np.float32 and got.shape == (n_params[k],) and np.isfinite(got).all(), k
        assert np.count_nonzero(got) > got.size // 2, k
        assert np.array_equal(np.sort(got), np.sort(ref)), k        # the same values, in bucket order
        grads[k] = got

    monkeypatch.setattr(bench, "DUMP_MAX_ELEMS", 1000)
    bench.dump_outputs(eng, str(tmp_path / "a"))
    bench.dump_outputs(eng, str(tmp_path / "b"))
    for k in names:
        a, b = np.load(tmp_path / "a" / f"grad_{k}.npy"), np.load(tmp_path / "b" / f"grad_{k}.npy")
        assert a.shape == (1000,) and np.array_equal(a, b) and np.isin(a, grads[k]).all(), k
