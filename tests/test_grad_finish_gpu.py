"""The fused gradient-finish kernel (csrc/grad_finish.hip) and its use by GradReducer.finish(): sanitised values bit for bit against
torch.nan_to_num on the same device, statistics exactly against float64 numpy on data whose every partial sum is an exact float64,
the worst-case bound of a float64 sum on random data, run-to-run identity, parity with the CPU path of the reducer, the launch log."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import _lib
from style_big_gan_amd.parallel import GradReducer
from style_big_gan_amd.torch_utils.ops import grad_finish

pytestmark = pytest.mark.gpu

INF = float("inf")
NONFINITE = [float("nan"), INF, -INF]
SPECIALS = NONFINITE + [-0.0, 1e-40, -3e-42, 3e30, -3e30]       # ... the negative zero, two subnormals, finite values whose fp32 square overflows


def chunk_len():
    """the chunk length of small buffers, found from the size query: the largest n that one record covers"""
    lo, hi = 1, 2
    while grad_finish.records(hi) == 1:
        lo, hi = hi, hi * 2
    while hi - lo > 1:
        mid = (lo + hi) // 2
        lo, hi = (mid, hi) if grad_finish.records(mid) == 1 else (lo, mid)
    assert grad_finish.records(lo) == 1 and grad_finish.records(lo + 1) == 2 and grad_finish.records(3 * lo + 7) == 4
    return lo


def sizes():
    c = chunk_len()
    return [1, 3, 4, 5, 63, 64, 65, 255, 256, 257, c - 1, c, c + 1, 3 * c + 7]


def make_data(n, c, magnitude, pool, seed, every=7):
    """integers in [-magnitude, magnitude] with the special values scattered in: at random places and at the first element, the last
    element, the first element of every chunk, the element before it and the scalar tail (the n % 4 elements behind the last vector)"""
    rng = np.random.RandomState(seed)
    x = rng.randint(-magnitude, magnitude + 1, size=n).astype(np.float32)
    where = set(rng.randint(0, n, size=max(n // every, 1)).tolist()) | {0, n - 1} | set(range(n - n % 4, n))
    where |= {i for k in range(c, n, c) for i in (k - 1, k)}
    for j, i in enumerate(sorted(where)):
        x[i] = np.float32(pool[(j + seed) % len(pool)])
    return x


def run_kernel(x, scale, dev):
    """-> (sanitised buffer, float64 [3] health), both on the device"""
    flat = torch.from_numpy(x).to(dev)
    parts = torch.full([grad_finish.records(flat.numel()), 3], -1.0, dtype=torch.float64, device=dev)
    grad_finish.sweep(flat, scale, parts)
    return flat, grad_finish.merge(parts)


def numpy_health(x, scale):
    with np.errstate(all="ignore"):
        y = x * np.float32(scale) if scale != 1.0 else x
    z = np.nan_to_num(y, nan=0.0, posinf=1e5, neginf=-1e5).astype(np.float32).astype(np.float64)
    return np.array([float((~np.isfinite(y)).sum()), (z * z).sum(), np.abs(z).max()], dtype=np.float64)


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_sanitised_values_are_exact(dev, scale):
    c = chunk_len()
    for n in sizes():
        x = make_data(n, c, magnitude=50, pool=SPECIALS, seed=n % 11)
        flat, _ = run_kernel(x, scale, dev)
        ref = torch.nan_to_num(torch.from_numpy(x).to(dev).mul(scale), nan=0, posinf=1e5, neginf=-1e5)
        assert torch.equal(flat.view(torch.int32), ref.view(torch.int32)), f"n={n}: sanitised bits differ from torch.nan_to_num"


@pytest.mark.parametrize("scale", [1.0, 0.5])
def test_statistics_are_exact(dev, scale):
    """integers up to 1000 (halves under the scale 0.5) and NaN / +-inf (0 and +-1e5 afterwards): every square and every partial sum is an
    exact float64, so the order is irrelevant"""
    c = chunk_len()
    for n in sizes():
        x = make_data(n, c, magnitude=1000, pool=NONFINITE, seed=n % 13)
        _, health = run_kernel(x, scale, dev)
        got, want = health.cpu().numpy(), numpy_health(x, scale)
        print(f"n={n} scale={scale}: got {got.tolist()} want {want.tolist()}")
        assert np.array_equal(got, want), f"n={n}: {got} != {want}"


def test_chunks_of_several_batches(dev):
    """above 2^24 elements the chunks grow instead of their number: a workgroup takes several batches of loads"""
    n = (1 << 24) + 5
    c = chunk_len()
    assert grad_finish.records(1 << 24) == (1 << 24) // c and grad_finish.records(n) == -(-n // (2 * c))
    x = make_data(n, 2 * c, magnitude=1000, pool=NONFINITE, seed=2, every=4096)       # few enough 1e5^2 for every sum to stay below 2^53 quarters
    flat, health = run_kernel(x, 0.5, dev)
    ref = torch.nan_to_num(torch.from_numpy(x).to(dev).mul(0.5), nan=0, posinf=1e5, neginf=-1e5)
    assert torch.equal(flat.view(torch.int32), ref.view(torch.int32))
    assert np.array_equal(health.cpu().numpy(), numpy_health(x, 0.5))


def test_random_normal_data(dev):
    for n in sizes():
        x = (np.random.RandomState(n % 17).standard_normal(n) * 3).astype(np.float32)
        flat_a, a = run_kernel(x, 1.0, dev)
        flat_b, b = run_kernel(x, 1.0, dev)
        want = numpy_health(x, 1.0)
        got = a.cpu().numpy()
        bound = n * 2.0 ** -52 * want[1]
        print(f"n={n}: sumsq {got[1]!r} numpy {want[1]!r} |diff| {abs(got[1] - want[1]):.3e} bound {bound:.3e}")
        assert got[0] == 0 and got[2] == want[2] and abs(got[1] - want[1]) <= bound
        assert torch.equal(a.view(torch.int64), b.view(torch.int64)) and torch.equal(flat_a.view(torch.int32), flat_b.view(torch.int32))
        assert torch.equal(flat_a.cpu(), torch.from_numpy(x))


def test_bad_buffers_are_errors(dev):
    parts = torch.zeros([4, 3], dtype=torch.float64, device=dev)
    whole = torch.zeros([64], device=dev)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        grad_finish.sweep(whole[1:], 1.0, parts)
    with pytest.raises(RuntimeError, match="float32"):
        grad_finish.sweep(whole.double(), 1.0, parts)
    with pytest.raises(RuntimeError, match="float32"):
        grad_finish.sweep(whole.half(), 1.0, parts)
    with pytest.raises(RuntimeError, match="partials hold"):
        grad_finish.sweep(torch.zeros([chunk_len() * 5], device=dev), 1.0, parts)
    with pytest.raises(RuntimeError, match="CPU|cpu"):
        grad_finish.sweep(torch.zeros([64]), 1.0, parts)
    assert grad_finish.records(0) == 0 and grad_finish.merge(parts[:0]).tolist() == [0.0, 0.0, 0.0]


def _three_layers(dev):
    torch.manual_seed(5)
    return torch.nn.Sequential(torch.nn.Linear(41, 49, bias=False), torch.nn.Linear(49, 31, bias=False), torch.nn.Linear(31, 7, bias=False)).to(dev)


def _write_grads(reducer, seed=9):
    """the same gradients, with non-finite values injected, into every bucket of `reducer` (generated on the host, copied to its device)"""
    rng = np.random.RandomState(seed)
    for b in reducer._buckets:
        g = (rng.standard_normal(b.flat.numel()) * 2).astype(np.float32)
        g[rng.randint(0, g.size, size=5)] = np.array([np.nan, np.inf, -np.inf, np.nan, 3e30], dtype=np.float32)
        g[-1] = np.inf
        b.flat.copy_(torch.from_numpy(g))


def test_grad_reducer_parity_with_the_cpu_path(dev):
    gpu = GradReducer(_three_layers(dev), bucket_bytes=4096)
    cpu = GradReducer(_three_layers("cpu"), bucket_bytes=4096)
    assert len(gpu._buckets) == len(cpu._buckets) == 3
    gpu.health = cpu.health = True
    _write_grads(gpu); _write_grads(cpu)
    preset = 7
    gpu.nonfinite = torch.full([], preset, dtype=torch.int64, device=dev)
    cpu.nonfinite = torch.full([], preset, dtype=torch.int64)
    gpu.finish(); cpu.finish()
    for bg, bc in zip(gpu._buckets, cpu._buckets):
        assert torch.equal(bg.flat.cpu().view(torch.int32), bc.flat.view(torch.int32))
    for pg, pc in zip(gpu.module.parameters(), cpu.module.parameters()):
        assert torch.equal(pg.grad.cpu().view(torch.int32), pc.grad.view(torch.int32)) and bool(torch.isfinite(pg.grad).all())
    hg, hc = gpu.last_health.cpu(), cpu.last_health
    n = sum(b.flat.numel() for b in cpu._buckets)
    print("health gpu", hg.tolist(), "cpu", hc.tolist())
    assert gpu.last_health.is_cuda and hg.dtype == torch.float64 and hg.shape == (3,)
    assert hg[0] == hc[0] and hg[0] >= 3 and hg[2] == hc[2] and abs(float(hg[1] - hc[1])) <= n * 2.0 ** -52 * float(hc[1])
    assert int(gpu.nonfinite) == preset + int(hg[0]) and int(cpu.nonfinite) == preset + int(hc[0])


def test_launch_log_shows_one_sweep_per_bucket_and_one_merge(dev):
    red = GradReducer(_three_layers(dev), bucket_bytes=4096)
    red.health = True
    _write_grads(red)
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        _lib.prof_fetch()
        red.finish()
        recs = [r for r in _lib.prof_fetch() if r["kind"] == "grad_finish"]
    finally:
        _lib.prof_enable(False)
    kinds = [_lib.GRAD_FINISH_VARIANTS[r["dims"][0]] for r in recs]
    assert kinds == ["sweep"] * 3 + ["merge"]
    assert [r["dims"][2] for r in recs[:3]] == [b.flat.numel() for b in red._buckets] and recs[3]["dims"][1] == 3
    assert [r["bytes"] for r in recs[:3]] == [8.0 * b.flat.numel() for b in red._buckets]


class _Exchanged:
    """an exchange that has completed: what `_Bucket.work` holds while an all-reduce is in flight"""

    def wait(self):
        pass


def test_the_scale_of_an_exchange_in_flight_is_folded_into_the_sweep(dev):
    """two ranks, every bucket still on the wire at finish(): the sweep multiplies by 1/world itself, and leaves the bits of the torch
    path's mul_ followed by nan_to_num"""
    fused, plain = GradReducer(_three_layers(dev), bucket_bytes=4096), GradReducer(_three_layers(dev), bucket_bytes=4096)
    fused.health = True
    for red in (fused, plain):
        red.world_size = 3              # no process group is touched: the stub stands for the exchange
        _write_grads(red)
        for b in red._buckets:
            b.work = _Exchanged()
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        _lib.prof_fetch()
        fused.finish(); plain.finish()
        recs = [r for r in _lib.prof_fetch() if r["kind"] == "grad_finish"]
    finally:
        _lib.prof_enable(False)
    assert [(r["dims"][0], r["dims"][3]) for r in recs] == [(0, 1)] * 3 + [(1, 0)]         # three scaled sweeps and the merge, all from `fused`
    assert plain.last_health is None and all(b.work is None for b in fused._buckets + plain._buckets)
    for bf, bp in zip(fused._buckets, plain._buckets):
        assert torch.equal(bf.flat.view(torch.int32), bp.flat.view(torch.int32))
    z = torch.cat([b.flat for b in plain._buckets]).double()
    h = fused.last_health
    assert h[0] == 14 and h[2] == z.abs().max() and abs(float(h[1] - z.square().sum())) <= z.numel() * 2.0 ** -52 * float(z.square().sum())


def test_without_health_finish_is_the_torch_path(dev):
    red = GradReducer(_three_layers(dev), bucket_bytes=4096)
    _write_grads(red)
    want = [torch.nan_to_num(b.flat.clone(), nan=0, posinf=1e5, neginf=-1e5) for b in red._buckets]
    red.nonfinite = torch.zeros([], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    try:
        _lib.prof_fetch()
        red.finish()
        recs = [r for r in _lib.prof_fetch() if r["kind"] == "grad_finish"]
    finally:
        _lib.prof_enable(False)
    assert recs == [] and red.last_health is None and int(red.nonfinite) == 14
    assert all(torch.equal(b.flat.view(torch.int32), w.view(torch.int32)) for b, w in zip(red._buckets, want))
