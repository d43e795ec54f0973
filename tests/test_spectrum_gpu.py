"""The spectrum kernels (csrc/spectrum.hip) on the device: the exact patterns, the same bits as the op layer's CPU arithmetic on inputs where
every step rounds (the value graph and the order of the float64 chain are the definition), the invariance of the chain
under the cut of a batch, the launch records, and the tool on both devices.  The shapes (B, C, R, P) are the smallest at which padding,
several rows per workgroup, a batch that fills no tile and more than one lane-owned ky can go wrong."""
import numpy as np
import pytest
import torch

import spectrum_util as SU
from exact_util import expect_launch
from style_big_gan_amd import avg_spectra as AS
from style_big_gan_amd.torch_utils.ops import spectrum
from test_calc_metrics_cpu import _run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("R", [16, 64])
def test_exact_patterns(dev, R):
    window, twiddle = SU.pattern_tables(R, dev)
    for name, (image, want) in SU.patterns(R).items():
        acc = torch.zeros([R // 2 + 1, R], dtype=torch.float64, device=dev)
        spectrum.accumulate(acc, torch.from_numpy(image.astype(np.float32))[None, None].to(dev), 1.0, 0.0, window, twiddle)
        assert np.array_equal(acc.cpu().numpy(), want), (name, np.argwhere(acc.cpu().numpy() != want)[:4])


_cpu_results = {}


def _cpu(kind, shape):
    """the CPU path's accumulator of a case, computed once"""
    if (kind, shape) not in _cpu_results:
        images, s, t, window, twiddle, acc = SU.case(kind, *shape)
        _cpu_results[kind, shape] = spectrum.accumulate(acc, images, s, t, window, twiddle)
    return _cpu_results[kind, shape]


@pytest.mark.parametrize("shape", SU.SHAPES)
@pytest.mark.parametrize("kind", ["float", "bytes", "bytes_f32"])
def test_device_equals_cpu_path_bit_for_bit(dev, kind, shape):
    images, s, t, window, twiddle, acc = SU.case(kind, *shape, device=dev)
    assert images.dtype == (torch.uint8 if kind == "bytes" else torch.float32)
    got = spectrum.accumulate(acc, images, s, t, window, twiddle)
    assert got is acc and SU.same_bits(got, _cpu(kind, shape))
    if kind == "bytes_f32":
        assert SU.same_bits(got, _cpu("bytes", shape))


@pytest.mark.parametrize("shape", [(5, 3, 32, 1), (5, 3, 16, 2)])
def test_batch_invariance(dev, shape):
    images, s, t, window, twiddle, acc = SU.case("float", *shape, device=dev)
    start = torch.from_numpy(np.random.RandomState(3).rand(*acc.shape) * 1e-3).to(dev)
    one = spectrum.accumulate(start.clone(), images, s, t, window, twiddle)
    two = spectrum.accumulate(start.clone(), images[:2], s, t, window, twiddle)
    spectrum.accumulate(two, images[2:], s, t, window, twiddle)
    each = spectrum.accumulate(start.clone(), images, s, t, window, twiddle, max_workspace_bytes=1)
    assert SU.same_bits(one, two) and SU.same_bits(one, each)
    assert not SU.same_bits(one, spectrum.accumulate(acc, images, s, t, window, twiddle))         # the starting values are part of the chain
    cpu = spectrum.accumulate(start.cpu().clone(), images.cpu(), s, t, window.cpu(), twiddle.cpu())
    assert SU.same_bits(one, cpu)


def test_launch_records(dev):
    """one rows record and one cols record per piece, dims (variant, BC, R, S)"""
    images, s, t, window, twiddle, acc = SU.case("bytes", 2, 3, 16, 4, device=dev)
    with expect_launch("spectrum", lambda d: d[:4] == (0, 6, 16, 64), "rows of the whole batch") as log:
        with expect_launch("spectrum", lambda d: d[:4] == (1, 6, 16, 64), "cols of the whole batch"):
            spectrum.accumulate(acc, images, s, t, window, twiddle)
    assert sorted(r["dims"][:4] for r in log if r["kind"] == "spectrum") == [(0, 6, 16, 64), (1, 6, 16, 64)]
    per = 8 * 33 * 16                                           # bytes of one image-channel's intermediate
    with expect_launch("spectrum", lambda d: d[:4] == (0, 4, 16, 64), "rows of a piece of four") as log:
        with expect_launch("spectrum", lambda d: d[:4] == (1, 2, 16, 64), "cols of the last piece"):
            spectrum.accumulate(acc, images, s, t, window, twiddle, max_workspace_bytes=4 * per + 7)
    assert [r["dims"][:4] for r in log if r["kind"] == "spectrum"] == [(0, 4, 16, 64), (1, 4, 16, 64), (0, 2, 16, 64), (1, 2, 16, 64)]


def test_tool_on_the_device_equals_the_cpu_run(dev, tmp_path, monkeypatch):
    _, overrides, snap, _ = _run(tmp_path)
    data, items = SU.tool_dataset(tmp_path)
    yy, xx = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    bank = (items.astype(np.int64) + (8 * (-1) ** (xx + yy))[None, None]).astype(np.uint8)
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", lambda config, state, device: SU.OrderedGenerator(bank).to(device))
    runs = {}
    for device in ("cuda", "cpu"):
        out = tmp_path / device
        AS.run_avg_spectra(overrides + [f"--data={data}", f"--device={device}", "--batch=7", "--interp=2", f"--outdir={out}", f"--snapshot={snap}", "--num=24"])
        runs[device] = {name: np.load(out / f"spectrum_{name}.npz") for name in ("real", "gen")}
    for name in ("real", "gen"):
        assert np.array_equal(runs["cuda"][name]["spectrum"], runs["cpu"][name]["spectrum"]), name
        assert float(runs["cuda"][name]["mean"]) == float(runs["cpu"][name]["mean"]) and float(runs["cuda"][name]["std"]) == float(runs["cpu"][name]["std"])
    assert open(tmp_path / "cuda" / "spectrum.json").read() == open(tmp_path / "cpu" / "spectrum.json").read()
    assert open(tmp_path / "cuda" / "spectrum.png", "rb").read() == open(tmp_path / "cpu" / "spectrum.png", "rb").read()


@pytest.mark.parametrize("shape", [(1, 1, 512, 1), (1, 2, 256, 4), (1, 1, 512, 4)])
def test_every_row_plan_bit_for_bit(dev, shape):
    """the row pass stages 16 lines side by side up to S = 256, then 8 (S = 512), 4 (1024), 2 (2048), and from S = 1024 on makes two passes
    with the first one's kept half parked in LDS; the column pass owns 2 .. 8 accumulator entries per lane here"""
    images, s, t, window, twiddle, acc = SU.case("float", *shape, device=dev)
    got = spectrum.accumulate(acc, images, s, t, window, twiddle)
    assert SU.same_bits(got, _cpu("float", shape))


def test_largest_side_under_the_derived_bound(dev):
    """R = 1024, P = 4: one line per workgroup in the row pass, 16 accumulator entries per lane in the column pass; against numpy's float64
    transform under the bound of the CPU accuracy test (the CPU path would take many seconds here)"""
    R, P, S = 1024, 4, 4096
    images, s, t, window, twiddle, acc = SU.case("bytes", 1, 1, R, P, device=dev)
    spectrum.accumulate(acc, images, s, t, window, twiddle)
    power = np.abs(SU.restatement(images.cpu().numpy(), s, t, window.cpu().numpy(), S)[0, 0]) ** 2
    tau = SU.tau(S)
    err = float(np.abs(acc.cpu().numpy() - power).sum())
    print(f"S=4096: sum |acc - ref| {err:.3e}, bound {(2 * tau + tau * tau) * power.sum():.3e}")
    assert err <= (2 * tau + tau * tau) * power.sum() * (1 + 2.0 ** -52)


@pytest.mark.parametrize("R", [256, 1024])
def test_exact_patterns_of_the_larger_row_plans(dev, R):
    window, twiddle = SU.pattern_tables(R, dev)
    for name, (image, want) in SU.patterns(R).items():
        acc = torch.zeros([R // 2 + 1, R], dtype=torch.float64, device=dev)
        spectrum.accumulate(acc, torch.from_numpy(image.astype(np.float32))[None, None].to(dev), 1.0, 0.0, window, twiddle)
        assert np.array_equal(acc.cpu().numpy(), want), (name, np.argwhere(acc.cpu().numpy() != want)[:4])
