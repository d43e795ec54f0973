"""torch_utils/ops/act_stats.py on the CPU: its numpy path against the independent restatement of tests/act_stats_util.py bit for bit, the fold's
independence of the batching, the n_peak merge, `derive`, and the refusals."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E402,F401
from style_big_gan_amd.torch_utils.ops import act_stats as A  # noqa: E402
import act_stats_util as U  # noqa: E402

# every dtype and layout; the plane sizes with a partial lane round (255, 257), one full round (256), several rounds (1089) and the small planes
CPU_CASES = [(d, l, n, c, p) for d in U.DTYPES for l in U.LAYOUTS for (n, c, p) in ((1, 3, 1), (5, 9, 1), (5, 7, 16), (1, 8, 255), (5, 3, 256),
                                                                                     (1, 9, 257), (5, 8, 1089))
             if (l == "2d") == (p == 1) or (l != "2d" and p == 1 and c == 9)]


@pytest.mark.parametrize("dtype,layout,n,c,p", CPU_CASES)
def test_cpu_path_equals_the_restatement(dtype, layout, n, c, p):
    x = U.build_case(dtype, layout, n, c, p, seed=len(layout) + p)
    counts, values = A.planes(x)
    want_counts, want_values = U.restate_planes(x)
    assert counts.dtype == torch.int64 and values.dtype == torch.float64
    assert U.same_bits(counts.numpy(), want_counts), U.first_difference(counts.numpy(), want_counts)
    assert U.same_bits(values.numpy(), want_values), U.first_difference(values.numpy(), want_values)


def test_the_planted_values_land_where_the_record_says():
    x = torch.tensor([0.0, -0.0, 2.0 ** -140, 2.0 ** -33, 2.0 ** -32, 2.0 ** -14, 2.0 ** 16, 2.0 ** 31, 2.0 ** 32, float("inf"), float("-inf"), float("nan"),
                      -3.0, 3.0, 1.5, 1.0], dtype=torch.float32).reshape(1, 1, 4, 4)
    counts, values = A.planes(x)
    k, v = counts[0, 0].numpy(), values[0, 0].numpy()
    assert list(k[:6]) == [16, 2, 1, 1, 1, 1]                                   # n, zeros, NaN, +inf, -inf, and the peak 2^32 once
    hist = {b - 32: int(h) for b, h in enumerate(k[6:]) if h}
    assert hist == {-32: 3, -14: 1, 0: 2, 1: 2, 16: 1, 31: 2}                   # the subnormal, 2^-33 and 2^-32 in the lowest bin; 2^31 and 2^32 in the top one
    assert v[2] == -3.0 and v[3] == 2.0 ** 32
    kept = [0.0, 0.0, 2.0 ** -140, 2.0 ** -33, 2.0 ** -32, 2.0 ** -14, 2.0 ** 16, 2.0 ** 31, 2.0 ** 32, 0.0, 0.0, 0.0, -3.0, 3.0, 1.5, 1.0]
    assert v[0] == U._lane_sum(kept) and v[1] == U._lane_sum([e * e for e in kept])


def test_bin_edges_one_by_one():
    for value, e in [(2.0 ** -140, -32), (2.0 ** -33, -32), (2.0 ** -32, -32), (2.0 ** -31, -31), (2.0 ** -14, -14), (1.0, 0), (1.999, 0), (2.0 ** 16, 16),
                     (65504.0, 15), (2.0 ** 31, 31), (2.0 ** 32, 31), (-(2.0 ** 100), 31)]:
        counts, _ = A.planes(torch.tensor([[value]], dtype=torch.float32))
        hist = counts[0, 0, 6:].numpy()
        assert hist.sum() == 1 and hist[e + 32] == 1, (value, e)


def _records(n=5, c=9, p=257, seed=3):
    x = U.build_case("bf16", "nchw", n, c, p, seed=seed)
    return A.planes(x)


def test_folding_does_not_depend_on_the_batching():
    counts, values = _records()
    runs = []
    for split in ([5], [2, 3], [1, 1, 1, 1, 1]):
        rc, rv = A.empty(9)
        lo = 0
        for size in split:
            A.fold(counts[lo:lo + size].contiguous(), values[lo:lo + size].contiguous(), rc, rv)
            lo += size
        runs.append((rc.numpy().copy(), rv.numpy().copy()))
    for rc, rv in runs[1:]:
        assert U.same_bits(rc, runs[0][0]) and U.same_bits(rv, runs[0][1])
    # and the running record is what the definition says: counts add, sums add in sample order, min / max combine
    rc, rv = runs[0]
    k, v = counts.numpy(), values.numpy()
    assert (rc[:, [0, 1, 2, 3, 4]] == k[:, :, [0, 1, 2, 3, 4]].sum(axis=0)).all() and (rc[:, 6:] == k[:, :, 6:].sum(axis=0)).all()
    s = np.zeros(9)
    for i in range(5):
        s = s + v[i, :, 0]
    assert U.same_bits(rv[:, 0], s)
    assert U.same_bits(rv[:, 2], v[:, :, 2].min(axis=0)) and U.same_bits(rv[:, 3], v[:, :, 3].max(axis=0))


def _record(n_peak, mn, mx):
    counts = torch.zeros([1, 1, A.COUNTS], dtype=torch.int64)
    values = torch.zeros([1, 1, A.VALUES], dtype=torch.float64)
    counts[0, 0, A.N_], counts[0, 0, A.N_PEAK] = 8, n_peak
    values[0, 0, A.MIN], values[0, 0, A.MAX] = mn, mx
    return counts, values


def test_n_peak_merge_larger_equal_smaller_and_empty():
    rc, rv = A.empty(1)
    A.fold(*_record(3, -2.0, 4.0), rc, rv)
    assert int(rc[0, A.N_PEAK]) == 3                                            # the first record against the empty one
    A.fold(*_record(2, -8.0, 1.0), rc, rv)                                      # a larger peak (negative): its count replaces
    assert int(rc[0, A.N_PEAK]) == 2 and float(rv[0, A.MIN]) == -8.0 and float(rv[0, A.MAX]) == 4.0
    A.fold(*_record(5, -1.0, 8.0), rc, rv)                                      # an equal peak: the counts add
    assert int(rc[0, A.N_PEAK]) == 7
    A.fold(*_record(9, -3.0, 3.0), rc, rv)                                      # a smaller peak: nothing changes
    assert int(rc[0, A.N_PEAK]) == 7
    A.fold(*_record(0, float("inf"), float("-inf")), rc, rv)                    # a plane without a finite element
    assert int(rc[0, A.N_PEAK]) == 7 and int(rc[0, A.N_]) == 40
    rc, rv = A.empty(1)
    A.fold(*_record(0, float("inf"), float("-inf")), rc, rv)
    assert int(rc[0, A.N_PEAK]) == 0 and float(rv[0, A.MIN]) == float("inf")


def test_derive():
    x = torch.zeros([4, 3, 8, 8], dtype=torch.float16)
    x[:, 0] = torch.randn(4, 8, 8).clamp(-1, 1) * 256                           # clamped: many elements on +-256
    x[:, 2] = 2.0 ** -16                                                        # an fp16 subnormal everywhere; channel 1 is dead
    x[0, 0, 0, 0] = float("inf")
    rc, rv = A.empty(3)
    A.fold(*A.planes(x), rc, rv)
    d = A.derive(rc, rv)
    assert d["dead_channels"] == [1] and d["nonfinite"] == 1 and d["n"] == 4 * 3 * 64
    assert d["absmax"] == 256.0 and d["fp16_headroom_bits"] == pytest.approx(np.log2(65504 / 256))
    finite = 4 * 3 * 64 - 1
    assert d["fp16_subnormal_share"] == pytest.approx(4 * 64 / finite) and d["fp16_overflow_share"] == 0 and d["zero_share"] == pytest.approx(4 * 64 / finite)
    on_peak = int((x[:, 0].abs() == 256).sum())
    assert on_peak > 10 and d["peak_share"] == pytest.approx(on_peak / finite)
    v = x.double()
    v[0, 0, 0, 0] = 0
    assert d["rms"] == pytest.approx(float(((v * v).sum() / finite).sqrt()), rel=1e-12)
    assert d["channels"]["rms"][2] == pytest.approx(2.0 ** -16) and d["channel_rms_spread"] > 1e6
    empty = A.derive(*A.empty(2))
    assert empty["absmax"] is None and empty["rms"] is None and empty["dead_channels"] == []


def test_refusals():
    with pytest.raises(RuntimeError, match="fp16, bf16 or fp32.*int64"):
        A.planes(torch.zeros([2, 3, 4, 4], dtype=torch.int64))
    with pytest.raises(RuntimeError, match=r"rank 2 .* or 4.*\(2, 3, 4\)"):
        A.planes(torch.zeros([2, 3, 4]))
    with pytest.raises(RuntimeError, match=r"overlap.*strides \(0, 16, 4, 1\)"):
        A.planes(torch.zeros([1, 3, 4, 4]).expand(2, 3, 4, 4))
    with pytest.raises(RuntimeError, match="one strided run"):
        A.planes(torch.zeros([2, 3, 4, 8])[:, :, :, :4])                        # rows with a gap: the pixels are no single run
    with pytest.raises(RuntimeError, match="overlap"):
        A.planes(torch.as_strided(torch.zeros([64]), (2, 3, 2, 2), (4, 2, 2, 1)))
    counts, values = _records(n=1, c=3, p=16)
    rc, rv = A.empty(3)
    with pytest.raises(RuntimeError, match="one device"):
        A.fold(counts, values, rc.to("meta"), rv)
    with pytest.raises(RuntimeError, match="run_counts must be a dense"):
        A.fold(counts, values, A.empty(4)[0], rv)
    with pytest.raises(RuntimeError, match="values must be a dense"):
        A.fold(counts, values.float(), rc, rv)


def test_the_abi_and_the_host_side_of_the_library():
    from style_big_gan_amd import _lib
    header = open(os.path.join(ROOT, "include", "sbg_hip.h")).read()
    declared = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()                                                           # every symbol resolves, or the load fails
    for name in ("sbg_act_stats_path", "sbg_act_stats_planes", "sbg_act_stats_fold"):
        assert f" {name}(" in header and name in declared and hasattr(lib, name)
    assert "SBG_K_ACT_STATS = 34" in header and _lib.KERNEL_KINDS[34] == "act_stats" and _lib.ACT_STATS_VARIANTS == {0: "planes", 1: "fold"}
    assert f"#define SBG_ACT_STATS_COUNTS {A.COUNTS}" in header and f"#define SBG_ACT_STATS_VALUES {A.VALUES}" in header
    # the mapping is decided on the host from the shape, the strides and the base address alone: (dtype, N, C, P, sn, sc, sp, base) -> mapping
    bf, f32 = _lib.SBG_BF16, _lib.SBG_F32
    for args, name in [((bf, 16, 128, 65536, 128 * 65536, 65536, 1, 4096), "staged"), ((bf, 16, 128, 65536, 128 * 65536, 65536, 1, 4098), "staged"),
                       ((bf, 16, 128, 65536, 128 * 65536, 1, 128, 4096), "cminor"), ((bf, 16, 128, 65536, 128 * 65536, 1, 128, 4104), "strided"),
                       ((bf, 16, 12, 65536, 12 * 65536, 1, 12, 4096), "strided"), ((f32, 16, 12, 65536, 12 * 65536, 1, 12, 4096), "cminor"),
                       ((bf, 2, 16, 65, 24 * 65, 1, 24, 4096), "cminor"), ((bf, 2, 16, 65, 20 * 65, 1, 20, 4096), "strided"),
                       ((bf, 16, 512, 16, 8192, 16, 1, 4096), "group"), ((bf, 16, 512, 64, 512 * 64, 1, 512, 4096), "group"), ((bf, 7, 33, 1, 33, 1, 0, 4096), "group")]:
        dtype, n, c, p, sn, sc, sp, base = args
        assert _lib.ACT_STATS_PATHS[lib.sbg_act_stats_path(base, dtype, n, c, p, sn, sc, sp)] == name, args
    for bad in ((7, 1, 1, 1, 0, 0, 0), (bf, 0, 1, 1, 0, 0, 0), (bf, 1, 1, 1 << 31, 0, 0, 1), (bf, 2, 1, 4, 0, 0, 1), (bf, 1 << 20, 1 << 12, 1, 1 << 12, 1, 0)):
        assert lib.sbg_act_stats_path(4096, *bad) == -1, bad
