"""The act_stats kernels on the device: `planes` and `fold` equal the op's CPU path bit for bit over every dtype, layout, plane size, channel count
and batch of tests/act_stats_util.py (the smallest shapes with a partial lane round, a partial channel vector, several rounds per lane and several
planes per workgroup; zeros of both signs, subnormals, bin edges, non-finite values, all-zero, all-NaN, clamped and negative-peak planes planted),
the mapping each layout takes, the launch records, and refusals that launch nothing."""
import pytest
import torch

import act_stats_util as U
from style_big_gan_amd import _lib
from style_big_gan_amd.torch_utils.ops import act_stats as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def on_device(x, dev):
    """the same view of a copy of x's whole storage on the device: shape, strides and the offset into the allocation are kept"""
    elements = x.untyped_storage().nbytes() // x.element_size()
    flat = torch.as_strided(x, (elements,), (1,), 0).to(dev)
    return torch.as_strided(flat, tuple(x.shape), x.stride(), x.storage_offset())


def _check(x, dev):
    xd = on_device(x, dev)
    assert xd.stride() == x.stride() and xd.shape == x.shape
    want_counts, want_values = A.planes(x)
    counts, values = A.planes(xd)
    assert counts.device == xd.device and counts.dtype == torch.int64 and values.dtype == torch.float64
    what = (str(x.dtype), tuple(x.shape), x.stride(), x.storage_offset())
    assert U.same_bits(counts.cpu().numpy(), want_counts.numpy()), (what, U.first_difference(counts.cpu().numpy(), want_counts.numpy()))
    assert U.same_bits(values.cpu().numpy(), want_values.numpy()), (what, U.first_difference(values.cpu().numpy(), want_values.numpy()))
    return xd, counts, values, want_counts, want_values


@pytest.mark.parametrize("layout", U.LAYOUTS)
@pytest.mark.parametrize("dtype", list(U.DTYPES))
def test_planes_and_fold_equal_the_cpu_path(dev, dtype, layout):
    taken = set()
    for p in U.PLANE_SHAPES:
        if layout == "2d" and p != 1:
            continue
        for c in U.CHANNELS:
            for n in U.BATCHES:
                x = U.build_case(dtype, layout, n, c, p, seed=c + n)
                xd, counts, values, want_counts, want_values = _check(x, dev)
                taken.add(A.path(xd))
                if layout == "offset":
                    assert xd.data_ptr() % 16 != 0
                rc, rv = A.empty(c, dev)
                wc, wv = A.empty(c)
                for lo, hi in ((0, 1), (1, x.shape[0])):                        # two folds into one running record
                    if hi > lo:
                        A.fold(counts[lo:hi].contiguous(), values[lo:hi].contiguous(), rc, rv)
                        A.fold(want_counts[lo:hi].contiguous(), want_values[lo:hi].contiguous(), wc, wv)
                assert U.same_bits(rc.cpu().numpy(), wc.numpy()) and U.same_bits(rv.cpu().numpy(), wv.numpy()), (dtype, layout, n, c, p)
    expected = {"nchw": {"group", "staged"}, "slice": {"group", "staged"}, "offset": {"group", "staged"}, "2d": {"group"},
                "channels_last": {"group", "staged", "cminor", "strided"}}[layout]      # C = 1 is dense along P; 8 and 72 fill whole channel vectors
    assert taken == expected, taken


def test_the_mapping_follows_the_header(dev):
    bf = torch.bfloat16
    cl = torch.channels_last
    cases = [(torch.zeros([2, 16, 32, 32], dtype=bf, device=dev), "staged"),
             (torch.zeros([2, 16, 32, 32], dtype=bf, device=dev).contiguous(memory_format=cl), "cminor"),
             (torch.zeros([2, 12, 32, 32], dtype=bf, device=dev).contiguous(memory_format=cl), "strided"),        # 12 channels: no whole 8-vector
             (torch.zeros([2, 12, 32, 32], dtype=torch.float32, device=dev).contiguous(memory_format=cl), "cminor"),
             (torch.zeros([2, 16, 32, 32], dtype=bf, device=dev).contiguous(memory_format=cl)[:, 8:], "cminor"),   # a channel slice, still aligned
             (torch.zeros([2, 16, 32, 32], dtype=bf, device=dev).contiguous(memory_format=cl)[:, 4:12], "strided"),    # 8 bytes off
             (torch.zeros([2, 16, 8, 8], dtype=bf, device=dev).contiguous(memory_format=cl), "group"),
             (torch.zeros([2, 16, 4, 4], dtype=bf, device=dev), "group"), (torch.zeros([7, 33], dtype=torch.float16, device=dev), "group")]
    for x, name in cases:
        assert A.path(x) == name, (tuple(x.shape), x.stride(), name)


def test_channel_slices_and_a_long_plane(dev):
    """the channel-vector mapping on a channel slice (sc == 1, rows wider than C), and 16-byte loads over many chunks with both loop tails"""
    g = torch.Generator().manual_seed(11)
    base = (torch.randn(3, 24, 19, 23, generator=g) * 40).to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
    base[1, 9] = 0
    base[2, 17, 3, 4] = float("nan")
    for x in (base[:, 8:], base[:, :16], base[:, 4:12], base[1:, 16:]):
        _check(x, dev)
    for p in (2048 * 3, 2048 * 3 + 1, 1024 * 5 - 1, 70001):
        x = (torch.randn(1, 2, 1, p, generator=g) * 1e3).to(torch.float16)
        _check(x, dev)
        _check(x.float()[:, :, :, 3:], dev)                                     # fp32, the plane 12 bytes off a 16-byte boundary


def test_launch_records_and_refusals_that_launch_nothing(dev):
    x = torch.ones([3, 8, 16, 16], dtype=torch.bfloat16, device=dev).contiguous(memory_format=torch.channels_last)
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    _lib.prof_fetch()
    try:
        counts, values = A.planes(x)
        A.fold(counts, values, *A.empty(8, dev))
        for bad in (x.to(torch.int32), x[:, :, :, :8], x[:1].expand(3, 8, 16, 16)):
            with pytest.raises(RuntimeError, match="act_stats.planes"):
                A.planes(bad)
        with pytest.raises(RuntimeError, match="one device"):
            A.fold(counts, values, *A.empty(8))
        torch.cuda.synchronize()
        records = [r["dims"] for r in _lib.prof_fetch() if r["kind"] == "act_stats"]
    finally:
        _lib.prof_enable(False)
    assert records == [(0, 3, 8, 256, 2, _lib.SBG_BF16, 0), (1, 3, 8, 0, 0, 0, 0)]
    lib = _lib.load()
    assert lib.sbg_act_stats_planes(x.data_ptr(), 7, 3, 8, 256, 2048, 1, 8, counts.data_ptr(), values.data_ptr(), _lib.stream_ptr(dev)) == 1
    assert b"act_stats_planes" in lib.sbg_last_error()
    assert lib.sbg_act_stats_planes(x.data_ptr(), 2, 3, 8, 0, 2048, 1, 8, counts.data_ptr(), values.data_ptr(), _lib.stream_ptr(dev)) == 1
    assert lib.sbg_act_stats_path(x.data_ptr(), 2, 3, 8, 1 << 31, 2048, 1, 8) == -1
