"""The sliced Wasserstein kernels (csrc/swd.hip) on the device: every stage bit for bit against the float64 restatement (tests/swd_util.py)
on inputs whose results are exactly representable, bit for bit against the op layer's CPU arithmetic on inputs that are not (the fixed
orders and the fmaf chain are part of the definition), and the whole score under a bound derived from the data."""
import numpy as np
import pytest
import torch

import swd_util as U
from exact_util import assert_exact, assert_range, expect_launch, qgrid, qint, qpow2
from style_big_gan_amd.metrics import scores
from style_big_gan_amd.torch_utils.ops import swd
from swd_cases import byte_sets, derived_bound, level_descriptors, small_tables

pytestmark = pytest.mark.gpu


def _bytes(seed, shape, hi=256):
    return np.random.RandomState(seed).randint(0, hi, size=shape).astype(np.float32)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.cpu().contiguous().view(torch.int32 if a.dtype == torch.float32 else torch.int64),
                                              b.cpu().contiguous().view(torch.int32 if b.dtype == torch.float32 else torch.int64))


def test_pyramid_one_level_down_and_lap_called_directly(dev):
    """16 x 16: every tap of a row can touch a boundary"""
    x = _bytes(0, (2, 3, 16, 16))
    xd = torch.from_numpy(x).to(dev)
    with expect_launch("swd", lambda d: d[:4] == (0, 2, 3, 16), "pyr_down"):
        coarse = swd.pyr_down(xd)
    ref_coarse = U.pyr_down(x.astype(np.float64))
    assert_exact(coarse, torch.from_numpy(ref_coarse), "pyr_down 16")
    ref_lap = x.astype(np.float64) - U.pyr_up(ref_coarse)
    with expect_launch("swd", lambda d: d[:4] == (1, 2, 3, 16), "pyr_lap"):
        lap = swd.pyr_lap(xd, coarse)
    assert_exact(lap, torch.from_numpy(ref_lap), "pyr_lap 16")
    assert torch.equal(xd.cpu(), torch.from_numpy(x))                # out of place: the input is intact
    assert swd.pyr_lap(xd, coarse, inplace=True) is xd
    assert_exact(xd, torch.from_numpy(ref_lap), "pyr_lap 16 in place")


@pytest.mark.parametrize("shape,hi,levels", [((2, 3, 32, 32), 256, 2), ((2, 1, 64, 64), 4, 3)])
def test_pyramid_levels_bit_for_bit(dev, shape, hi, levels):
    x = _bytes(1, shape, hi)
    ref = U.laplacian_pyramid(x, levels)
    got = swd.laplacian_pyramid(torch.from_numpy(x).to(dev), levels)
    cpu = swd.laplacian_pyramid(torch.from_numpy(x), levels)
    assert len(got) == levels
    for i in range(levels):
        assert_exact(got[i], torch.from_numpy(ref[i]), f"level {i} of {shape}")
        assert _same_bits(got[i], cpu[i])


def test_pyramid_device_and_cpu_agree_where_nothing_is_exact(dev):
    """random floats, 64 x 64, three levels: the chain's order is the definition, so the two devices give the same bits"""
    x = torch.randn(3, 3, 64, 64, generator=torch.Generator().manual_seed(2)) * 100
    for g, c in zip(swd.laplacian_pyramid(x.to(dev), 3), swd.laplacian_pyramid(x, 3)):
        assert _same_bits(g, c)


def _centres(seed, b, p, s):
    c = np.random.RandomState(seed).randint(3, s - 3, size=(b, p, 2)).astype(np.int32)
    c[0, 0], c[0, 1], c[b - 1, p - 1], c[b - 1, 0] = (3, 3), (3, s - 4), (s - 4, s - 4), (s - 4, 3)
    return c


@pytest.mark.parametrize("channels", [1, 3])
def test_gather_exact_copy(dev, channels):
    s, b, p, offset = 16, 3, 5, 4
    level = _bytes(3, (b, channels, s, s))
    centres = _centres(4, b, p, s)
    out = torch.full([offset + b * p + 2, 49 * channels], -7.0, device=dev)
    with expect_launch("swd", lambda d: d[:5] == (2, b, channels, s, p), "gather"):
        swd.gather_descriptors(torch.from_numpy(level).to(dev), torch.from_numpy(centres).to(dev), out, row_offset=offset)
    ref = U.descriptors(level, centres).reshape(b * p, -1)
    assert torch.equal(out[offset:offset + b * p].cpu(), torch.from_numpy(ref))
    assert bool((out[:offset] == -7).all()) and bool((out[offset + b * p:] == -7).all())        # rows outside the batch are not touched
    bad = centres.copy()
    bad[1, 2] = (2, 8)              # outside [3, S - 4]: never dereferenced, the row is NaN on both devices
    bad[2, 0] = (8, s - 3)
    cpu = torch.zeros([b * p, 49 * channels])
    swd.gather_descriptors(torch.from_numpy(level), torch.from_numpy(bad), cpu)
    got = torch.zeros([b * p, 49 * channels], device=dev)
    swd.gather_descriptors(torch.from_numpy(level).to(dev), torch.from_numpy(bad).to(dev), got)
    assert bool(got[7].isnan().all()) and bool(got[10].isnan().all()) and int(got.isnan().any(dim=1).sum()) == 2
    assert torch.equal(got.cpu().nan_to_num(-1.0), cpu.nan_to_num(-1.0))


def _exact_descriptors(case):
    """descriptors of an exactly representable pyramid level: (fp32 [M, 49 C], C, fractional bits)"""
    if case == 15:          # 3 images x 5 patches of the 16 x 16 Gaussian level of byte images: 8 fractional bits
        x = _bytes(5, (3, 3, 32, 32))
        level = U.laplacian_pyramid(x, 2)[1]
        return U.descriptors(level, _centres(6, 3, 5, 16)).reshape(15, -1).astype(np.float32), 3, 8
    x = _bytes(7, (2, 1, 64, 64), 4)        # 2 images x 65 patches of the 64 x 64 Laplacian level of images with values 0..3: 14 fractional bits
    level = U.laplacian_pyramid(x, 3)[0]
    return U.descriptors(level, _centres(8, 2, 65, 64)).reshape(130, -1).astype(np.float32), 1, 14


@pytest.mark.parametrize("m", [15, 130])
def test_moments_exact_on_the_exact_pyramid(dev, m):
    desc, channels, frac = _exact_descriptors(m)
    v = desc.astype(np.float64).reshape(m, channels, 49)
    assert np.array_equal(v * 2.0 ** frac, np.round(v * 2.0 ** frac))
    assert m * 49 * np.abs(v).max() ** 2 * 4.0 ** frac < 2.0 ** 53           # every partial sum of squares is an exact float64, in any order
    with expect_launch("swd", lambda d: d[:4] == (3, m, channels, 1), "moments"):
        got = swd.channel_moments(torch.from_numpy(desc).to(dev), channels)
    assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), np.stack([v.sum((0, 2)), (v * v).sum((0, 2))], axis=1))


def test_moments_order_is_the_cpu_path_order(dev):
    """2100 rows = three chunks, random floats: the sums are inexact, the order makes them equal"""
    desc = torch.randn(2100, 147, generator=torch.Generator().manual_seed(9)) * 37 + 5
    with expect_launch("swd", lambda d: d[:3] == (6, 6, 3), "merge of three chunks"):
        got = swd.channel_moments(desc.to(dev), 3)
    assert _same_bits(got, swd.channel_moments(desc, 3))
    ints = torch.from_numpy(_bytes(10, (2100, 49)))
    v = ints.numpy().astype(np.float64)
    assert np.array_equal(swd.channel_moments(ints.to(dev), 1).cpu().numpy(), np.array([[v.sum(), (v * v).sum()]]))


def _project_case(seed, m, k, d, pitch=None):
    gen = torch.Generator().manual_seed(seed)
    c = k // 49
    x = qint(gen, [m, k], hi=8)
    s = qpow2(gen, [c], exps=(-1, 0, 1))
    t = qgrid(gen, [c], -2.0, 2.0, 0.25)
    dirs = qpow2(gen, [k, pitch or d]) * (torch.randint(0, 2, [k, pitch or d], generator=gen, dtype=torch.int64) * 2 - 1).to(torch.float64)
    # x_hat is a multiple of 1/4 below 8 * 2 + 2, a product a multiple of 1/16 below 36: every partial sum is exact in fp32
    assert_range("swd.project", k * (8 * 2 + 2) * 2, frac_bits=4)
    xhat = x * s.repeat_interleave(49)[None, :] + t.repeat_interleave(49)[None, :]
    return x, s, t, dirs, (dirs[:, :d].t() @ xhat.t())


@pytest.mark.parametrize("m,k,d", [(15, 49, 1), (130, 147, 33), (257, 147, 128), (130, 49, 161)])
def test_project_exact(dev, m, k, d):
    """row tails (15, 130, 257 against tiles of 128), K = 49 and 147 (odd: the last MFMA carries one padded k), direction tails (1, 33),
    a second direction tile (161), and directions taken as a column slice of a wider table"""
    x, s, t, dirs, ref = _project_case(m + d, m, k, d, pitch=d + 7)
    f = lambda v: v.to(torch.float32).to(dev)
    with expect_launch("swd", lambda r: r[:4] == (4, m, k, d), "project"):
        got = swd.project(f(x), f(s), f(t), f(dirs)[:, :d])
    assert_exact(got, ref, f"project {m} x {k} x {d}")
    assert _same_bits(got, swd.project(x.float(), s.float(), t.float(), dirs.float()[:, :d]))


def test_project_is_the_fmaf_chain(dev):
    """random floats: every step rounds; the matrix cores and the CPU path's emulated fmaf chain give the same bits"""
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(130, 147, generator=gen) * 60 + 100
    s, t = torch.tensor([0.013, 0.021, 0.017]), torch.tensor([-1.3, -2.2, -1.7])
    dirs = torch.from_numpy(U.unit_directions(np.random.RandomState(13), 147, 33))
    got = swd.project(x.to(dev), s.to(dev), t.to(dev), dirs.to(dev))
    assert _same_bits(got, swd.project(x, s, t, dirs))
    xhat = x.double() * s.double().repeat_interleave(49) + t.double().repeat_interleave(49)
    bound = (147 + 3) * 2.0 ** -24 * xhat.norm(dim=1)                # and it is a projection: (K + 3) u ||x_hat_m||, unit directions
    assert bool(((got.cpu().double() - dirs.double().t() @ xhat.t()).abs() <= bound[None, :]).all())


def test_sorted_l1(dev):
    gen = torch.Generator().manual_seed(14)
    a, b = qgrid(gen, [33, 130], -64.0, 64.0, 2.0 ** -10), qgrid(gen, [33, 130], -64.0, 64.0, 2.0 ** -10)
    with expect_launch("swd", lambda r: r[:4] == (5, 33, 130, 1), "l1"):
        got = swd.sorted_l1(a.float().to(dev), b.float().to(dev))
    assert got.dtype == torch.float64 and torch.equal(got.cpu(), (a - b).abs().sum(dim=1))      # grid values: exact in any order
    # three chunks of a direction, random floats: inexact sums, equal through the fixed order
    a, b = torch.randn(2, 40000, generator=gen) * 3, torch.randn(2, 40000, generator=gen) * 3
    with expect_launch("swd", lambda r: r[:3] == (6, 2, 3), "merge of three chunks"):
        got = swd.sorted_l1(a.to(dev), b.to(dev))
    assert _same_bits(got, swd.sorted_l1(a, b))
    # 258 chunks of a direction: a lane of the merge adds two partials
    m = 257 * 16384 + 5
    a, b = torch.randn(2, m, generator=gen) * 3, torch.randn(2, m, generator=gen) * 3
    with expect_launch("swd", lambda r: r[:3] == (6, 2, 258), "merge of 258 chunks"):
        got = swd.sorted_l1(a.to(dev), b.to(dev))
    assert _same_bits(got, swd.sorted_l1(a, b))


def test_end_to_end_against_the_restatement(dev):
    """two random byte sets [24, 3, 32, 32], 8 patches per image, 2 repeats x 16 directions.  Sorting is non-expansive in the max norm, so
    |score_dev - score_ref| <= 1e3 * 2 * max |p_dev - p_ref|, and a projection entry errs by at most (K + 3) 2^-24 ||x_hat_m||_2 because the
    directions have unit norm: the bound is computed from the data.  The CPU path gives the device's score bit for bit."""
    real, fake = byte_sets()
    tables = small_tables(3, 24, 32, 3, 8, 32)
    ref, ref_desc = U.score(real, fake, tables["centres"], tables["dirs"], 2, 16)
    dr, df = level_descriptors(real, tables, dev), level_descriptors(fake, tables, dev)
    cr, cf = level_descriptors(real, tables), level_descriptors(fake, tables)
    for i, res in enumerate((32, 16)):
        with expect_launch("swd", lambda r: r[:4] == (4, 192, 147, 32), "project"):
            got = scores.sliced_wasserstein(dr[i], df[i], tables["dirs"], 2, 16, what=f"level {res}")
        bound = derived_bound([ref_desc[res]], 147)
        print(f"level {res}: device {got!r}, restatement {ref[res]!r}, |difference| {abs(got - ref[res]):.3e}, bound {bound:.3e}")
        assert abs(got - ref[res]) <= bound
        assert got == scores.sliced_wasserstein(cr[i], cf[i], tables["dirs"], 2, 16, what=f"level {res}")
