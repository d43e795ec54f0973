"""Exact-arithmetic helpers shared by the kernel-path tests (tests/test_kernel_paths_gpu.py, tests/test_stream_kernels_gpu.py).

Exact mode: operands are small integers or dyadic values, so every product is exact and every fp32 partial sum is exact in any order while
its magnitude stays below 2^(24 - d), d = fractional bits (`assert_range`).  A kernel's result must then equal the fp64 reference rounded
ONCE to the output dtype, bit for bit (`assert_exact`).  `expect_launch` asserts, from the library's launch log, which kernel served a launch."""
import contextlib

import torch

from style_big_gan_amd import _lib

U_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11, torch.float32: 0.0}
U32 = 2.0 ** -24


def qint(gen, shape, hi=2):
    """fp64 CPU tensor of nonzero integers in [-hi, -1] u [1, hi]"""
    mag = torch.randint(1, hi + 1, shape, generator=gen, dtype=torch.int64)
    sign = torch.randint(0, 2, shape, generator=gen, dtype=torch.int64) * 2 - 1
    return (mag * sign).to(torch.float64)


def qgrid(gen, shape, lo, hi, step):
    """fp64 CPU tensor of multiples of `step` (a power of two) in [lo, hi]"""
    k = torch.randint(int(round(lo / step)), int(round(hi / step)) + 1, shape, generator=gen, dtype=torch.int64)
    return k.to(torch.float64) * step


def qpow2(gen, shape, exps=(-2, -1, 0, 1)):
    """fp64 CPU tensor of powers of two 2^e, e drawn from `exps`"""
    e = torch.tensor(exps, dtype=torch.float64)[torch.randint(0, len(exps), shape, generator=gen)]
    return torch.pow(2.0, e)


def assert_range(what, bound, frac_bits=0):
    """exact-mode precondition: every partial sum is an fp32 integer multiple of 2^-frac_bits below 2^24 of them"""
    assert bound * 2.0 ** frac_bits < 2.0 ** 24, f"{what}: exact-mode range precondition fails ({bound} with {frac_bits} fractional bits)"


def assert_exact(got, ref64, what):
    """got (any device, dtype D) == ref64 (fp64) rounded once to D, bit for bit; reports the first mismatching index"""
    got = got.detach().cpu()
    assert tuple(got.shape) == tuple(ref64.shape), f"{what}: shape {tuple(got.shape)} vs {tuple(ref64.shape)}"
    r32 = ref64.to(torch.float32)
    assert torch.equal(r32.to(torch.float64), ref64), f"{what}: reference is not exact in fp32 (test precondition)"
    want = r32.to(got.dtype)            # fp32 -> 16 bit: round-to-nearest-even, the only rounding
    g, w = got.contiguous(), want.contiguous()
    ibits = {2: torch.int16, 4: torch.int32}[g.element_size()]
    bad = (g.view(ibits) != w.view(ibits)) & ~((g == 0) & (w == 0))        # +0 / -0 are one value (a zero dy times a negative x)
    if bool(bad.any()):
        idx = tuple(int(i) for i in bad.nonzero()[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {idx}: got {float(g[idx])!r}, "
                             f"want {float(w[idx])!r} (exact {float(ref64[idx])!r})")


def within_bound(got, ref, bound):
    return bool(((got.double() - ref).abs() <= bound).all())


_rec_depth = [0]
_rec_log = []


@contextlib.contextmanager
def expect_launch(kind, predicate, what):
    """asserts that a launch of `kind` whose dims satisfy `predicate` was logged inside the block (nestable: one launch log for all)"""
    if _rec_depth[0] == 0:
        torch.cuda.synchronize()
        _lib.prof_enable(True)
        _lib.prof_fetch()
        _rec_log.clear()
    _rec_depth[0] += 1
    try:
        yield _rec_log
    finally:
        torch.cuda.synchronize()
        _rec_log.extend(_lib.prof_fetch())
        _rec_depth[0] -= 1
        if _rec_depth[0] == 0:
            _lib.prof_enable(False)
    seen = [r["dims"] for r in _rec_log if r["kind"] == kind]
    assert any(predicate(d) for d in seen), f"{what}: no {kind} launch matched; logged {seen}"
