"""The attention kernels' shape contract (include/sbg_hip.h), pinned without a device: sbg_attention_supported and sbg_attention_bwd_supported
are host-only predicates, and layers.attention_core launches whatever they accept.  They must therefore accept exactly what sbg_attention_fwd /
sbg_attention_bwd dispatch: for M <= 256 the whole key strip is held at once and only M / 16 in {1, 2, 4, 8, 16} is instantiated; above 256
the streamed kernels take any multiple of 16.  The backward adds ceil(D / 16) in {1, 2, 4} and DV / 16 in {1, 2, 4, 8, 16}."""
import pytest

from style_big_gan_amd import _lib

TILES = (1, 2, 4, 8, 16)


def fwd_rule(q, m, d, dv):
    ok = q >= 16 and q % 16 == 0 and m >= 16 and m % 16 == 0 and d >= 4 and d % 4 == 0 and dv >= 16 and dv % 16 == 0
    return bool(ok and (m > 256 or m // 16 in TILES))


def bwd_rule(q, m, d, dv):
    return fwd_rule(q, m, d, dv) and (d + 15) // 16 in (1, 2, 4) and dv // 16 in TILES


@pytest.mark.parametrize("m", list(range(16, 257, 16)))
def test_single_chunk_key_counts(m):
    lib = _lib.load()
    for d in (4, 24, 64):
        for dv in (16, 48, 256):
            want = m // 16 in TILES
            assert fwd_rule(16, m, d, dv) == want
            assert lib.sbg_attention_supported(16, m, d, dv) == int(want), (m, d, dv)
            assert lib.sbg_attention_bwd_supported(16, m, d, dv) == int(want and dv != 48), (m, d, dv)


@pytest.mark.parametrize("m", [272, 528])
def test_streamed_key_counts(m):
    lib = _lib.load()
    for d in (4, 24, 64):
        for dv in (16, 48, 256):
            assert lib.sbg_attention_supported(16, m, d, dv) == 1, (m, d, dv)
            assert lib.sbg_attention_bwd_supported(16, m, d, dv) == int(dv != 48), (m, d, dv)


@pytest.mark.parametrize("shape", [(16, 8, 4, 16), (16, 264, 4, 16), (16, 16, 6, 16), (16, 64, 6, 16), (16, 16, 4, 24), (16, 512, 4, 24),
                                   (24, 16, 4, 16), (24, 512, 4, 16), (8, 16, 4, 16), (16, 0, 4, 16), (16, 16, 0, 16), (16, 16, 4, 0)],
                         ids=lambda s: "x".join(map(str, s)))
def test_refused_neighbours(shape):
    lib = _lib.load()
    assert not fwd_rule(*shape)
    assert lib.sbg_attention_supported(*shape) == 0 and lib.sbg_attention_bwd_supported(*shape) == 0


@pytest.mark.parametrize("m", [16, 128, 256, 272])
def test_backward_tile_counts(m):
    lib = _lib.load()
    for d, dt_ok in ((4, True), (16, True), (20, True), (32, True), (36, False), (48, False), (52, True), (64, True), (68, False), (128, False)):
        for dv, dvt_ok in ((16, True), (32, True), (48, False), (64, True), (96, False), (128, True), (256, True), (272, False), (512, False)):
            assert lib.sbg_attention_supported(64, m, d, dv) == 1, (m, d, dv)          # the forward loops over D and DV: any multiple
            assert bwd_rule(64, m, d, dv) == (dt_ok and dvt_ok)
            assert lib.sbg_attention_bwd_supported(64, m, d, dv) == int(dt_ok and dvt_ok), (m, d, dv)


def test_predicates_follow_the_rule_on_a_grid():
    lib = _lib.load()
    for q in (16, 24, 80):
        for m in list(range(8, 300, 8)) + [512, 528, 1024]:
            for d in (4, 6, 12, 24, 36, 64, 68):
                for dv in (16, 24, 48, 64, 256):
                    assert lib.sbg_attention_supported(q, m, d, dv) == int(fwd_rule(q, m, d, dv)), (q, m, d, dv)
                    assert lib.sbg_attention_bwd_supported(q, m, d, dv) == int(bwd_rule(q, m, d, dv)), (q, m, d, dv)
