"""The preconditions of tests/test_biggan_exact_gpu.py, asserted without a device for every case of its tables (tests/biggan_exact_util.py):
what makes the expected results exact in fp32 for any summation order, and that the closed-form expectations are the float64 compositions."""
import math

import numpy as np
import pytest
import torch

import biggan_exact_util as BU
from exact_util import assert_range

ALL_ATT = [c + (zi,) for c in BU.ATT_CASES for zi in (0, 1, 2)]


def _is_pow2(t):
    t = t.long()
    return bool(((t > 0) & ((t & (t - 1)) == 0)).all())


@pytest.mark.parametrize("case", ALL_ATT, ids=lambda c: BU.att_case_id(c) + f"-z{c[5]}")
def test_attention_selection_preconditions(case):
    q, m, d, dv, where, zi = case
    assert d == BU.min_d(m) or d in (24, 64)
    z = BU.z_sets(m, where)[zi]
    assert len(z) == zi
    cs = BU.att_case(2, q, m, d, dv, z, seed=len(z))
    T = BU.att_terms(cs)
    S = T["S"]
    s32 = torch.bmm(cs["theta"].float(), cs["phi"].float().transpose(1, 2))
    assert torch.equal(s32.double(), S) and torch.equal(S, S.round())                    # integer logits, the same in fp32
    assert_range("logits", float((cs["theta"].abs() @ cs["phi"].abs().transpose(1, 2)).max()))
    assert bool((T["mx"] == 0).all())                                                     # the shift dimension: the row maximum is exactly 0
    ties = (S == 0).sum(-1)
    assert _is_pow2(ties) and int(ties.max()) == 2 ** zi                                  # P = 2^-j on 2^j keys ...
    assert float(S[S != 0].max()) <= -128                                                 # ... and exp(s - max) = 0 in fp32 on every other key
    assert np.exp(np.float32(-128)) == 0 and np.exp(np.float32(0)) == 1
    assert torch.equal(T["P"], (S == 0).double() / ties.unsqueeze(-1))
    assert bool((S.gather(2, cs["targets"].unsqueeze(-1)) == 0).all())                    # the target is among the winners
    # targets: a permutation per sample (every key is a target once Q >= M), other targets in the other sample
    for s in range(2):
        t = cs["targets"][s]
        assert len(set(t[:min(q, m)].tolist())) == min(q, m)
        if q > m:
            assert torch.equal(t[m:], t[:q - m])                                          # several queries share a key: dg sums several rows
    assert not torch.equal(cs["targets"][0], cs["targets"][1])
    # winners in the first chunk only, in the last chunk only, and in the 16-key remainder chunk
    if m > BU.ATT_MAX_M:
        win = S == 0
        last0 = (m - 1) // BU.ATT_CHUNK * BU.ATT_CHUNK
        if zi == 0 or where == "low":                                                     # ('high' tie sets straddle the chunks instead)
            assert bool((win[..., :BU.ATT_CHUNK].any(-1) & ~win[..., BU.ATT_CHUNK:].any(-1)).any())
            assert bool((win[..., last0:].any(-1) & ~win[..., :last0].any(-1)).any())
        if m % BU.ATT_CHUNK == 16:
            assert m - last0 == 16
        if zi and where == "high":
            nchunks = torch.stack([win[..., c0:c0 + BU.ATT_CHUNK].any(-1) for c0 in range(0, m, BU.ATT_CHUNK)]).sum(0)
            assert int(nchunks.max()) >= 2                                                # a tie set straddles two chunks
    if zi and where == "high" and m >= 32:
        ntiles = torch.stack([(S == 0)[..., c0:c0 + 16].any(-1) for c0 in range(0, m, 16)]).sum(0)
        assert int(ntiles.max()) >= 2                                                     # ... and two 16-key tiles
    # every sum of the forward and backward is a dyadic with zi (P) or 2 zi (dS) fractional bits, far below 2^24 of them
    A_dP = cs["dout"].abs() @ cs["g"].abs().transpose(1, 2)
    assert_range("out", float((T["P"] @ cs["g"].abs()).max()), zi)
    assert_range("dP", float(A_dP.max()))
    assert_range("delta", float((T["P"] * A_dP).sum(-1).max()), zi)
    assert_range("dS", float(T["A_dS"].max()), 2 * zi)
    assert_range("dtheta", float(T["A_dtheta"].max()), 2 * zi)
    assert_range("dg", float(T["A_dg"].max()), zi)
    if zi:                                                                                # every 16-column tile of D holds nonzero gradients
        assert bool((T["dtheta"][..., d - 1] != 0).any())
        for c0 in range(0, d, 16 if zi == 1 else d):                                      # (|Z| = 1: dphi is nonzero off Z only)
            assert bool((T["dphi"][..., c0:c0 + 16] != 0).any()), c0
    if zi == 0:
        assert_range("dphi", float(T["A_dphi"].max()))
        assert bool((T["dS"] == 0).all()) and bool((T["dtheta"] == 0).all()) and bool((T["dphi"] == 0).all())
        assert torch.equal(T["out"], torch.gather(cs["g"], 1, cs["targets"].unsqueeze(-1).expand(-1, -1, dv)))
        for s in range(2):                                                                # dg: the per-key sum of the dout rows
            assert torch.equal(T["dg"][s], torch.zeros(m, dv, dtype=torch.float64).index_add_(0, cs["targets"][s], cs["dout"][s]))
    # the closed forms are the float64 composition and its autograd gradients, up to the exp(-128) = 2.6e-56 that float64 keeps on the losers
    ins = [cs[k].clone().requires_grad_(True) for k in ("theta", "phi", "g")]
    out = torch.bmm(torch.softmax(torch.bmm(ins[0], ins[1].transpose(1, 2)), -1), ins[2])
    grads = torch.autograd.grad(out, ins, cs["dout"])
    for name, gr in zip(("out", "dtheta", "dphi", "dg"), (out.detach(),) + grads):
        assert float((gr - T[name]).abs().max()) < 1e-45 and torch.equal(gr.float(), T[name].float()), name
    for name in ("out", "dtheta", "dg"):
        assert torch.equal(T[name].float().double(), T[name]), name                       # representable in fp32


def test_attention_case_table_covers_every_instantiation():
    """from the dispatch rules alone (the device test reads the same from the launch log)"""
    seen = set()
    for q, m, d, dv, _ in BU.ATT_CASES:
        dims = (2, q, m, d, dv)
        bwd = dv // 16 in BU.TILE_COUNTS
        if m <= BU.ATT_MAX_M:
            assert m // 16 in BU.TILE_COUNTS
            variants = [("single", 0)] + ([("single", 1)] if bwd else [])
        else:
            variants = [("stream", 0)] + ([("stream_stats", 1), ("stream_dq", 1), ("stream_dkv", 1)] if bwd else [])
        for v, b in variants:
            seen.update(BU.att_instantiations(v, dims + (b,)))
    assert sorted(seen) == BU.ALL_INSTANTIATIONS
    assert len(BU.ALL_INSTANTIATIONS) == 5 + 5 + 10 + 3 + 15
    ms = {c[1] for c in BU.ATT_CASES}
    assert ms == {16, 32, 64, 128, 256, 272, 512, 528, 1024}
    assert {(c[0], c[1]) for c in BU.ATT_CASES} >= {(qq, mm) for qq in (16, 80) for mm in (16, 32, 64, 128, 256)}


def test_attention_one_hot_without_shift():
    q, m, d, dv = BU.ATT_ONE_HOT_NO_SHIFT
    cs = BU.att_case(2, q, m, d, dv, (), shift=False)
    T = BU.att_terms(cs)
    assert bool((T["mx"] == 256).all()) and float((T["S"] - T["mx"])[T["S"] != 256].max()) <= -128
    assert bool(((T["S"] == 256).sum(-1) == 1).all())
    assert float(np.float32(256) + np.log(np.float32(1))) == 256.0                       # lse = max + log(1)


def test_two_pass_restatement_ratio():
    """the constant of the tied-row bounds (see test_attention_selection_tied on the device): worst ratio of the float32 two-pass restatement"""
    worst = {}
    for q, m, d, dv, where in BU.ATT_CASES:
        for z in BU.z_sets(m, where)[1:]:
            cs = BU.att_case(2, q, m, d, dv, z, seed=len(z))
            T, R = BU.att_terms(cs), BU.att_two_pass_f32(cs)
            for name in ("dtheta", "dphi", "dg"):
                worst[name] = max(worst.get(name, 0.0), BU.bound_ratio(R[name], T[name], T["A_" + name]))
    print("two-pass float32 restatement, worst |err| / (2^-24 A):", worst)
    assert all(math.isfinite(v) for v in worst.values())
    assert BU.ATT_TIED_C == BU.pow2_ceil(4 * max(worst.values())), worst
    assert BU.pow2_ceil(0) == 0 and BU.pow2_ceil(4 * 0.3) == 2 and BU.pow2_ceil(4 * 0.5) == 2 and BU.pow2_ceil(4 * 1.1) == 8


# ---------------------------------------------------------------------------------------------------------------- spectral norm

@pytest.mark.parametrize("shape", BU.SN_EXACT_CASES, ids=lambda s: "x".join(map(str, s)))
def test_hadamard_rows(shape):
    rows, cols = shape
    W = BU.sn_exact_case(rows, cols)
    assert W.shape == (rows, cols) and bool((W.abs() == 1).all())
    gram = W @ W.t()
    assert torch.equal(gram, cols * torch.eye(rows, dtype=torch.float64))                 # distinct, orthogonal rows of norm sqrt(cols)
    assert math.sqrt(cols) in (16.0, 32.0) and rows > 32                                  # more than one 32-row block
    assert_range("column sums / 2^a", 1.0)                                                # one nonzero term (scaling by 2^a is exact)
    assert_range("|v_raw|^2 / 4^a", cols)
    assert_range("row sums", cols / math.sqrt(cols), int(math.log2(math.sqrt(cols))))      # sums of +-1/16 (1/32): at most cols of them
    for i in BU.sn_exact_rows(rows):
        assert 0 <= i < rows
        for a in BU.SN_EXACT_EXPONENTS:
            u = torch.zeros(1, rows, dtype=torch.float64)
            u[0, i] = 2.0 ** a
            want = BU.sn_exact_expect(W, i, a)
            for got, w in zip(BU.sn_reference(W, u), want):
                assert torch.equal(got, w)                                                # the float64 F.normalize composition gives the same
    assert {0, 32, rows - 1} <= set(BU.sn_exact_rows(rows))


# ---------------------------------------------------------------------------------------------------------------- minibatch std

@pytest.mark.parametrize("shape", BU.MBSTD_EXACT, ids=lambda s: "x".join(map(str, s)))
def test_mbstd_exact_preconditions(shape):
    N, C, HW, G, F = shape
    M, c = N // G, C // F
    unit = c * HW * G
    assert unit & (unit - 1) == 0 and sum(BU.MBSTD_SIGNS[G]) == 0
    cs = BU.mbstd_case(shape)
    x = cs["x"].reshape(G, M, C, HW)
    assert torch.equal(x.mean(0), cs["a"].reshape(M, C, HW))                              # sample g M + m belongs to group m
    assert torch.equal(x.var(0, unbiased=False), cs["d"].reshape(M, C, HW) ** 2)
    d2 = (cs["d"] ** 2).numpy().astype(np.float32)
    assert np.array_equal(d2 + np.float32(1e-8), d2) and np.array_equal(np.sqrt(d2), cs["d"].numpy().astype(np.float32))
    assert_range("x", float(x.abs().sum(0).max()))
    assert_range("sum of sqrt(var)", float(cs["d"].reshape(M, F, c * HW).sum(-1).max()))
    assert_range("dstat", float(cs["dy"][:, C:].reshape(G, M, F, HW).abs().sum((0, 3)).max()))
    y, dx = BU.mbstd_exact_expect(shape, cs)
    assert torch.equal(y.float().double(), y) and torch.equal(dx.float().double(), dx)
    # the closed forms are the float64 composition rounded to fp32 (it carries the 1e-8 the fp32 kernel's sqrt cannot see)
    y64, dx64 = BU.mbstd_composite64(cs["x"], G, F, cs["dy"])
    assert torch.equal(y64.float(), y.float())
    assert float((y64 - y).abs().max()) < 1e-8 and float((dx64 - dx).abs().max()) < 1e-7          # (dx has exact zeros: no rounding to compare)
    if F > 1 or M > 1:                                                                    # a swapped n = g M + m or a wrong F split shows
        stat = y[:M, C:, 0, 0]
        assert len({float(v) for v in stat.reshape(-1)}) == M * F


def test_mbstd_ragged_case():
    N, C, HW, G, F = BU.MBSTD_RAGGED
    cs = BU.mbstd_case(BU.MBSTD_RAGGED)
    assert cs["T"] is None and (C // F) * HW == 90 and G == 3
    x = cs["x"].reshape(G, N // G, C, HW)
    assert torch.equal(x.sum(0), 3 * cs["a"].reshape(N // G, C, HW))
    y64, dx64 = BU.mbstd_composite64(cs["x"], G, F, cs["dy"])
    assert float(dx64.abs().min()) > 0.5                                                  # no cancellation: an ulp of dx is an ulp of dy


# ---------------------------------------------------------------------------------------------------------------- grouped GEMM

@pytest.mark.parametrize("count,empty_at", BU.GG_TABLES)
def test_grouped_gemm_tables(count, empty_at):
    table = BU.gg_table(count, empty_at)
    assert len(table) == count
    nonempty = sum(pr["m"] > 0 for pr in table)
    assert BU.GG_LAUNCHES[(count, empty_at)] == [16] * (nonempty // 16) + ([nonempty % 16] if nonempty % 16 else [])
    for pr in table:
        assert_range("c", pr["bound"], 1)
        assert torch.equal(pr["c"].float().double(), pr["c"])
        for a, b, al in pr["terms"]:
            assert math.log2(abs(al)).is_integer()
    assert [i for i, pr in enumerate(table) if pr["m"] == 0] == ([] if empty_at is None else [empty_at])
    assert empty_at is None or 0 < empty_at < count - 1                                   # in the middle: neighbours on both sides
    ks = {pr["terms"][0][0].shape[1] for pr in table}
    assert ks >= {0, 15, 16, 17}
    assert {pr["m"] for pr in table} >= {63, 64, 65} and {pr["n"] for pr in table} >= {63, 64, 65, 130}
    assert {(pr["a_form"], pr["b_form"]) for pr in table} == {(a, b) for a in ("row", "col") for b in ("row", "col")}
    two = [pr for pr in table if len(pr["terms"]) == 2]
    assert two and all(pr["terms"][0][0].shape[1] != pr["terms"][1][0].shape[1] for pr in two)
    assert any(pr["rowsum"] is not None and pr["n"] > 64 for pr in table)
    assert any(pr["terms"][0][0].shape[1] == 0 and pr["bias"] is not None for pr in table)
    assert any(pr["terms"][0][0].shape[1] == 0 and pr["bias"] is None and len(pr["terms"]) == 1 for pr in table)
    assert any(pr["strided_c"] for pr in table)
    if count == 33:
        assert {(pr["m"], pr["n"], pr["terms"][0][0].shape[1]) for pr in table} >= {(m, n, k) for m in (63, 65) for n in (63, 65) for k in (15, 17)}
