"""Exact-arithmetic tests of the attention kernels and the BigGAN-side fp32 kernels (csrc/biggan_ops.hip, mbstd.hip, grouped_gemm.hip) through
their Python ops.  Exact mode (helpers in exact_util.py, generators in biggan_exact_util.py): operands for which every product and every fp32
partial sum is exact in any order, so the device result must equal the float64 reference bit for bit; the preconditions of every case are
asserted without a device in tests/test_biggan_exact_cases_cpu.py.  The launch log names the kernel that served each launch; where a
composition could stand in for a kernel it is replaced by a function that raises.  Bound mode only where stated: the attention shape
contract and the spectral-norm edge sweep at the suite's max_rel < 1e-5, the ragged minibatch-std case at 2 ulp."""
import warnings

import numpy as np
import pytest
import torch

import style_big_gan_amd  # noqa: F401
import biggan_exact_util as BU
from exact_util import assert_exact, assert_range, expect_launch
from golden_util import max_rel
from style_big_gan_amd import _lib
from style_big_gan_amd.biggan import layers as L

pytestmark = pytest.mark.gpu


def _attention_records(fn):
    """run fn with the launch log on -> (result, [(variant name, dims[:6])] of the attention records, in launch order)"""
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    _lib.prof_fetch()
    try:
        res = fn()
        torch.cuda.synchronize()
        log = _lib.prof_fetch()
    finally:
        _lib.prof_enable(False)
    return res, [(_lib.ATT_VARIANTS[r["dims"][6]], r["dims"][:6]) for r in log if r["kind"] == "attention"]


def _no_composition(monkeypatch):
    """from here on the torch bmm / softmax / bmm composition raises instead of running in a kernel's place"""
    def refuse(*a, **k):
        raise AssertionError("the torch composition ran in place of the HIP attention kernels")
    monkeypatch.setattr(L, "_attention_reference", refuse)
    monkeypatch.setattr(torch, "bmm", refuse)
    monkeypatch.setattr(torch.nn.functional, "softmax", refuse)


def _expected_records(shape, backward):
    n, q, m, d, dv = shape
    if m <= BU.ATT_MAX_M:
        return [("single", shape + (0,))] + ([("single", shape + (1,))] if backward else [])
    return [("stream", shape + (0,))] + ([(v, shape + (1,)) for v in ("stream_stats", "stream_dq", "stream_dkv")] if backward else [])


# ---------------------------------------------------------------------------------------------------------------- 1. the shape contract

# (shape, forward on the kernels, backward on the kernels)
CONTRACT = [((2, 32, 32, 8, 16), True, True), ((1, 16, 128, 12, 32), True, True), ((1, 16, 256, 64, 16), True, True),
            ((1, 16, 272, 4, 48), True, False),       # streamed forward with DVT = 1 and grid.z = 3; DV / 16 = 3 has no backward kernel
            ((1, 32, 64, 44, 32), True, False),       # D = 44 needs three column tiles in the backward
            ((1, 32, 48, 8, 16), False, False), ((1, 32, 96, 8, 16), False, False), ((1, 32, 240, 8, 16), False, False)]


@pytest.mark.parametrize("shape,fwd_kernel,bwd_kernel", CONTRACT, ids=lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else str(int(s)))
def test_attention_contract_boundaries(dev, shape, fwd_kernel, bwd_kernel):
    """both sides of every boundary of sbg_attention_supported / sbg_attention_bwd_supported through attention_core, forward and first-order
    backward, against the float64 composition on the CPU: max_rel < 1e-5.  A shape the kernels refuse takes the composition and says so once
    per direction and shape; it never reaches _lib.check with an unsupported launch."""
    n, q, m, d, dv = shape
    lib = _lib.load()
    assert bool(lib.sbg_attention_supported(q, m, d, dv)) == fwd_kernel and bool(lib.sbg_attention_bwd_supported(q, m, d, dv)) == bwd_kernel
    gen = torch.Generator().manual_seed(21)
    ins = [torch.randn(n, q, d, generator=gen), torch.randn(n, m, d, generator=gen), torch.randn(n, m, dv, generator=gen)]
    dout = torch.randn(n, q, dv, generator=gen)
    ref_in = [t.double().requires_grad_(True) for t in ins]
    ref_out = L._attention_reference(*ref_in)
    ref = torch.autograd.grad(ref_out, ref_in, dout.double())
    dev_in = [t.to(dev).requires_grad_(True) for t in ins]
    for direction in ("forward", "backward"):
        L._composition_warned.discard((direction, (q, m, d, dv)))

    def run():
        out = L.attention_core(*dev_in)
        return out, torch.autograd.grad(out, dev_in, dout.to(dev))

    def run_recorded():
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            res, recs = _attention_records(run)
        return res, recs, [str(w.message) for w in caught if issubclass(w.category, UserWarning) and "attention_core" in str(w.message)]

    (out, got), recs, said = run_recorded()
    want = (_expected_records(shape, bwd_kernel) if fwd_kernel else [])
    assert recs == want, recs
    names = ([] if fwd_kernel else ["forward"]) + (["backward"] if fwd_kernel and not bwd_kernel else [])
    assert len(said) == len(names), said
    for msg, direction in zip(said, names):
        assert f"attention_core {direction}: Q={q} M={m} D={d} DV={dv} " in msg, msg
    errs = dict(out=max_rel(out, ref_out.float()))
    for name, a, b in zip(("dtheta", "dphi", "dg"), got, ref):
        errs[name] = max_rel(a, b.float())
    print("contract", shape, {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(e < 1e-5 for e in errs.values()), (shape, errs)
    (out2, got2), recs2, said2 = run_recorded()          # once per shape and direction: the second pass is silent, and gives the same bits
    assert recs2 == want and said2 == []
    assert torch.equal(out, out2) and all(torch.equal(a, b) for a, b in zip(got, got2))


# ---------------------------------------------------------------------------------------------------------------- 2. attention, exact selection

def _run_selection(dev, cs, backward):
    ins = [cs[k].float().to(dev).requires_grad_(backward) for k in ("theta", "phi", "g")]
    dout = cs["dout"].float().to(dev)

    def run():
        if not backward:
            with torch.no_grad():
                return L.attention_core(*ins), None
        out = L.attention_core(*ins)
        return out, torch.autograd.grad(out, ins, dout)

    (out, grads), recs = _attention_records(run)
    out2, grads2 = run()                                 # fixed summation order, no atomics: the same bits
    assert torch.equal(out, out2) and (not backward or all(torch.equal(a, b) for a, b in zip(grads, grads2)))
    return out, grads, recs


@pytest.mark.parametrize("case", BU.ATT_CASES, ids=BU.att_case_id)
def test_attention_selection(dev, monkeypatch, case):
    """the selection construction (biggan_exact_util.py) with |Z| = 0, 1, 2 zeroed code digits: P is exactly 2^-j on 2^j keys, 0 elsewhere.
    out is exact in every mode.  One-hot rows (|Z| = 0): out is the gather of g rows, also for Gaussian g; dg is the per-key sum of dout rows,
    dtheta and dphi are exactly zero.  Tied rows: dtheta of the single-chunk kernel is exact; dphi, dg and the streamed dtheta go through
    P = expf(S - lse) with lse = logf(2^j) and are held element by element to |got - ref64| <= c 2^-24 A, A = the gradient expression with the
    absolute value of every factor.  c = BU.ATT_TIED_C is 4 x the worst ratio |err| / (2^-24 A) of the float32 numpy restatement of the
    two-pass formulation (BU.att_two_pass_f32) over the case table, rounded up to a power of two.  Restatement on the CPU: worst ratio 0.0
    for dtheta, dphi and dg (logf(2^j) rounded to float32 and expf of its negative round back to exactly 2^-j for j = 1, 2), hence c = 0 and
    the bound asks for the exact result.  Measured on an MI355X: worst ratio 0.0 for dtheta, dphi and dg in every case, single-chunk and
    streamed (each case prints its ratios).  DV = 48 (three output tiles) has no backward kernel: forward only."""
    q, m, d, dv, where = case
    shape = (2, q, m, d, dv)
    backward = dv // 16 in BU.TILE_COUNTS
    lib = _lib.load()
    assert lib.sbg_attention_supported(q, m, d, dv) == 1 and lib.sbg_attention_bwd_supported(q, m, d, dv) == int(backward)
    _no_composition(monkeypatch)
    streamed = m > BU.ATT_MAX_M
    for z in BU.z_sets(m, where):
        cs = BU.att_case(2, q, m, d, dv, z, seed=len(z))
        T = BU.att_terms(cs)
        out, grads, recs = _run_selection(dev, cs, backward)
        assert recs == _expected_records(shape, backward), recs
        what = f"{BU.att_case_id(case)} Z={z}"
        assert_exact(out, T["out"], what + " out")
        if not backward:
            continue
        dtheta, dphi, dg = grads
        if not z:
            assert_exact(dg, T["dg"], what + " dg")
            assert bool((dtheta == 0).all()) and bool((dphi == 0).all()), what
            continue
        ratios = {name: BU.bound_ratio(got, T[name], T["A_" + name]) for name, got in (("dtheta", dtheta), ("dphi", dphi), ("dg", dg))}
        print("tied", what, "streamed" if streamed else "single", {k: f"{v:.3f}" for k, v in ratios.items()})
        if not streamed:
            assert_exact(dtheta, T["dtheta"], what + " dtheta")
        assert all(r <= BU.ATT_TIED_C for r in ratios.values()), (what, ratios)
    # a pure gather: Gaussian g, one-hot rows
    cs = BU.att_case(2, q, m, d, dv, (), seed=7, gaussian_g=True)
    out, _, recs = _run_selection(dev, cs, False)
    assert recs == _expected_records(shape, False)
    want = torch.gather(cs["g"].float(), 1, cs["targets"].unsqueeze(-1).expand(-1, -1, dv))
    assert torch.equal(out.cpu(), want), BU.att_case_id(case)


def test_attention_one_hot_without_shift(dev, monkeypatch):
    """D = 4, M = 16: the four code digits and no shift dimension, so the row maximum is 256 and lse = 256 + logf(1) is still exact"""
    q, m, d, dv = BU.ATT_ONE_HOT_NO_SHIFT
    _no_composition(monkeypatch)
    cs = BU.att_case(2, q, m, d, dv, (), shift=False)
    T = BU.att_terms(cs)
    out, (dtheta, dphi, dg), recs = _run_selection(dev, cs, True)
    assert recs == _expected_records((2, q, m, d, dv), True)
    assert_exact(out, T["out"], "out")
    assert_exact(dg, T["dg"], "dg")
    assert bool((dtheta == 0).all()) and bool((dphi == 0).all())


def test_attention_instantiations_reached(dev, monkeypatch):
    """every kernel template instantiation of the attention family is reached by a case of the table: read from the launch log (the record's
    dims fix MT, DVT and DT through the dispatch rules restated in BU.att_instantiations)"""
    _no_composition(monkeypatch)
    first = {}
    for case in BU.ATT_CASES:
        q, m, d, dv, _ = case
        backward = dv // 16 in BU.TILE_COUNTS
        _, _, recs = _run_selection(dev, BU.att_case(2, q, m, d, dv, ()), backward)
        for variant, dims in recs:
            for inst in BU.att_instantiations(variant, dims):
                first.setdefault(inst, BU.att_case_id(case))
    for inst in sorted(first):
        print("instantiation", inst, "<-", first[inst])
    assert sorted(first) == BU.ALL_INSTANTIATIONS


# ---------------------------------------------------------------------------------------------------------------- 3. spectral norm

def _sigma(W, u, dev):
    with expect_launch("sn_power", lambda d: d[:2] == tuple(W.shape), f"power iteration {tuple(W.shape)}"):
        return L._SpectralSigma.apply(W, u.float().to(dev), 1e-12)


@pytest.mark.parametrize("shape", BU.SN_SWEEP + ["transposed"], ids=lambda s: s if isinstance(s, str) else "x".join(map(str, s)))
def test_power_iteration_edges(dev, shape):
    """_SpectralSigma.apply against the float64 F.normalize composition on the CPU, max_rel < 1e-5 for sigma, u_new, v and d sigma / d W =
    outer(u_new, v): rows on both sides of the 32-row block, columns on both sides of the 256-column block, one row (the discriminator's
    final SNLinear(., 1)), one column, a class embedding, and a transposed (non-contiguous) weight view"""
    transposed = shape == "transposed"
    rows, cols = (33, 257) if transposed else shape
    gen = torch.Generator().manual_seed(31)
    W, u = torch.randn(rows, cols, generator=gen), torch.randn(1, rows, generator=gen)
    s_ref, u_ref, v_ref = BU.sn_reference(W.double(), u.double())
    base = (W.t().contiguous() if transposed else W).to(dev).requires_grad_(True)
    Wd = base.t() if transposed else base
    assert Wd.is_contiguous() != transposed
    sigma, u_new, v = _sigma(Wd, u, dev)
    (gw,) = torch.autograd.grad(sigma, base)
    g_ref = torch.outer(u_ref[0], v_ref[0])
    errs = dict(sigma=max_rel(sigma, s_ref.float()), u_new=max_rel(u_new, u_ref.float()), v=max_rel(v, v_ref.float()),
                dW=max_rel(gw, (g_ref.t() if transposed else g_ref).float()))
    print("sn", shape, {k: f"{v:.2e}" for k, v in errs.items()})
    assert sigma.shape == () and u_new.shape == (1, rows) and v.shape == (1, cols)
    assert all(e < 1e-5 for e in errs.values()), (shape, errs)


@pytest.mark.parametrize("shape", [(33, 257), (1, 2048)], ids=lambda s: "x".join(map(str, s)))
def test_power_iteration_degenerate(dev, shape):
    """u = 0 and W = 0: the max(norm, eps) branch; every output is exactly 0 and finite, as F.normalize gives"""
    rows, cols = shape
    gen = torch.Generator().manual_seed(32)
    for W, u in ((torch.randn(rows, cols, generator=gen), torch.zeros(1, rows)), (torch.zeros(rows, cols), torch.randn(1, rows, generator=gen))):
        for t in BU.sn_reference(W.double(), u.double()):
            assert bool((t == 0).all())
        Wd = W.to(dev).requires_grad_(True)
        sigma, u_new, v = _sigma(Wd, u, dev)
        (gw,) = torch.autograd.grad(sigma, Wd)
        for t in (sigma, u_new, v, gw):
            assert bool(torch.isfinite(t).all()) and bool((t == 0).all())


@pytest.mark.parametrize("shape", BU.SN_EXACT_CASES, ids=lambda s: "x".join(map(str, s)))
def test_power_iteration_exact(dev, shape):
    """W = distinct rows of a Hadamard matrix, u = 2^a e_i: v_raw = 2^a W[i], v = W[i] / sqrt(cols), t = sqrt(cols) e_i, u_new = e_i and
    sigma = sqrt(cols) = 16 or 32, bit for bit -- every other row's sum is a sum of +-1/16 (1/32) that cancels exactly in any order"""
    rows, cols = shape
    W = BU.sn_exact_case(rows, cols)
    Wd = W.float().to(dev)
    for i in BU.sn_exact_rows(rows):
        for a in BU.SN_EXACT_EXPONENTS:
            u = torch.zeros(1, rows, dtype=torch.float64)
            u[0, i] = 2.0 ** a
            s_want, u_want, v_want = BU.sn_exact_expect(W, i, a)
            sigma, u_new, v = _sigma(Wd, u, dev)
            assert_exact(sigma, s_want, f"sigma (row {i}, 2^{a})")
            assert_exact(u_new, u_want, f"u_new (row {i}, 2^{a})")
            assert_exact(v, v_want, f"v (row {i}, 2^{a})")


# ---------------------------------------------------------------------------------------------------------------- 4. minibatch std

def _mbstd_run(dev, monkeypatch, shape, cs):
    from style_big_gan_amd.train_parts import discriminators as PD

    def refuse(*a, **k):
        raise AssertionError("the tensor-op composition ran in place of the minibatch-std kernels")
    monkeypatch.setattr(PD, "_minibatch_std_composite", refuse)
    N, C, HW, G, F = shape
    x = cs["x"].float().to(dev).requires_grad_(True)
    y = PD.MinibatchStdLayer(G, F)(x)
    (dx,) = torch.autograd.grad(y, x, cs["dy"].float().to(dev))
    y2 = PD.MinibatchStdLayer(G, F)(x)
    (dx2,) = torch.autograd.grad(y2, x, cs["dy"].float().to(dev))
    assert torch.equal(y, y2) and torch.equal(dx, dx2)
    assert y.shape == (N, C + F, cs["side"], cs["side"]) and torch.equal(y[:, :C], x)             # the copy of x, bit for bit
    return y.detach(), dx


@pytest.mark.parametrize("shape", BU.MBSTD_EXACT, ids=lambda s: "x".join(map(str, s)))
def test_minibatch_std_exact(dev, monkeypatch, shape):
    """x = a + s[g] d with integer a, d in {1, 2, 4}, balanced signs: mean a, variance d^2, d^2 + 1e-8f = d^2 in fp32, sqrtf exact, and with
    c HW a power of two the statistic (the mean of d) is exact; the extra channel's dy sums to T c HW G per group, so dx = dy + T s[g]
    exactly.  (8, 32, 16, 2, 2) has M = 4 groups and F = 2 with a distinct statistic each: a swapped n = g M + m or F split changes it."""
    N, C, HW, G, F = shape
    cs = BU.mbstd_case(shape)
    y_want, dx_want = BU.mbstd_exact_expect(shape, cs)
    y, dx = _mbstd_run(dev, monkeypatch, shape, cs)
    assert_exact(y[:, C:], y_want[:, C:], "statistic channels")
    assert_exact(dx, dx_want, "dx")


def test_minibatch_std_ragged(dev, monkeypatch):
    """(6, 20, 9, 3, 2): G = 3 and c HW = 90, no power of two anywhere, so every division rounds (correctly, once): within 2 ulp of the
    float64 composition per element, statistic channels and dx"""
    shape = BU.MBSTD_RAGGED
    N, C, HW, G, F = shape
    cs = BU.mbstd_case(shape)
    y64, dx64 = BU.mbstd_composite64(cs["x"], G, F, cs["dy"])
    y, dx = _mbstd_run(dev, monkeypatch, shape, cs)
    for name, got, ref in (("statistic", y[:, C:], y64[:, C:]), ("dx", dx, dx64)):
        got, ref = got.cpu().double().numpy(), ref.numpy()
        ulps = np.abs(got - ref) / np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        print("mbstd ragged", name, "max ulp", float(ulps.max()))
        assert float(ulps.max()) <= 2.0, (name, float(ulps.max()))


# ---------------------------------------------------------------------------------------------------------------- 5. grouped GEMM

def _place(t, form, dev):
    """fp64 CPU matrix -> fp32 device matrix with unit column stride ('row') or unit row stride ('col': the transpose of a dense tensor)"""
    t = t.float()
    return t.contiguous().to(dev) if form == "row" else t.t().contiguous().to(dev).t()


@pytest.mark.parametrize("count,empty_at", BU.GG_TABLES)
def test_grouped_gemm_exact(dev, count, empty_at):
    """tables of exactly 16, 17 and 33 problems (one launch takes 16), and 17 with an M = 0 problem in the middle (16 non-empty: one
    launch): c and rowsum bit for bit the float64 result, for M, N in {63, 64, 65} and K in {15, 16, 17}, K0 = 0 (the bias alone, or zeros),
    a second term with K1 != K0, both stride forms of A and of B, a strided c whose neighbours stay NaN, row sums with three column tiles"""
    from style_big_gan_amd.torch_utils.ops import grouped_gemm
    table = BU.gg_table(count, empty_at)
    nan = float("nan")
    probs, fulls = [], []
    for pr in table:
        assert_range("c", pr["bound"], 1)
        m, n = pr["m"], pr["n"]
        full = torch.full([m, n + 3], nan, device=dev) if pr["strided_c"] else torch.full([m, n], nan, device=dev)
        c = full[:, 1:n + 1] if pr["strided_c"] else full
        terms = [(_place(a, pr["a_form"], dev), _place(b, pr["b_form"], dev), al) for a, b, al in pr["terms"]]
        for a, b, _ in terms:
            if min(a.shape) > 1 and min(b.shape) > 1:
                assert (a.stride(1) == 1) == (pr["a_form"] == "row") and (b.stride(0) == 1) == (pr["b_form"] == "col")
        dp = dict(c=c, terms=terms)
        if pr["bias"] is not None:
            dp["bias"], dp["bias_scale"] = pr["bias"].float().to(dev), pr["bias_scale"]
        if pr["rowsum"] is not None:
            dp["rowsum"], dp["rowsum_scale"] = torch.full([m], nan, device=dev), pr["rowsum_scale"]
        probs.append(dp); fulls.append(full)
    with expect_launch("grouped_gemm", lambda d: True, "grouped gemm") as log:
        grouped_gemm.launch(probs, dev)
    assert [r["dims"][0] for r in log if r["kind"] == "grouped_gemm"] == BU.GG_LAUNCHES[(count, empty_at)]
    for i, (pr, dp, full) in enumerate(zip(table, probs, fulls)):
        what = f"problem {i} (M {pr['m']}, N {pr['n']}, K {[t[0].shape[1] for t in pr['terms']]}, A {pr['a_form']}, B {pr['b_form']})"
        assert_exact(dp["c"], pr["c"], what + " c")
        if pr["strided_c"]:
            assert bool(torch.isnan(full[:, 0]).all()) and bool(torch.isnan(full[:, pr["n"] + 1:]).all()), what
        if pr["rowsum"] is not None:
            assert_exact(dp["rowsum"], pr["rowsum"], what + " rowsum")
