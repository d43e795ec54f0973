"""GPU: the fused DiffAugment kernels (csrc/diffaug.hip) against the float64 restatement of the published ops (tests/diffaug_util.py).

Exact mode: dyadic inputs and parameters make every intermediate value of the kernels exactly representable, so forward and adjoint
must equal the float64 reference bit for bit in any summation order.  Tolerance mode: random inputs at C = 3; the yardstick `e32` is the
error the fp32 torch composition on the CPU makes against float64 on the same inputs, the kernel gets max(4 e32, 8 * 2^-24 * max|y|)
(a different summation order in the mean and fma contraction, nothing more).  Measured kernel / e32 ratios (1 x MI355X): DESIGN.md
section 17."""
import itertools

import pytest
import torch

import style_big_gan_amd
from exact_util import U32, assert_exact, assert_range, expect_launch, qgrid
from style_big_gan_amd import _lib
from style_big_gan_amd.torch_utils.ops import diffaug as D
from style_big_gan_amd.train_parts import augmentations as A

import diffaug_util as U

pytestmark = pytest.mark.gpu


def _to(params, dev):
    return D.pack(params).to(dev)


# ---------------------------------------------------------------------------------------------------------------------------
# exact mode

def _exact_param_sets(gen, N, H, W):
    """every combination of the shifts {-lim, 0, +lim, the full extent (all zeros), an odd one} and rectangles {empty, the whole image,
    one touching each border}, in batches of N, with b a multiple of 1/8, s in {0, 0.5, 1, 2}, k in {0.5, 1, 1.5}"""
    lh, lw = int(H * 0.125 + 0.5), int(W * 0.125 + 0.5)
    shifts = [(-lh, -lw), (0, 0), (lh, lw), (H, 0), (0, -W), (lh, -lw), (-1, 3)]
    rects = [(0, 0, 0, 0), (0, H, 0, W), (0, H // 2, 1, W - 1), (H // 2, H, 1, W - 1), (1, H - 1, 0, W // 2), (1, H - 1, W // 2, W)]
    combos = list(itertools.product(shifts, rects))
    combos += combos[:(-len(combos)) % N]
    s_vals, k_vals = torch.tensor([0.0, 0.5, 1.0, 2.0]), torch.tensor([0.5, 1.0, 1.5])
    for i in range(0, len(combos), N):
        t = [c[0] for c in combos[i:i + N]]
        r = [c[1] for c in combos[i:i + N]]
        yield U.make_params(qgrid(gen, [N], -0.5, 0.5, 0.125), s_vals[torch.randint(0, 4, [N], generator=gen)],
                            k_vals[torch.randint(0, 3, [N], generator=gen)], t, r)


@pytest.mark.parametrize("shape", [(3, 1, 8, 16), (2, 4, 8, 8), (2, 4, 32, 64)], ids=lambda s: "x".join(map(str, s)))
def test_exact_forward_and_adjoint(dev, shape):
    N, C, H, W = shape
    n = C * H * W
    frac = 3 + (n.bit_length() - 1) + 1 + 2 + 1
    # Range.  x, b: multiples of 2^-3.  The sums: multiples of 2^-3 below n = 2^m in magnitude -> assert_range(n, 3).  M, S = sum / 2^m:
    # 3 + m fractional bits; (1 - k) halves it: + 1; the channel mean of w (C = 4): + 2; (1 - s) halves it: + 1.  With m = 13 that is
    # 20 fractional bits on values below 8: 23 bits.  (The forward alone needs 3 + m + 1 = 17.)
    assert n & (n - 1) == 0
    assert_range("diffaug sums", n, 3)
    assert_range("diffaug values", 8, frac)
    gen = torch.Generator().manual_seed(17 + n)
    variant_f, variant_a = ((4,), (5,)) if n <= 4096 else ((0, 1), (2, 3))
    for prm in _exact_param_sets(gen, N, H, W):
        x = qgrid(gen, [N, C, H, W], -1.0, 1.0, 0.125)
        g = qgrid(gen, [N, C, H, W], -1.0, 1.0, 0.125)
        y_ref, dx_ref = U.published_with_adjoint(x, g, prm)
        table = _to(prm, dev)
        with expect_launch("diffaug", lambda d: d[0] == variant_f[-1] and tuple(d[1:5]) == shape and d[5] == 1, "forward"):
            y = D.diffaug(x.float().to(dev), table)
        with expect_launch("diffaug", lambda d: d[0] == variant_a[-1] and tuple(d[1:5]) == shape and d[5] == 1, "adjoint"):
            dx = D.diffaug_adjoint(g.float().to(dev), table)
        assert_exact(y, y_ref, f"forward {shape} t={prm['t'].tolist()} rect={prm['rect'].tolist()}")
        assert_exact(dx, dx_ref, f"adjoint {shape} t={prm['t'].tolist()} rect={prm['rect'].tolist()}")
        full = (prm["t"][:, 0].abs() >= H) | (prm["t"][:, 1].abs() >= W)
        assert not bool(y[full.to(dev)].any())          # a shift of the full extent: all zeros


# ---------------------------------------------------------------------------------------------------------------------------
# tolerance mode

def _tolerance_case(shape):
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(N * 1000 + H * 10 + W)
    prm = U.random_params(gen, N, H, W)
    prm["t"][0] = torch.tensor([1, -1], dtype=torch.int32)      # an odd shift in both axes whatever was drawn
    x = torch.rand([N, C, H, W], generator=gen) * 2 - 1
    g = torch.randn([N, C, H, W], generator=gen)
    y64, dx64 = U.published_with_adjoint(x, g, prm)
    xr = x.clone().requires_grad_(True)                         # the fp32 torch composition on the CPU: the yardstick
    y32 = D.diffaug_reference(xr, prm)
    dx32, = torch.autograd.grad((y32 * g).sum(), xr)
    e32_y, e32_dx = float((y32.detach().double() - y64).abs().max()), float((dx32.double() - dx64).abs().max())
    return prm, x, g, y64, dx64, e32_y, e32_dx


@pytest.mark.parametrize("shape", [(4, 3, 6, 10), (3, 3, 13, 7), (8, 3, 32, 32), (2, 3, 64, 64)], ids=lambda s: "x".join(map(str, s)))
def test_tolerance_forward_and_adjoint(dev, shape):
    prm, x, g, y64, dx64, e32_y, e32_dx = _tolerance_case(shape)
    table = _to(prm, dev)
    xg = x.to(dev).requires_grad_(True)
    y = D.diffaug(xg, table)
    dx, = torch.autograd.grad((y * g.to(dev)).sum(), xg)        # the adjoint through autograd, as training runs it
    e_y, e_dx = float((y.detach().cpu().double() - y64).abs().max()), float((dx.cpu().double() - dx64).abs().max())
    b_y, b_dx = max(4 * e32_y, 8 * U32 * float(y64.abs().max())), max(4 * e32_dx, 8 * U32 * float(dx64.abs().max()))
    print(f"diffaug tolerance {shape}: forward err {e_y:.3e} e32 {e32_y:.3e} ratio {e_y / e32_y:.2f} bound {b_y:.3e} max|y| {float(y64.abs().max()):.2f}; "
          f"adjoint err {e_dx:.3e} e32 {e32_dx:.3e} ratio {e_dx / e32_dx:.2f} bound {b_dx:.3e}")
    assert e_y <= b_y and e_dx <= b_dx, (e_y, b_y, e_dx, b_dx)


# ---------------------------------------------------------------------------------------------------------------------------
# identity, batch independence

def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def test_identity_returns_the_input_bits(dev):
    torch.manual_seed(0)
    for shape in [(3, 3, 32, 32), (2, 3, 13, 7), (2, 3, 64, 64), (2, 1, 9, 12)]:
        x = torch.randn(shape, device=dev)
        assert _bits_equal(D.diffaug(x, _to(D.identity_params(shape[0]), dev)), x), shape
        pipe = A.DiffAugmentPipe(color=1, translation=1, cutout=1).to(dev)
        pipe.p.copy_(torch.as_tensor(0.0))
        assert _bits_equal(pipe(x), x), shape
    xh = torch.randn(2, 3, 16, 16, device=dev).to(torch.bfloat16)          # cast to fp32 and back: still the same values
    yh = D.diffaug(xh, _to(D.identity_params(2), dev))
    assert yh.dtype == torch.bfloat16 and torch.equal(yh, xh)


@pytest.mark.parametrize("shape", [(6, 3, 16, 16), (3, 3, 36, 40)], ids=lambda s: "x".join(map(str, s)))
def test_batch_independence_and_reproducibility(dev, shape):
    """a sample's bits depend on neither the batch size, its place in the batch nor the run (the second shape takes the two-launch path)"""
    N, C, H, W = shape
    gen = torch.Generator().manual_seed(9)
    prm = U.random_params(gen, N, H, W)
    x = (torch.rand(shape, generator=gen) * 2 - 1).to(dev)
    g = torch.randn(shape, generator=gen).to(dev)
    table = _to(prm, dev)
    y, dx = D.diffaug(x, table), D.diffaug_adjoint(g, table)
    assert _bits_equal(D.diffaug(x, table), y) and _bits_equal(D.diffaug_adjoint(g, table), dx)
    for n in range(N):
        tn = table[n:n + 1].contiguous()
        assert _bits_equal(D.diffaug(x[n:n + 1].contiguous(), tn), y[n:n + 1]), n
        assert _bits_equal(D.diffaug_adjoint(g[n:n + 1].contiguous(), tn), dx[n:n + 1]), n


# ---------------------------------------------------------------------------------------------------------------------------
# second order, launch records, validation

def _r1_chain(x, q, fn):
    """the chain of test_pipe_second_order_matches_oracle: a nonlinear head, then |d/dx|^2 -> (d, dr1/dq, dr1/dx)"""
    y = fn(x)
    d, = torch.autograd.grad((y * y * q).sum(), x, create_graph=True)
    r1 = d.square().sum()
    gq, gx = torch.autograd.grad(r1, [q, x])
    return d.detach(), gq, gx


def test_second_order_matches_the_reference_chain(dev):
    """R1 differentiates the discriminator's input gradient through the pipe.  Reference: the same chain through `diffaug_reference` in
    float64; bound: 4 x the error of that chain in fp32 on the CPU, per tensor of the chain (max abs)."""
    N, C, H, W = 4, 3, 16, 16
    gen = torch.Generator().manual_seed(21)
    prm = U.random_params(gen, N, H, W)
    x0 = torch.rand([N, C, H, W], generator=gen) * 2 - 1
    q0 = torch.randn([N, C, H, W], generator=gen)
    ref = _r1_chain(x0.double().requires_grad_(True), q0.double().requires_grad_(True), lambda t: D.diffaug_reference(t, prm))
    f32 = _r1_chain(x0.clone().requires_grad_(True), q0.clone().requires_grad_(True), lambda t: D.diffaug_reference(t, prm))
    table = _to(prm, dev)
    with expect_launch("diffaug", lambda d: d[0] == 4, "forward"), expect_launch("diffaug", lambda d: d[0] == 5, "adjoint"):
        got = _r1_chain(x0.to(dev).requires_grad_(True), q0.to(dev).requires_grad_(True), lambda t: D.diffaug(t, table))
    for name, a, b, r in zip(("d", "dr1/dq", "dr1/dx"), got, f32, ref):
        e, e32 = float((a.cpu().double() - r).abs().max()), float((b.double() - r).abs().max())
        print(f"diffaug second order {name}: err {e:.3e} e32 {e32:.3e} ratio {e / e32:.2f}")
        assert e <= 4 * e32, (name, e, e32)


def test_launch_records_cover_forward_adjoint_and_double_backward(dev):
    for shape, fwd, adj in [((2, 3, 16, 16), (4,), (5,)), ((2, 3, 48, 48), (0, 1), (2, 3)), ((2, 3, 13, 7), (4,), (5,))]:
        access = 1 if shape[3] % 4 == 0 else 2
        prm = U.random_params(torch.Generator().manual_seed(1), *[shape[0], shape[2], shape[3]])
        table = _to(prm, dev)
        x = torch.randn(shape, device=dev, requires_grad=True)
        gy = torch.randn(shape, device=dev, requires_grad=True)
        key = lambda v: (lambda d: d[0] == v and tuple(d[1:5]) == shape and d[5] == access)
        with expect_launch("diffaug", key(fwd[0]), "forward") as log, expect_launch("diffaug", key(fwd[-1]), "forward"):
            y = D.diffaug(x, table)
        assert [r["dims"][0] for r in log if r["kind"] == "diffaug"] == list(fwd)
        with expect_launch("diffaug", key(adj[0]), "adjoint") as log, expect_launch("diffaug", key(adj[-1]), "adjoint"):
            dx, = torch.autograd.grad(y, x, gy, create_graph=True)
        assert [r["dims"][0] for r in log if r["kind"] == "diffaug"] == list(adj)
        with expect_launch("diffaug", key(fwd[0]), "double backward") as log, expect_launch("diffaug", key(fwd[-1]), "double backward"):
            ddy, = torch.autograd.grad(dx, gy, torch.ones_like(dx))
        assert [r["dims"][0] for r in log if r["kind"] == "diffaug"] == list(fwd)       # the forward form again, served by the kernels
        # ... without the brightness offset: it is the linear part applied to ones
        want = D.diffaug(torch.ones_like(x), table) - D.diffaug(torch.zeros_like(x), table)
        assert float((ddy - want).abs().max()) <= 1e-5


def test_validation_before_any_launch(dev):
    x = torch.randn(2, 3, 8, 8, device=dev)
    table = _to(D.identity_params(2), dev)
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    _lib.prof_fetch()
    try:
        with pytest.raises(RuntimeError, match="diffaug"):
            D.diffaug(x.permute(0, 1, 3, 2), table)                      # not dense
        with pytest.raises(RuntimeError, match="diffaug"):
            D.diffaug(x, table.cpu())                                    # a packed table on another device
        with pytest.raises(RuntimeError, match="diffaug"):
            D.diffaug(x, table[:1])                                      # wrong batch size
        with pytest.raises(RuntimeError, match="diffaug"):
            D.diffaug(x, table.float())                                  # wrong dtype
        with pytest.raises(RuntimeError, match="diffaug"):
            D.diffaug(torch.randn(2, 5, 8, 8, device=dev), table)        # 5 channels
        torch.cuda.synchronize()
        assert not [r for r in _lib.prof_fetch() if r["kind"] == "diffaug"]
    finally:
        _lib.prof_enable(False)
    # extreme integers are safe: nothing is read outside the image, the result is zeros / a clipped rectangle
    big = 2 ** 31 - 1
    prm = U.make_params([0.0, 0.0], [1.0, 1.0], [1.0, 1.0], [[big, -big - 1], [0, 0]], [[0, 0, 0, 0], [-big, big, 4, big]])
    y = D.diffaug(x, _to(prm, dev))
    assert not bool(y[0].any()) and not bool(y[1, :, :, 4:].any()) and _bits_equal(y[1, :, :, :4], x[1, :, :, :4])


# ---------------------------------------------------------------------------------------------------------------------------
# the training step

def _engine(dev, **kw):
    from style_big_gan_amd.torch_utils import training_stats
    from style_big_gan_amd.train_parts import trainers
    gk = dict(z_dim=64, c_dim=0, w_dim=64, img_resolution=32, img_channels=3, mapping_kwargs=dict(num_layers=2),
              synthesis_kwargs=dict(channel_base=1024, channel_max=64, num_fp16_res=2, block_kwargs=dict(conv_clamp=256)))
    dk = dict(c_dim=0, img_resolution=32, img_channels=3, architecture='orig', channel_base=1024, channel_max=64, num_fp16_res=2,
              conv_clamp=256, epilogue_kwargs=dict(mbstd_group_size=4))
    training_stats.init_multiprocessing(rank=0, sync_device=None)
    return trainers.StepEngine(dev, gen_kwargs=gk, disc_kwargs=dk, loss_arch_kwargs=dict(style_mixing_prob=0), dis_regs=[('r1', dict(r1_gamma=0.01))],
                               d_reg_interval=2, batch=8, batch_gpu=4, augment_type="diffaug",
                               augment_kwargs=dict(A.diffaug_specs["color_translation_cutout"]), **kw)


def test_training_step_with_diffaug(dev):
    """StepEngine as in test_training_step_with_ada, with the DiffAugment pipe at p = 1 in front of D and R1 running through it"""
    eng = _engine(dev, augment_p=1.0)
    assert isinstance(eng.augment_pipe, A.DiffAugmentPipe) and eng.loss.augment_pipe is eng.augment_pipe and float(eng.augment_pipe.p) == 1.0
    before = [p.detach().clone() for p in eng.D.parameters()]
    gen = torch.Generator(device=dev); gen.manual_seed(5)
    with expect_launch("diffaug", lambda d: d[0] == 4, "forward in the step"), expect_launch("diffaug", lambda d: d[0] == 5, "adjoint in the step"):
        for _ in range(3):
            eng.train_iteration(torch.rand([8, 3, 32, 32], device=dev, generator=gen) * 2 - 1, None)
    assert all(torch.isfinite(p).all() for p in list(eng.G.parameters()) + list(eng.D.parameters()))
    assert sum(float((a - b).abs().sum()) for a, b in zip(before, eng.D.parameters())) > 0
    assert float(eng.augment_pipe.p) == 1.0 and eng.augment_pipe._strength() == 1.0

    eng = _engine(dev, augment_p=1.0, ada_target=0.6, ada_interval=2, ada_kimg=0.1)         # the ADA heuristic moves this pipe's p as well
    strengths = []
    for _ in range(2):
        eng.train_iteration(torch.rand([8, 3, 32, 32], device=dev, generator=gen) * 2 - 1, None)
        strengths.append(float(eng.augment_pipe.p))
    step = 8 * 2 / (0.1 * 1000)
    assert strengths[0] == pytest.approx(1.0) and abs(abs(strengths[1] - 1.0) - step) < 1e-5
    assert all(torch.isfinite(p).all() for p in list(eng.G.parameters()) + list(eng.D.parameters()))
