"""Non-local attention above 32x32 (more than 256 keys) on the streamed (online-softmax) HIP kernels: sbg_attention_fwd / sbg_attention_bwd
at M > 256, through attention_core, layers.Attention and whole networks.

Bounds of the op tests: max_rel < 1e-5 against the float64 composition on the CPU, forward and per gradient -- the bound the single-chunk
kernels are held to in tests/test_biggan_gpu.py.  Measured on an MI355X at the five shapes below (seed 11), largest figure over
the shapes: streamed kernels forward 3.2e-6, dtheta 2.6e-6, dphi 3.2e-6, dg 1.8e-6 (each shape's figures are printed by the test).
The bound held with room to spare, so the fall-back rule (4x the fp32 torch composition's own error) was not needed."""
import warnings

import numpy as np
import pytest
import torch

import style_big_gan_amd  # noqa: F401
from golden_util import max_rel
from style_big_gan_amd import _lib
from style_big_gan_amd.biggan import layers as L
from style_big_gan_amd.train_parts import trainers

pytestmark = pytest.mark.gpu

_reference = L._attention_reference          # the float64 oracle on the CPU; the device runs below must never reach it

STREAM_SHAPES = [(2, 48, 272, 4, 16), (1, 64, 512, 24, 32), (2, 128, 528, 16, 64), (1, 4096, 1024, 16, 64), (1, 256, 1024, 64, 256)]


def _attention_log(fn):
    """run fn with the launch log on -> (result, [(variant name, dims)] of the attention records)"""
    _lib.prof_enable(True)
    _lib.prof_fetch()
    try:
        res = fn()
        torch.cuda.synchronize()
        recs = [(_lib.ATT_VARIANTS[r["dims"][6]], r["dims"]) for r in _lib.prof_fetch() if r["kind"] == "attention"]
    finally:
        _lib.prof_enable(False)
    return res, recs


def _no_composition(monkeypatch, aten=True):
    """from here on the torch bmm / softmax / bmm composition raises instead of running in a kernel's place; aten: torch.bmm and
    F.softmax themselves raise as well (op-level tests, where nothing else may call them)"""
    def refuse(*a, **k):
        raise AssertionError("the torch composition ran in place of the HIP attention kernels")
    monkeypatch.setattr(L, "_attention_reference", refuse)
    if aten:
        monkeypatch.setattr(torch, "bmm", refuse)
        monkeypatch.setattr(torch.nn.functional, "softmax", refuse)


@pytest.mark.parametrize("shape", STREAM_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_stream_against_fp64(dev, monkeypatch, shape):
    n, q, m, d, dv = shape
    lib = _lib.load()
    assert lib.sbg_attention_supported(q, m, d, dv) and lib.sbg_attention_bwd_supported(q, m, d, dv)
    gen = torch.Generator().manual_seed(11)
    ins = [torch.randn(n, q, d, generator=gen), torch.randn(n, m, d, generator=gen), torch.randn(n, m, dv, generator=gen)]
    dout = torch.randn(n, q, dv, generator=gen)
    ref_in = [t.double().requires_grad_(True) for t in ins]
    ref_out = _reference(*ref_in)
    ref = torch.autograd.grad(ref_out, ref_in, dout.double())
    _no_composition(monkeypatch)
    dev_in = [t.to(dev).requires_grad_(True) for t in ins]

    def run():
        out = L.attention_core(*dev_in)
        return out, torch.autograd.grad(out, dev_in, dout.to(dev))

    (out, got), recs = _attention_log(run)
    assert [(v, dims[:6]) for v, dims in recs] == [("stream", (n, q, m, d, dv, 0)), ("stream_stats", (n, q, m, d, dv, 1)),
                                                   ("stream_dq", (n, q, m, d, dv, 1)), ("stream_dkv", (n, q, m, d, dv, 1))], recs
    errs = dict(out=max_rel(out, ref_out.float()))
    for name, a, b in zip(("dtheta", "dphi", "dg"), got, ref):
        errs[name] = max_rel(a, b.float())
    print("stream", shape, {k: f"{v:.2e}" for k, v in errs.items()})
    assert all(e < 1e-5 for e in errs.values()), (shape, errs)
    again = run()[1]                                     # fixed summation order, no atomics: the same bits
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_spiky_logits_across_chunks(dev, monkeypatch):
    """|logit| ~ 1e4, M = 528 (the last chunk is the 16-key remainder): the row maximum sits in the last chunk for the even rows and in the
    first chunk for the odd rows, so a rescale in the wrong direction, or none, leaves a wrong row"""
    gen = torch.Generator().manual_seed(5)
    n, q, m, d, dv = 2, 64, 528, 16, 32
    t = torch.randn(n, q, d, generator=gen) * 30; p = torch.randn(n, m, d, generator=gen) * 30; gg = torch.randn(n, m, dv, generator=gen)
    k_first, k_last = 5, 520
    t[:, :, :2] = 0; p[:, :, :2] = 0
    t[:, 0::2, 1] = 150; t[:, 1::2, 0] = 150             # even rows look along axis 1, odd rows along axis 0
    p[:, k_first, 0] = 150; p[:, k_last, 1] = 150
    arg = torch.bmm(t.double(), p.double().transpose(1, 2)).argmax(-1)
    assert bool((arg[:, 0::2] == k_last).all()) and bool((arg[:, 1::2] == k_first).all())
    ref = _reference(t.double(), p.double(), gg.double()).float()
    _no_composition(monkeypatch)
    out, recs = _attention_log(lambda: L.attention_core(t.to(dev), p.to(dev), gg.to(dev)))
    assert [v for v, _ in recs] == ["stream"]
    assert max_rel(out, ref) < 1e-3


def test_exact_uniform_softmax(dev, monkeypatch):
    """theta = 0: every logit is 0, the softmax is uniform and out is the mean of g.  With small integers in g every product and sum is
    exact in fp32 (|sum| <= 8 * 512 < 2^24), the only rounding is the final division by the row sum: at most 1 ulp from the correctly
    rounded mean, for every key chunk and output column."""
    n, q, m, d, dv = 2, 48, 512, 8, 48
    gg = torch.randint(-8, 9, (n, m, dv), generator=torch.Generator().manual_seed(7)).float()
    assert len({tuple(r.tolist()) for r in gg.reshape(n * m, dv)}) == n * m        # a distinct integer pattern per key
    want = gg.double().mean(1, keepdim=True).expand(n, q, dv).float().numpy()
    _no_composition(monkeypatch)
    out, recs = _attention_log(lambda: L.attention_core(torch.zeros(n, q, d, device=dev), torch.randn(n, m, d, device=dev), gg.to(dev)))
    assert [v for v, _ in recs] == ["stream"]
    got = out.cpu().numpy()
    assert np.all(np.abs(got - want) <= np.spacing(np.abs(want))), float(np.abs(got - want).max())


def test_small_shapes_keep_the_single_chunk_kernels(dev):
    for (n, q, m, d, dv) in [(3, 1024, 256, 16, 64), (2, 64, 16, 4, 16)]:
        ins = [torch.randn(n, q, d, device=dev, requires_grad=True), torch.randn(n, m, d, device=dev, requires_grad=True),
               torch.randn(n, m, dv, device=dev, requires_grad=True)]
        _, recs = _attention_log(lambda: torch.autograd.grad(L.attention_core(*ins).sum(), ins))
        assert [(v, dims[5]) for v, dims in recs] == [("single", 0), ("single", 1)], recs
    t, p, gg = torch.randn(1, 16, 4), torch.randn(1, 512, 4), torch.randn(1, 512, 16)
    assert torch.equal(L.attention_core(t, p, gg), _reference(t, p, gg))        # on the CPU attention_core is the composition


def test_unsupported_cuda_shape_warns_once(dev):
    """a CUDA shape outside the contract (M = 264 is no multiple of 16) takes the composition, and says so once per shape"""
    t, p, gg = torch.randn(1, 16, 4, device=dev), torch.randn(1, 264, 4, device=dev), torch.randn(1, 264, 16, device=dev)
    L._composition_warned.discard(("forward", (16, 264, 4, 16)))
    with pytest.warns(UserWarning, match="M=264"):
        out = L.attention_core(t, p, gg)
    assert max_rel(out, _reference(t.double().cpu(), p.double().cpu(), gg.double().cpu()).float()) < 1e-5
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        L.attention_core(t, p, gg)


def test_attention_module_64x64(dev):
    """layers.Attention(32) on [1, 32, 64, 64] (Q 4096, M 1024, D 4, DV 16) against the float64 restatement of the module on the CPU
    (oracle/biggan.py, same state dict): activations 2e-4, gradients 2e-3, the second-order gradient through create_graph=True 1e-2"""
    from oracle import biggan as OB
    torch.manual_seed(3)
    att = L.Attention(32)
    torch.nn.init.constant_(att.gamma, 0.5)
    x = torch.randn(1, 32, 64, 64)
    sd = {"a." + k: v.detach().double() for k, v in att.state_dict().items()}
    names = [k for k, _ in att.named_parameters()]
    for k in names:
        sd["a." + k].requires_grad_(True)
    xr = x.double().requires_grad_(True)
    yr = OB.attention(sd, "a", xr, True, {})
    ref = torch.autograd.grad(yr.square().sum(), [xr] + [sd["a." + k] for k in names], create_graph=True)
    ref2 = torch.autograd.grad(ref[0].square().sum(), xr)[0]

    att = att.to(dev).train()
    xd = x.to(dev).requires_grad_(True)
    params = dict(att.named_parameters())

    def run():
        y = att(xd)
        return y, torch.autograd.grad(y.square().sum(), [xd] + [params[k] for k in names])

    (y, got), recs = _attention_log(run)
    assert [v for v, _ in recs] == ["stream", "stream_stats", "stream_dq", "stream_dkv"], recs
    assert max_rel(y, yr.float()) < 2e-4
    for k, a, b in zip(["x"] + names, got, ref):
        assert max_rel(a, b.float()) < 2e-3, k
    att.load_state_dict({k[2:]: v.detach().float() for k, v in sd.items()})     # the power iteration advanced u0 in the first pass
    y2 = att(xd)
    (gx,) = torch.autograd.grad(y2.square().sum(), xd, create_graph=True)
    g2 = torch.autograd.grad(gx.square().sum(), xd)[0]
    assert bool(torch.isfinite(g2).all()) and max_rel(g2, ref2.float()) < 1e-2


def test_no_map_in_memory(dev):
    """forward + backward at (4, 4096, 1024, 16, 64): inputs, outputs, gradients and row statistics are under 10 MiB; the [N, Q, M] fp32 map
    alone is 64 MiB, so staying below it means no map was allocated"""
    n, q, m, d, dv = 4, 4096, 1024, 16, 64
    ins = [torch.randn(n, q, d, device=dev, requires_grad=True), torch.randn(n, m, d, device=dev, requires_grad=True),
           torch.randn(n, m, dv, device=dev, requires_grad=True)]
    dout = torch.randn(n, q, dv, device=dev)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    grads = torch.autograd.grad(L.attention_core(*ins), ins, dout)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated(dev) - base
    assert all(bool(torch.isfinite(g).all()) for g in grads)
    assert peak < n * q * m * 4, peak


def _finite_and_moved(eng, before_g, before_d):
    for net, before in ((eng.G, before_g), (eng.D, before_d)):
        assert all(bool(torch.isfinite(p).all()) for p in net.parameters())
        assert sum(float((a - b).abs().sum()) for a, b in zip(before, net.parameters())) > 0


def _one_iteration(eng, real, c):
    for mod in list(eng.G.modules()) + list(eng.D.modules()):
        if type(mod).__name__ == "Attention":
            torch.nn.init.constant_(mod.gamma, 0.5)          # gamma starts at 0 (identity); open the branch
    bg, bd = [p.detach().clone() for p in eng.G.parameters()], [p.detach().clone() for p in eng.D.parameters()]
    _, recs = _attention_log(lambda: eng.train_iteration(real, c))
    _finite_and_moved(eng, bg, bd)
    eng.close()
    return [v for v, _ in recs]


def test_sg2_classic_with_attention_at_64(dev, monkeypatch):
    """a tiny sg2_classic pair at 64x64 with attentions=[64] in G and D.  G's block attends after its up-sampling, at 64x64 (Q 4096, M 1024):
    streamed, forward and backward.  D's block attends after its down-sampling, at 32x32 (M 256): the single-chunk kernels, as before.
    No attention launch of the iteration leaves the library."""
    gk = dict(z_dim=32, c_dim=0, w_dim=32, img_resolution=64, img_channels=3, attentions=[64], mapping_kwargs=dict(num_layers=2),
              synthesis_kwargs=dict(channel_base=2048, channel_max=32, num_fp16_res=8, block_kwargs=dict(conv_clamp=256)))
    dk = dict(c_dim=0, img_resolution=64, img_channels=3, attentions=[64], architecture="orig", channel_base=2048, channel_max=32, num_fp16_res=8,
              conv_clamp=256, epilogue_kwargs=dict(mbstd_group_size=4))
    eng = trainers.StepEngine(dev, gen_kwargs=gk, disc_kwargs=dk, loss_arch_kwargs=dict(style_mixing_prob=0), dis_regs=[], g_reg_interval=16,
                              d_reg_interval=4, batch=4, batch_gpu=4, ema_kimg=0.02)      # no regulariser: the reg slots idle, every pass is first order
    _no_composition(monkeypatch, aten=False)
    variants = _one_iteration(eng, torch.rand(4, 3, 64, 64, device=dev) * 2 - 1, None)
    assert set(variants) == {"single", "stream", "stream_stats", "stream_dq", "stream_dkv"}, variants


def test_big_gan_with_attention_at_64(dev, monkeypatch):
    """a tiny big_gan at 64x64 with G_attn='64' (the canonical placement; ch 16 -> Attention(32))"""
    opt = ("adam", dict(lr=2e-4, betas=[0.0, 0.999], eps=1e-8))
    eng = trainers.StepEngine(dev, generator="big_gan", discriminator="big_gan", loss_arch="base", loss="hinge", loss_arch_kwargs=dict(),
                              gen_kwargs=dict(c_dim=10, img_resolution=64, G_ch=16, G_shared=False, G_attn="64", G_init="N02", n_classes=10),
                              disc_kwargs=dict(c_dim=10, img_resolution=64, D_ch=16, D_attn="0", D_init="N02", n_classes=10), optim_gen=opt, optim_disc=opt,
                              gen_regs=[], dis_regs=[], g_reg_interval=0, d_reg_interval=0, n_dis=1, batch=4, batch_gpu=4, ema_kimg=0.02)
    _no_composition(monkeypatch, aten=False)
    c = torch.nn.functional.one_hot(torch.arange(4, device=dev) % 10, 10).float()
    variants = _one_iteration(eng, torch.rand(4, 3, 64, 64, device=dev) * 2 - 1, c)
    assert variants and set(variants) == {"stream", "stream_stats", "stream_dq", "stream_dkv"}, variants
