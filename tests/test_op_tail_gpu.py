"""GPU: the wiring of the op layer's records through the fused autograd Functions (values are held elsewhere: test_fused_modconv_training_layer,
test_fused_up_synthesis_layer, test_conv_bias_act_backward_exact, test_synthesis_block_chained_backward_heads).

* the transposed low-pass of _FirBiasAct.backward and of the fallback of _ConvBiasActFir.backward is the launch _Upfirdn2d.backward makes;
* every fused Function hands back a gradient of the operand's own dtype and shape for each differentiable operand that asks for one, None otherwise.
"""
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import style_big_gan_amd  # noqa: E402,F401
from style_big_gan_amd.torch_utils.ops import bias_act, conv2d_resample, conv_bias_act, fromrgb, modconv, upfirdn2d  # noqa: E402
from style_big_gan_amd.train_parts import generators as PG  # noqa: E402

pytestmark = pytest.mark.gpu
BF, CL = torch.bfloat16, torch.channels_last
N, C, R = 2, 64, 16


def _bf16_cl(*shape, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g).to(dev, BF).contiguous(memory_format=CL)


@pytest.mark.parametrize("pad", [1, 2])
def test_unit_rate_adjoint_is_the_upfirdn2d_backward(dev, pad, monkeypatch):
    """The gradient tensor is bf16 channels-last 2 x 64 x 16 x 16, the filter outer([1, 3, 3, 1]), the forward low-pass has pads (p, p, p, p) and gain 4
    (so its input is 17 x 17 for p = 1, 15 x 15 for p = 2).  Three ways to the gradient of the low-pass's input: upfirdn2d's own backward; the fused
    tail _FirBiasAct with an identity tail (linear, gain 1, no clamp, no operands: its backward head passes dy through unchanged); _ConvBiasActFir
    behind an identity 1 x 1 convolution with an identity tail, its one-launch backward switched off so that the composition runs.  All three make
    the same transposed-FIR launch on the same values, and the kernels are deterministic: bit for bit."""
    f = upfirdn2d.setup_filter([1, 3, 3, 1], device=dev)
    h = R + 3 - 2 * pad
    x0 = _bf16_cl(N, C, h, h, dev=dev, seed=pad)
    dy = _bf16_cl(N, C, R, R, dev=dev, seed=10 + pad)

    def grad_of(fn):
        x = x0.clone(memory_format=torch.preserve_format).requires_grad_(True)
        y = fn(x)
        assert y.shape == dy.shape
        return y, torch.autograd.grad(y, x, dy)[0]

    y_ref, ref = grad_of(lambda x: upfirdn2d.upfirdn2d(x, f, padding=[pad] * 4, gain=4.0))
    assert type(y_ref.grad_fn).__name__ == "_Upfirdn2dBackward"

    y_a, got_a = grad_of(lambda x: upfirdn2d.fir_bias_act(x, f, [pad] * 4, 4.0, None, None, None, act="linear", alpha=0.0, act_gain=1.0, clamp=-1.0))
    assert type(y_a.grad_fn).__name__ == "_FirBiasActBackward"
    assert got_a.shape == ref.shape and got_a.dtype == ref.dtype and torch.equal(got_a, ref)

    monkeypatch.setattr(upfirdn2d, "fir_transposed_dact", lambda *a, **k: None)         # the fallback is the subject
    eye = torch.eye(C, device=dev, dtype=BF).reshape(C, C, 1, 1)
    y_b, got_b = grad_of(lambda x: conv_bias_act.conv2d_bias_act_fir(x, eye, None, f, [pad] * 4, act="linear", fgain=4.0))
    assert type(y_b.grad_fn).__name__ == "_ConvBiasActFirBackward"
    assert got_b.shape == ref.shape and got_b.dtype == ref.dtype and torch.equal(got_b, ref)


def _leaf(t, grad=True):
    return t.detach().clone(memory_format=torch.preserve_format).requires_grad_(grad)


def _conv_case(dev, monkeypatch, skip, with_fir):
    """_ConvBiasAct / _ConvBiasActFir (first_order on), fp32 master weight and bias with bf16 activations: x, w, b"""
    monkeypatch.setattr(conv_bias_act, "first_order", True)
    g = torch.Generator().manual_seed(1)
    x = _leaf(_bf16_cl(N, C, R, R, dev=dev, seed=2), skip != "x")
    w = _leaf(torch.randn(C, C, 3, 3, generator=g).to(dev), skip != "w")
    b = _leaf(torch.randn(C, generator=g).to(dev), skip != "b")
    if not with_fir:
        assert conv_bias_act.fusable(x, w, "lrelu")
        return conv_bias_act.conv2d_bias_act(x, w, b, padding=1, act="lrelu", clamp=4.0, wgain=0.05), [x, w, b]
    f = upfirdn2d.setup_filter([1, 3, 3, 1], device=dev)
    assert conv_bias_act.fir_fusable(x, w, "lrelu", f)
    return conv_bias_act.conv2d_bias_act_fir(x, w, b, f, conv2d_resample.lowpass_padding(f, 2, 1), padding=1, act="lrelu", clamp=4.0, wgain=0.05), [x, w, b, None]


def _modconv_case(dev, monkeypatch, skip, per_sample):
    """_ModConvBiasAct: x, w, styles, dcoefs, noise (per sample / constant), b"""
    g = torch.Generator().manual_seed(3)
    x = _leaf(_bf16_cl(N, C, R, R, dev=dev, seed=4))
    w = _leaf(torch.randn(C, C, 3, 3, generator=g).to(dev))
    styles = _leaf(torch.randn(N, C, generator=g).to(dev))
    dcoefs = _leaf(torch.rand(N, C, generator=g).to(dev) + 0.5, skip != "dcoefs")
    noise = _leaf(torch.randn([N, 1, R, R] if per_sample else [R, R], generator=g).to(dev), skip != "noise")
    b = _leaf(torch.randn(C, generator=g).to(dev), skip != "b")
    assert modconv.usable(x, w, "lrelu", 1)
    return modconv.modconv_bias_act(x, w, styles, dcoefs, noise, b, padding=1, act="lrelu", clamp=4.0), [x, w, styles, dcoefs, noise, b]


def _fir_case(dev, monkeypatch, skip, per_sample):
    """_FirBiasAct as SynthesisLayer(up=2) reaches it: t (the transposed convolution's output), dcoefs, noise (per sample / constant), b"""
    torch.manual_seed(5)
    layer = PG.SynthesisLayer(in_channels=C, out_channels=C, w_dim=32, resolution=R, up=2, conv_clamp=256).to(dev)
    with torch.no_grad():
        layer.noise_strength.fill_(0.3)
    layer.noise_strength.requires_grad_(skip != "noise")
    layer.bias.requires_grad_(skip != "b")
    seen = {}
    inner = upfirdn2d.fir_bias_act

    def recording(x, f, padding, gain, dcoefs, noise, b, *a, **k):
        seen["operands"] = [x, None, dcoefs, noise, b]
        return inner(x, f, padding, gain, dcoefs, noise, b, *a, **k)
    monkeypatch.setattr(upfirdn2d, "fir_bias_act", recording)
    x = _bf16_cl(N, C, R // 2, R // 2, dev=dev, seed=6).requires_grad_(True)
    y = layer(x, torch.randn(N, 32, device=dev), noise_mode="random" if per_sample else "const")
    assert y.shape == (N, C, R, R) and "operands" in seen, "the fused low-pass tail did not take the layer"
    t, _, dcoefs, noise, b = seen["operands"]
    assert t.requires_grad and dcoefs.requires_grad and noise.requires_grad == (skip != "noise") and b.requires_grad == (skip != "b")
    assert tuple(noise.shape) == ((N, 1, R, R) if per_sample else (R, R))
    return y, seen["operands"]


def _fromrgb_case(dev, monkeypatch, skip, _):
    """_FromRGB: the fp32 planar image, the [Co, Ci] weight, the bias"""
    monkeypatch.setattr(fromrgb, "enabled", True)
    g = torch.Generator().manual_seed(7)
    img = _leaf(torch.randn(N, 3, R, R, generator=g).to(dev), skip != "img")
    w2d = _leaf(torch.randn(C, 3, generator=g).to(dev), skip != "w")
    b = _leaf(torch.randn(C, generator=g).to(dev), skip != "b")
    assert fromrgb.usable(img, w2d.reshape(C, 3, 1, 1), "lrelu", BF)
    return fromrgb._FromRGB.apply(img, w2d, b, bias_act.Act.make("lrelu", clamp=4.0), BF), [img, w2d, b]


# (Function, how to reach it, variant, its name, the operands left without requires_grad in turn; None = all requested)
PRESENCE = [("_ConvBiasAct", _conv_case, False, "plain", (None, "x", "w", "b")),
            ("_ConvBiasActFir", _conv_case, True, "lowpass", (None, "x", "w", "b")),
            ("_ModConvBiasAct", _modconv_case, True, "noise_per_sample", (None, "dcoefs", "noise", "b")),
            ("_ModConvBiasAct", _modconv_case, False, "noise_const", (None, "noise")),
            ("_FirBiasAct", _fir_case, True, "noise_per_sample", (None, "noise", "b")),
            ("_FirBiasAct", _fir_case, False, "noise_const", (None, "noise")),
            ("_FromRGB", _fromrgb_case, None, "plain", (None, "img", "w", "b"))]


@pytest.mark.parametrize("name,case,variant,skip", [(n, c, v, s) for n, c, v, _, skips in PRESENCE for s in skips],
                         ids=[f"{n}-{label}-{'all' if s is None else 'no_' + s}" for n, _, _, label, skips in PRESENCE for s in skips])
def test_fused_functions_return_their_gradients(dev, monkeypatch, name, case, variant, skip):
    """Each fused Function returns, for every differentiable operand that requires grad, a gradient of the operand's own dtype and shape, and None
    for one that does not (and for every non-tensor argument).  N = 2, 64 channels, 16 x 16: the smallest shapes at which the fused paths engage
    (64-channel blocks; 16 rows for the low-pass tails), with per-sample and with constant noise where there is noise.  The backward
    is called as the engine calls it (grad mode off) and its result is read BEFORE the engine validates or casts it.  Presence, dtype and shape
    only: the values are held by the tests named in the module docstring."""
    y, operands = case(dev, monkeypatch, skip, variant)
    assert type(y.grad_fn).__name__ == name + "Backward", type(y.grad_fn).__name__
    with torch.no_grad():
        grads = y.grad_fn.apply(torch.randn_like(y))
    assert len(grads) >= len(operands) and all(g is None for g in grads[len(operands):])
    for i, (t, g) in enumerate(zip(operands, grads)):
        if t is None or not t.requires_grad:
            assert g is None, (name, i)
        else:
            assert g is not None, (name, i)
            assert g.dtype == t.dtype and g.shape == t.shape, (name, i, g.dtype, t.dtype, tuple(g.shape), tuple(t.shape))
