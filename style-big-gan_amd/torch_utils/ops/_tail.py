"""The fused tail of a layer, as the Python op layer carries it.

A layer's tail is ``y = clamp(act(acc * oscale[n, c] + noise[n, pixel] + bias[c]) * gain) (* post[n, c])``: demodulation, noise, bias_act and,
on inference passes, the next layer's style modulation.  The convolution epilogue (ops/conv2d_gradfix.py), the low-pass epilogue
(ops/upfirdn2d.py) and the one-pass backward head (``sbg_modconv_bwd``) all take it, so it has one record: ``bias_act.Act`` for the settings
and ``Tail`` for the settings with the operands.

Autograd does not see a tensor inside a record: a Function receives the differentiable operands (demodulation coefficients, noise, bias) as
positional tensor arguments and only the ``Act`` among its settings, and puts the ``Tail`` together for the launch.
"""
import typing

import torch

from .bias_act import Act


class Tail(typing.NamedTuple):
    """settings + operands of one fused tail; every operand may be None.  Holds what the caller gave it and nothing per launch, so it may sit
    on a tensor (upfirdn2d.TailHandle) without keeping temporaries alive."""
    act: Act = Act()
    oscale: typing.Optional[torch.Tensor] = None        # [N, C] demodulation coefficients
    noise: typing.Optional[torch.Tensor] = None         # [N, 1, H, W] per sample, or H * W values shared by the batch
    bias: typing.Optional[torch.Tensor] = None          # [C]
    post: typing.Optional[torch.Tensor] = None          # [N, C] (inference) the reader's style modulation, applied on the way out

    @classmethod
    def make(cls, act="linear", alpha=None, gain=None, clamp=None, oscale=None, noise=None, bias=None, post=None):
        """the one constructor: `alpha` / `gain` / `clamp` None take the defaults of the activation (Act.make)"""
        return cls(Act.make(act, alpha, gain, clamp), oscale, noise, bias, post)

    def operands(self, n, c, oh, ow):
        """-> (oscale [n, c], noise [n | 1, oh * ow], noise_stride_n, bias [c], post [n, c]): what a kernel reads for an [n, c, oh, ow] output,
        fp32 and dense, None where the tail has none.  The caller keeps them until its launch has returned."""
        def f32(t, shape):
            return None if t is None else t.detach().to(torch.float32).reshape(shape).contiguous()
        oscale, bias = f32(self.oscale, [n, c]), f32(self.bias, [c])
        per_sample = self.noise is not None and self.noise.numel() != oh * ow
        noise = f32(self.noise, [n if per_sample else 1, oh * ow])
        return oscale, noise, (oh * ow if per_sample else 0), bias, f32(self.post, [n, c])


def finish_grads(tail, sums, dn, dc32, want_oscale, want_noise, want_bias):
    """(d oscale, d noise, d bias) of `tail` from what the backward head left: sums [2, N, C] (bias / demodulation partial sums), dn [N, 1, H, W]
    (per-pixel noise gradient or None), dc32 (the fp32 coefficients the head divided by).  Each in its operand's dtype and shape, None if unwanted."""
    doscale = dnoise = dbias = None
    if tail.oscale is not None and want_oscale:
        doscale = (sums[1] / dc32).to(tail.oscale.dtype).reshape(tail.oscale.shape)
    if tail.bias is not None and want_bias:
        dbias = sums[0].sum(0).to(tail.bias.dtype)
    if tail.noise is not None and want_noise and dn is not None:
        per_sample = tail.noise.numel() != dn.shape[2] * dn.shape[3]
        dnoise = (dn if per_sample else dn.sum(0, keepdim=True)).reshape(tail.noise.shape).to(tail.noise.dtype)
    return doscale, dnoise, dbias
