"""Convolution with the bias + activation + gain + clamp tail fused into the matrix-core kernel's epilogue.

What the reference's layers compute as ``conv2d_resample(...)`` followed by ``bias_act.bias_act(...)``
(train_parts/discriminators.py:115-124, generators.py:176-185) becomes one launch: the pre-activation tensor is never written.
Exact for every derivative order with the piecewise-linear activations ('linear', 'relu', 'lrelu'): the backward is
``bias_act``'s own gradient Function on the saved OUTPUT followed by the differentiable data / weight gradient Functions of
``conv2d_gradfix``, so R1's double backward goes through unchanged.
"""
import torch

from . import bias_act as _ba
from . import conv2d_gradfix as _cg
from . import upfirdn2d as _up
from ._tail import Act, Tail

# Set by the loss orchestration (train_parts/losses_base.py) for passes that differentiate the discriminator ONCE (like ops/fromrgb.enabled):
# layer pairs may then run as first-order-only fused Functions (_ConvBiasActFir).  Off by default: direct callers get arbitrary-order autograd.
first_order = False


def _act_backward(act, dy, y, want_db):
    """(d1, db | None): dy (channel-minor) through the gradient of the bias_act `act` at its saved output y; first order with a bias
    gradient wanted: both in one pass over (dy, y), else bias_act's own differentiable gradient Function"""
    if act.trivial:
        return dy, None
    bcfg = _ba._Cfg(act, 1)
    fused = _ba._grad_and_bias_sum(dy, y, bcfg) if want_db else None
    return fused if fused is not None else (_ba._BiasActGrad.apply(dy, None, None, y, bcfg, torch.channels_last), None)


def _backward_from_dy(ctx, x, w, d1, db_fused, needs):
    """data / weight / bias gradients of conv_bias_act given d1 = gradient w.r.t. the convolution's output (pre-activation)"""
    dx = dw = db = None
    if needs[0]:
        dx = _cg._Conv.apply(d1, w, ctx.ccfg.adjoint(x.shape[2:], d1.shape[2:], w.shape[2:]))
    if needs[1] and not _cg.weight_gradients_disabled:
        dw = _cg._ConvWgrad.apply(d1, x, ctx.ccfg, tuple(w.shape), _cg.wmeta_of(x, w))
    if ctx.has_bias and needs[2]:
        db = (db_fused if db_fused is not None else _ba._sum_to_bias(d1, 1)).to(ctx.b_dtype)
    return dx, dw, db


def _forward(ctx, x, w, b, ccfg, act):
    """the convolution with its fused epilogue; notes on ctx what both backwards read"""
    y = _cg._conv_forward(x, w, ccfg.stride, ccfg.padding, epi=Tail(act, bias=b), wgain=ccfg.wgain)
    ctx.ccfg, ctx.act = ccfg, act
    ctx.has_bias = b is not None
    ctx.b_dtype = b.dtype if b is not None else None       # fp32 parameters may be passed as they are: the epilogue reads fp32
    return y


class _ConvBiasAct(torch.autograd.Function):
    """ccfg: ConvCfg (plain), act: the tail's settings (bias_act.Act); w in x's dtype, or the fp32 master weight (see conv2d_gradfix._Conv)"""

    @staticmethod
    def forward(ctx, x, w, b, ccfg, act):
        y = _forward(ctx, x, w, b, ccfg, act)
        ctx.save_for_backward(x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        d1, db_fused = _act_backward(ctx.act, dy.contiguous(memory_format=torch.channels_last), y, ctx.has_bias and ctx.needs_input_grad[2])
        return (*_backward_from_dy(ctx, x, w, d1, db_fused, ctx.needs_input_grad), None, None)


class _ConvBiasActFir(torch.autograd.Function):
    """F = upfirdn2d(bias_act(conv2d(x, w) + b), f, padding) -- a discriminator block's conv0 followed by the low-pass of its down-sampling conv1
    (reference train_parts/discriminators.py:286-291 -> Conv2dLayer -> conv2d_resample.py:110-112).  Forward: the convolution with its fused epilogue,
    then the low-pass.  Backward, FIRST ORDER ONLY: the transposed low-pass multiplies its result by the activation's slope at the saved conv output and
    adds up the bias gradient in the same launch (upfirdn2d.fir_transposed_dact), so the gradient w.r.t. the activation's output -- a full-resolution
    tensor the unfused chain writes, then reads again together with the output -- never exists.
    ccfg, act as _ConvBiasAct; fcfg: FirCfg of the low-pass (up = down = 1)."""

    @staticmethod
    def forward(ctx, x, w, b, f, ccfg, act, fcfg):
        y = _forward(ctx, x, w, b, ccfg, act)
        out = _up._launch(y, f, *fcfg)
        ctx.save_for_backward(x, w, y, f)
        ctx.fcfg = fcfg
        return out

    @staticmethod
    def backward(ctx, dout):
        if torch.is_grad_enabled():
            raise RuntimeError("conv_bias_act_fir: first-order only; leave torch_utils.ops.conv_bias_act.first_order = False for graphs that are differentiated twice")
        x, w, y, f = ctx.saved_tensors
        fused = _up.fir_transposed_dact(dout, f, ctx.fcfg, y.shape[2:], y, *ctx.act)
        if fused is not None:
            d1, db_fused = fused
        else:       # the composition: transposed low-pass, then the activation gradient (+ bias sum) from (dy, y)
            gcfg = ctx.fcfg.adjoint(y.shape[2:], dout.shape[2:], f)
            dy = _up._Upfirdn2d.apply(dout.to(y.dtype), f, gcfg).contiguous(memory_format=torch.channels_last)
            d1, db_fused = _act_backward(ctx.act, dy, y, True)
        return (*_backward_from_dy(ctx, x, w, d1, db_fused, ctx.needs_input_grad), None, None, None, None)


def fir_fusable(x, w, act, f, groups=1):
    """may conv2d_bias_act(x, w) followed by a 4 x 4 low-pass f run as _ConvBiasActFir?  (16-bit channel-minor activations, 64-channel blocks,
    taps exact in the dtype: what the sliding-window matrix-core FIR needs; smaller images fall back inside the backward)"""
    return (first_order and fusable(x, w, act, groups) and x.dtype in (torch.bfloat16, torch.float16) and w.shape[0] % 64 == 0
            and f is not None and f.ndim == 2 and tuple(f.shape) == (4, 4) and x.shape[2] >= 16 and _up._taps_exact(f, x.dtype))


def conv2d_bias_act_fir(x, w, b, f, fpad, stride=1, padding=0, act="linear", alpha=None, gain=None, clamp=None, wgain=1.0, flip_filter=False, fgain=1.0):
    """upfirdn2d(conv2d_bias_act(x, w, b, ...), f, padding=fpad) as one first-order Function (see _ConvBiasActFir; check fir_fusable first)"""
    fcfg = _up.FirCfg(1, 1, 1, 1, *_up._parse_padding(fpad), bool(flip_filter), float(fgain))
    return _ConvBiasActFir.apply(x, w, b, f, _cg.ConvCfg.make(False, stride, padding, wgain=wgain), Act.make(act, alpha, gain, clamp), fcfg)


def fusable(x, w, act, groups=1):
    return (groups == 1 and x.device.type == "cuda" and _cg.epilogue_fusable(x) and Act(act).fused
            and (x.dtype == w.dtype or _cg.is_mixed(x, w)))


def conv2d_bias_act(x, w, b=None, stride=1, padding=0, act="linear", alpha=None, gain=None, clamp=None, wgain=1.0):
    """bias_act(conv2d(x, w, stride, padding), b, act=act, alpha=alpha, gain=gain, clamp=clamp) in one kernel (16-bit tensors)"""
    return _ConvBiasAct.apply(x, w, b, _cg.ConvCfg.make(False, stride, padding, wgain=wgain), Act.make(act, alpha, gain, clamp))
