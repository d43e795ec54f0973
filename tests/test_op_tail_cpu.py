"""CPU: the records of the Python op layer (no library, no GPU).

* bias_act.Act -- the settings of a fused tail: kernel code, defaults rule, `fused`, and `trivial` / `needs_y` against the truth table of
  the per-module definitions it replaced;
* _tail.Tail.operands -- the fp32 dense operands and the noise stride a kernel is handed;
* upfirdn2d.FirCfg.adjoint -- against autograd of the CPU oracle (oracle/ops.py::upfirdn2d) in float64;
* conv2d_gradfix.ConvCfg.adjoint -- plain <-> transposed, with the output padding that restores the input size;
* upfirdn2d.fir_transposed_dact takes the record and the plain 10-tuple alike.
"""
import itertools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import style_big_gan_amd  # noqa: E402,F401
from style_big_gan_amd.torch_utils.ops import bias_act, conv2d_gradfix, upfirdn2d  # noqa: E402
from style_big_gan_amd.torch_utils.ops._tail import Tail  # noqa: E402
from oracle import ops as O  # noqa: E402

ACTS = ["linear", "relu", "lrelu", "tanh", "sigmoid", "elu", "selu", "softplus", "swish"]


def test_act_code_fused_defaults():
    assert sorted(bias_act.activation_funcs) == sorted(ACTS)
    for name in ACTS:
        spec = bias_act.activation_funcs[name]
        a = bias_act.Act.make(name)
        assert a.code == spec.cuda_idx
        assert a.fused == (name in ("linear", "relu", "lrelu"))
        assert a == (name, float(spec.def_alpha), float(spec.def_gain), -1.0)
        assert all(isinstance(v, float) for v in a[1:]) and hash(a) == hash(bias_act.Act.make(name))
        assert bias_act.Act.make(name, alpha=0.5, gain=3, clamp=7) == (name, 0.5, 3.0, 7.0)
        assert bias_act.Act.make(name, clamp=0) == (name, float(spec.def_alpha), float(spec.def_gain), 0.0)     # 0 is a clamp, not "none"


# (activation, clamp) -> (needs_y, gains at which the op is trivial); gain None = the activation's default (1 for linear, sqrt 2 for relu / lrelu / swish)
ACT_TABLE = {
    ("linear", None): (False, {None, 1}), ("linear", 0): (True, set()), ("linear", 1): (True, set()),
    ("relu", None): (True, set()), ("relu", 0): (True, set()), ("relu", 1): (True, set()),
    ("lrelu", None): (True, set()), ("lrelu", 0): (True, set()), ("lrelu", 1): (True, set()),
    ("tanh", None): (True, set()), ("tanh", 0): (True, set()), ("tanh", 1): (True, set()),
    ("sigmoid", None): (True, set()), ("sigmoid", 0): (True, set()), ("sigmoid", 1): (True, set()),
    ("elu", None): (True, set()), ("elu", 0): (True, set()), ("elu", 1): (True, set()),
    ("selu", None): (True, set()), ("selu", 0): (True, set()), ("selu", 1): (True, set()),
    ("softplus", None): (True, set()), ("softplus", 0): (True, set()), ("softplus", 1): (True, set()),
    ("swish", None): (False, set()), ("swish", 0): (False, set()), ("swish", 1): (False, set()),
}


def test_act_trivial_needs_y_truth_table():
    assert len(ACT_TABLE) == len(ACTS) * 3
    for (name, clamp), (needs_y, trivial_gains) in ACT_TABLE.items():
        for gain in (None, 1, 2):
            a = bias_act.Act.make(name, gain=gain, clamp=clamp)
            assert a.needs_y == needs_y, (name, clamp, gain)
            assert a.trivial == (gain in trivial_gains), (name, clamp, gain)


@pytest.mark.parametrize("post", [False, True])
@pytest.mark.parametrize("noise_shape,stride", [((5, 6), 0), ((2, 1, 5, 6), 30), ((1, 1, 5, 6), 0)])
def test_tail_operands(noise_shape, stride, post):
    n, c, h, w = 2, 4, 5, 6
    g = torch.Generator().manual_seed(3)
    oscale = torch.randn(n, c, generator=g).to(torch.bfloat16)
    noise = torch.randn(noise_shape, generator=g, dtype=torch.float64)
    bias = torch.randn(2 * c, generator=g)[::2]                      # not dense
    ps = torch.randn(c, n, generator=g).t() if post else None       # [n, c], not dense
    tail = Tail.make("lrelu", clamp=4, oscale=oscale, noise=noise, bias=bias, post=ps)
    assert tail.act == bias_act.Act.make("lrelu", clamp=4) and tail.post is ps
    osc32, nz32, nsn, b32, post32 = tail.operands(n, c, h, w)
    assert nsn == stride
    assert nz32.shape == ((n if stride else 1), h * w) and torch.equal(nz32, noise.to(torch.float32).reshape(nz32.shape))
    assert osc32.shape == (n, c) and torch.equal(osc32, oscale.to(torch.float32))
    assert b32.shape == (c,) and torch.equal(b32, bias)
    assert (post32 is None) == (not post) and (not post or (post32.shape == (n, c) and torch.equal(post32, ps)))
    for t in (osc32, nz32, b32, post32):
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad)
    assert Tail.make("relu").operands(n, c, h, w) == (None, None, 0, None, None)


FIR_GRID = list(itertools.product((1, 2, 3), (1, 2, 3), ((4, 4), (1, 1), (3, 5)), ((0, 0, 0, 0), (2, 1, 1, 2), (3, -1, -1, 3)), (False, True),
                                  ((2, 3, 7, 9), (2, 3, 8, 8))))


@pytest.mark.parametrize("up,down,fshape,pad,flip,xshape", FIR_GRID)
def test_fir_adjoint_is_the_gradient(up, down, fshape, pad, flip, xshape):
    """d/dx <upfirdn2d(x, f, up, down, padding, flip, gain 1.5), dy> == upfirdn2d(dy, f, **adjoint), in float64 on the oracle.  A wiring check:
    a wrong pad gives another shape or an O(1) error, the right one differs by rounding (8.9e-15 at worst over the grid); bound 1e-12."""
    g = torch.Generator().manual_seed(hash((up, down, fshape, pad, flip, xshape)) % (1 << 31))
    f = torch.rand(fshape, generator=g, dtype=torch.float64).to(torch.float32) + 0.1
    x = torch.randn(xshape, generator=g, dtype=torch.float64, requires_grad=True)
    y = O.upfirdn2d(x, f, up=up, down=down, padding=pad, flip_filter=flip, gain=1.5)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    ref = torch.autograd.grad(y, x, dy)[0]
    a = upfirdn2d.FirCfg(up, up, down, down, *pad, flip, 1.5).adjoint(x.shape[2:], y.shape[2:], f)
    assert isinstance(a, upfirdn2d.FirCfg)
    got = O.upfirdn2d(dy, f, up=(a.upx, a.upy), down=(a.downx, a.downy), padding=(a.padx0, a.padx1, a.pady0, a.pady1), flip_filter=a.flip, gain=a.gain)
    assert got.shape == x.shape
    assert float((got - ref).abs().max()) <= 1e-12


def test_fir_adjoint_grid_is_whole():
    """the grid is the 324-case cross product, each case a test of its own above"""
    assert len(FIR_GRID) == len(set(FIR_GRID)) == 324


def test_fir_adjoint_unit_rate_form():
    """up = down = 1: the form the fused backward paths wrote out by hand"""
    f = torch.ones(3, 5)        # fh 3, fw 5
    a = upfirdn2d.FirCfg(padx0=2, padx1=1, pady0=0, pady1=3, flip=True, gain=4.0).adjoint((16, 12), (17, 11), f)
    assert a == (1, 1, 1, 1, 5 - 2 - 1, 12 - 11 + 2, 3 - 0 - 1, 16 - 17 + 0, False, 4.0)


@pytest.mark.parametrize("stride,padding,k,size", list(itertools.product((1, 2), (0, 1), (1, 3), (7, 8))))
def test_conv_adjoint(stride, padding, k, size):
    cfg = conv2d_gradfix.ConvCfg.make(False, stride, padding, wgain=0.5)
    assert cfg == (False, (stride, stride), (padding, padding), (0, 0), 0.5)
    out = (size + 2 * padding - k) // stride + 1
    t = cfg.adjoint((size, size), (out, out), (k, k))
    assert isinstance(t, conv2d_gradfix.ConvCfg) and t.transpose and (t.stride, t.padding, t.wgain) == (cfg.stride, cfg.padding, 0.5)
    # the transposed convolution of an `out`-sized tensor has the input's size (F.conv_transpose2d's size formula)
    assert all((out - 1) * stride - 2 * padding + k + op == size and 0 <= op < stride for op in t.output_padding)
    back = t.adjoint((out, out), (size, size), (k, k))
    assert back == cfg and back.output_padding == (0, 0)
    x = torch.zeros(1, 1, out, out)
    assert torch.nn.functional.conv_transpose2d(x, torch.zeros(1, 1, k, k), stride=stride, padding=padding, output_padding=t.output_padding).shape[2:] == (size, size)


class _CudaShaped:
    """what fir_transposed_dact reads of dy before the launch: a device, a shape, two conversions"""
    device = torch.device("cuda")

    def __init__(self, *shape):
        self.shape = torch.Size(shape)

    def to(self, dtype):
        return self

    def contiguous(self, memory_format=None):
        return self


def test_fir_transposed_dact_takes_record_and_plain_tuple(monkeypatch):
    calls = []
    monkeypatch.setattr(upfirdn2d, "_launch", lambda x, f, *cfg, **kw: calls.append((cfg, kw["dact"][1])) or "launched")
    f = torch.ones(4, 4)
    y = torch.zeros(1, 64, 16, 16, dtype=torch.bfloat16)
    plain = (1, 1, 1, 1, 2, 2, 2, 2, False, 1.0)
    for cfg in (plain, upfirdn2d.FirCfg(*plain)):
        assert upfirdn2d.fir_transposed_dact(_CudaShaped(1, 64, 17, 17), f, cfg, (16, 16), y, "lrelu", 0.5, 2.0, 40.0) == "launched"
    assert calls[0] == calls[1] == ((1, 1, 1, 1, 1, 1, 1, 1, True, 1.0), bias_act.Act("lrelu", 0.5, 2.0, 40.0))
    assert upfirdn2d.fir_transposed_dact(_CudaShaped(1, 64, 9, 9), f, (1, 1, 2, 2, 2, 2, 2, 2, False, 1.0), (16, 16), y, "lrelu", 0.5, 2.0, 40.0) is None
