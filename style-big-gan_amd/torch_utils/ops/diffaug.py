"""DiffAugment (Zhao et al., "Differentiable Augmentation for Data-Efficient GAN Training", NeurIPS 2020) as one fused op
(csrc/diffaug.hip): colour (brightness, saturation, contrast), zero-padded integer translation, cutout.

Per sample the parameters are ``b, s, k`` (float), ``t_row, t_col`` (int) and the half-open cutout rectangle ``r0, r1, c0, c1`` (int);
images are ``[N, C, H, W]``, rows are axis 2.  ``params`` is either a dict of tensors

    b, s, k: [N]    t: [N, 2] (row, column)    rect: [N, 4] (r0, r1, c0, c1)

or the packed table ``pack(params)`` makes of it: int32 ``[N, 12]``, words 0..2 the fp32 bit patterns of b, s, k, words 3..4 the shift,
5..8 the rectangle, 9..11 zero (``SBG_DIFFAUG_WORDS`` in include/sbg_hip.h).  ``identity_params(n)`` is b = 0, s = k = 1, no shift, empty
rectangle: the output is then the input bit for bit.

The published chain is affine in the image, so it collapses to, with M = mean(x[n]) + b,

    y[:, i, j] = k v + (1 - k) M,   v = s v0 + (1 - s) mean_c(v0),   v0 = x[:, i + t_row, j + t_col] + b

where (i, j) is outside the rectangle and its source inside the image, and 0 elsewhere; the adjoint has the same shape, and the adjoint's
adjoint is the forward form with b = 0.  ``diffaug`` runs two autograd Functions that call each other, so every order of derivative is
served by the same two kernels (R1 differentiates the discriminator's input gradient through the pipe).

Device tensors run the HIP kernels or raise ``RuntimeError``: there is no quiet torch path.  Inputs that are not fp32 are cast and cast
back.  CPU tensors run the same two Functions over a torch restatement of the fused form in the input's dtype (float64 makes
``gradcheck`` meaningful).  ``diffaug_reference`` is the published composition, op by op, in plain torch for any device and dtype.
"""
import torch

from ... import _lib

WORDS = _lib.DIFFAUG_WORDS


def identity_params(n):
    return dict(b=torch.zeros([n]), s=torch.ones([n]), k=torch.ones([n]), t=torch.zeros([n, 2], dtype=torch.int32),
                rect=torch.zeros([n, 4], dtype=torch.int32))


def pack(params):
    """dict of per-sample parameters (tensors on one device) -> the packed int32 [N, 12] table on that device"""
    b = torch.as_tensor(params["b"])
    n = b.shape[0]
    f = torch.stack([b.reshape(n).to(torch.float32), params["s"].reshape(n).to(torch.float32), params["k"].reshape(n).to(torch.float32)], dim=1)
    t, rect = params["t"], params["rect"]
    if tuple(t.shape) != (n, 2) or tuple(rect.shape) != (n, 4) or t.is_floating_point() or rect.is_floating_point():
        raise RuntimeError(f"diffaug: t must be an integer [N, 2] and rect an integer [N, 4] tensor, got {tuple(t.shape)} {t.dtype} and {tuple(rect.shape)} {rect.dtype}")
    table = torch.zeros([n, WORDS], dtype=torch.int32, device=f.device)
    table[:, 0:3] = f.contiguous().view(torch.int32)
    table[:, 3:5] = t.to(torch.int32)
    table[:, 5:9] = rect.to(torch.int32)
    return table


def unpack(table):
    """packed table -> dict(b, s, k fp32 [N]; t int32 [N, 2]; rect int32 [N, 4])"""
    f = table[:, 0:3].contiguous().view(torch.float32)
    return dict(b=f[:, 0], s=f[:, 1], k=f[:, 2], t=table[:, 3:5], rect=table[:, 5:9])


def _as_table(x, params):
    """validation of everything but the device path's layout demands; -> the table on x's device"""
    if not isinstance(x, torch.Tensor) or x.ndim != 4:
        raise RuntimeError("diffaug: expects images [N, C, H, W]")
    if not x.is_floating_point():
        raise RuntimeError(f"diffaug: expects floating-point images, got {x.dtype}")
    table = pack(params) if isinstance(params, dict) else params
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or tuple(table.shape) != (x.shape[0], WORDS):
        raise RuntimeError(f"diffaug: the parameter table must be int32 [{x.shape[0]}, {WORDS}] (see pack()), got "
                           f"{getattr(table, 'dtype', type(table))} {tuple(getattr(table, 'shape', ()))}")
    if x.device.type == "cuda" and not (x.is_contiguous() and table.is_contiguous()):
        raise RuntimeError("diffaug: expects dense NCHW images and a dense parameter table on the device (call .contiguous() first)")
    if table.device != x.device:
        if isinstance(params, dict):
            table = table.to(x.device)
        else:
            raise RuntimeError(f"diffaug: the parameter table is on '{table.device}', the images on '{x.device}'")
    return table.contiguous()


# ---------------------------------------------------------------------------------------------------------------------------
# the fused form in torch (CPU tensors; any dtype)

def _geometry(table, H, W):
    """the unpacked parameters, the pixel coordinates and the cutout mask of the output pixels [N, H, W]"""
    p = unpack(table)
    t, rect = p["t"].to(torch.int64), p["rect"].to(torch.int64)
    i = torch.arange(H, device=table.device).reshape(1, H, 1)
    j = torch.arange(W, device=table.device).reshape(1, 1, W)
    col = lambda v: v.reshape(-1, 1, 1)
    cutm = (i >= col(rect[:, 0])) & (i < col(rect[:, 1])) & (j >= col(rect[:, 2])) & (j < col(rect[:, 3]))       # of output pixels
    return p, t, i, j, col, cutm


def _fused_forward_torch(x, table, drop_b):
    n, c, H, W = x.shape
    p, t, i, j, col, cutm = _geometry(table, H, W)
    bc = lambda v: v.to(x.dtype).reshape(n, 1, 1, 1)
    b, s, k = (torch.zeros_like(bc(p["b"])) if drop_b else bc(p["b"])), bc(p["s"]), bc(p["k"])
    M = x.mean(dim=(1, 2, 3), keepdim=True) + b
    v = x + b
    v = s * v + (1 - s) * v.mean(dim=1, keepdim=True)
    v = k * v + (1 - k) * M
    si, sj = i + col(t[:, 0]), j + col(t[:, 1])
    live = (si >= 0) & (si < H) & (sj >= 0) & (sj < W) & ~cutm
    idx = (si.clamp(0, H - 1) * W + sj.clamp(0, W - 1)).reshape(n, 1, H * W).expand(n, c, H * W)
    y = v.reshape(n, c, H * W).gather(2, idx).reshape(n, c, H, W)
    return torch.where(live.unsqueeze(1), y, torch.zeros_like(y))


def _fused_adjoint_torch(g, table):
    n, c, H, W = g.shape
    p, t, i, j, col, cutm = _geometry(table, H, W)
    bc = lambda v: v.to(g.dtype).reshape(n, 1, 1, 1)
    s, k = bc(p["s"]), bc(p["k"])
    oi, oj = i - col(t[:, 0]), j - col(t[:, 1])                 # the output pixel that read source pixel (i, j)
    exists = (oi >= 0) & (oi < H) & (oj >= 0) & (oj < W)
    idx = (oi.clamp(0, H - 1) * W + oj.clamp(0, W - 1)).reshape(n, H * W)
    live = exists & ~cutm.reshape(n, H * W).gather(1, idx).reshape(n, H, W)
    u = g.reshape(n, c, H * W).gather(2, idx.reshape(n, 1, H * W).expand(n, c, H * W)).reshape(n, c, H, W)
    u = torch.where(live.unsqueeze(1), u, torch.zeros_like(u))
    S = u.sum(dim=(1, 2, 3), keepdim=True) / (c * H * W)
    w = k * u + (1 - k) * S
    return s * w + (1 - s) * w.mean(dim=1, keepdim=True)


# ---------------------------------------------------------------------------------------------------------------------------
# the kernels

def _launch(x, table, adjoint, drop_b):
    """x: device tensor [N, C, H, W]; fp32 dense is what the kernels take, anything else is cast / compacted here and cast back"""
    n, c, H, W = x.shape
    if not 1 <= c <= 4:
        raise RuntimeError(f"diffaug: {c} channels; the kernels take 1..4")
    xc = x.to(torch.float32).contiguous()
    y = torch.empty_like(xc)
    if y.numel():
        lib = _lib.load()
        ws = _lib.workspace(lib.sbg_diffaug_workspace(n, c, H, W), x.device, "diffaug: sbg_diffaug_workspace")
        if adjoint:
            _lib.check(lib.sbg_diffaug_adj(xc.data_ptr(), table.data_ptr(), y.data_ptr(), ws.data_ptr(), n, c, H, W, _lib.stream_ptr(x.device)),
                       "diffaug: sbg_diffaug_adj")
        else:
            _lib.check(lib.sbg_diffaug_fwd(xc.data_ptr(), table.data_ptr(), y.data_ptr(), ws.data_ptr(), n, c, H, W, int(drop_b), _lib.stream_ptr(x.device)),
                       "diffaug: sbg_diffaug_fwd")
    return y.to(x.dtype)


def _run(x, table, adjoint, drop_b):
    if x.device.type == "cuda":
        return _launch(x, table, adjoint, drop_b)
    if x.device.type != "cpu":
        raise RuntimeError(f"diffaug: tensor is on '{x.device}'; the op runs as HIP kernels on a ROCm device (device type 'cuda') or as its torch restatement on the CPU")
    return _fused_adjoint_torch(x, table) if adjoint else _fused_forward_torch(x, table, drop_b)


class _Forward(torch.autograd.Function):
    """y = A(x) + a0 per sample; its gradient is the adjoint A^T"""

    @staticmethod
    def forward(ctx, x, table, drop_b):
        ctx.save_for_backward(table)
        return _run(x, table, False, drop_b)

    @staticmethod
    def backward(ctx, dy):
        table, = ctx.saved_tensors
        return (_Adjoint.apply(dy, table) if ctx.needs_input_grad[0] else None), None, None


class _Adjoint(torch.autograd.Function):
    """dx = A^T g; linear in g, its gradient is A: the forward form without the brightness offset"""

    @staticmethod
    def forward(ctx, g, table):
        ctx.save_for_backward(table)
        return _run(g, table, True, False)

    @staticmethod
    def backward(ctx, ddx):
        table, = ctx.saved_tensors
        return (_Forward.apply(ddx, table, True) if ctx.needs_input_grad[0] else None), None


def diffaug(x, params):
    """x [N, C, H, W] (C = 1..4 on a device), params: the dict or the packed table described above -> the augmented images, differentiable
    to any order with respect to x.  Everything is validated before the first launch; errors are RuntimeErrors naming `diffaug`."""
    table = _as_table(x, params)
    return _Forward.apply(x, table, False)


def diffaug_adjoint(g, params):
    """the adjoint of the linear part of `diffaug` applied to g (what `diffaug`'s backward runs); differentiable likewise"""
    table = _as_table(g, params)
    return _Adjoint.apply(g, table)


def diffaug_reference(x, params):
    """The published composition, one torch op after the other, on x's device in x's dtype; differentiable by autograd."""
    p = unpack(pack(params)) if isinstance(params, dict) else unpack(params)
    n, c, H, W = x.shape
    dev = x.device
    bc = lambda v: v.to(device=dev, dtype=x.dtype).reshape(n, 1, 1, 1)
    # colour: brightness, saturation, contrast
    x = x + bc(p["b"])
    m = x.mean(dim=1, keepdim=True)
    x = (x - m) * bc(p["s"]) + m
    m = x.mean(dim=[1, 2, 3], keepdim=True)
    x = (x - m) * bc(p["k"]) + m
    # translation: one ring of zeros, the shifted index clamped into it
    t = p["t"].to(device=dev, dtype=torch.int64)
    gb = torch.arange(n, device=dev).reshape(n, 1, 1)
    gi = torch.arange(H, device=dev).reshape(1, H, 1)
    gj = torch.arange(W, device=dev).reshape(1, 1, W)
    pi = torch.clamp(gi + t[:, 0].reshape(n, 1, 1) + 1, 0, H + 1)
    pj = torch.clamp(gj + t[:, 1].reshape(n, 1, 1) + 1, 0, W + 1)
    xp = torch.nn.functional.pad(x, [1, 1, 1, 1, 0, 0, 0, 0])
    x = xp.permute(0, 2, 3, 1).contiguous()[gb, pi, pj].permute(0, 3, 1, 2)
    # cutout: a mask of ones with the rectangle's rows and columns cleared
    r = p["rect"].to(device=dev, dtype=torch.int64)
    rows = (gi >= r[:, 0].reshape(n, 1, 1)) & (gi < r[:, 1].reshape(n, 1, 1))
    cols = (gj >= r[:, 2].reshape(n, 1, 1)) & (gj < r[:, 3].reshape(n, 1, 1))
    mask = 1 - (rows & cols).to(x.dtype)
    return x * mask.unsqueeze(1)
