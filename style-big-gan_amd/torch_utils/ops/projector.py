"""The latent projector's arithmetic around the generator and the detector as HIP kernels (csrc/projector.hip).

Each function restates one piece of the reference's ``project()`` (stylegan2ada/projector.py:25-131): the LPIPS distance (:97-98), the
noise regulariser (:101-110) and the noise renormalisation (:125-129).  Device tensors run the kernels; CPU tensors run the reference's
own formulas in torch, so the projector's plumbing is testable without a GPU.  On the device an unsupported input is an error, never a
quiet torch fallback.  The regulariser and the distance are autograd Functions, so ``loss = dist + reg * weight; loss.backward()``
works unchanged.
"""
import ctypes

import torch
import torch.nn.functional as F

from ... import _lib


def num_levels(res):
    """pyramid levels of a res x res noise buffer: res, res / 2, ... down to the first side <= 8 (the reference's loop, :104-110)"""
    n, levels = res, 1
    while n > 8:
        n //= 2
        levels += 1
    return levels


# ---------------------------------------------------------------------------------------------------------------- reference formulas

def noise_reg_reference(bufs):
    """the reference's regulariser (:101-110): sum over buffers and pyramid levels of mean(P * roll(P, 1, W))^2 + mean(P * roll(P, 1, H))^2"""
    reg_loss = 0.0
    for v in bufs:
        noise = v[None, None, :, :]
        while True:
            reg_loss += (noise * torch.roll(noise, shifts=1, dims=3)).mean() ** 2
            reg_loss += (noise * torch.roll(noise, shifts=1, dims=2)).mean() ** 2
            if noise.shape[2] <= 8:
                break
            noise = F.avg_pool2d(noise, kernel_size=2)
    return reg_loss


def noise_means_reference(bufs):
    """the per-level means of the regulariser, in its order (buffer, level, W before H)"""
    out = []
    for v in bufs:
        noise = v[None, None, :, :]
        while True:
            out.append((noise * torch.roll(noise, shifts=1, dims=3)).mean())
            out.append((noise * torch.roll(noise, shifts=1, dims=2)).mean())
            if noise.shape[2] <= 8:
                break
            noise = F.avg_pool2d(noise, kernel_size=2)
    return torch.stack(out)


# ---------------------------------------------------------------------------------------------------------------- device plumbing

def _same_device(tensors, what):
    """every tensor on the first one's device: a host pointer handed to a kernel would fault, so a mix is an error"""
    dev = tensors[0].device
    for t in tensors[1:]:
        if t.device != dev:
            raise RuntimeError(f"{what}: every tensor must be on the same device ({dev}), got one on {t.device}")
    return dev


def _noise_table(bufs, what):
    if not bufs:
        raise RuntimeError(f"{what}: no noise buffers")
    if _same_device(bufs, what).type != "cuda":
        raise RuntimeError(f"{what}: the buffers must all be on the device")
    for b in bufs:
        if b.dtype != torch.float32 or b.ndim != 2 or b.shape[0] != b.shape[1] or not b.is_contiguous():
            raise RuntimeError(f"{what}: expects dense square float32 buffers, got {b.dtype} {list(b.shape)}")
    n = len(bufs)
    ptrs = (ctypes.c_void_p * n)(*[b.data_ptr() for b in bufs])
    res = (ctypes.c_int * n)(*[int(b.shape[0]) for b in bufs])
    return ptrs, res, n


def _noise_reg_device(bufs):
    """-> (means [2M], reg [], workspace holding the pyramid)"""
    lib = _lib.load()
    ptrs, res, n = _noise_table(bufs, "proj noise reg")
    dev = bufs[0].device
    ws = _lib.workspace(lib.sbg_proj_noise_reg_workspace(res, n), dev, "sbg_proj_noise_reg_workspace")
    means = torch.empty([2 * sum(num_levels(int(b.shape[0])) for b in bufs)], dtype=torch.float32, device=dev)
    reg = torch.empty([], dtype=torch.float32, device=dev)
    _lib.check(lib.sbg_proj_noise_reg(ptrs, res, n, means.data_ptr(), reg.data_ptr(), ws.data_ptr(), _lib.stream_ptr(dev)), "sbg_proj_noise_reg")
    return means, reg, ws


def noise_means(bufs):
    """the per-level means [2M] (device: the forward kernels; CPU: the reference's formulas)"""
    bufs = list(bufs)
    if not bufs:
        return torch.zeros([0])
    if _same_device(bufs, "proj noise means").type != "cuda":
        return noise_means_reference(bufs)
    with torch.no_grad():
        return _noise_reg_device([b.detach() for b in bufs])[0]


class _NoiseReg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, *bufs):
        means, reg, ws = _noise_reg_device([b.detach() for b in bufs])
        ctx.save_for_backward(means, ws, *bufs)
        return reg

    @staticmethod
    def backward(ctx, g):
        means, ws, *bufs = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        grads = [torch.empty_like(b) for b in bufs]
        ptrs, res, n = _noise_table(bufs, "proj noise reg backward")
        gptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in grads])
        _lib.check(_lib.load().sbg_proj_noise_reg_bwd(ptrs, gptrs, res, n, means.data_ptr(), g.data_ptr(), ws.data_ptr(),
                                                      _lib.stream_ptr(g.device)), "sbg_proj_noise_reg_bwd")
        return tuple(t if need else None for t, need in zip(grads, ctx.needs_input_grad))


def noise_reg(bufs):
    """the noise regulariser over the whole set of buffers -> a 0-dim tensor, differentiable with respect to every buffer.  A generator
    without noise buffers gets the reference's 0.0."""
    bufs = list(bufs)
    if not bufs:
        return 0.0
    if _same_device(bufs, "proj noise reg").type != "cuda":
        return noise_reg_reference(bufs)
    return _NoiseReg.apply(*bufs)


def noise_normalize_(bufs):
    """in place, for every buffer: buf -= buf.mean(); buf *= buf.square().mean().rsqrt() (:125-129)"""
    bufs = list(bufs)
    if not bufs:
        return
    with torch.no_grad():
        if _same_device(bufs, "proj noise normalize").type != "cuda":
            for buf in bufs:
                buf -= buf.mean()
                buf *= buf.square().mean().rsqrt()
            return
        lib = _lib.load()
        ptrs, res, n = _noise_table([b.detach() for b in bufs], "proj noise normalize")
        dev = bufs[0].device
        ws = _lib.workspace(lib.sbg_proj_noise_normalize_workspace(res, n), dev, "sbg_proj_noise_normalize_workspace")
        _lib.check(lib.sbg_proj_noise_normalize(ptrs, res, n, ws.data_ptr(), _lib.stream_ptr(dev)), "sbg_proj_noise_normalize")


class _SqDist(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, s):
        tf, sf = (_lib.require_dtype(x.detach(), torch.float32, "proj sqdist").contiguous().reshape(-1) for x in (t, s))
        lib = _lib.load()
        Fn = tf.numel()
        ws = _lib.workspace(lib.sbg_proj_sqdist_workspace(Fn), tf.device, "sbg_proj_sqdist_workspace")
        dist = torch.empty([], dtype=torch.float32, device=tf.device)
        _lib.check(lib.sbg_proj_sqdist(tf.data_ptr(), sf.data_ptr(), dist.data_ptr(), ws.data_ptr(), Fn, _lib.stream_ptr(tf.device)), "sbg_proj_sqdist")
        ctx.save_for_backward(tf, sf)
        ctx.shape = s.shape
        return dist

    @staticmethod
    def backward(ctx, g):
        tf, sf = ctx.saved_tensors
        g = g.to(torch.float32).contiguous()
        ds = torch.empty_like(sf)
        _lib.check(_lib.load().sbg_proj_sqdist_bwd(tf.data_ptr(), sf.data_ptr(), g.data_ptr(), ds.data_ptr(), sf.numel(),
                                                   _lib.stream_ptr(g.device)), "sbg_proj_sqdist_bwd")
        ds = ds.reshape(ctx.shape)
        return (-ds if ctx.needs_input_grad[0] else None), (ds if ctx.needs_input_grad[1] else None)


def sqdist(target, synth):
    """the LPIPS term (:98): (target - synth).square().sum() -> a 0-dim tensor.  On the device the sum has a fixed order (the same value
    on every run); the gradient with respect to synth is 2 g (synth - target)."""
    if target.shape != synth.shape:
        raise RuntimeError(f"proj sqdist: shapes differ, {list(target.shape)} vs {list(synth.shape)}")
    if _same_device([synth, target], "proj sqdist").type != "cuda":
        return (target - synth).square().sum()
    return _SqDist.apply(target, synth)
