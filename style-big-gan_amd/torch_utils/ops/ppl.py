"""The perceptual-path-length sampler's arithmetic around the generator and the detector as HIP kernels (csrc/ppl.hip).

Each function restates one step of the reference's ``PPLSampler.forward`` (stylegan2ada/metrics/perceptual_path_length.py:49-94) and
``slerp`` (:23-32).  Device tensors run the kernels; CPU tensors run the reference's own formulas in torch, so the metric's plumbing
is testable without a GPU.  On the device a missing kernel or an unsupported input is an error, never a quiet torch fallback.
"""
import torch

from ... import _lib


def slerp(a, b, t):
    """the reference's spherical interpolation of a batch of vectors (:23-32)"""
    a = a / a.norm(dim=-1, keepdim=True)
    b = b / b.norm(dim=-1, keepdim=True)
    d = (a * b).sum(dim=-1, keepdim=True)
    p = t * torch.acos(d)
    c = b - d * a
    c = c / c.norm(dim=-1, keepdim=True)
    d = a * torch.cos(p) + c * torch.sin(p)
    d = d / d.norm(dim=-1, keepdim=True)
    return d


def slerp_endpoints(z0, z1, t, epsilon):
    """z0, z1 [B, D], t [B] -> [2B, D]: cat[slerp(z0, z1, t), slerp(z0, z1, t + epsilon)] (:64-65)"""
    B, D = z0.shape
    assert z1.shape == (B, D) and t.shape == (B,)
    if z0.device.type != "cuda":
        t = t.unsqueeze(1)
        return torch.cat([slerp(z0, z1, t), slerp(z0, z1, t + epsilon)])
    z0, z1, t = (_lib.require_dtype(x, torch.float32, "ppl slerp").contiguous() for x in (z0, z1, t))
    out = torch.empty([2 * B, D], dtype=torch.float32, device=z0.device)
    _lib.check(_lib.load().sbg_ppl_slerp_endpoints(z0.data_ptr(), z1.data_ptr(), t.data_ptr(), float(epsilon), out.data_ptr(), B, D,
                                                   _lib.stream_ptr(z0.device)), "sbg_ppl_slerp_endpoints")
    return out


def lerp_endpoints(w0, w1, t, epsilon):
    """w0, w1 [B, ...], t [B] -> [2B, ...]: cat[w0.lerp(w1, t), w0.lerp(w1, t + epsilon)] with t broadcast over each sample (:59-60)"""
    B = w0.shape[0]
    assert w1.shape == w0.shape and t.shape == (B,)
    if w0.device.type != "cuda":
        tb = t.reshape([B] + [1] * (w0.ndim - 1))
        return torch.cat([w0.lerp(w1, tb), w0.lerp(w1, tb + epsilon)])
    w0, w1, t = (_lib.require_dtype(x, torch.float32, "ppl lerp").contiguous() for x in (w0, w1, t))
    out = torch.empty([2 * B] + list(w0.shape[1:]), dtype=torch.float32, device=w0.device)
    _lib.check(_lib.load().sbg_ppl_lerp_endpoints(w0.data_ptr(), w1.data_ptr(), t.data_ptr(), float(epsilon), out.data_ptr(), B, w0[0].numel(),
                                                  _lib.stream_ptr(w0.device)), "sbg_ppl_lerp_endpoints")
    return out


def prep_images(img, crop, factor):
    """synthesis output [N, C, H, W] -> detector input [N, 3 | C, S, S] fp32 dense (:77-89): optional centre crop, area mean over
    factor x factor boxes when factor > 1, (x + 1) * 255 / 2, grey -> RGB.  On the device the input is read with its own strides."""
    N, C, H, W = img.shape
    factor = max(int(factor), 1)       # G.img_resolution // 256 is 0 below 256x256: no downsampling
    if img.device.type != "cuda":
        if crop:
            assert H == W
            c = H // 8
            img = img[:, :, c * 3: c * 7, c * 2: c * 6]
        if factor > 1:
            img = img.reshape([-1, img.shape[1], img.shape[2] // factor, factor, img.shape[3] // factor, factor]).mean([3, 5])
        img = (img + 1) * (255 / 2)
        if C == 1:
            img = img.repeat([1, 3, 1, 1])
        return img
    if img.dtype != torch.float32:
        raise RuntimeError(f"ppl prep: expects the float32 synthesis output, got {img.dtype}")
    hh = (H // 8) * 4 if crop else H
    ww = (W // 8) * 4 if crop else W
    out = torch.empty([N, 3 if C == 1 else C, hh // factor, ww // factor], dtype=torch.float32, device=img.device)
    sn, sc, sh, sw = img.stride()
    _lib.check(_lib.load().sbg_ppl_prep_images(img.data_ptr(), out.data_ptr(), N, C, H, W, sn, sc, sh, sw, int(bool(crop)), factor,
                                               _lib.stream_ptr(img.device)), "sbg_ppl_prep_images")
    return out


def lpips_distance(feats, epsilon):
    """detector features [2B, F] -> [B]: (f[:B] - f[B:]).square().sum(1) / epsilon ** 2 (:91-93).  On the device the sum has a fixed
    order (same value on every run) and the division by the fp32 value of epsilon ** 2 happens once, at the end."""
    assert feats.ndim == 2 and feats.shape[0] % 2 == 0
    if feats.device.type != "cuda":
        f0, f1 = feats.chunk(2)
        return (f0 - f1).square().sum(1) / epsilon ** 2
    feats = _lib.require_dtype(feats, torch.float32, "ppl distance").contiguous()
    B, F = feats.shape[0] // 2, feats.shape[1]
    lib = _lib.load()
    ws = _lib.workspace(lib.sbg_ppl_dist_workspace(B, F), feats.device, "sbg_ppl_dist_workspace")
    dist = torch.empty([B], dtype=torch.float32, device=feats.device)
    eps2 = float(torch.tensor(epsilon ** 2, dtype=torch.float32))
    _lib.check(lib.sbg_ppl_dist(feats.data_ptr(), dist.data_ptr(), ws.data_ptr(), B, F, eps2, _lib.stream_ptr(feats.device)), "sbg_ppl_dist")
    return dist
