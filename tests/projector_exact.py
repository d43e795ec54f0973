"""Exact-arithmetic inputs and fp64 references for the projector kernels (tests/test_projector_gpu.py).

Two kinds of noise buffer keep every intermediate of the regulariser exact in fp32:
* "blocky": constant on (R / 8) x (R / 8) blocks (whole buffer side <= 8: per pixel), a few nonzero blocks of small integers, so every
  pooled level holds integers and every product sum is a small integer times a power of two;
* "spiky": zero but for a few adjacent pairs of +-1 / +-2 pixels, so every pooled value is a small integer / 4^k and a level's
  product sum has only a handful of terms.
`check_exact` asserts the precondition: every pooled value, product, product sum (in ANY order: all terms are multiples of one
power of two q and the sum of their magnitudes is below 2^24 q), mean, square and every step of the backward is an fp32 value."""
import numpy as np
import torch
import torch.nn.functional as F


def blocky(gen, R, nonzero=3):
    c = min(R, 8)
    coarse = torch.zeros([c, c], dtype=torch.float64)
    idx = torch.randperm(c * c, generator=gen)[:nonzero]
    coarse.view(-1)[idx] = torch.randint(1, 3, [nonzero], generator=gen).double() * (torch.randint(0, 2, [nonzero], generator=gen) * 2 - 1)
    return coarse.repeat_interleave(R // c, 0).repeat_interleave(R // c, 1)


def spiky(gen, R, pairs=3):
    b = torch.zeros([R, R], dtype=torch.float64)
    for p in range(pairs):
        y, x = (int(v) for v in torch.randint(0, R, [2], generator=gen))
        if p == 0:
            y, x = R - 1, R - 1           # a pair across the wrap-around
        v = float(torch.randint(1, 3, [1], generator=gen)) * (1 if p % 2 == 0 else -1)
        b[y, x] = v
        if p % 2 == 0:
            b[y, (x + 1) % R] = -v
        else:
            b[(y + 1) % R, x] = v
    return b


def levels(P):
    out = [P]
    while out[-1].shape[0] > 8:
        out.append(F.avg_pool2d(out[-1][None, None], 2)[0, 0])
    return out


def _exact32(x):
    x = torch.as_tensor(x, dtype=torch.float64)
    return bool(torch.equal(x, x.float().double()))


def _any_order_exact(terms):
    """every partial sum of `terms` (fp64, each an fp32 value) in any order is an fp32 value"""
    t = terms.reshape(-1).double().numpy()
    t = t[t != 0]
    if t.size == 0:
        return True
    m, e = np.frexp(t)
    mi = np.abs((m * 2.0 ** 53).astype(np.int64))
    low = e - 53 + np.log2((mi & -mi).astype(np.float64)).astype(np.int64)      # exponent of the lowest set bit of each term
    q = 2.0 ** int(low.min())
    return float(np.abs(t).sum()) / q < 2.0 ** 24


def reference(bufs, g=1.0):
    """fp64: means [2M] in the reference's order, reg (fp32 in-order accumulation of the fp32 squares, the kernel's stated order) and
    the gradients g * sum_k G_k / 4^k, with the precondition checked on every intermediate"""
    means, grads = [], []
    for P0 in bufs:
        lv = levels(P0)
        for P in lv:
            assert _exact32(P), "pooled value not exact"
            px, py = P * torch.roll(P, 1, 1), P * torch.roll(P, 1, 0)
            assert _exact32(px) and _exact32(py), "product not exact"
            assert _any_order_exact(px) and _any_order_exact(py), "product sum not exact in every order"
            n2 = P.shape[0] ** 2
            mx, my = px.sum() / n2, py.sum() / n2
            assert _exact32(mx) and _exact32(my) and _exact32(mx * mx) and _exact32(my * my), "mean or square not exact"
            means += [mx, my]
        acc = None
        ms = means[-2 * len(lv):]
        for k in range(len(lv) - 1, -1, -1):
            P, n = lv[k], lv[k].shape[0]
            hx = torch.roll(P, 1, 1) + torch.roll(P, -1, 1)
            hy = torch.roll(P, 1, 0) + torch.roll(P, -1, 0)
            tx, ty = ms[2 * k] * hx, ms[2 * k + 1] * hy
            G = 2 * (tx + ty) / n ** 2
            for x in (hx, hy, tx, ty, tx + ty, G):
                assert _exact32(x), "backward term not exact"
            up = lambda a: a.repeat_interleave(2, 0).repeat_interleave(2, 1)
            if acc is None:
                acc = G
            else:
                q = up(acc) * 0.25
                G_full = G
                assert _exact32(q) and _exact32(G_full + q), "backward sum not exact"
                acc = G_full + q
        assert _exact32(acc * g), "gradient not exact"
        grads.append(acc * g)
    means = torch.stack(means)
    reg = np.float32(0.0)
    for m in means.float().numpy():
        reg = np.float32(reg + np.float32(m * m))
    return means, float(reg), grads
