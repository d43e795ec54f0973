"""Independent float64 restatement of the published DiffAugment ops (Zhao et al., NeurIPS 2020) for tests/test_diffaug_*.py.

Nothing here shares code with style_big_gan_amd/torch_utils/ops/diffaug.py: the colour steps are the published `(x - mean) * a + mean`
expressions, the translation pads the image by its own extent and slices the shifted window out, the cutout scatters zeros into a mask of
ones at the published clamped indices.  One sample at a time, float64, CPU.  The adjoint of anything is taken by autograd through it."""
import torch


def scatter_indices(offset, size, extent):
    """the published cutout indices of one axis: clamp(i + offset - size // 2, 0, extent - 1), i < size"""
    return torch.clamp(torch.arange(size) + int(offset) - size // 2, 0, extent - 1)


def scatter_mask(H, W, size_h, size_w, o_row, o_col):
    """[H, W] float64 mask of ones with zeros scattered at the published indices (the outer product of the two axes' index lists)"""
    mask = torch.ones([H, W], dtype=torch.float64)
    rows, cols = scatter_indices(o_row, size_h, H), scatter_indices(o_col, size_w, W)
    mask[rows.reshape(-1, 1), cols.reshape(1, -1)] = 0
    return mask


def rect_mask(rect, H, W):
    """[H, W] float64 mask with the half-open rectangle (r0, r1, c0, c1), clipped to the image, scattered to zero"""
    r0, r1, c0, c1 = (int(v) for v in rect)
    mask = torch.ones([H, W], dtype=torch.float64)
    rows = torch.arange(max(r0, 0), min(r1, H)) if r1 > r0 else torch.arange(0)
    cols = torch.arange(max(c0, 0), min(c1, W)) if c1 > c0 else torch.arange(0)
    if rows.numel() and cols.numel():
        mask[rows.reshape(-1, 1), cols.reshape(1, -1)] = 0
    return mask


def published_sample(x, b, s, k, t_row, t_col, mask):
    """x float64 [C, H, W] of one sample -> the published chain: brightness, saturation, contrast, translation, cutout"""
    C, H, W = x.shape
    x = x + b
    m = x.mean(dim=0, keepdim=True)
    x = (x - m) * s + m
    m = x.mean()
    x = (x - m) * k + m
    tr, tc = max(-H, min(H, int(t_row))), max(-W, min(W, int(t_col)))           # a shift of the extent already leaves nothing
    xp = torch.nn.functional.pad(x, [W, W, H, H])
    x = xp[:, H + tr:H + tr + H, W + tc:W + tc + W]
    return x * mask


def published(x, params):
    """x [N, C, H, W] (any float dtype, CPU) and a parameter dict (b, s, k [N]; t [N, 2]; rect [N, 4]) -> float64 [N, C, H, W]"""
    x = x.to(torch.float64)
    N, C, H, W = x.shape
    out = []
    for n in range(N):
        out.append(published_sample(x[n], float(params["b"][n]), float(params["s"][n]), float(params["k"][n]),
                                    int(params["t"][n, 0]), int(params["t"][n, 1]), rect_mask(params["rect"][n], H, W)))
    return torch.stack(out)


def published_with_adjoint(x, g, params):
    """-> (y, dx) in float64: y = published(x), dx = d(sum(y * g)) / dx by autograd"""
    xr = x.detach().to(torch.float64).requires_grad_(True)
    y = published(xr, params)
    dx, = torch.autograd.grad((y * g.to(torch.float64)).sum(), xr)
    return y.detach(), dx


def make_params(b, s, k, t, rect):
    f = lambda v: torch.as_tensor(v, dtype=torch.float32).reshape(-1)
    return dict(b=f(b), s=f(s), k=f(k), t=torch.as_tensor(t, dtype=torch.int32).reshape(-1, 2), rect=torch.as_tensor(rect, dtype=torch.int32).reshape(-1, 4))


def take(params, idx):
    """the parameter dict of the samples `idx` (a slice or an index list)"""
    return {k: v[idx] for k, v in params.items()}


def random_params(gen, N, H, W, translation_ratio=0.125, cutout_ratio=0.5):
    """published ranges, every group on: b in [-0.5, 0.5), s in [0, 2), k in [0.5, 1.5), shifts within +-lim, a published cutout rectangle"""
    r = lambda: torch.rand([N], generator=gen)
    lim_h, lim_w = int(H * translation_ratio + 0.5), int(W * translation_ratio + 0.5)
    size_h, size_w = int(H * cutout_ratio + 0.5), int(W * cutout_ratio + 0.5)
    t = torch.stack([torch.randint(-lim_h, lim_h + 1, [N], generator=gen), torch.randint(-lim_w, lim_w + 1, [N], generator=gen)], dim=1)
    rect = []
    for n in range(N):
        o_row = int(torch.randint(0, H + (1 - size_h % 2), [1], generator=gen))
        o_col = int(torch.randint(0, W + (1 - size_w % 2), [1], generator=gen))
        rows, cols = scatter_indices(o_row, size_h, H), scatter_indices(o_col, size_w, W)
        rect.append([int(rows.min()), int(rows.max()) + 1, int(cols.min()), int(cols.max()) + 1])
    return make_params(r() - 0.5, r() * 2, r() + 0.5, t, rect)
