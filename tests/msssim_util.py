"""What the MS-SSIM tests share: an independent float64 restatement of DESIGN.md section 23 (the 11 x 11 outer-product window through
torch.nn.functional.conv2d, avg_pool2d between the levels, plain means -- no use of the op layer), the derived bounds, the case builders
and the stand-ins of the tool tests."""
import json
import os

import numpy as np
import torch

TERM_ATOL = 1e-9        # per-level term: values <= 255, moments <= 65025, under 40 float64 roundings per moment: below 3e-10 per moment;
                        # the denominators are >= C1 = 6.5 and >= C2 = 58.5
SCORE_RTOL = 1e-8       # pair score, on pairs whose every level term is >= 0.1 (the power is not Lipschitz near 0)
PUBLISHED = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
GPU_SHAPES = [(1, 1, 16), (5, 3, 32), (2, 3, 64), (1, 1, 512)]     # (N, C, S): a 6 x 6 map; a ragged 22 x 22 map, odd image-channel count; 54 x 54:
                                                                    # 4 x 2 tiles; 502 x 502: 32 x 16 = 512 tiles, two rounds per lane of the merge


def ref_window2d():
    k = torch.arange(11, dtype=torch.float64)
    g = torch.exp(-(k - 5) ** 2 / 4.5)
    g = g / g.sum()
    return torch.outer(g, g)


def ref_level_terms(x, y):
    """x, y [N, C, S, S] of any real dtype -> float64 [N, C, 2]: the plain means of the cs and the ssim map"""
    n, c, s = x.shape[0], x.shape[1], x.shape[3]
    a, b = (v.detach().cpu().to(torch.float64).reshape(n * c, 1, s, s) for v in (x, y))
    w = ref_window2d()[None, None]
    conv = lambda v: torch.nn.functional.conv2d(v, w)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    m1, m2 = conv(a), conv(b)
    s11, s22, s12 = conv(a * a) - m1 * m1, conv(b * b) - m2 * m2, conv(a * b) - m1 * m2
    cs = (2 * s12 + c2) / (s11 + s22 + c2)
    ssim = (2 * m1 * m2 + c1) / (m1 * m1 + m2 * m2 + c1) * cs
    return torch.stack([cs.mean(dim=(1, 2, 3)), ssim.mean(dim=(1, 2, 3))], dim=1).reshape(n, c, 2)


def ref_num_levels(s):
    return min(5, int(np.log2(s)) - 3)


def ref_pair_scores(x, y):
    """-> (float64 [N] scores, float64 [N, C, L] terms)"""
    s = x.shape[3]
    num = ref_num_levels(s)
    w = np.array(PUBLISHED[:num], dtype=np.float64)
    if num < 5:
        w = w / w.sum()
    a, b = x.detach().cpu().to(torch.float64), y.detach().cpu().to(torch.float64)
    terms = []
    for i in range(num):
        t = ref_level_terms(a, b)
        terms.append(t[:, :, 1 if i == num - 1 else 0])
        if i + 1 < num:
            a, b = torch.nn.functional.avg_pool2d(a, 2), torch.nn.functional.avg_pool2d(b, 2)
    terms = torch.stack(terms, dim=2)
    score = (terms.clamp(min=0) ** torch.from_numpy(w)).prod(dim=2).mean(dim=1)
    return score, terms


def random_pair(kind, n, c, s, seed=0, device="cpu"):
    """'float': fp32 uniform in [0, 255]; 'bytes': independent uint8"""
    rng = np.random.RandomState(seed + 1000 * s + 10 * n + c)
    if kind == "float":
        x, y = (torch.from_numpy((rng.rand(n, c, s, s) * 255).astype(np.float32)) for _ in range(2))
    else:
        x, y = (torch.from_numpy(rng.randint(0, 256, [n, c, s, s], dtype=np.uint8)) for _ in range(2))
    return x.to(device), y.to(device)


def smooth_images(n, c, s, seed=0):
    """image-like uint8 [n, c, s, s]: a random 4 x 4 grid of levels in [30, 220] interpolated linearly along both axes, plus +-6 of texture"""
    rng = np.random.RandomState(seed)
    at = np.linspace(0.0, 3.0, s)
    out = np.empty([n, c, s, s])
    for i in range(n):
        for ch in range(c):
            grid = 30.0 + 190.0 * rng.rand(4, 4)
            rows = np.stack([np.interp(at, np.arange(4), grid[j]) for j in range(4)])          # [4, s]
            out[i, ch] = np.stack([np.interp(at, np.arange(4), rows[:, x]) for x in range(s)], axis=1)
    return np.clip(np.round(out + rng.randint(-6, 7, out.shape)), 0, 255).astype(np.uint8)


def correlated_pair(n, c, s, seed=0, device="cpu"):
    """an image-like x and y = clip(x + integer noise in [-20, 20]) -> uint8 tensors"""
    x = smooth_images(n, c, s, seed)
    noise = np.random.RandomState(seed + 77).randint(-20, 21, x.shape)
    y = np.clip(x.astype(np.int64) + noise, 0, 255).astype(np.uint8)
    return torch.from_numpy(x).to(device), torch.from_numpy(y).to(device)


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    view = {torch.float64: torch.int64, torch.float32: torch.int32}[a.dtype]
    return torch.equal(a.view(view), b.view(view))


# ------------------------------------------------------------------------------------------------ the tool's stand-ins

class ClassGenerator(torch.nn.Module):
    """image of (seed i, class k) = bank[(i + shift * k) % len(bank)]: looks the latent of seed i up in the table of the seeds' latents (the tool
    draws them as generate.py does) and returns the float whose `clamp` quantisation is that byte on any device"""

    def __init__(self, bank, c_dim=0, shift=0, z_dim=16):
        super().__init__()
        bank = torch.as_tensor(bank)
        self.register_buffer("bank", bank.clone())
        self.z_dim, self.c_dim, self.img_resolution, self.img_channels = z_dim, c_dim, int(bank.shape[2]), int(bank.shape[1])
        self.shift = shift
        first = np.stack([np.random.RandomState(i).randn(z_dim)[0] for i in range(bank.shape[0])])
        assert len(set(first.tolist())) == len(first)
        self.register_buffer("first", torch.from_numpy(first))

    def forward(self, z, c, truncation_psi=1, noise_mode="const"):
        idx = (z[:, :1].to(torch.float64) == self.first[None, :]).to(torch.int64).argmax(dim=1)
        if self.c_dim:
            idx = (idx + self.shift * c.argmax(dim=1)) % self.bank.shape[0]
        return ((self.bank[idx].to(torch.float32) + 0.5) - 128) / 127.5


def tool_dataset(tmp_path, images, labels=None, name="div_data"):
    """a folder of the uint8 [n, 3, s, s] `images` as PNG files, with a dataset.json of the class indices `labels` when given -> its path"""
    import PIL.Image
    root = str(tmp_path / name)
    os.makedirs(root, exist_ok=True)
    names = []
    for i, img in enumerate(images):
        names.append(f"img{i:05d}.png")
        PIL.Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)), "RGB").save(os.path.join(root, names[-1]))
    if labels is not None:
        with open(os.path.join(root, "dataset.json"), "w") as f:
            json.dump({"labels": [[nm, int(k)] for nm, k in zip(names, labels)]}, f)
    return root
