"""What the spectrum tests share: the float64 restatement of DESIGN.md section 22 with numpy's own transform, the derived error bound, the
exact patterns, the random cases and the small data set of the tool tests."""
import numpy as np
import torch

from style_big_gan_amd.torch_utils.ops import spectrum

U = 2.0 ** -24
SHAPES = [(1, 1, 16, 1), (2, 3, 16, 4), (5, 3, 32, 1), (3, 1, 64, 2)]          # (B, C, R, P)


def tau(S):
    """Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2, once per pass: 2 log2(S) eta, eta = u + gamma_4 (sqrt 2 + u), plus
    3 u for the rounded normalisation and the two window products"""
    gamma4 = 4 * U / (1 - 4 * U)
    eta = U + gamma4 * (np.sqrt(2.0) + U)
    return 2 * np.log2(S) * eta + 3 * U


def restatement(images, s, t, window, S):
    """images [B, C, R, R] (any real dtype), the fp32 tables -> complex128 [B, C, S/2 + 1, S] = Y[kx, ky]: numpy.fft.fft2 of the float64
    products of the same fp32 tables"""
    x = np.asarray(images).astype(np.float64)
    w = np.asarray(window).astype(np.float64)
    u = (x * np.float64(np.float32(s)) + np.float64(np.float32(t))) * w[None, None, None, :] * w[None, None, :, None]
    Y = np.fft.fft2(u, s=(S, S))                            # [.., ky, kx]
    return np.ascontiguousarray(Y[..., :S // 2 + 1].transpose(0, 1, 3, 2))


def patterns(R, v=3.0):
    """name -> (fp32 image [R, R], the expected accumulator float64 [R/2 + 1, R] = acc[kx, ky]) for window = 0.5, s = 1, t = 0, S = R"""
    S, half = R, R // 2
    yy, xx = np.meshgrid(np.arange(R), np.arange(R), indexing="ij")
    p4 = np.array([1.0, 0.0, -1.0, 0.0])
    one, four = (R * R / 4.0) ** 2, (R * R / 8.0) ** 2

    def acc(entries):
        a = np.zeros([half + 1, S], dtype=np.float64)
        for kx, ky, val in entries:
            a[kx, ky] = val
        return a

    return {
        "constant": (np.full([R, R], v), acc([(0, 0, (v * R * R / 4.0) ** 2)])),
        "checkerboard": ((-1.0) ** (xx + yy), acc([(half, half, one)])),
        "alternating_x": ((-1.0) ** xx, acc([(half, 0, one)])),
        "alternating_y": ((-1.0) ** yy, acc([(0, half, one)])),
        "period4_x": (p4[xx % 4], acc([(S // 4, 0, four)])),
        "period4_y": (p4[yy % 4], acc([(0, S // 4, four), (0, 3 * S // 4, four)])),
    }


def pattern_tables(R, device="cpu"):
    """window = 0.5 everywhere, the twiddles of S = R"""
    return torch.full([R], 0.5, dtype=torch.float32, device=device), spectrum.tables(R, R)[1].to(device)


def random_images(kind, B, C, R, seed=0):
    """'float': fp32 normal values; 'bytes': uint8; 'bytes_f32': the same bytes as fp32"""
    rng = np.random.RandomState(seed + 1000 * R + 10 * B + C)
    if kind == "float":
        return torch.from_numpy((rng.randn(B, C, R, R) * 40 + 100).astype(np.float32))
    b = torch.from_numpy(rng.randint(0, 256, [B, C, R, R], dtype=np.uint8))
    return b if kind == "bytes" else b.to(torch.float32)


def case(kind, B, C, R, P, device="cpu", seed=0):
    """-> (images, s, t, window, twiddle, a zero accumulator) on `device`"""
    S = R * P
    window, twiddle = spectrum.tables(R, S)
    s, t = spectrum.scale_shift(101.3, 47.9)
    acc = torch.zeros([S // 2 + 1, S], dtype=torch.float64, device=device)
    return random_images(kind, B, C, R, seed).to(device), s, t, window.to(device), twiddle.to(device), acc


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    return a.shape == b.shape and a.dtype == b.dtype == torch.float64 and torch.equal(a.view(torch.int64), b.view(torch.int64))


def tool_dataset(tmp_path, n=24, res=16, seed=21):
    """a folder of n smooth res x res RGB images (a random 4 x 4 grid of levels in [20, 220], interpolated linearly along both axes) -> (path,
    its images uint8 [n, 3, res, res] in item order).  Smooth on purpose: like a photograph, and unlike white noise, such a set holds next to
    nothing in the outer band, so energy that a generator adds there can show; and no byte is within 8 of the ends of the range."""
    import json
    import os
    import PIL.Image
    from style_big_gan_amd.train_parts.datasets import ImageFolderDataset
    rng = np.random.RandomState(seed)
    root = str(tmp_path / "spectrum_data")
    os.makedirs(root, exist_ok=True)
    at = np.linspace(0.0, 3.0, res)
    names = []
    for i in range(n):
        grid = 20.0 + 200.0 * rng.rand(3, 4, 4)
        rows = np.stack([[np.interp(at, np.arange(4), grid[c, j]) for j in range(4)] for c in range(3)])           # [3, 4, res]
        img = np.stack([[np.interp(at, np.arange(4), rows[c, :, x]) for x in range(res)] for c in range(3)])       # [3, res (x), res (y)]
        names.append(f"img{i:05d}.png")
        PIL.Image.fromarray(np.round(img.transpose(2, 1, 0)).astype(np.uint8), "RGB").save(os.path.join(root, names[-1]))
    with open(os.path.join(root, "dataset.json"), "w") as f:
        json.dump({"labels": [[nm, 0] for nm in names]}, f)
    dataset = ImageFolderDataset(path=root, xflip=False)
    items = np.stack([dataset[i][0] for i in range(len(dataset))])
    dataset.close()
    assert items.shape == (n, 3, res, res) and items.min() >= 8 and items.max() <= 247
    return root, items


class OrderedGenerator(torch.nn.Module):
    """image of seed i = bank[i]: looks the latent of seed i up in the table of the seeds' latents (the tool draws them as generate.py does),
    and returns the float whose `clamp` quantisation is that byte on any device, as nearest_util.BankGenerator"""

    def __init__(self, bank, z_dim=16):
        super().__init__()
        bank = torch.as_tensor(bank)
        self.register_buffer("bank", bank.clone())
        self.z_dim, self.c_dim, self.img_resolution, self.img_channels = z_dim, 0, int(bank.shape[2]), int(bank.shape[1])
        first = np.stack([np.random.RandomState(i).randn(1, z_dim)[0, 0] for i in range(bank.shape[0])])
        assert len(set(first.tolist())) == len(first)
        self.register_buffer("first", torch.from_numpy(first))

    def forward(self, z, c, truncation_psi=1, noise_mode="const"):
        idx = (z[:, :1].to(torch.float64) == self.first[None, :]).to(torch.int64).argmax(dim=1)
        return ((self.bank[idx].to(torch.float32) + 0.5) - 128) / 127.5
