"""Inputs shared by tests/test_swd_cpu.py and tests/test_swd_gpu.py: byte image sets, small random tables, descriptor matrices through
the package's accumulator, the derived bound of the end-to-end comparison and a stand-in generator."""
import numpy as np
import torch

from style_big_gan_amd.metrics import scores

U32 = 2.0 ** -24


class TinyG(torch.nn.Module):
    """a generator's call surface: every image is a function of its own latent alone (float64 inside, so the bytes do not depend on the batch)"""

    def __init__(self, res=32, channels=3, z_dim=8, c_dim=0):
        super().__init__()
        self.z_dim, self.c_dim, self.shape = z_dim, c_dim, (channels, res, res)
        g = torch.Generator().manual_seed(11)
        self.register_buffer("w", torch.randn(z_dim, channels * res * res, generator=g, dtype=torch.float64))

    def forward(self, z, c, **kw):
        return torch.tanh(z.double() @ self.w).reshape(-1, *self.shape).float()


def byte_sets(seed=0, n=24, c=3, res=32):
    rs = np.random.RandomState(seed)
    return rs.randint(0, 256, size=[n, c, res, res]).astype(np.uint8), rs.randint(0, 256, size=[n, c, res, res]).astype(np.uint8)


def small_tables(seed, n, res, c, patches, num_dirs):
    return scores.swd_tables(seed, n, res, c, nhoods_per_image=patches, num_dirs=num_dirs)


def level_descriptors(images_u8, tables, device="cpu", batch=5):
    n, c, res = images_u8.shape[0], images_u8.shape[1], images_u8.shape[3]
    acc = scores.SwdDescriptors(n, res, c, tables["centres"], device)
    for start in range(0, n, batch):
        acc.add(start, torch.from_numpy(images_u8[start:start + batch]))
    return acc.desc


def derived_bound(desc_pairs, k):
    """|score - reference| <= 1e3 * 2 * max_m (K + 3) 2^-24 ||x_hat_m||_2: sorting is non-expansive in the max norm and the directions
    have unit norm (x_hat: the restatement's finalised descriptors of either set)"""
    worst = max(float(np.sqrt((d.astype(np.float64) ** 2).sum(axis=1)).max()) for pair in desc_pairs for d in pair)
    return 1e3 * 2 * (k + 3) * U32 * worst
