"""What the mode coverage tests share: the scalar Python-int restatement of the centroid update, seeded tables (random and planted), the bank
data set of four colour modes with its stand-in generators, and the closed formulas of the bin statistics."""
import math
import os

import numpy as np
import torch

from nearest_util import BankGenerator

UPDATE_CASES = [(1, 1, 16), (5, 3, 16), (257, 2, 48), (1000, 256, 64)]          # (N, K, F); (5, 3, 16) has an empty cluster


def table(n, k, f, seed=None, empty=None):
    """-> (points uint8 [n, f], labels int32 [n], old centroids uint8 [k, f]); cluster `empty` gets no row"""
    rng = np.random.RandomState(n + 7 * k + f if seed is None else seed)
    points = rng.randint(0, 256, [n, f], dtype=np.uint8)
    labels = rng.randint(0, k, [n]).astype(np.int32)
    if empty is not None:
        labels[labels == empty] = (empty + 1) % k
    return points, labels, rng.randint(0, 256, [k, f], dtype=np.uint8)


def update_case(n, k, f):
    return table(n, k, f, empty=1 if (n, k, f) == (5, 3, 16) else None)


def scalar_update(points, labels, old):
    """the contract in Python ints, one row and one value at a time -> (centroids uint8 [K, F], counts int64 [K], sums int64 [K, F])"""
    k, f = old.shape
    sums = [[0] * f for _ in range(k)]
    counts = [0] * k
    for row, label in zip(points.tolist(), labels.tolist()):
        counts[label] += 1
        acc = sums[label]
        for j, v in enumerate(row):
            acc[j] += v
    cent = [[(2 * s + counts[c]) // (2 * counts[c]) for s in sums[c]] if counts[c] else old[c].tolist() for c in range(k)]
    return np.array(cent, dtype=np.uint8).reshape(k, f), np.array(counts, dtype=np.int64), np.array(sums, dtype=np.int64).reshape(k, f)


def same_update(got, want):
    return all(isinstance(g, torch.Tensor) and g.dtype == torch.from_numpy(w).dtype and np.array_equal(g.cpu().numpy(), w) for g, w in zip(got, want))


def planted_table(per_group=40, f=48, seed=5):
    """4 tight groups far apart: group g has the byte 30 + 60 g everywhere, plus noise in [-3, 3], rows shuffled -> (points uint8 [4 per_group, f],
    the group of every row)"""
    rng = np.random.RandomState(seed)
    group = np.repeat(np.arange(4), per_group)
    points = (30 + 60 * group[:, None] + rng.randint(-3, 4, [4 * per_group, f])).astype(np.uint8)
    order = rng.permutation(len(group))
    return points[order], group[order]


def rounded_means(points, group):
    """the mean of every group rounded half up, in Python ints -> uint8 [groups, f]"""
    out = []
    for g in range(int(group.max()) + 1):
        rows = points[group == g].astype(np.int64)
        n = len(rows)
        out.append([(2 * int(s) + n) // (2 * n) for s in rows.sum(0)])
    return np.array(out, dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- the statistics

def closed_z(n_ref, N_ref, n_other, N_other):
    p = (n_ref + n_other) / (N_ref + N_other)
    se = math.sqrt(p * (1 - p) * (1 / N_ref + 1 / N_other))
    return (n_ref / N_ref - n_other / N_other) / se if se > 0 else 0.0


def closed_js(p, q):
    """Jensen-Shannon divergence in bits of two distributions given as lists"""
    total = 0.0
    for a, b in zip(p, q):
        m = (a + b) / 2
        total += (a * math.log2(a / m) if a > 0 else 0.0) / 2 + (b * math.log2(b / m) if b > 0 else 0.0) / 2
    return total


# ---------------------------------------------------------------------------------------------------------------- the tool's data set

MODE_COLOURS = [(40, 60, 200), (200, 50, 60), (60, 200, 70), (220, 210, 40)]


def mode_images(per_mode=60, res=16, seed=3):
    """4 modes of `per_mode` images each, uint8 [4 per_mode, 3, res, res]: a constant colour plus noise in [-4, 4]; image i belongs to mode i % 4"""
    rng = np.random.RandomState(seed)
    mode = np.arange(4 * per_mode) % 4
    colour = np.array(MODE_COLOURS, dtype=np.int64)[mode]
    return (colour[:, :, None, None] + rng.randint(-4, 5, [4 * per_mode, 3, res, res])).astype(np.uint8), mode


def write_folder(root, images, labels=None):
    """the images as an image folder of PNGs in item order, with a dataset.json of class indices when `labels` is given -> root"""
    import json
    import PIL.Image
    os.makedirs(root, exist_ok=True)
    names = [f"img{i:05d}.png" for i in range(len(images))]
    for name, img in zip(names, images):
        PIL.Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0))).save(os.path.join(root, name))
    if labels is not None:
        with open(os.path.join(root, "dataset.json"), "w") as f:
            json.dump({"labels": [[name, int(label)] for name, label in zip(names, labels)]}, f)
    return root


class ClassGenerator(BankGenerator):
    """a conditional stand-in: the image of (z, c) is one of the bank's images of class argmax(c); bank uint8 [classes, per class, C, H, W]"""

    def __init__(self, bank, z_dim=16):
        super().__init__(bank.reshape(-1, *bank.shape[2:]), z_dim=z_dim)
        self.c_dim, self.per_class = int(bank.shape[0]), int(bank.shape[1])

    def forward(self, z, c, truncation_psi=1, noise_mode="const"):
        assert c.shape == (z.shape[0], self.c_dim) and bool((c.sum(1) == 1).all())
        pick = c.argmax(1) * self.per_class + self.index(z) % self.per_class
        return ((self.bank[pick].to(torch.float32) + 0.5) - 128) / 127.5


class ListGenerator(BankGenerator):
    """BankGenerator whose image for seed s is bank[s % len(bank)]: the proportions of the bank, exactly, for any number of whole rounds.  The
    index is recovered from the seed's own latent, which is looked up in a table of the first `seeds` seeds."""

    def __init__(self, bank, seeds, z_dim=16):
        super().__init__(bank, z_dim=z_dim)
        first = np.stack([np.random.RandomState(s).randn(z_dim)[0] for s in range(seeds)])
        order = np.argsort(first)
        self.register_buffer("keys", torch.from_numpy(first[order]))
        self.register_buffer("seed_of", torch.from_numpy(order.astype(np.int64)))

    def index(self, z):
        pos = torch.searchsorted(self.keys, z[:, 0].to(torch.float64).contiguous()).clamp(max=len(self.keys) - 1)
        assert bool((self.keys[pos] == z[:, 0].to(torch.float64)).all()), "a latent outside the seed table"
        return self.seed_of[pos] % self.bank.shape[0]
