"""What the nearest_neighbors tests share: a stand-in generator whose bytes are known on every device, and the brute-force search over
`dataset[i]` in item order that the tool must equal."""
import numpy as np
import torch


class BankGenerator(torch.nn.Module):
    """a 'generator' that returns images out of a fixed uint8 bank [B, C, H, W]: image floor(|z[0]| * 1000) mod B, as the float whose
    `clamp` quantisation is that byte on any device (the centre of the byte's bin, so the rounding of x * 127.5 + 128 cannot matter)"""

    def __init__(self, bank, z_dim=16):
        super().__init__()
        self.register_buffer("bank", torch.as_tensor(bank).clone())
        self.z_dim, self.c_dim, self.img_resolution, self.img_channels = z_dim, 0, int(bank.shape[2]), int(bank.shape[1])

    def index(self, z):
        return (z[:, 0].to(torch.float64).abs() * 1000).floor().to(torch.int64) % self.bank.shape[0]

    def forward(self, z, c, truncation_psi=1, noise_mode="const"):
        return ((self.bank[self.index(z)].to(torch.float32) + 0.5) - 128) / 127.5


def seed_bytes(G, seeds):
    """the bytes BankGenerator makes for `seeds` -> uint8 ndarray [N, C, H, W]"""
    z = torch.from_numpy(np.concatenate([np.random.RandomState(s).randn(1, G.z_dim) for s in seeds]))
    return G.bank.cpu()[G.index(z)].numpy()


def make_bank(dataset, n, seed=11):
    """n images: training images, mirrored training images, training images with a few bytes changed, and noise"""
    rng = np.random.RandomState(seed)
    bank = []
    for i in range(n):
        img = dataset[int(rng.randint(len(dataset)))][0].copy()
        kind = i % 4
        if kind == 1:
            img = img[:, :, ::-1].copy()
        elif kind == 2:
            flat = img.reshape(-1)
            flat[rng.randint(0, flat.size, size=5)] ^= 0x55
        elif kind == 3:
            img = rng.randint(0, 256, img.shape, dtype=np.uint8)
        bank.append(img)
    return np.stack(bank)


def dataset_items(dataset, reduce=None):
    """every item of the data set in item order, through `reduce` (uint8 [C, H, W] -> uint8 [C, h, w]) -> int64 [len, F]"""
    items = [dataset[i][0] for i in range(len(dataset))]
    if reduce is not None:
        items = [reduce(x) for x in items]
    return np.stack(items).reshape(len(items), -1).astype(np.int64)


def brute_force(queries, items, k, skip=None):
    """queries [Q, ...] uint8, items int64 [N, F]; skip: per query a bool [N] of items left out -> (d2 int64 [Q, k], item [Q, k]),
    ascending by (d2, item)"""
    q = np.asarray(queries).reshape(len(queries), -1).astype(np.int64)
    d2_out, item_out = [], []
    for r in range(q.shape[0]):
        d2 = ((items - q[r][None, :]) ** 2).sum(1)
        if skip is not None:
            d2 = np.where(skip[r], np.iinfo(np.int64).max, d2)
        order = np.argsort(d2, kind="stable")[:k]
        d2_out.append(d2[order])
        item_out.append(order)
    return np.stack(d2_out), np.stack(item_out)


def brute_train_to_train(dataset, reduce=None):
    """d2 from every stored image (in storage order) to the nearest item of the data set that is not that stored image, in either
    orientation"""
    items = dataset_items(dataset, reduce)
    raw_idx = np.asarray(dataset._raw_idx)
    raw = np.unique(raw_idx)
    first = [int(np.nonzero((raw_idx == r) & (np.asarray(dataset._xflip) == 0))[0][0]) for r in raw]
    skip = raw_idx[None, :] == raw[:, None]
    return brute_force(items[first], items, 1, skip)[0][:, 0]
