"""Shared pieces of the image-export tests: the fixture (tests/golden/image_export.npz, written by
tests/golden/make_golden_image_export.py from the reference), the toy data sets both sides build from a seed, the tie vectors, and
the CPU restatement of the fixture's generators behind the surface generate_images / generate_style_mix use."""
import numpy as np
import torch

from golden_util import Golden
from oracle import networks as ON
import projector_util as pu


def fixture():
    return Golden("image_export")


class _Details:
    def __init__(self, raw_label):
        self.raw_label = raw_label


class ToyDataset:
    """what `setup_snapshot_image_grid` reads of a data set: image_shape, has_labels, len, indexing -> (uint8 image, float32 label),
    get_details(idx).raw_label.  Seeded; records the indices it is asked for."""

    def __init__(self, n, shape, num_classes, seed):
        rng = np.random.RandomState(seed)
        self.image_shape = list(shape)
        self.has_labels = num_classes > 0
        self.images = rng.randint(0, 256, [n] + list(shape)).astype(np.uint8)
        self.raw = rng.randint(0, max(num_classes, 1), [n]).astype(np.int64)
        self.num_classes = num_classes
        self.asked = []

    def __len__(self):
        return len(self.images)

    def get_details(self, idx):
        return _Details(self.raw[idx].copy())

    def __getitem__(self, idx):
        self.asked.append(int(idx))
        label = np.zeros([self.num_classes], dtype=np.float32)
        if self.has_labels:
            label[self.raw[idx]] = 1
        return self.images[idx].copy(), label


TOY_SETS = dict(labelled=dict(n=41, shape=(3, 4, 8), num_classes=3, seed=11), grey=dict(n=23, shape=(1, 8, 8), num_classes=0, seed=12))


def tie_vector():
    """fp32 [1, 1, 1, 264]: x = (k + 0.5) / 127.5 - 1 for k = 0..254 (many of them exact ties of the grid rule at drange [-1, 1]), then
    values outside the range and just inside its ends"""
    k = np.arange(255, dtype=np.float32)
    x = (k + np.float32(0.5)) / np.float32(127.5) - np.float32(1)
    extra = np.asarray([-1.0, 1.0, -1.004, 1.004, -3.0, 3.0, -1e30, 1e30, 0.0], dtype=np.float32)
    return np.concatenate([x, extra]).astype(np.float32).reshape(1, 1, 1, -1)


def flip_cap(img_ref):
    """the largest share of uint8 pixels that may differ between two fp32 evaluations of the same generator: the images agree within
    e = 1e-4 * max|img| (the bound test_forward_fp32 holds the device to), a byte can change only if the value lies within e of a
    rounding boundary, and boundaries are 1 / 127.5 apart -> share <= 2 e / (1 / 127.5) = 255e-4 * max|img|"""
    return 255 * 1e-4 * float(np.abs(img_ref).max())


def net_meta(g, tag):
    m = dict(g.meta["nets"][tag])
    return dict(z_dim=m["z_dim"], w_dim=m["w_dim"], c_dim=m["c_dim"], img_resolution=m["res"], channel_base=m["channel_base"],
                channel_max=m["channel_max"], mapping_layers=m["mapping_layers"], conv_clamp=m["conv_clamp"])


class OracleGenerator(pu.OracleGenerator):
    """projector_util.OracleGenerator plus what the image tools use: labels, num_ws / w_dim, G(z, c, truncation_psi, noise_mode) with the
    reference mapping network's truncation (torch.lerp(w_avg, w, psi), stylegan2ada/training/networks.py:241-248) and `mapping.w_avg`"""

    def __init__(self, m, state):
        super().__init__(m, state)
        self.cfg = ON.default_cfg(z_dim=m["z_dim"], w_dim=m["w_dim"], c_dim=m["c_dim"], img_resolution=m["img_resolution"],
                                  channel_base=m["channel_base"], channel_max=m["channel_max"], mapping_layers=m["mapping_layers"],
                                  g_architecture="skip", conv_clamp=m["conv_clamp"])
        self.c_dim, self.w_dim, self.num_ws = m["c_dim"], m["w_dim"], self.mapping.num_ws

    def forward(self, z, c, truncation_psi=1, noise_mode="const"):
        ws = self.mapping(z.to(torch.float32), c)
        if truncation_psi != 1:
            ws = self.mapping.w_avg.lerp(ws, truncation_psi)
        return self.synthesis(ws, noise_mode=noise_mode)


def oracle_generator(g, tag):
    return OracleGenerator(net_meta(g, tag), g.state_dict(f"{tag}/G"))


def product_generator(g, tag, device):
    """the package's sg2_classic generator with the fixture's weights, fp32 throughout"""
    from style_big_gan_amd.train_parts.generators import generators
    m = net_meta(g, tag)
    G = generators["sg2_classic"](z_dim=m["z_dim"], c_dim=m["c_dim"], w_dim=m["w_dim"], img_resolution=m["img_resolution"], img_channels=3,
                                  mapping_kwargs=dict(num_layers=m["mapping_layers"]),
                                  synthesis_kwargs=dict(channel_base=m["channel_base"], channel_max=m["channel_max"], num_fp16_res=0,
                                                        block_kwargs=dict(conv_clamp=m["conv_clamp"])))
    G.load_state_dict(g.state_dict(f"{tag}/G"), strict=True)
    return G.eval().requires_grad_(False).to(device)
