"""Shared pieces of the variation tests: the three ops restated in plain Python ints, the byte tables of the test shapes and the op's CPU results
computed once per session, a stand-in generator whose bytes are an integer function of ws and of the noise inputs (exact in fp32 on both devices,
so a comparison of the tool across devices does not rest on convolution rounding), the CPU restatement of the package's generator with per-layer
noise inputs (the package's own runs only on the device), and the comparison of two output directories."""
import functools
import os

import numpy as np
import torch

import projector_util
from directions_util import _Mapping, same_bits  # noqa: F401  (same_bits is re-exported to the tests)
from oracle import networks as ON
from style_big_gan_amd.torch_utils.ops import moments_u8 as ops

KINDS = ("zeros", "full", "random")
FILES = ["variation.json", "variation.npz", "variation.png"]


# ---------------------------------------------------------------------------------------------------------------- restatements

def restate_accumulate(images, sum0=None, sumsq0=None):
    """uint8 [G, N, F] -> (sum, sumsq) as nested lists of Python ints, on top of the running values given"""
    g, n, f = images.shape
    total, squares = [], []
    for gi in range(g):
        columns = list(zip(*images[gi].tolist())) if n else [()] * f           # Python ints, one tuple per column
        total.append([(int(sum0[gi][fi]) if sum0 is not None else 0) + sum(col) for fi, col in enumerate(columns)])
        squares.append([(int(sumsq0[gi][fi]) if sumsq0 is not None else 0) + sum(v * v for v in col) for fi, col in enumerate(columns)])
    return total, squares


def restate_numerator(total, squares, n):
    """[G][C][P] Python ints -> [G][P]"""
    return [[sum(int(n) * int(squares[g][c][p]) - int(total[g][c][p]) ** 2 for c in range(len(total[g]))) for p in range(len(total[g][0]))]
            for g in range(len(total))]


def restate_render(num, thresholds, table):
    """[G][P] Python ints -> (heat [G][3][P], dominant [P])"""
    g, p = len(num), len(num[0])
    level = [[sum(1 for t in thresholds if int(t) <= num[gi][pi]) for pi in range(p)] for gi in range(g)]
    heat = [[[int(table[level[gi][pi]][ch]) for pi in range(p)] for ch in range(3)] for gi in range(g)]
    dominant = []
    for pi in range(p):
        best, who = 0, 255
        for gi in range(g):
            if num[gi][pi] > best:
                best, who = num[gi][pi], gi
        dominant.append(who)
    return heat, dominant


# ---------------------------------------------------------------------------------------------------------------- test tables

@functools.lru_cache(maxsize=None)
def byte_images(g, n, f, kind="random"):
    """uint8 [G, N, F], read-only"""
    if kind == "random":
        x = np.random.RandomState(10000 * g + 100 * n + f % 97).randint(0, 256, [g, n, f], dtype=np.uint8)
    else:
        x = np.full([g, n, f], 255 if kind == "full" else 0, dtype=np.uint8)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def cpu_moments(g, n, f, kind="random"):
    """(sum, sumsq) int64 [G, F] of `byte_images` through the op's CPU path from zero, computed once per session and read-only"""
    total, squares = torch.zeros([g, f], dtype=torch.int64), torch.zeros([g, f], dtype=torch.int64)
    ops.accumulate(torch.from_numpy(byte_images(g, n, f, kind).copy()), total, squares)
    out = total.numpy(), squares.numpy()
    for v in out:
        v.setflags(write=False)
    return out


def thresholds_for(values):
    """255 ascending int64 thresholds that hit some of `values` exactly"""
    values = np.unique(np.asarray(values, dtype=np.int64).reshape(-1))
    picks = values[np.linspace(0, len(values) - 1, 255).astype(np.int64)]
    return np.sort(np.maximum(picks, 1)).astype(np.int64)


def colour_table():
    t = np.arange(256, dtype=np.int64)
    return np.stack([t, 255 - t, (t * 7) % 256], axis=1).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------------------- generators

class _NoiseLayer(torch.nn.Module):
    def __init__(self, res, index):
        super().__init__()
        self.use_noise, self.resolution, self.noise_input = True, res, None
        self.register_buffer("noise_const", ((torch.arange(res * res).reshape(res, res) * (index + 2)) % 5 - 2).to(torch.float32) * 0.5)
        self.noise_strength = torch.nn.Parameter(torch.ones([]))


class _Block(torch.nn.Module):
    def __init__(self, res, first, last, index):
        super().__init__()
        self.num_conv, self.num_torgb = (1 if first else 2), 1
        if not first:
            self.conv0 = _NoiseLayer(res, index)
        self.conv1 = _NoiseLayer(res, index + 1)


class _Synthesis(torch.nn.Module):
    def __init__(self, w_dim, res):
        super().__init__()
        self.res = res
        self.block_resolutions = [4, 8][:2 if res == 8 else 1]
        index = 0
        for r in self.block_resolutions:
            block = _Block(r, r == 4, r == res, index)
            index += block.num_conv
            setattr(self, f"b{r}", block)
        self.num_ws = index + 1
        self.register_buffer("pixel", (torch.arange(3 * res * res) * 7 + 3) % (self.num_ws * w_dim))

    def layers(self):
        for r in self.block_resolutions:
            for name in ("conv0", "conv1"):
                layer = getattr(getattr(self, f"b{r}"), name, None)
                if layer is not None:
                    yield layer

    def forward(self, ws, noise_mode="const"):
        assert noise_mode in ("const", "none")
        n = ws.shape[0]
        t = torch.round(ws.reshape(n, -1)[:, self.pixel] * 4).reshape(n, 3, self.res, self.res)
        for weight, layer in enumerate(self.layers(), 1):
            if noise_mode == "none":
                continue
            noise = layer.noise_input if layer.noise_input is not None else layer.noise_const.expand(n, 1, -1, -1)
            up = self.res // layer.resolution
            b = torch.round(noise.to(ws.device) * layer.noise_strength * 2)
            t = t + float(weight) * b.repeat_interleave(up, dim=2).repeat_interleave(up, dim=3)
        return (t / 32).clamp(-1, 1)


class ExactVariationGenerator(torch.nn.Module):
    """mapping: directions_util's (selection, sign, powers of two); synthesis: with a = round(4 ws) and b_l = round(2 noise_l noise_strength_l),
    integers, pixel (c, y, x) = clamp((a.flat[(7 p + 3) % (L D)] + sum_l l b_l[y / up, x / up]) / 32, -1, 1): the layers are those of a 4 x 4 and an
    8 x 8 block ('b4.conv1', 'b8.conv0', 'b8.conv1'), four ws indices; every operation is exact in fp32"""

    def __init__(self, z_dim=12, w_dim=24, res=8):
        super().__init__()
        self.synthesis = _Synthesis(w_dim, res)
        self.num_ws = self.synthesis.num_ws
        self.z_dim, self.c_dim, self.w_dim, self.img_resolution, self.img_channels = z_dim, 0, w_dim, res, 3
        self.mapping = _Mapping(z_dim, w_dim, self.num_ws)

    def forward(self, z, c, truncation_psi=1, noise_mode="const", **kw):
        return self.synthesis(self.mapping(z, c, truncation_psi=truncation_psi), noise_mode=noise_mode)


class OracleVariationGenerator(projector_util.OracleGenerator):
    """the snapshot's weights under the CPU restatement of the package's generator (oracle/networks.py), with the surface the variation tool
    reads: block_resolutions, the blocks' layer counts, and noise layers whose `noise_input` reaches the restatement's `noises`"""

    def __init__(self, m, state):
        super().__init__(m, state)
        self.w_dim = m["w_dim"]
        self.num_ws = self.mapping.num_ws
        self.synthesis.block_resolutions = [2 ** i for i in range(2, int(np.log2(m["img_resolution"])) + 1)]
        for res in self.synthesis.block_resolutions:
            block = getattr(self.synthesis, f"b{res}")
            block.num_conv, block.num_torgb = (1 if res == 4 else 2), 1
            for name in ("conv0", "conv1"):
                layer = getattr(block, name, None)
                if layer is not None:
                    layer.use_noise, layer.resolution, layer.noise_input = True, res, None

    def _mapping(self, z, c, truncation_psi=1, truncation_cutoff=None):
        assert truncation_psi == 1 and truncation_cutoff is None
        return super()._mapping(z, c)

    def _synthesis(self, ws, noise_mode="const"):
        noises = {}
        for res in self.synthesis.block_resolutions:
            for name in ("conv0", "conv1"):
                layer = getattr(getattr(self.synthesis, f"b{res}"), name, None)
                if layer is not None and layer.noise_input is not None and noise_mode != "none":
                    noises[f"synthesis.b{res}.{name}"] = layer.noise_input
        return ON.synthesis(self._sd(), "synthesis", ws, self.cfg, noise_mode=noise_mode, noises=noises)

    def forward(self, z, c, truncation_psi=1, noise_mode="const", **kw):
        return self.synthesis(self.mapping(z, c, truncation_psi=truncation_psi), noise_mode=noise_mode)


def oracle_variation_generator(config, state, device):
    """stands in for tool_support.build_generator on the CPU, at the shape of test_calc_metrics_cpu.SG2_YAML"""
    assert config.gen.generator == "sg2_classic" and torch.device(device).type == "cpu"
    m = dict(z_dim=16, w_dim=16, img_resolution=16, channel_base=256, channel_max=16, mapping_layers=2, conv_clamp=256)
    return OracleVariationGenerator(m, state).eval().requires_grad_(False)


def set_noise_strength(snapshot, value, silent=()):
    """rewrite every noise_strength of the snapshot's generator (a fresh network has 0); the layers named in `silent` ('b8.conv0') get 0"""
    snap = torch.load(snapshot, map_location="cpu", weights_only=True)
    for state in snap.values():
        for k in state:
            if k.endswith(".noise_strength"):
                quiet = any(k == f"synthesis.{name}.noise_strength" for name in silent)
                state[k] = torch.full_like(state[k], 0.0 if quiet else float(value))
    torch.save(snap, snapshot)


# ---------------------------------------------------------------------------------------------------------------- files

def same_outputs(a, b):
    """two output directories hold the same three files: equal bytes for the json and the png, equal arrays for the npz (the archive stores the
    time it was written)"""
    if sorted(os.listdir(a)) != FILES or sorted(os.listdir(b)) != FILES:
        return False
    x, y = np.load(os.path.join(a, "variation.npz")), np.load(os.path.join(b, "variation.npz"))
    if sorted(x.files) != sorted(y.files) or not all(same_bits(x[k], y[k]) for k in x.files):
        return False
    return all(open(os.path.join(a, n), "rb").read() == open(os.path.join(b, n), "rb").read() for n in ("variation.json", "variation.png"))
