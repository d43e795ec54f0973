"""Shared pieces of the latent-projector tests: the fixture (tests/golden/projector.npz, written by
tests/golden/make_golden_projector.py from the reference's project()), its generators, its recorded draws and the CPU restatement of
the generator behind the surface project() uses."""
import numpy as np
import torch

from golden_util import Golden
from oracle import networks as ON

# Relative bound on w_out (max |w - w_ref| / max |w_ref|) between the reference's project() and another fp32 evaluation of the same
# loop (different op compositions, CPU or GPU).  Every step moves w by Adam's normalised update, lr * m / (sqrt(v) + 1e-8), whose
# size is ~lr whatever the gradient's scale, so a relative rounding difference delta in the gradient changes the update by ~lr * delta.
# The gradient of a depth-L fp32 synthesis + detector differs by ~1e-6 relative between compositions; over the fixture's 10 steps
# (lr <= 0.1, |w| ~ 1) that is ~10 * 0.1 * 1e-6 ~ 1e-6 of |w|.  Measured: 2.3e-7 .. 4.9e-7 for the CPU restatement
# (oracle/networks.py), 3.1e-7 .. 6.1e-7 for the device path.  Bound: 5e-6, eight times the worst measured.
# What the bound rejects: a regulariser scaled by 1/2 moves w_out by 1.4e-4 (g32) and 8.6e-6 (g16), a missing deepest pyramid
# level by ~0.1; on g512 (2 steps, the first with lr = 0) neither is visible, so that case checks the area path and the synthesis.
# The kernels' own exactness tests pin the regulariser's scale independently.
REL_BOUND = 5e-6


def fixture():
    return Golden("projector")


def case(g, tag):
    return next(c for c in g.meta["cases"] if c["tag"] == tag)


def net_meta(g, c):
    return dict(z_dim=g.meta["z_dim"], w_dim=g.meta["w_dim"], c_dim=0, img_resolution=c["res"], channel_base=c["channel_base"],
                channel_max=c["channel_max"], mapping_layers=g.meta["mapping_layers"], conv_clamp=g.meta["synthesis"]["conv_clamp"])


def target(g, c):
    """[3, R, R] uint8 as a tensor (stored up to 32x32; regenerated from the case's seed above that and checked against the stored sum)"""
    key = f"{c['tag']}/target"
    if key in g:
        t = g.npz[key]
    else:
        seed = {"g32": 720, "g16": 721, "g512": 722}[c["tag"]]
        t = np.random.RandomState(seed).randint(0, 256, [3, c["res"], c["res"]]).astype(np.uint8)
    assert int(t.astype(np.int64).sum()) == int(g.npz[f"{c['tag']}/target_sum"])
    return torch.from_numpy(t.copy())


def draws(g, c):
    """the recorded draws of a case: 'noise' in the order of the reference's noise buffers (which is this package's `named_buffers`
    order too), 'w_noise' [num_steps, 1, w_dim]"""
    tag = c["tag"]
    names = c["noise_names"]
    if f"{tag}/noise/{names[0]}" in g:
        noise = [g.t(f"{tag}/noise/{n}") for n in names]
    else:
        torch.manual_seed(c["draw_seed"])
        noise = []
        for n in names:             # b<res>.conv<i>.noise_const is [res, res]; drawn by randn_like in this order
            res = int(n.split(".")[0][1:])
            noise.append(torch.randn([res, res]))
        for v, s in zip(noise, g.npz[f"{tag}/noise_sums"]):
            assert abs(float(v.double().sum()) - float(s)) <= 1e-9 * max(1.0, abs(float(s))), "the CPU generator no longer replays the draws"
    return dict(noise=noise, w_noise=g.t(f"{tag}/w_noise"))


def product_generator(g, c, device):
    """the package's sg2_classic generator with the fixture's weights, fp32 throughout (num_fp16_res=0, as the fixture's)"""
    from style_big_gan_amd.train_parts.generators import generators
    m = net_meta(g, c)
    G = generators["sg2_classic"](z_dim=m["z_dim"], c_dim=0, w_dim=m["w_dim"], img_resolution=m["img_resolution"], img_channels=3,
                                  mapping_kwargs=dict(num_layers=m["mapping_layers"]),
                                  synthesis_kwargs=dict(channel_base=m["channel_base"], channel_max=m["channel_max"], num_fp16_res=0,
                                                        block_kwargs=dict(conv_clamp=m["conv_clamp"])))
    missing, unexpected = G.load_state_dict(g.state_dict(f"{c['tag']}/G"), strict=False)
    assert not unexpected and all(k.endswith(".noise_const") for k in missing), (missing, unexpected)
    return G.eval().requires_grad_(False).to(device)


class _Part(torch.nn.Module):
    """`mapping` / `synthesis` of OracleGenerator: evaluates the CPU restatement on the whole generator's state"""

    def __init__(self, root, what, **attrs):
        super().__init__()
        object.__setattr__(self, "root", root)      # not a submodule; deepcopy of the generator maps it to the copy
        self.what = what
        for k, v in attrs.items():
            setattr(self, k, v)

    def forward(self, *a, **k):
        return getattr(self.root, self.what)(*a, **k)


class OracleGenerator(torch.nn.Module):
    """the fixture's generator as the CPU restatement (oracle/networks.py) behind the surface project() uses: z_dim, img_resolution,
    img_channels, mapping(z, c) with mapping.num_ws, synthesis(ws, noise_mode), and the weights / noise buffers under the generator's
    own state-dict names, so the `.noise_const` buffers can be optimised in place.  `state`: a state dict with the noise buffers."""

    def __init__(self, m, state):
        super().__init__()
        self.cfg = ON.default_cfg(z_dim=m["z_dim"], w_dim=m["w_dim"], c_dim=0, img_resolution=m["img_resolution"],
                                  channel_base=m["channel_base"], channel_max=m["channel_max"], mapping_layers=m["mapping_layers"],
                                  g_architecture="skip", conv_clamp=m["conv_clamp"])
        self.z_dim, self.c_dim, self.img_resolution, self.img_channels = m["z_dim"], 0, m["img_resolution"], 3
        num_ws = ON.synthesis_num_ws(self.cfg)
        self.mapping, self.synthesis = _Part(self, "_mapping", num_ws=num_ws), _Part(self, "_synthesis")
        for k, v in state.items():
            *path, leaf = k.split(".")
            mod = self
            for p in path:
                if p not in mod._modules:
                    mod.add_module(p, torch.nn.Module())
                mod = mod._modules[p]
            mod.register_buffer(leaf, v.clone())

    def _sd(self):
        return dict(self.state_dict(keep_vars=True))

    def _mapping(self, z, c):
        return ON.mapping(self._sd(), "mapping", z, c, self.cfg, num_ws=self.mapping.num_ws)

    def _synthesis(self, ws, noise_mode="const"):
        return ON.synthesis(self._sd(), "synthesis", ws, self.cfg, noise_mode=noise_mode)


def oracle_generator(g, c):
    state = g.state_dict(f"{c['tag']}/G")
    for n in c["noise_names"]:                  # the fixture leaves them out; project() draws them anew
        res = int(n.split(".")[0][1:])
        state[f"synthesis.{n}"] = torch.zeros([res, res])
    return OracleGenerator(net_meta(g, c), state)
