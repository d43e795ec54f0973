"""Generate tests/golden/ppl.npz by running the REFERENCE's perceptual-path-length sampler on CPU.

Run in the dev container only (the reference checkout does not travel to the GPU box):

    PYTHONPATH=/root/reference python tests/golden/make_golden_ppl.py

The reference's own ``PPLSampler`` (stylegan2ada/metrics/perceptual_path_length.py:36-94) runs seeded, small ``Generator``s of
``stylegan2ada.training.networks`` with a stand-in LPIPS network (the real one is the vgg16.pt download; nothing is fetched here:
``metric_utils.get_feature_detector`` is replaced before anything could ask for it).  Every torch RNG call of the sampler is wrapped
and recorded: t, z and -- at 16x16 -- every noise buffer are stored; at 512x512 the noise would not fit a fixture, so its per-buffer
sums are stored and the test regenerates it from the stored seed (the CPU generator is deterministic), checking the sums.

Stand-in LPIPS (restated in tests/test_ppl_cpu.py and tests/test_ppl_gpu.py): a two-scale feature pyramid on img in [0, 255]
    x = img / 127.5 - 1
    level l = 1, 2:  x = relu(conv2d(x, w_l, b_l, padding=1)) (level 2 on avg_pool2d(level 1, 2));
                     n = x / sqrt(sum_c x^2 + 1e-10);  feature_l = (n * g_l[c]).flatten(1) / sqrt(H_l * W_l)
    features = cat[feature_1, feature_2]
w_1 [8, 3, 3, 3], w_2 [8, 8, 3, 3], b_l, g_l [8] are stored as lpips/*.

Also the reference's ``compute_ppl`` tail (:128-133, percentiles + trimmed mean) on a synthetic distance array with ties at both
percentiles; the sampler, the detector and the data set are patched out (as make_golden.gen_metrics does for its feature loops).
"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import R_net, dnnlib, _import_train_parts, npy, save    # noqa: E402

EPS = 1e-4


class StandInLPIPS(torch.nn.Module):
    def __init__(self, seed=700):
        super().__init__()
        g = torch.Generator().manual_seed(seed)
        self.register_buffer("w1", torch.randn(8, 3, 3, 3, generator=g) / 27 ** 0.5)
        self.register_buffer("b1", torch.randn(8, generator=g) * 0.1)
        self.register_buffer("g1", torch.rand(8, generator=g) + 0.5)
        self.register_buffer("w2", torch.randn(8, 8, 3, 3, generator=g) / 72 ** 0.5)
        self.register_buffer("b2", torch.randn(8, generator=g) * 0.1)
        self.register_buffer("g2", torch.rand(8, generator=g) + 0.5)

    def forward(self, img, resize_images=False, return_lpips=True):
        x = img / 127.5 - 1
        feats = []
        for lvl, (w, b, gw) in enumerate([(self.w1, self.b1, self.g1), (self.w2, self.b2, self.g2)]):
            if lvl:
                x = torch.nn.functional.avg_pool2d(x, 2)
            x = torch.relu(torch.nn.functional.conv2d(x, w, b, padding=1))
            n = x / (x.square().sum(1, keepdim=True) + 1e-10).sqrt()
            feats.append((n * gw.view(1, -1, 1, 1)).flatten(1) / (x.shape[2] * x.shape[3]) ** 0.5)
        return torch.cat(feats, 1)


class RecordRNG:
    """wraps torch.rand / torch.randn / torch.randn_like and records what they return, in call order"""

    def __init__(self):
        self.calls = []

    def __enter__(self):
        self.saved = torch.rand, torch.randn, torch.randn_like
        def wrap(name, fn):
            def f(*a, **k):
                out = fn(*a, **k)
                self.calls.append((name, out.detach().clone()))
                return out
            return f
        torch.rand, torch.randn, torch.randn_like = wrap("rand", self.saved[0]), wrap("randn", self.saved[1]), wrap("randn_like", self.saved[2])
        return self

    def __exit__(self, *exc):
        torch.rand, torch.randn, torch.randn_like = self.saved


def make_G(seed, res, c_dim, cbase, cmax):
    torch.manual_seed(seed)
    G = R_net.Generator(z_dim=16, c_dim=c_dim, w_dim=16, img_resolution=res, img_channels=3, mapping_kwargs=dnnlib.EasyDict(num_layers=2),
                        synthesis_kwargs=dnnlib.EasyDict(channel_base=cbase, channel_max=cmax, num_fp16_res=4, conv_clamp=256))
    with torch.no_grad():       # non-trivial noise strengths and biases so every term reaches the images
        for name, p in G.named_parameters():
            if name.endswith("noise_strength"):
                p.fill_(0.3)
            if name.endswith(".bias") and "affine" not in name and "mapping" not in name:
                p.copy_(torch.randn_like(p) * 0.1)
    return G.eval().requires_grad_(False)


def main():
    _import_train_parts()
    from stylegan2ada.metrics import metric_utils as R_mu
    R_mu.get_feature_detector = lambda *a, **k: None        # compute_ppl asks for the vgg16 URL: never fetched, the sampler is patched out
    from stylegan2ada.metrics import perceptual_path_length as R_ppl

    lpips = StandInLPIPS().eval()
    arrays = {f"lpips/{k}": npy(v) for k, v in lpips.state_dict().items()}
    nets = dict(g16c0=make_G(710, 16, 0, 256, 32), g16c3=make_G(711, 16, 3, 256, 32), g512=make_G(712, 512, 0, 4096, 8))
    for tag, G in nets.items():
        arrays.update({f"{tag}/{k}": npy(v) for k, v in G.state_dict().items() if not k.endswith(".noise_const")})     # redrawn per batch
    runs = [("g16c0", "z", "full", True), ("g16c0", "w", "end", True), ("g16c0", "w", "end", False),
            ("g16c3", "z", "full", True), ("g16c3", "w", "end", True), ("g16c3", "w", "end", False),
            ("g512", "w", "full", True)]
    cases = []
    for idx, (tag, space, sampling, crop) in enumerate(runs):
        G = nets[tag]
        sampler = R_ppl.PPLSampler(G=G, G_kwargs={}, epsilon=EPS, space=space, sampling=sampling, crop=crop, vgg16=lpips).eval()
        names = [n for n, _ in sampler.G.named_buffers() if n.endswith(".noise_const")]
        key = f"r{idx}"
        batches = []
        for bi in range(2):             # two batches: the second one's noise must replace the first one's everywhere
            seed = 9000 + 10 * idx + bi
            c = torch.nn.functional.one_hot(torch.tensor([bi, bi + 1]) % 3, 3).float()[:, :G.c_dim]
            torch.manual_seed(seed)
            with RecordRNG() as rec, torch.no_grad():
                dist = sampler(c)
            kinds = [k for k, _ in rec.calls]
            assert kinds == ["rand", "randn"] + ["randn_like"] * len(names), kinds
            t, z = rec.calls[0][1], rec.calls[1][1]
            noise = [v for _, v in rec.calls[2:]]
            bkey = f"{key}/b{bi}"
            arrays.update({f"{bkey}/c": npy(c), f"{bkey}/t": npy(t), f"{bkey}/z": npy(z), f"{bkey}/dist": npy(dist),
                           f"{bkey}/noise_sums": np.asarray([float(v.double().sum()) for v in noise])})
            if G.img_resolution <= 16:
                for n, v in zip(names, noise):
                    arrays[f"{bkey}/noise/{n}"] = npy(v)
            batches.append(dict(seed=seed))
        cases.append(dict(key=key, G=tag, space=space, sampling=sampling, crop=crop, batches=batches, noise_names=names))

    # compute_ppl's tail on synthetic distances with ties at both percentiles; num_samples is not a multiple of the batch
    rng = np.random.RandomState(720)
    n = 301
    dist = rng.gamma(2.0, 50.0, size=n + 1).astype(np.float32)
    order = np.argsort(dist)
    dist[order[:6]] = dist[order[3]]                # ties around the 1st percentile ('lower')
    dist[order[-7:]] = dist[order[-4]]              # and around the 99th ('higher')
    arrays["tail/dist"] = dist

    class FakeSampler(torch.nn.Module):
        def __init__(self, *a, **k):
            super().__init__()
            self.pos = 0

        def forward(self, c):
            out = torch.from_numpy(dist[self.pos: self.pos + c.shape[0]].copy())
            self.pos += c.shape[0]
            return out

    class FakeDataset:
        def __init__(self, **kw):
            pass

        def __len__(self):
            return 4

        def get_label(self, idx):
            return np.zeros([0], dtype=np.float32)

    saved = R_ppl.PPLSampler, R_ppl.datasets, torch.Tensor.pin_memory
    R_ppl.PPLSampler, R_ppl.datasets = FakeSampler, {"image_folder": FakeDataset}
    torch.Tensor.pin_memory = lambda self: self
    try:
        opts = R_mu.MetricOptions(G=None, num_gpus=1, rank=0, device=torch.device("cpu"), cache=False)
        arrays["tail/ppl"] = np.asarray(R_ppl.compute_ppl(opts, num_samples=n, epsilon=EPS, space="w", sampling="end", crop=True, batch_size=2),
                                        dtype=np.float64)
    finally:
        R_ppl.PPLSampler, R_ppl.datasets, torch.Tensor.pin_memory = saved
    save("ppl", arrays, dict(epsilon=EPS, cases=cases, tail_num_samples=n, z_dim=16, w_dim=16, mapping_layers=2,
                             nets=dict(g16c0=dict(res=16, c_dim=0, channel_base=256, channel_max=32),
                                       g16c3=dict(res=16, c_dim=3, channel_base=256, channel_max=32),
                                       g512=dict(res=512, c_dim=0, channel_base=4096, channel_max=8)),
                             synthesis=dict(num_fp16_res=4, conv_clamp=256)))


if __name__ == "__main__":
    main()
