"""Perceptual path length, host side: the registry, the sampler against the reference's own PPLSampler (tests/golden/ppl.npz), the
reduction against the reference's compute_ppl tail, the multi-rank exchange and the trainer's setup guard.

The package's generator runs only on the device, so the CPU sampler runs the CPU restatement of the same network (oracle/networks.py)
behind a module with the generator's surface (mapping / synthesis / named noise buffers); the sampler's own arithmetic takes the op
layer's CPU branch (the reference's formulas).  The fixture's stand-in LPIPS network is restated in tests/ppl_util.py."""
import os
import sys
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from oracle import networks as ON
from style_big_gan_amd.metrics import metric_main, metric_utils
from style_big_gan_amd.metrics import perceptual_path_length as ppl
from golden_util import make_image_folder
import ppl_util

PPL_NAMES = ["ppl_zfull", "ppl_wfull", "ppl_zend", "ppl_wend", "ppl2_wend"]


class _Part(torch.nn.Module):
    """`mapping` / `synthesis` of OracleGenerator: holds its weights, evaluates the CPU restatement on the whole generator's state"""

    def __init__(self, root, what):
        super().__init__()
        object.__setattr__(self, "root", root)      # not a submodule; deepcopy of the generator maps it to the copy
        self.what = what

    def forward(self, *a, **k):
        return getattr(self.root, self.what)(*a, **k)


class OracleGenerator(torch.nn.Module):
    """the fixture's generator as the CPU restatement (oracle/networks.py) behind the surface PPLSampler uses: z_dim, c_dim,
    img_resolution, img_channels, mapping(z, c), synthesis(ws, noise_mode, force_fp32), and the weights / noise buffers under the
    generator's own state-dict names (so `.noise_const` buffers can be redrawn in place)"""

    def __init__(self, g, tag):
        super().__init__()
        m = ppl_util.net_meta(g, tag)
        self.cfg = ON.default_cfg(z_dim=m["z_dim"], w_dim=m["w_dim"], c_dim=m["c_dim"], img_resolution=m["img_resolution"],
                                  channel_base=m["channel_base"], channel_max=m["channel_max"], mapping_layers=m["mapping_layers"],
                                  g_architecture="skip", conv_clamp=m["conv_clamp"])
        self.z_dim, self.c_dim, self.img_resolution, self.img_channels = m["z_dim"], m["c_dim"], m["img_resolution"], 3
        self.num_ws = ON.synthesis_num_ws(self.cfg)
        self.mapping, self.synthesis = _Part(self, "_mapping"), _Part(self, "_synthesis")
        state = g.state_dict(tag)
        case = next(c for c in g.meta["cases"] if c["G"] == tag)
        for n in case["noise_names"]:          # the fixture leaves them out; they are redrawn per batch anyway
            res = int(n.split(".")[1][1:])
            state[n] = torch.zeros([res, res])
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
        return ON.mapping(self._sd(), "mapping", z, c, self.cfg, num_ws=self.num_ws)

    def _synthesis(self, ws, noise_mode="const", force_fp32=True):
        return ON.synthesis(self._sd(), "synthesis", ws, self.cfg, noise_mode=noise_mode)


def _sampler(g, case, G, **kw):
    return ppl.PPLSampler(G=G, G_kwargs={}, epsilon=g.meta["epsilon"], space=case["space"], sampling=case["sampling"], crop=case["crop"],
                          vgg16=ppl_util.StandInLPIPS(g), vgg16_kwargs={}, **kw).eval().requires_grad_(False)


def test_all_five_ppl_metrics_are_registered():
    for name in PPL_NAMES:
        assert metric_main.is_valid_metric(name), name
    assert "perceptual-path-length family" in metric_main.__doc__ and "not registered" not in metric_main.__doc__


_G = ppl_util.fixture()


@pytest.mark.parametrize("case", _G.meta["cases"], ids=[f"{c['G']}-{c['space']}-{c['sampling']}-{'crop' if c['crop'] else 'nocrop'}" for c in _G.meta["cases"]])
def test_sampler_reproduces_the_reference_per_pair(case):
    """replayed draws, per-pair distances within ppl_util.REL_BOUND of the reference's (both fp32 on the CPU: the rounding of two different
    but equivalent op compositions, amplified by 1 / eps^2 -- derivation at REL_BOUND); the second batch's noise replaces the first's"""
    g = _G
    sampler = _sampler(g, case, OracleGenerator(g, case["G"]))
    names = [n[len("G."):] for n, _ in sampler.named_buffers() if n.endswith(".noise_const")]
    assert names == case["noise_names"]
    for bi in range(len(case["batches"])):
        key = f"{case['key']}/b{bi}"
        draws = ppl_util.batch_draws(g, case, bi, names)
        with torch.no_grad():
            d = sampler(g.t(f"{key}/c"), draws=draws)
        ref = g.t(f"{key}/dist")
        rel = ((d - ref).abs() / ref.abs()).max().item()
        assert rel < ppl_util.REL_BOUND, (key, d, ref, rel)


def test_default_draws_follow_the_reference_call_order():
    """no draws handed in: the sampler draws t, z and the noise itself, in the reference's order -- after the batch's seed it reproduces the
    replayed result exactly"""
    g = _G
    case = g.meta["cases"][0]
    sampler = _sampler(g, case, OracleGenerator(g, case["G"]))
    names = [n[len("G."):] for n, _ in sampler.named_buffers() if n.endswith(".noise_const")]
    key = f"{case['key']}/b0"
    with torch.no_grad():
        replay = sampler(g.t(f"{key}/c"), draws=ppl_util.batch_draws(g, case, 0, names))
        torch.manual_seed(case["batches"][0]["seed"])
        own = sampler(g.t(f"{key}/c"))
    assert torch.equal(own, replay)


def test_reduction_matches_the_reference_tail():
    g = _G
    n = g.meta["tail_num_samples"]
    d = g.npz["tail/dist"]
    assert ppl.ppl_from_distances(d[:n]) == float(g.npz["tail/ppl"])


class _ListSampler:
    """deterministic stand-in sampler: batch k of this rank's loop is values[(k * world + rank) * B : ... + B]"""

    def __init__(self, values, batch, world=1, rank=0):
        self.values, self.batch, self.world, self.rank, self.k = values, batch, world, rank, 0

    def __call__(self, c):
        i = (self.k * self.world + self.rank) * self.batch
        self.k += 1
        out = np.zeros(self.batch, dtype=np.float32)
        chunk = self.values[i:i + self.batch]
        out[:len(chunk)] = chunk
        return torch.from_numpy(out).to(c.device)


def test_compute_ppl_tail_single_process(tmp_path):
    """compute_ppl's loop (labels from the data set, batches of 2, truncation to num_samples) + tail == the reference's compute_ppl on the same
    distances (fixture: num_samples = 301, not a multiple of the batch)"""
    g = _G
    n = g.meta["tail_num_samples"]
    d = g.npz["tail/dist"]
    path = make_image_folder(str(tmp_path / "data"), n=6, res=16)
    opts = metric_utils.MetricOptions(dataset_kwargs=dict(path=path), num_gpus=1, rank=0, device=torch.device("cpu"), cache=False)
    got = ppl.compute_ppl(opts, num_samples=n, epsilon=1e-4, space="w", sampling="end", crop=True, batch_size=2, sampler=_ListSampler(d, 2))
    assert got == float(g.npz["tail/ppl"])


def _world_worker(rank, world, init_file, results, path, values, num_samples, batch):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import style_big_gan_amd  # noqa: F401
    from style_big_gan_amd.metrics import metric_utils as mu, perceptual_path_length as P
    dist.init_process_group("gloo", init_method=f"file://{init_file}", rank=rank, world_size=world)
    try:
        opts = mu.MetricOptions(dataset_kwargs=dict(path=path), num_gpus=world, rank=rank, device=torch.device("cpu"), cache=False)
        got = P.compute_ppl(opts, num_samples=num_samples, epsilon=1e-4, space="w", sampling="end", crop=True, batch_size=batch,
                            sampler=_ListSampler(values, batch, world, rank))
        results[rank] = got
    finally:
        dist.destroy_process_group()


def test_compute_ppl_world2_gloo(tmp_path):
    """two ranks: rank 0's value equals the single-process value on the reference's interleaving (iteration by iteration, ranks in order),
    with num_samples (301) not a multiple of batch x world (4): the last round's surplus is cut off after interleaving"""
    rng = np.random.RandomState(3)
    values = rng.gamma(2.0, 50.0, size=400).astype(np.float32)
    num_samples, batch, world = 301, 2, 2
    expect = ppl.ppl_from_distances(values[:num_samples])
    path = make_image_folder(str(tmp_path / "data"), n=6, res=16)
    with tempfile.TemporaryDirectory() as d:
        mgr = mp.Manager()
        results = mgr.dict()
        ctx = mp.get_context("spawn")
        procs = [ctx.Process(target=_world_worker, args=(r, world, os.path.join(d, "rdzv"), results, path, values, num_samples, batch))
                 for r in range(world)]
        for p in procs:
            p.start()
        for p in procs:
            p.join(timeout=180)
        for p in procs:
            assert p.exitcode == 0, f"worker exit code {p.exitcode}"
        res = dict(results)
    assert res[0] == expect and np.isnan(res[1])


# -- trainer setup guard ------------------------------------------------------------------------------------------------------

class _Scripted(torch.nn.Module):
    def forward(self, images: torch.Tensor) -> torch.Tensor:
        return images.flatten(1)


def _detector_dir(root, names):
    os.makedirs(root, exist_ok=True)
    for n in names:
        torch.jit.script(_Scripted()).save(os.path.join(root, n))
    return root


def _guard(detector, generator, metrics=("ppl_wend",)):
    from style_big_gan_amd.train_parts.trainers import trainers
    t = trainers["base"]()
    t.metrics, t.metric_detector = list(metrics), detector
    t._check_ppl_metrics(generator)


def test_trainer_refuses_ppl_without_vgg16_or_mapping(tmp_path):
    incep = _detector_dir(str(tmp_path / "incep"), ["inception-2015-12-05.pt"])
    both = _detector_dir(str(tmp_path / "both"), ["inception-2015-12-05.pt", "vgg16.pt"])
    with pytest.raises(ValueError, match="vgg16.pt"):                   # a single Inception file
        _guard(os.path.join(incep, "inception-2015-12-05.pt"), "sg2_classic")
    with pytest.raises(ValueError, match="vgg16.pt"):                   # a directory without vgg16.pt
        _guard(incep, "sg2_classic")
    for gen in ("big_gan", "cnn32_dcgan", "cnn48_dcgan"):               # no mapping / synthesis
        with pytest.raises(ValueError, match="mapping and synthesis"):
            _guard(both, gen)
    _guard(both, "sg2_classic")                                         # accepted
    _guard(os.path.join(both, "vgg16.pt"), "sg2_classic")
    _guard(incep, "big_gan", metrics=("fid50k_full",))                  # other metrics: the existing rules alone


def test_training_setup_refuses_ppl_metric(tmp_path):
    """through the trainer's real setup: log.metrics=[ppl_wend] with a directory lacking vgg16.pt, and with a generator that has no
    mapping network, are refused before anything trains"""
    if torch.cuda.is_available():
        pytest.skip("plumbing test is for the CPU container")
    import yaml
    from style_big_gan_amd import starter
    path = make_image_folder(str(tmp_path / "data"), n=8, res=32)
    incep = _detector_dir(str(tmp_path / "incep"), ["inception-2015-12-05.pt"])
    both = _detector_dir(str(tmp_path / "both"), ["inception-2015-12-05.pt", "vgg16.pt"])
    cfg = {"exp": {"trainer": "base"},
           "gen": {"kimg": 1, "batch": 8, "batch_gpu": 8, "loss_arch": "base", "loss": "bcew", "generator": "cnn32_dcgan", "discriminator": "cnn32_dcgan",
                   "g_reg_interval": 0, "d_reg_interval": 0},
           "gens_args": {"cnn32_dcgan": {"z_dim": 16}}, "ema": {"use_ema": False}, "aug": {"aug": "noaug"},
           "log": {"output": str(tmp_path / "logs"), "metrics": ["ppl_wend"]},
           "data": {"dataset": "image_folder", "dataset_path": path}, "dataloaders_args": {"basic": {"num_workers": 0}}}
    with open(tmp_path / "run.yaml", "w") as fh:
        yaml.safe_dump(cfg, fh)
    argv = ["exp.config_dir=" + str(tmp_path), "exp.config=run.yaml", "exp.name=m"]
    with pytest.raises(ValueError, match="vgg16.pt"):
        starter.main(argv + [f"log.metric_detector={incep}"], max_iterations=0)
    with pytest.raises(ValueError, match="mapping and synthesis"):
        starter.main(argv + [f"log.metric_detector={both}"], max_iterations=0)
