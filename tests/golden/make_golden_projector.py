"""Generate tests/golden/projector.npz by running the REFERENCE's latent projector on CPU.

Run in the dev container only (the reference checkout does not travel to the GPU box):

    PYTHONPATH=/root/reference python tests/golden/make_golden_projector.py

The reference's own ``project()`` (stylegan2ada/projector.py:25-131) runs seeded, small ``Generator``s of
``stylegan2ada.training.networks`` (fp32: num_fp16_res=0) with the PPL fixture's stand-in LPIPS network
(``make_golden_ppl.StandInLPIPS``); the vgg16 URL is never opened: ``dnnlib.util.open_url`` and ``torch.jit.load`` are replaced for
the call, before anything could fetch it.  The module imports ``imageio`` for its video output, which is not needed here: an empty
stand-in module takes its place.  Every ``torch.randn_like`` of the call is recorded, in call order: one per noise buffer (the
initial noise), then one per step (the w noise).

Cases (small w_avg_samples and step counts; the schedules still run over their whole [0, 1) range):
  g32:  32x32, 10 steps, every draw stored, the final noise buffers stored
  g16:  16x16, 10 steps, every draw stored, the final noise buffers stored
  g512: 512x512 with tiny channels, 2 steps -- the target and the synthesis go through the area downsampling to 256x256.  Its
        noise draws would not fit a fixture: their seed and per-buffer sums are stored and the test regenerates them (the CPU
        generator is deterministic); the w draws are stored.  Its target is regenerated from the case's seed too.
Stored per case: the weights (noise buffers left out), the target [3, R, R] uint8 (np.random.RandomState(seed).randint(0, 256)) and
its sum, the draws, w_out [num_steps, num_ws, w_dim].
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import R_net, dnnlib, _import_train_parts, npy, save    # noqa: E402
from make_golden_ppl import RecordRNG, StandInLPIPS                       # noqa: E402

W_AVG_SAMPLES = 64
CASES = [("g32", 720, 32, 256, 16, 10), ("g16", 721, 16, 256, 16, 10), ("g512", 722, 512, 512, 4, 2)]


def make_G(seed, res, cbase, cmax):
    torch.manual_seed(seed)
    G = R_net.Generator(z_dim=16, c_dim=0, w_dim=16, img_resolution=res, img_channels=3, mapping_kwargs=dnnlib.EasyDict(num_layers=2),
                        synthesis_kwargs=dnnlib.EasyDict(channel_base=cbase, channel_max=cmax, num_fp16_res=0, conv_clamp=256))
    with torch.no_grad():       # non-trivial noise strengths and biases so every noise buffer reaches the images
        for name, p in G.named_parameters():
            if name.endswith("noise_strength"):
                p.fill_(0.3)
            if name.endswith(".bias") and "affine" not in name and "mapping" not in name:
                p.copy_(torch.randn_like(p) * 0.1)
    return G.eval().requires_grad_(False)


@contextlib.contextmanager
def capture_optimizer_params(out):
    """torch.optim.Adam records its parameter list ([w_opt] + the noise buffers, :76) into `out`"""
    saved = torch.optim.Adam

    class Adam(saved):
        def __init__(self, params, *a, **k):
            params = list(params)
            out.extend(params)
            super().__init__(params, *a, **k)

    torch.optim.Adam = Adam
    try:
        yield
    finally:
        torch.optim.Adam = saved


@contextlib.contextmanager
def no_fetch(detector):
    """the reference's vgg16 load (:63-65) returns `detector`; nothing is opened"""
    import stylegan2ada.dnnlib.util as du
    saved = du.open_url, torch.jit.load
    du.open_url = lambda *a, **k: contextlib.nullcontext(None)
    torch.jit.load = lambda *a, **k: detector
    try:
        yield
    finally:
        du.open_url, torch.jit.load = saved


def main():
    _import_train_parts()
    sys.modules.setdefault("imageio", types.ModuleType("imageio"))
    from stylegan2ada import projector as R_proj

    lpips = StandInLPIPS().eval()
    arrays = {f"lpips/{k}": npy(v) for k, v in lpips.state_dict().items()}
    meta_cases = []
    for tag, seed, res, cbase, cmax, steps in CASES:
        G = make_G(seed, res, cbase, cmax)
        names = [n for n, _ in G.synthesis.named_buffers() if "noise_const" in n]
        arrays.update({f"{tag}/G/{k}": npy(v) for k, v in G.state_dict().items() if not k.endswith(".noise_const")})
        rng = np.random.RandomState(seed)
        target = rng.randint(0, 256, [3, res, res]).astype(np.uint8)
        if res <= 32:
            arrays[f"{tag}/target"] = target
        arrays[f"{tag}/target_sum"] = np.asarray(int(target.astype(np.int64).sum()))
        draw_seed = 9100 + seed
        torch.manual_seed(draw_seed)
        params = []
        with no_fetch(lpips), capture_optimizer_params(params), RecordRNG() as rec:
            w_out = R_proj.project(G, torch.from_numpy(target), num_steps=steps, w_avg_samples=W_AVG_SAMPLES, device=torch.device("cpu"))
        kinds = [k for k, _ in rec.calls]
        assert kinds == ["randn_like"] * (len(names) + steps), kinds
        noise = [v for _, v in rec.calls[:len(names)]]
        w_noise = torch.stack([v.reshape(1, -1) for _, v in rec.calls[len(names):]])        # [steps, 1, w_dim]
        arrays[f"{tag}/w_noise"] = npy(w_noise)
        arrays[f"{tag}/noise_sums"] = np.asarray([float(v.double().sum()) for v in noise])
        arrays[f"{tag}/w_out"] = npy(w_out)
        if res <= 32:
            for n, v, final in zip(names, noise, params[1:]):
                arrays[f"{tag}/noise/{n}"] = npy(v)
                arrays[f"{tag}/final_noise/{n}"] = npy(final)
        meta_cases.append(dict(tag=tag, res=res, channel_base=cbase, channel_max=cmax, num_steps=steps, draw_seed=draw_seed,
                               noise_names=names, num_ws=int(G.mapping.num_ws)))
    save("projector", arrays, dict(cases=meta_cases, w_avg_samples=W_AVG_SAMPLES, z_dim=16, w_dim=16, mapping_layers=2,
                                   synthesis=dict(num_fp16_res=0, conv_clamp=256)))


if __name__ == "__main__":
    main()
