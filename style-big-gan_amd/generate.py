"""Generate images from a trained generator.

Counterpart of the reference's ``stylegan2ada/generate.py`` (``generate_images`` :46-121): same options, same file names
(``seed%04d.png`` / ``proj%02d.png``), same latents (one ``RandomState`` per seed, ``tool_support.seed_latents``), same failures and warnings.
Differences:
* the float -> uint8 step (``(img.permute(0, 2, 3, 1) * 127.5 + 128).clamp(0, 255).to(torch.uint8)``, :98,120) is one HIP kernel
  (torch_utils/ops/image_export.py, the ``clamp`` rule) instead of five tensor ops; CPU tensors take the reference's expression;
* ``generate_images`` is a function of a generator, returns the uint8 images as well as writing them (``outdir=None`` writes nothing),
  and takes ``projected_w`` as a file name or an array;
* the CLI builds G from the run's config (the ``key=value`` list ``starter`` takes) and loads a ``network-snapshot-*.pt`` of this build.

    python -m style_big_gan_amd.generate exp.config_dir=<dir> exp.config=<file.yaml> --snapshot=<network-snapshot-*.pt> --outdir=<dir> \\
        [--seeds=a,b,c | a-c] [--trunc=1] [--class=<idx>] [--noise-mode=const|random|none] [--projected-w=<projected_w.npz>]
"""
import argparse
import os

import numpy as np
import torch

from .tool_support import (add_sampling_options, add_snapshot_option, class_label, config_overrides, device_of, load_generator, num_range, save_png,
                           seed_latents, to_uint8)


@torch.no_grad()
def generate_images(G, seeds=None, truncation_psi=1, noise_mode='const', class_idx=None, projected_w=None, outdir=None, device=None):
    """-> uint8 images [N, H, W, 3], one per seed (or per projected w), written to `outdir` when it is given"""
    device = device_of(G, device)
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)

    # Synthesize the result of a W projection.
    if projected_w is not None:
        if seeds is not None:
            print('warn: --seeds is ignored when using --projected-w')
        if isinstance(projected_w, (str, os.PathLike)):
            print(f'Generating images from projected W "{projected_w}"')
            projected_w = np.load(projected_w)['w']
        ws = torch.as_tensor(projected_w).to(device)
        assert ws.shape[1:] == (G.num_ws, G.w_dim)
        images = []
        for idx, w in enumerate(ws):
            images.append(to_uint8(G.synthesis(w.unsqueeze(0), noise_mode=noise_mode))[0])
            if outdir is not None:
                save_png(images[-1], f'{outdir}/proj{idx:02d}.png')
        return np.stack(images)

    if seeds is None:
        raise ValueError('--seeds option is required when not using --projected-w')

    # Generate images.
    label = class_label(G, class_idx, device)
    images = []
    for seed_idx, seed in enumerate(seeds):
        print('Generating image for seed %d (%d/%d) ...' % (seed, seed_idx, len(seeds)))
        z = torch.from_numpy(seed_latents(G, [seed])).to(device)
        images.append(to_uint8(G(z, label, truncation_psi=truncation_psi, noise_mode=noise_mode))[0])
        if outdir is not None:
            save_png(images[-1], f'{outdir}/seed{seed:04d}.png')
    return np.stack(images) if images else np.zeros([0, G.img_resolution, G.img_resolution, 3], dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- CLI

def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.generate', description=__doc__.split('\n')[0])
    add_snapshot_option(ap)
    ap.add_argument('--seeds', type=num_range, help='list of random seeds')
    add_sampling_options(ap)
    ap.add_argument('--projected-w', help='projection result file (projected_w.npz of the projector)')
    ap.add_argument('--outdir', required=True, help='where to save the output images')
    args, rest = ap.parse_known_args(argv)
    if args.seeds is None and args.projected_w is None:
        ap.error('--seeds option is required when not using --projected-w')
    return config_overrides(ap, rest), args


def run_generate(argv=None):
    overrides, args = parse_args(argv)
    from . import arguments
    config = arguments.load_config(overrides)
    device = torch.device('cuda')
    G = load_generator(config, args.snapshot, device)
    return generate_images(G, seeds=args.seeds, truncation_psi=args.truncation_psi, noise_mode=args.noise_mode, class_idx=args.class_idx,
                           projected_w=args.projected_w, outdir=args.outdir, device=device)


if __name__ == '__main__':
    run_generate()
