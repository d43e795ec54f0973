"""Generate images from a trained generator.

Counterpart of the reference's ``stylegan2ada/generate.py`` (``generate_images`` :46-121): same options, same file names
(``seed%04d.png`` / ``proj%02d.png``), same latents (``np.random.RandomState(seed).randn(1, z_dim)``), same failures and warnings.
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
import re

import numpy as np
import torch

from .snapshot_io import build_generator, config_overrides, snapshot_generator_state
from .torch_utils.ops import image_export

NOISE_MODES = ('const', 'random', 'none')


def num_range(s):
    """a comma separated list of numbers 'a,b,c' or a range 'a-c' -> list of ints (the reference's option type, :25-33)"""
    m = re.match(r'^(\d+)-(\d+)$', s)
    if m:
        return list(range(int(m.group(1)), int(m.group(2)) + 1))
    return [int(x) for x in s.split(',')]


def save_rgb(img, path):
    """uint8 [H, W, 3] -> PNG, the way the reference's tools write every image (`PIL.Image.fromarray(img, 'RGB').save`)"""
    import PIL.Image
    PIL.Image.fromarray(np.ascontiguousarray(img), 'RGB').save(path)


def to_uint8(img):
    """synthesis output [N, C, H, W] -> uint8 [N, H, W, C] on the host (:98, :120)"""
    return image_export.quantize(img.to(torch.float32), 'clamp').cpu().numpy()


@torch.no_grad()
def generate_images(G, seeds=None, truncation_psi=1, noise_mode='const', class_idx=None, projected_w=None, outdir=None, device=None):
    """-> uint8 images [N, H, W, 3], one per seed (or per projected w), written to `outdir` when it is given"""
    device = torch.device(device) if device is not None else next(iter(G.buffers())).device
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
                save_rgb(images[-1], f'{outdir}/proj{idx:02d}.png')
        return np.stack(images)

    if seeds is None:
        raise ValueError('--seeds option is required when not using --projected-w')

    # Labels.
    label = torch.zeros([1, G.c_dim], device=device)
    if G.c_dim != 0:
        if class_idx is None:
            raise ValueError('Must specify class label with --class when using a conditional network')
        label[:, class_idx] = 1
    elif class_idx is not None:
        print('warn: --class=lbl ignored when running on an unconditional network')

    # Generate images.
    images = []
    for seed_idx, seed in enumerate(seeds):
        print('Generating image for seed %d (%d/%d) ...' % (seed, seed_idx, len(seeds)))
        z = torch.from_numpy(np.random.RandomState(seed).randn(1, G.z_dim)).to(device)
        images.append(to_uint8(G(z, label, truncation_psi=truncation_psi, noise_mode=noise_mode))[0])
        if outdir is not None:
            save_rgb(images[-1], f'{outdir}/seed{seed:04d}.png')
    return np.stack(images) if images else np.zeros([0, G.img_resolution, G.img_resolution, 3], dtype=np.uint8)


# ---------------------------------------------------------------------------------------------------------------- CLI

def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.generate', description=__doc__.split('\n')[0])
    ap.add_argument('--snapshot', required=True, help='network-snapshot-*.pt of this build (G_ema, or G when there is no EMA)')
    ap.add_argument('--seeds', type=num_range, help='list of random seeds')
    ap.add_argument('--trunc', dest='truncation_psi', type=float, default=1, help='truncation psi (default: 1)')
    ap.add_argument('--class', dest='class_idx', type=int, help='class label (unconditional if not specified)')
    ap.add_argument('--noise-mode', choices=NOISE_MODES, default='const', help='noise mode (default: const)')
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
    print(f'Loading networks from "{args.snapshot}"...')
    device = torch.device('cuda')
    G = build_generator(config, snapshot_generator_state(args.snapshot), device)
    return generate_images(G, seeds=args.seeds, truncation_psi=args.truncation_psi, noise_mode=args.noise_mode, class_idx=args.class_idx,
                           projected_w=args.projected_w, outdir=args.outdir, device=device)


if __name__ == '__main__':
    run_generate()
