"""Generate a style mixing image matrix from a trained generator.

Counterpart of the reference's ``stylegan2ada/style_mixing.py`` (``generate_style_mix`` :45-110): same options, the same image
dictionary (keys ``(row_seed, col_seed)``, ``(seed, seed)`` for the unmixed images), the same files (``<row>-<col>.png`` and
``grid.png`` with its black top-left cell).  Differences:
* the truncated latent of every seed and the mixed latent of every (row, column) pair come from one HIP kernel
  (``image_export.truncate_mix``: ``w_avg + (w - w_avg) * psi`` in the reference's order, then the per-layer selection), and the
  matrix is synthesised in batches of ``batch`` instead of one call per cell -- the samples of a batch are independent at
  ``noise_mode='const'``; ``batch=1`` is the reference's one-by-one form;
* the float -> uint8 step is the ``clamp`` rule kernel (see generate.py);
* ``generate_style_mix`` is a function of a generator and returns the image dictionary (``outdir=None`` writes nothing); the CLI
  builds G from the run's config and a ``network-snapshot-*.pt`` of this build.

    python -m style_big_gan_amd.style_mixing exp.config_dir=<dir> exp.config=<file.yaml> --snapshot=<network-snapshot-*.pt> --outdir=<dir> \\
        --rows=85,100,75 --cols=55,821,1789 [--styles=0-6] [--trunc=1] [--noise-mode=const|random|none]
"""
import argparse
import os

import numpy as np
import torch

from .tool_support import (add_sampling_options, add_snapshot_option, config_overrides, device_of, load_generator, num_range, save_png, seed_latents,
                           to_uint8)
from .torch_utils.ops import image_export


def grid_canvas(image_dict, row_seeds, col_seeds, resolution):
    """the reference's grid (:97-109) -> uint8 [(R + 1) * H, (Cn + 1) * W, 3]: the top row holds the column seeds' own images, the left
    column the row seeds', the top-left cell stays black"""
    H = W = resolution
    canvas = np.zeros([H * (len(row_seeds) + 1), W * (len(col_seeds) + 1), 3], dtype=np.uint8)
    for row_idx, row_seed in enumerate([0] + list(row_seeds)):
        for col_idx, col_seed in enumerate([0] + list(col_seeds)):
            if row_idx == 0 and col_idx == 0:
                continue
            key = (row_seed, col_seed)
            if row_idx == 0:
                key = (col_seed, col_seed)
            if col_idx == 0:
                key = (row_seed, row_seed)
            canvas[H * row_idx: H * (row_idx + 1), W * col_idx: W * (col_idx + 1)] = image_dict[key]
    return canvas


@torch.no_grad()
def generate_style_mix(G, row_seeds, col_seeds, col_styles=range(0, 7), truncation_psi=1, noise_mode='const', outdir=None, device=None, batch=16):
    """-> {(row_seed, col_seed): uint8 [H, W, 3]} in the reference's order: the unmixed images first, then the matrix row by row"""
    device = device_of(G, device)
    row_seeds, col_seeds, col_styles = list(row_seeds), list(col_seeds), list(col_styles)
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)

    print('Generating W vectors...')
    # The reference's `list(set(row_seeds + col_seeds))`: the order is whatever Python's set iteration gives.  It decides the batch order
    # of the mapping and synthesis calls and the order of the (seed, seed) keys only, never a result; it is reproduced as Python gives it.
    all_seeds = list(set(row_seeds + col_seeds))
    all_w = G.mapping(torch.from_numpy(seed_latents(G, all_seeds)).to(device), None).to(torch.float32)
    w_avg = G.mapping.w_avg
    where = {seed: i for i, seed in enumerate(all_seeds)}
    S = len(all_seeds)
    table = torch.cat([image_export.truncate_mix(all_w, w_avg, truncation_psi, range(S), [0], []),
                       image_export.truncate_mix(all_w, w_avg, truncation_psi, [where[s] for s in row_seeds], [where[s] for s in col_seeds], col_styles)])

    print('Generating images...')
    images = np.concatenate([to_uint8(G.synthesis(ws, noise_mode=noise_mode)) for ws in table.split(max(int(batch), 1))])
    image_dict = {(seed, seed): image for seed, image in zip(all_seeds, list(images[:S]))}
    for i, (row_seed, col_seed) in enumerate((r, c) for r in row_seeds for c in col_seeds):
        image_dict[(row_seed, col_seed)] = images[S + i]

    if outdir is not None:
        print('Saving images...')
        for (row_seed, col_seed), image in image_dict.items():
            save_png(image, f'{outdir}/{row_seed}-{col_seed}.png')
        print('Saving image grid...')
        save_png(grid_canvas(image_dict, row_seeds, col_seeds, G.img_resolution), f'{outdir}/grid.png')
    return image_dict


# ---------------------------------------------------------------------------------------------------------------- CLI

def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.style_mixing', description=__doc__.split('\n')[0])
    add_snapshot_option(ap)
    ap.add_argument('--rows', dest='row_seeds', type=num_range, required=True, help='random seeds to use for image rows')
    ap.add_argument('--cols', dest='col_seeds', type=num_range, required=True, help='random seeds to use for image columns')
    ap.add_argument('--styles', dest='col_styles', type=num_range, default=num_range('0-6'), help='style layer range (default: 0-6)')
    add_sampling_options(ap, class_idx=False)
    ap.add_argument('--outdir', required=True, help='where to save the output images')
    args, rest = ap.parse_known_args(argv)
    return config_overrides(ap, rest), args


def run_style_mix(argv=None):
    overrides, args = parse_args(argv)
    from . import arguments
    config = arguments.load_config(overrides)
    device = torch.device('cuda')
    G = load_generator(config, args.snapshot, device)
    return generate_style_mix(G, row_seeds=args.row_seeds, col_seeds=args.col_seeds, col_styles=args.col_styles, truncation_psi=args.truncation_psi,
                              noise_mode=args.noise_mode, outdir=args.outdir, device=device)


if __name__ == '__main__':
    run_style_mix()
