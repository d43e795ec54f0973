"""Average 2-D power spectra of a data set and of a generator: does the generator put energy where the data has none?

The tool of Karras et al., "Alias-Free Generative Adversarial Networks" (NeurIPS 2021, ``avg_spectra.py`` of their code; the reference has no
such tool), as one definition on both devices (``torch_utils/ops/spectrum.py``): every image-channel is normalised with
the mean and std of the REAL set's bytes, multiplied by a separable Kaiser window (beta 8, unit energy), zero-padded by ``--interp`` and
transformed in fp32 with a stated value graph; the power is averaged in float64 in image order.  ``--device=cpu`` and ``cuda`` write the
same bits.  Checkerboard energy shows at the Nyquist corner, aliasing and a skipped low-pass as excess in the outer band, blur as a deficit.

* The data set alone (no ``--snapshot``): ``spectrum_real.npz`` -- ``spectrum`` (float64 [S, S/2 + 1], the mean power P[ky, kx]; the other
  half is P[ky, kx] = P[(S - ky) % S, (S - kx) % S]), ``mean``, ``std``, ``image_size``, ``interp``, ``channels``, ``num_images``.
  Real images are items 0 .. N - 1 of the data set without mirroring, N = min(--num, len(data set)).
* With ``--snapshot``: also ``spectrum_gen.npz`` (generated image i is the bytes ``generate.py`` writes for seed i, i < N), ``spectrum.json``
  (radial profiles and the 0 / 45 degree slices of both sets in dB with their frequency in cycles per image, ``lsd_db``: the rms difference of
  the radial profiles, ``hf_excess_db``: their mean difference over the outer half band -- positive: excess fine-scale energy, negative:
  blur) and ``spectrum.png`` (both fft-shifted spectra side by side in grey: real left, generated right; ``--db-range=lo,hi``, by default
  the 80 dB below the ceiling of the largest value).
* ``--against=<spectrum_*.npz>`` takes the mean, the std and the "real" spectrum from a saved file and reads no data set: a data set's
  ``spectrum_real.npz`` computed once, or another snapshot's / another build's ``spectrum_gen.npz`` (the spectrum of the same seeds from two
  builds shows where a kernel change moved energy).  N is then ``--num``.  ``image_size``, ``interp`` and ``channels`` must match.

The numbers are comparable between runs of one resolution and one ``--interp`` only, and say nothing about semantics.

    python -m style_big_gan_amd.avg_spectra exp.config_dir=<dir> exp.config=<file.yaml> --outdir=<dir> [--snapshot=<network-snapshot-*.pt>] \\
        [--data=<folder|zip>] [--against=<spectrum_*.npz>] [--num=16384] [--interp=1|2|4] [--trunc=1] [--class=<idx>] \\
        [--noise-mode=const|random|none] [--device=auto|cuda|cpu] [--batch=64] [--db-range=lo,hi]
"""
import argparse
import contextlib
import json
import os

import numpy as np
import torch

from .tool_support import (SNAPSHOT_HELP, add_device_option, add_sampling_options, add_snapshot_option, class_label, config_overrides, device_of,
                           generated_images, load_generator, open_dataset, require_file, save_png, tool_device)
from .torch_utils.ops import resident_set, spectrum

NPZ_KEYS = ('spectrum', 'mean', 'std', 'image_size', 'interp', 'channels', 'num_images')
DEFAULT_NUM = 16384
DB_SPAN = 80.0


def byte_moments(batches):
    """uint8 batches -> (sum, sum of squares, count) of all their values as Python integers (exact: int64 sums per batch)"""
    total = total_sq = count = 0
    for b in batches:
        if b.numel() * 255 * 255 >= 1 << 63:
            raise OverflowError(f'a batch of {b.numel()} byte values: its sum of squares does not fit the int64 range it is gathered in')
        total += int(b.sum(dtype=torch.int64))
        total_sq += int(b.to(torch.int32).square().sum(dtype=torch.int64))
        count += b.numel()
    return total, total_sq, count


def mean_spectrum(batches, R, interp, mean, std, device):
    """uint8 batches [B, C, R, R] on `device` -> (float64 ndarray [S, S/2 + 1], image-channels seen)"""
    S = R * interp
    window, twiddle = (v.to(device) for v in spectrum.tables(R, S))
    s, t = spectrum.scale_shift(mean, std)
    acc = torch.zeros([S // 2 + 1, S], dtype=torch.float64, device=device)
    count = 0
    for b in batches:
        spectrum.accumulate(acc, b, s, t, window, twiddle)
        count += b.shape[0] * b.shape[1]
    return spectrum.half_spectrum(acc, count), count


def save_npz(path, half, mean, std, image_size, interp, channels, num_images):
    np.savez(path, spectrum=half, mean=np.float64(mean), std=np.float64(std), image_size=np.int64(image_size), interp=np.int64(interp),
             channels=np.int64(channels), num_images=np.int64(num_images))


def load_against(path, image_size, interp, channels):
    """a saved spectrum_*.npz -> dict of its fields; refused by name when it does not describe `image_size`, `interp`, `channels`"""
    with np.load(path) as f:
        missing = [k for k in NPZ_KEYS if k not in f.files]
        if missing:
            raise ValueError(f'--against={path}: not a spectrum file, it lacks {", ".join(missing)}')
        got = {k: f[k] for k in NPZ_KEYS}
    for name, want in (('image_size', image_size), ('interp', interp), ('channels', channels)):
        if want is not None and int(got[name]) != int(want):
            raise ValueError(f'--against={path}: its {name} is {int(got[name])}, this run has {name}={int(want)}')
    S = int(got['image_size']) * int(got['interp'])
    if got['spectrum'].dtype != np.float64 or got['spectrum'].shape != (S, S // 2 + 1):
        raise ValueError(f'--against={path}: its spectrum is {got["spectrum"].dtype} {got["spectrum"].shape}, expected float64 {(S, S // 2 + 1)}')
    return dict(spectrum=got['spectrum'], mean=float(got['mean']), std=float(got['std']), image_size=int(got['image_size']),
                interp=int(got['interp']), channels=int(got['channels']), num_images=int(got['num_images']))


def db_bytes(db, lo, hi):
    """g = clamp((dB - lo) / (hi - lo), 0, 1) -> uint8 floor(255 g + 0.5)"""
    g = np.clip((db - lo) / (hi - lo), 0.0, 1.0)
    return np.floor(255.0 * g + 0.5).astype(np.uint8)


def heatmaps(real_full, gen_full, db_range=None):
    """the two fft-shifted spectra side by side -> (uint8 [S, 2 S, 1], (lo, hi))"""
    real_db, gen_db = spectrum.to_db(real_full), spectrum.to_db(gen_full)
    if db_range is None:
        hi = float(np.ceil(max(real_db.max(), gen_db.max())))
        db_range = (hi - DB_SPAN, hi)
    lo, hi = float(db_range[0]), float(db_range[1])
    if not hi > lo:
        raise ValueError(f'--db-range={lo},{hi}: hi must be above lo')
    canvas = np.concatenate([db_bytes(np.fft.fftshift(real_db), lo, hi), db_bytes(np.fft.fftshift(gen_db), lo, hi)], axis=1)
    return canvas[:, :, None], (lo, hi)


def profiles(full):
    """the radial profile and both slices of one spectrum in dB"""
    s0, s45 = spectrum.slices(full)
    return dict(radial_db=spectrum.to_db(spectrum.radial_profile(full)).tolist(), slice_0_db=spectrum.to_db(s0).tolist(),
                slice_45_db=spectrum.to_db(s45).tolist())


@torch.no_grad()
def average_spectra(G=None, dataset=None, against=None, num=DEFAULT_NUM, interp=1, truncation_psi=1, noise_mode='const', class_idx=None, batch=64,
                    outdir=None, device=None, max_gib=None, db_range=None):
    """The mean power spectrum of `dataset` (a train_parts.datasets.Dataset; items 0 .. N - 1 without their mirrored copies) or of the
    file `against`, and of G's images of seeds 0 .. N - 1 when G is given.  -> dict with `real` / `gen` (float64 [S, S/2 + 1]), `mean`,
    `std`, and with G `stats` (what spectrum.json holds) and `canvas`.  With `outdir` the files of the module docstring are written."""
    from .train_parts.dataloaders import ResidentDataloader
    num, interp, batch = int(num), int(interp), int(batch)
    if num < 1:
        raise ValueError(f'--num={num}: must be at least 1')
    if batch < 1:
        raise ValueError(f'--batch={batch}: must be at least 1')
    if interp not in spectrum.PADS:
        raise ValueError(f'--interp={interp}: the padding factor must be one of {spectrum.PADS}')
    if dataset is None and against is None:
        raise ValueError('one of a data set and --against is required')
    if against is not None and G is None:
        raise ValueError('--against replaces the data set pass: it needs --snapshot, there is nothing else to compute')
    device = device_of(G, 'cpu' if device is None and G is None else device)
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)

    if G is not None:
        R, C = int(G.img_resolution), int(getattr(G, 'img_channels', 3))
    if against is None:
        Cd, H, W = dataset.image_shape
        if H != W:
            raise ValueError(f'the data set holds {Cd} x {H} x {W} images: square images only')
        if G is not None and (R, R, C) != (H, W, Cd):
            raise ValueError(f'the generator makes {C} x {R} x {R} images, the data set holds {Cd} x {H} x {W}')
        R, C = int(H), int(Cd)
    spectrum.check_sizes(R, R * interp, f'{C} x {R} x {R} images with --interp={interp}')
    result = dict(image_size=R, interp=interp, channels=C)

    if against is None:
        store = ResidentDataloader(dataset, sampler=(), batch_size=1, device=device, max_gib=max_gib).store
        _, slot, flip = resident_set.tables(dataset)
        rows = slot[flip == 0][:num].to(torch.int64).to(device)            # items in order, flips off
        N = int(rows.numel())

        def real_batches():
            for lo in range(0, N, batch):
                yield store.index_select(0, rows[lo:lo + batch])

        mean, std = spectrum.normalisation(*byte_moments(real_batches()))
        real, _ = mean_spectrum(real_batches(), R, interp, mean, std, device)
        num_real = N
        if outdir is not None:
            save_npz(os.path.join(outdir, 'spectrum_real.npz'), real, mean, std, R, interp, C, N)
    else:
        saved = load_against(against, R, interp, C)
        real, mean, std, num_real, N = saved['spectrum'], saved['mean'], saved['std'], saved['num_images'], num
    result.update(real=real, mean=mean, std=std, num_real=num_real)
    if G is None:
        return result

    label = class_label(G, class_idx, device)

    def gen_batches():
        for lo in range(0, N, batch):
            yield generated_images(G, list(range(lo, min(lo + batch, N))), label, truncation_psi, noise_mode, device)

    gen, _ = mean_spectrum(gen_batches(), R, interp, mean, std, device)
    real_full, gen_full = spectrum.full_from_half(real), spectrum.full_from_half(gen)
    canvas, (lo, hi) = heatmaps(real_full, gen_full, db_range)
    S = R * interp
    k = np.arange(S // 2 + 1, dtype=np.float64)
    stats = dict(image_size=R, interp=interp, channels=C, num_real=num_real, num_gen=N, mean=mean, std=std, **spectrum.compare(real_full, gen_full),
                 frequency=(k / interp).tolist(), frequency_45=(k * np.sqrt(2.0) / interp).tolist(), real=profiles(real_full),
                 gen=profiles(gen_full),
                 options=dict(num=num, interp=interp, trunc=truncation_psi, class_idx=class_idx, noise_mode=noise_mode, batch=batch, db_range=[lo, hi]))
    result.update(gen=gen, num_gen=N, stats=stats, canvas=canvas)
    if outdir is not None:
        save_npz(os.path.join(outdir, 'spectrum_gen.npz'), gen, mean, std, R, interp, C, N)
        with open(os.path.join(outdir, 'spectrum.json'), 'w') as f:
            json.dump(stats, f, indent=2)
        save_png(canvas, os.path.join(outdir, 'spectrum.png'))
    return result


# ---------------------------------------------------------------------------------------------------------------- CLI

def db_pair(s):
    parts = s.split(',')
    if len(parts) != 2:
        raise argparse.ArgumentTypeError(f'expected lo,hi, got {s!r}')
    lo, hi = float(parts[0]), float(parts[1])
    if not hi > lo:
        raise argparse.ArgumentTypeError(f'hi must be above lo, got {s!r}')
    return lo, hi


def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.avg_spectra', description=__doc__.split('\n')[0])
    ap.add_argument('--outdir', required=True, help='where to save spectrum_real.npz / spectrum_gen.npz / spectrum.json / spectrum.png')
    add_snapshot_option(ap, required=False, help=SNAPSHOT_HELP + '; without it only the data set is measured')
    ap.add_argument('--data', help='data set to measure, folder or zip (default: the run\'s data.dataset_path)')
    ap.add_argument('--against', help='a saved spectrum_*.npz that stands in for the data set (mean, std and the "real" spectrum)')
    ap.add_argument('--num', type=int, default=DEFAULT_NUM, help=f'images per set: min(N, the data set\'s size) (default: {DEFAULT_NUM})')
    ap.add_argument('--interp', type=int, choices=spectrum.PADS, default=1, help='zero-padding factor of the transform (default: 1)')
    add_sampling_options(ap)
    add_device_option(ap)
    ap.add_argument('--batch', type=int, default=64, help='images measured at a time (default: 64)')
    ap.add_argument('--db-range', type=db_pair, help='lo,hi of the grey scale of spectrum.png in dB (default: the 80 dB below the largest value)')
    args, rest = ap.parse_known_args(argv)
    if args.num < 1:
        ap.error('--num must be at least 1')
    if args.batch < 1:
        ap.error('--batch must be at least 1')
    require_file(ap, '--snapshot', args.snapshot)
    require_file(ap, '--against', args.against)
    if args.against is not None and args.snapshot is None:
        ap.error('--against replaces the data set pass: it needs --snapshot')
    if args.against is not None and args.data is not None:
        ap.error('--against and --data exclude each other: the file stands in for the data set')
    return config_overrides(ap, rest), args


def run_avg_spectra(argv=None):
    overrides, args = parse_args(argv)
    from . import arguments
    from .train_parts.trainers import training_set_kwargs_from_config
    config = arguments.load_config(overrides)
    device = tool_device(args.device)
    G = load_generator(config, args.snapshot, device) if args.snapshot is not None else None
    kw = training_set_kwargs_from_config(config, seed=config.gen.seed, path=args.data, mirror=False, use_labels=False) if args.against is None else None
    with open_dataset(config, kw) if kw is not None else contextlib.nullcontext() as dataset:         # --against: no data set
        result = average_spectra(G, dataset, against=args.against, num=args.num, interp=args.interp, truncation_psi=args.truncation_psi,
                                 noise_mode=args.noise_mode, class_idx=args.class_idx, batch=args.batch, outdir=args.outdir, device=device,
                                 db_range=args.db_range)
    if 'stats' in result:
        print(json.dumps({k: result['stats'][k] for k in ('lsd_db', 'hf_excess_db', 'num_real', 'num_gen', 'image_size', 'interp')}))
    return result


if __name__ == '__main__':
    run_avg_spectra()
