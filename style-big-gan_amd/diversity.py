"""Pairwise MS-SSIM of generated images and of a data set: has the generator collapsed, without any detector file?

The detector-free diversity figure that Karras et al. ("Progressive Growing of GANs", ICLR 2018) report next to the sliced Wasserstein distance
and Odena et al. ("Conditional Image Synthesis with Auxiliary Classifier GANs", ICML 2017) report per class against the training set: the
multi-scale structural similarity (Wang, Simoncelli, Bovik 2003) between random pairs of images.  Pairs that are more alike than pairs of real
images of the same class mean lost modes.  The reference has no such tool.  One definition on both devices (``torch_utils/ops/msssim.py``,
DESIGN section 23): ``--device=cpu`` and ``cuda`` write the same numbers.

* Generated pairs (``--snapshot``): pair p is the bytes ``generate.py`` writes for the seeds 2p and 2p + 1.  On a conditional network
  ``--class=i`` puts every pair in class i; without it pair p has class p mod c_dim.
* Real pairs (``--data``): mirrored copies are off; the items are walked in the order ``RandomState(--seed).permutation(len(data set))``.
  Without labels consecutive items form the pairs; with class labels an item pairs with the pending item of its class, or becomes the pending
  one.  The walk stops at ``--pairs`` pairs or at its end.  ``--seed`` changes the real pairs only.
* ``diversity.json``: per set (``gen``, ``real``) ``msssim`` (the mean of the pair scores, added left to right), ``msssim_std`` (population),
  the quantiles ``p01 p10 p50 p90 p99``, ``levels`` (the mean term per level side: cs, and ssim on the coarsest), ``num_pairs``, with several
  classes ``per_class``; with both sets ``fraction_above_real_p99``: the share of generated pairs that score at or above the 99 % quantile of
  the real pairs -- the collapse flag (a pair of identical images always counts).
* ``diversity_pairs.npz``: per set the pair scores (``*_scores``), the per-level terms (``*_terms`` [pairs, channels, levels]), the classes
  (``*_classes``, -1 without) and ``gen_seeds`` / ``real_items`` [pairs, 2].
* ``closest_pairs.png`` (with ``--snapshot`` and ``--closest`` > 0): the ``--closest`` most similar generated pairs, one pair per row, ties to the
  lower pair index; ``diversity.json`` lists their pair indices as ``closest_pairs``.

The score is comparable between runs of one resolution only (the number of levels follows the resolution), and it measures pixel structure,
not semantics.

    python -m style_big_gan_amd.diversity exp.config_dir=<dir> exp.config=<file.yaml> --outdir=<dir> [--snapshot=<network-snapshot-*.pt>] \\
        [--data=<folder|zip>] [--pairs=10000] [--seed=0] [--trunc=1] [--class=<idx>] [--noise-mode=const|random|none] \\
        [--device=auto|cuda|cpu] [--batch=64] [--closest=8]
"""
import argparse
import contextlib
import json
import os

import numpy as np
import torch

from .tool_support import (SNAPSHOT_HELP, add_device_option, add_sampling_options, add_snapshot_option, class_label, config_overrides,
                           dataset_kwargs_for, device_of, generated_images, load_generator, open_dataset, require_file, save_png, tool_device)
from .torch_utils.ops import msssim

DEFAULT_PAIRS = 10000
QUANTILES = (0.01, 0.10, 0.50, 0.90, 0.99)


def mean_left_to_right(values):
    """the float64 mean of a 1-d array, its values added in order"""
    acc = np.float64(0.0)
    for v in np.asarray(values, dtype=np.float64):
        acc = acc + v
    return float(acc / np.float64(len(values)))


def generated_classes(G, class_idx, pairs):
    """-> int64 [pairs]: --class for every pair, else p mod c_dim; -1 on an unconditional network"""
    if G.c_dim == 0:
        return np.full([pairs], -1, dtype=np.int64)
    if class_idx is None:
        return np.arange(pairs, dtype=np.int64) % G.c_dim
    if not 0 <= class_idx < G.c_dim:
        raise ValueError(f'--class={class_idx}: the network has the classes 0..{G.c_dim - 1}')
    return np.full([pairs], class_idx, dtype=np.int64)


def item_classes(dataset):
    """-> int64 [len(dataset)]: the class index of every item, or None when the data set has no class labels"""
    if not dataset.has_labels or not dataset.has_onehot_labels:
        return None
    return np.array([int(dataset.get_details(i).raw_label) for i in range(len(dataset))], dtype=np.int64)


def real_pairs(num_items, classes, pairs, seed):
    """the walk over RandomState(seed).permutation(num_items) -> (items int64 [P, 2], classes int64 [P]), P <= pairs"""
    order = np.random.RandomState(seed).permutation(num_items)
    items, cls = [], []
    pending = {}
    for i in order:
        if len(items) >= pairs:
            break
        k = -1 if classes is None else int(classes[i])
        if k in pending:
            items.append((pending.pop(k), int(i)))
            cls.append(k)
        else:
            pending[k] = int(i)
    return np.array(items, dtype=np.int64).reshape(-1, 2), np.array(cls, dtype=np.int64)


def closest_order(scores, k):
    """the indices of the k largest scores, descending, ties to the lower index"""
    return np.argsort(-np.asarray(scores, dtype=np.float64), kind='stable')[:k]


def score_pairs(batches, closest=0):
    """`batches` yields (x, y) uint8 [B, C, S, S] -> (scores float64 [P], terms float64 [P, C, L], the `closest` most similar pairs as
    (pair indices, uint8 [k, 2, C, S, S]))"""
    scores, terms = [], []
    best_idx, best_score, best_img = np.zeros([0], dtype=np.int64), np.zeros([0], dtype=np.float64), None
    seen = 0
    for x, y in batches:
        s, t = msssim.pair_scores(x, y)
        scores.append(s.numpy())
        terms.append(t.numpy())
        if closest > 0:                                     # the candidates stay in ascending pair order, so a tie goes to the lower pair
            local = np.sort(closest_order(s.numpy(), closest))
            sel = torch.from_numpy(local).to(x.device)
            img = torch.stack([x.index_select(0, sel), y.index_select(0, sel)], dim=1).cpu().numpy()
            best_idx, best_score = np.concatenate([best_idx, seen + local]), np.concatenate([best_score, s.numpy()[local]])
            best_img = img if best_img is None else np.concatenate([best_img, img])
            keep = np.sort(closest_order(best_score, closest))
            best_idx, best_score, best_img = best_idx[keep], best_score[keep], best_img[keep]
        seen += x.shape[0]
    if closest > 0:
        final = closest_order(best_score, closest)
        best_idx, best_img = best_idx[final], best_img[final]
    return np.concatenate(scores), np.concatenate(terms), (best_idx, best_img)


def summary(scores, terms, classes, sides):
    """what diversity.json holds for one set"""
    def stats(sel):
        v = scores[sel]
        out = dict(msssim=mean_left_to_right(v), msssim_std=float(np.std(v)), num_pairs=int(v.size))
        out.update({f'p{round(100 * q):02d}': float(p) for q, p in zip(QUANTILES, np.quantile(v, QUANTILES))})
        out['levels'] = {str(side): mean_left_to_right(terms[sel][:, :, i].reshape(-1)) for i, side in enumerate(sides)}
        return out

    out = stats(np.ones(scores.shape, dtype=bool))
    present = sorted(set(int(k) for k in classes if k >= 0))
    if len(present) > 1:
        out['per_class'] = {str(k): stats(classes == k) for k in present}
    return out


def pair_canvas(images):
    """uint8 [k, 2, C, S, S] -> uint8 [k S, 2 S, C]: one pair per row"""
    k, _, c, s, _ = images.shape
    return np.ascontiguousarray(images.transpose(0, 3, 1, 4, 2).reshape(k * s, 2 * s, c))


@torch.no_grad()
def pairwise_diversity(G=None, dataset=None, pairs=DEFAULT_PAIRS, seed=0, truncation_psi=1, noise_mode='const', class_idx=None, batch=64, closest=8,
                       outdir=None, device=None):
    """MS-SSIM between `pairs` pairs of G's images and between pairs of `dataset`'s (a train_parts.datasets.Dataset without mirrored copies),
    whichever is given -> dict with `stats` (what diversity.json holds), `arrays` (what diversity_pairs.npz holds) and with G and `closest`
    > 0 `canvas`.  With `outdir` the files of the module docstring are written."""
    pairs, batch, closest, seed = int(pairs), int(batch), int(closest), int(seed)
    if pairs < 1:
        raise ValueError(f'--pairs={pairs}: must be at least 1')
    if batch < 1:
        raise ValueError(f'--batch={batch}: must be at least 1')
    if closest < 0:
        raise ValueError(f'--closest={closest}: must not be negative')
    if G is None and dataset is None:
        raise ValueError('at least one of --snapshot and --data is required')
    device = device_of(G, 'cpu' if device is None and G is None else device)

    if G is not None:
        S, C = int(G.img_resolution), int(getattr(G, 'img_channels', 3))
    if dataset is not None:
        Cd, H, W = dataset.image_shape
        if H != W:
            raise ValueError(f'the data set holds {Cd} x {H} x {W} images: square images only')
        if G is not None and (S, S, C) != (H, W, Cd):
            raise ValueError(f'the generator makes {C} x {S} x {S} images, the data set holds {Cd} x {H} x {W}')
        S, C = int(H), int(Cd)
    msssim.check_side(S, f'{C} x {S} x {S} images')
    if C not in (1, 3):
        raise ValueError(f'{C} x {S} x {S} images: 1 or 3 channels only')
    sides, weights = msssim.levels(S)
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)
    stats = dict(image_size=S, channels=C, level_sides=sides, weights=weights.tolist(),
                 options=dict(pairs=pairs, seed=seed, trunc=truncation_psi, class_idx=class_idx, noise_mode=noise_mode, batch=batch, closest=closest))
    arrays, result = {}, dict(stats=stats)

    if G is not None:
        classes = generated_classes(G, class_idx, pairs)
        if G.c_dim == 0:
            class_label(G, class_idx, device)               # its warning about an ignored --class

        def gen_batches():
            for lo in range(0, pairs, batch):
                hi = min(lo + batch, pairs)
                seeds = list(range(2 * lo, 2 * hi))
                label = torch.zeros([len(seeds), G.c_dim], device=device)
                if G.c_dim != 0:
                    label[torch.arange(len(seeds)), torch.from_numpy(np.repeat(classes[lo:hi], 2))] = 1
                img = generated_images(G, seeds, label, truncation_psi, noise_mode, device)
                yield img[0::2].contiguous(), img[1::2].contiguous()

        scores, terms, (best, best_img) = score_pairs(gen_batches(), closest)
        stats['gen'] = summary(scores, terms, classes, sides)
        arrays.update(gen_scores=scores, gen_terms=terms, gen_classes=classes, gen_seeds=np.arange(2 * pairs, dtype=np.int64).reshape(pairs, 2))
        if closest > 0:
            stats['closest_pairs'] = [int(p) for p in best]
            result['canvas'] = pair_canvas(best_img)

    if dataset is not None:
        items, classes = real_pairs(len(dataset), item_classes(dataset), pairs, seed)
        if len(items) == 0:
            raise ValueError(f'the data set of {len(dataset)} items holds no pair of one class')

        def real_batches():
            for lo in range(0, len(items), batch):
                both = np.stack([np.stack([dataset[int(i)][0] for i in pair]) for pair in items[lo:lo + batch]])        # [B, 2, C, S, S]
                both = torch.from_numpy(both).to(device)
                yield both[:, 0].contiguous(), both[:, 1].contiguous()

        scores, terms, _ = score_pairs(real_batches())
        stats['real'] = summary(scores, terms, classes, sides)
        arrays.update(real_scores=scores, real_terms=terms, real_classes=classes, real_items=items)

    if 'gen' in stats and 'real' in stats:
        stats['fraction_above_real_p99'] = float(np.mean(arrays['gen_scores'] >= np.quantile(arrays['real_scores'], 0.99)))
    result['arrays'] = arrays
    if outdir is not None:
        with open(os.path.join(outdir, 'diversity.json'), 'w') as f:
            json.dump(stats, f, indent=2)
        np.savez(os.path.join(outdir, 'diversity_pairs.npz'), **arrays)
        if 'canvas' in result:
            save_png(result['canvas'], os.path.join(outdir, 'closest_pairs.png'))
    return result


# ---------------------------------------------------------------------------------------------------------------- CLI

def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.diversity', description=__doc__.split('\n')[0])
    ap.add_argument('--outdir', required=True, help='where to save diversity.json / diversity_pairs.npz / closest_pairs.png')
    add_snapshot_option(ap, required=False, help=SNAPSHOT_HELP + '; without it only the data set is measured')
    ap.add_argument('--data', help='data set whose pairs are measured, folder or zip; without it only the generator is measured')
    ap.add_argument('--pairs', type=int, default=DEFAULT_PAIRS, help=f'pairs per set (default: {DEFAULT_PAIRS})')
    ap.add_argument('--seed', type=int, default=0, help='seed of the walk over the data set (default: 0)')
    add_sampling_options(ap)
    add_device_option(ap)
    ap.add_argument('--batch', type=int, default=64, help='pairs measured at a time (default: 64)')
    ap.add_argument('--closest', type=int, default=8, help='most similar generated pairs shown in closest_pairs.png (default: 8)')
    args, rest = ap.parse_known_args(argv)
    if args.pairs < 1:
        ap.error('--pairs must be at least 1')
    if args.batch < 1:
        ap.error('--batch must be at least 1')
    if args.closest < 0:
        ap.error('--closest must not be negative')
    if args.seed < 0:
        ap.error('--seed must not be negative')
    if args.snapshot is None and args.data is None:
        ap.error('at least one of --snapshot and --data is required')
    require_file(ap, '--snapshot', args.snapshot)
    return config_overrides(ap, rest), args


def run_diversity(argv=None):
    overrides, args = parse_args(argv)
    from . import arguments
    from .train_parts.trainers import training_set_kwargs_from_config
    config = arguments.load_config(overrides)
    device = tool_device(args.device)
    G = load_generator(config, args.snapshot, device) if args.snapshot is not None else None
    kw = None
    if args.data is not None:                               # the labels follow the network, or the run's data.cond without one
        kw = dataset_kwargs_for(config, G, args.data, mirror=False) if G is not None else \
            training_set_kwargs_from_config(config, seed=config.gen.seed, path=args.data, mirror=False)
    with open_dataset(config, kw) if kw is not None else contextlib.nullcontext() as dataset:
        result = pairwise_diversity(G, dataset, pairs=args.pairs, seed=args.seed, truncation_psi=args.truncation_psi, noise_mode=args.noise_mode,
                                    class_idx=args.class_idx, batch=args.batch, closest=args.closest, outdir=args.outdir, device=device)
    stats = result['stats']
    line = {name: {k: stats[name][k] for k in ('msssim', 'msssim_std', 'num_pairs')} for name in ('gen', 'real') if name in stats}
    if 'fraction_above_real_p99' in stats:
        line['fraction_above_real_p99'] = stats['fraction_above_real_p99']
    print(json.dumps(line))
    return result


if __name__ == '__main__':
    run_diversity()
