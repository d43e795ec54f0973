"""Per-image realism scores of generated images: which of these samples are good?

The other snapshot tools judge a whole set of images; this one ranks single images.  Kynkaanniemi et al. ("Improved Precision and Recall Metric
for Assessing Generative Models", NeurIPS 2019, section 5) define, next to the precision / recall that ``pr50k3_full`` computes, the realism score
of a generated image with feature g:

    R(g) = max over real features r of  radius_k(r) / |g - r|

where radius_k(r) is the distance from r to its k-th nearest real feature and the half of the real balls with the largest radii is discarded
first (``--keep``): balls that reach far stand for sparsely sampled regions.  R >= 1 exactly when the image lies inside the pruned real
manifold; larger means closer to densely populated real data.  The reference has no such tool.

* The manifold is the ``vgg16.pt`` feature (``return_features=True``) of every data set item in item order, mirrored copies off, cached where
  the metrics' features are cached when the detector is a file.  The queries are the bytes ``generate.py`` writes, through the same detector.
  Both are rounded to fp16, so ``--device=cpu`` and ``cuda`` score the same numbers with ``knn_manifold.realism``: on the
  fp16 distance d, score = max radius / d as one fp32 division, +inf for an exact copy of a kept real feature, 0 when no ball is kept; ``item``
  is the lowest data set item that attains it.
* ``realism.json``: ``k``, ``keep``, ``F``, ``manifold_points``, ``kept_points``, ``num``; for ``generated`` and for ``real`` -- the baseline:
  every data set item against the kept balls of the others, its own left out -- ``min``, the quantiles ``p01 p10 p50 p90 p99``,
  ``fraction_realistic`` (score >= 1) and ``num_infinite``; and ``fraction_below_real_p01``: the share of generated images at or below the 1 %
  quantile of the baseline.  Statistics are taken over scores clipped to SCORE_CLIP = 65504, so the file is strict JSON.
* ``realism.npz``: ``seeds``, ``score``, ``item`` (unclipped); ``real_score``, ``real_item``; ``radius`` (fp16 per data set item, -1 where pruned).
* ``realism.png``: row 1 the ``--show`` highest-scoring generated images in descending order, row 2 the ``--show`` lowest in ascending order; ties
  go to the lower seed.  The images are kept as running lists over the batches: nothing is generated twice.

What the number does not say: it is relative to the data set given and to k; it inherits the detector's blind spots; a memorised training image
scores +inf, so a high score alone is no sign of a good generator (``nearest_neighbors`` answers that); and scores of different data sets are not
comparable.  The baseline tells how real images themselves score against the rest of the data.

    python -m style_big_gan_amd.realism exp.config_dir=<dir> exp.config=<file.yaml> --snapshot=<network-snapshot-*.pt> --detector=<vgg16.pt | dir> \\
        --outdir=<dir> [--seeds=0-63 | --num=N] [--k=3] [--keep=0.5] [--show=8] [--data=<folder|zip>] [--trunc=1] [--class=<idx>] \\
        [--noise-mode=const|random|none] [--device=auto|cuda|cpu] [--batch=64]
"""
import argparse
import json
import os

import numpy as np
import torch

from .tool_support import (add_device_option, add_sampling_options, add_snapshot_option, checked_features, class_label, config_overrides, dataset_features,
                           dataset_kwargs_for, device_of, generated_images, load_generator, num_range, open_dataset, require_file, save_png, tool_device,
                           vgg16_feature_options)
from .torch_utils.ops import knn_manifold

QUANTILES = (0.01, 0.10, 0.50, 0.90, 0.99)
SCORE_CLIP = 65504.0            # statistics are taken over min(score, SCORE_CLIP): the largest finite fp16, above every finite ratio of interest
MAX_K = 7                       # knn_manifold.kth_radius: k + 1 <= 8
ROW_BATCH = 10000               # probe rows per launch of the radius and realism passes


def check_options(k, keep, show, batch):
    if not 1 <= int(k) <= MAX_K:
        raise ValueError(f'--k={k}: must be between 1 and {MAX_K}')
    if not 0 < float(keep) <= 1:
        raise ValueError(f'--keep={keep}: must be above 0 and at most 1')
    if int(show) < 0:
        raise ValueError(f'--show={show}: must not be negative')
    if int(batch) < 1:
        raise ValueError(f'--batch={batch}: must be at least 1')


def ranked(score, seeds, count, best):
    """positions of the `count` highest (`best`) or lowest scores, in that order, ties to the lower seed"""
    score = np.asarray(score, dtype=np.float64)
    return np.lexsort((np.asarray(seeds), -score if best else score))[:count]


def summary(score):
    """what realism.json holds for one set of scores"""
    clipped = np.minimum(np.asarray(score, dtype=np.float64), SCORE_CLIP)
    out = dict(min=float(clipped.min()))
    out.update({f'p{round(100 * q):02d}': float(v) for q, v in zip(QUANTILES, np.quantile(clipped, QUANTILES))})
    out.update(fraction_realistic=float(np.mean(np.asarray(score) >= 1)), num_infinite=int(np.isinf(score).sum()))
    return out


@torch.no_grad()
def realism_ranking(G, dataset, seeds, k=3, keep=0.5, show=8, truncation_psi=1, noise_mode='const', class_idx=None, batch=64, outdir=None, device=None,
                    detector=None, dataset_kwargs=None, dataset_name='image_folder', cache_dir=None):
    """Realism scores of G's images for `seeds` against `dataset` (a train_parts.datasets.Dataset without mirrored copies) -> dict with `stats`
    (what realism.json holds), `arrays` (what realism.npz holds), `canvas` (uint8 [2 H, min(show, num) W, C]) and `shown` (the seeds of its two
    rows, `best` and `worst`).  With `outdir` the files of the module docstring are written.  `detector`, `dataset_kwargs`, `dataset_name` and `cache_dir` as in `nearest_neighbors`."""
    from .metrics import metric_utils, scores
    check_options(k, keep, show, batch)
    k, keep, show, batch = int(k), float(keep), int(show), int(batch)
    seeds = [int(s) for s in seeds]
    if not seeds:
        raise ValueError('no seeds: one of --seeds and --num is required')
    if detector is None:
        raise ValueError('--detector is required: a TorchScript vgg16.pt, a directory holding it, or a callable')
    if dataset_kwargs is None:
        raise ValueError('dataset_kwargs are required: the feature pass builds its own loader of the data set')
    device = device_of(G, device)
    C, H, W = dataset.image_shape
    if (G.img_resolution, G.img_resolution) != (H, W) or getattr(G, 'img_channels', C) != C:
        raise ValueError(f'the generator makes {G.img_resolution} x {G.img_resolution} images, the data set holds {C} x {H} x {W}')
    if len(dataset) < k + 1:
        raise ValueError(f'--k={k}: the data set holds {len(dataset)} items, the radius of a ball needs {k + 1}')
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)
    label = class_label(G, class_idx, device)

    opts = vgg16_feature_options(detector, dataset_kwargs, device, cache_dir)
    call_kw = metric_utils.detector_call_kwargs(opts, scores.VGG16, dict(return_features=True))
    detect = metric_utils._detector(opts, scores.VGG16)
    manifold = checked_features(dataset_features(opts, dataset, dataset_name, '--detector').to(device), 'the data set', '--detector')
    N, F = manifold.shape
    radius = scores.realism_radii(manifold, k, keep, ROW_BATCH)
    real_score, real_item = scores.realism_sweep(manifold, manifold, radius, ROW_BATCH, own=True)

    num = len(seeds)
    cols = min(show, num)
    score, item = [], []
    lists = {best: (np.zeros([0], dtype=np.float32), np.zeros([0], dtype=np.int64), np.zeros([0, C, H, W], dtype=np.uint8)) for best in (True, False)}
    for lo in range(0, num, batch):
        batch_seeds = seeds[lo:lo + batch]
        images = generated_images(G, batch_seeds, label, truncation_psi, noise_mode, device)
        feats = checked_features(detect(metric_utils._as_rgb(images), **call_kw).to(torch.float32), 'the generated images', '--detector')
        s, i = knn_manifold.realism(feats, manifold, radius)
        s, i = s.cpu().numpy(), i.cpu().numpy()
        score.append(s)
        item.append(i)
        for best, (ls, lseed, limg) in lists.items():          # the running lists: this batch's candidates join, the `cols` first stay
            pick = ranked(s, batch_seeds, cols, best)
            sel = torch.from_numpy(pick).to(device)
            ls, lseed = np.concatenate([ls, s[pick]]), np.concatenate([lseed, np.asarray(batch_seeds, dtype=np.int64)[pick]])
            limg = np.concatenate([limg, images.index_select(0, sel).cpu().numpy()])
            order = ranked(ls, lseed, cols, best)
            lists[best] = (ls[order], lseed[order], limg[order])
    score, item = np.concatenate(score), np.concatenate(item)
    real_score, real_item, radius = real_score.cpu().numpy(), real_item.cpu().numpy(), radius.cpu().numpy()

    canvas = np.concatenate([lists[best][2].transpose(2, 0, 3, 1).reshape(H, cols * W, C) for best in (True, False)])
    real_clipped = np.minimum(real_score.astype(np.float64), SCORE_CLIP)
    stats = dict(k=k, keep=keep, F=F, manifold_points=N, kept_points=int((radius >= 0).sum()), num=num, generated=summary(score), real=summary(real_score),
                 fraction_below_real_p01=float(np.mean(np.minimum(score.astype(np.float64), SCORE_CLIP) <= np.quantile(real_clipped, 0.01))))
    arrays = dict(seeds=np.asarray(seeds, dtype=np.int64), score=score, item=item, real_score=real_score, real_item=real_item, radius=radius)
    result = dict(stats=stats, arrays=arrays, canvas=canvas, shown=dict(best=lists[True][1].tolist(), worst=lists[False][1].tolist()))
    if outdir is not None:
        with open(os.path.join(outdir, 'realism.json'), 'w') as f:
            json.dump(stats, f, indent=2, allow_nan=False)
        np.savez(os.path.join(outdir, 'realism.npz'), **arrays)
        save_png(canvas, os.path.join(outdir, 'realism.png'))
    return result


# ---------------------------------------------------------------------------------------------------------------- CLI

def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.realism', description=__doc__.split('\n')[0])
    add_snapshot_option(ap)
    ap.add_argument('--detector', required=True, help='the local TorchScript vgg16.pt, or a directory holding it')
    ap.add_argument('--outdir', required=True, help='where to save realism.json / realism.npz / realism.png')
    ap.add_argument('--seeds', type=num_range, help='seeds whose images are scored')
    ap.add_argument('--num', type=int, help='score the images of seeds 0..N-1')
    ap.add_argument('--k', type=int, default=3, help=f'neighbour whose distance is a real ball\'s radius, 1 to {MAX_K} (default: 3)')
    ap.add_argument('--keep', type=float, default=0.5, help='share of the real balls kept, those of smallest radius (default: 0.5)')
    ap.add_argument('--show', type=int, default=8, help='highest- and lowest-scoring images shown in realism.png (default: 8)')
    ap.add_argument('--data', help='data set that forms the manifold, folder or zip (default: the run\'s data.dataset_path)')
    add_sampling_options(ap)
    add_device_option(ap)
    ap.add_argument('--batch', type=int, default=64, help='images generated and scored at a time (default: 64)')
    args, rest = ap.parse_known_args(argv)
    if (args.seeds is None) == (args.num is None):
        ap.error('exactly one of --seeds and --num is required')
    if args.num is not None and args.num < 1:
        ap.error('--num must be at least 1')
    try:
        check_options(args.k, args.keep, args.show, args.batch)
    except ValueError as err:
        ap.error(str(err))
    if not os.path.exists(args.detector):
        ap.error(f'--detector={args.detector}: no such TorchScript file or directory (detectors are not downloaded in this build)')
    require_file(ap, '--snapshot', args.snapshot)
    if args.num is not None:
        args.seeds = list(range(args.num))
    return config_overrides(ap, rest), args


def run_realism(argv=None):
    overrides, args = parse_args(argv)
    from . import arguments
    config = arguments.load_config(overrides)
    device = tool_device(args.device)
    G = load_generator(config, args.snapshot, device)
    kw = dataset_kwargs_for(config, G, data=args.data, mirror=False)
    with open_dataset(config, kw) as dataset:
        result = realism_ranking(G, dataset, args.seeds, k=args.k, keep=args.keep, show=args.show, truncation_psi=args.truncation_psi,
                                 noise_mode=args.noise_mode, class_idx=args.class_idx, batch=args.batch, outdir=args.outdir, device=device,
                                 detector=args.detector, dataset_kwargs=kw, dataset_name=config.data.dataset)
    print(json.dumps(result['stats'], allow_nan=False))
    return result


if __name__ == '__main__':
    run_realism()
