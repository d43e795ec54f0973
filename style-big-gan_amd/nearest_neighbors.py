"""Nearest training images of generated images: is the generator copying its data?

The reference has no such tool; the ADA, DiffAugment and BigGAN papers answer the question with nearest-neighbour figures in pixel space
(``--space=pixel``, the default), the BigGAN paper in VGG-16 feature space as well (``--space=vgg16``).  In pixel space the training set is decoded once into the resident loader's uint8 store on the device
(``train_parts/dataloaders.py``), the queries are exactly the bytes ``generate.py`` would write (``image_export.quantize(..., 'clamp')``),
and the search is exact integer arithmetic on the i8 matrix cores (``torch_utils/ops/nn_u8.py``): d2 = sum of squared byte differences.

* ``--seeds``: ``neighbors.png`` (one row per seed: the generated image, then its k nearest training images at full resolution, mirrored
  where the mirrored copy matched) and ``neighbors.json`` (per seed a list of ``{item, file, flip, d2, rmse}``, rmse = sqrt(d2 / F)).
* ``--num=N``: seeds 0..N-1 in batches; ``nn_stats.npz`` holds the exact int64 nearest d2 of every generated image (``gen_to_train``) and
  the baseline ``train_to_train``, the nearest *other* stored image of every stored image (its own row is excluded in both
  orientations); ``nn_stats.json`` holds, for both, min / 1, 5, 25, 50, 75 % quantiles / mean of the rmse, and
  ``fraction_below_train_p01``: the share of generated images at or below the 1 % quantile of ``train_to_train`` -- the memorisation flag
  (an exact copy always counts).
* ``--res=R`` (a power of two, 4 <= R <= the data resolution) compares box-reduced copies (``resample_u8.resize(..., 'box')``) of the
  store and the queries; the store is reduced once, in chunks.  Without it the search runs at full size.
* Mirrored data sets (``data.mirror`` / ``--mirror=1``): d2(q, mirrored x) = d2(mirrored q, x), so the search runs twice over the one
  store, with the queries and with ``queries.flip(3)``, and the two lists are merged by (d2, flip, row).  A mirrored data set lists
  every image as stored and then every image mirrored, both in the store's order, so this is the order (d2, item): the result equals a
  brute-force search over ``dataset[i]`` in item order, ties to the lower item.  (A box reduction by a power of two commutes with
  mirroring, so the same holds under ``--res``.)

``--space=vgg16 --detector=<TorchScript file | directory holding vgg16.pt>`` searches in the feature space of the ``vgg16.pt`` detector that
``pr50k3_full`` uses (``return_features=True``): a shifted or re-coloured copy is far from its source in bytes and stays close there.
* The manifold is the feature of every data set item in item order (``metric_utils.compute_feature_stats_for_dataset(...,
  capture_all=True)``, cached as ``.npz`` when the detector is a file; a cached array whose row count is not ``len(dataset)`` is not used),
  the queries are the bytes ``generate.py`` writes, through the same detector.  Both are rounded to fp16, so ``--device=cpu`` and ``cuda``
  search the same numbers, with ``knn_manifold.topk``: d2 = max((n(x) + n(y)) - 2 s, 0) in fp32, ascending by (d2, item) (DESIGN
  section 19).  Features must be finite and their width a multiple of 8; ``--res`` is refused (the detector sees full-size images).
* A mirrored data set lists its mirrored items as rows of their own -- feature(mirror x) is not mirror(feature x) -- so there is one
  search, item = row, and ``flip`` / ``file`` come from the data set's tables.
* ``neighbors.json``: ``{space, F, k, seeds}`` with entries ``{item, file, flip, d2, dist}``, dist = sqrt(d2); ``neighbors.png`` as above.
  ``nn_stats.npz``: float32 d2; ``train_to_train`` has one entry per stored image: from its unmirrored item to the nearest item that is
  neither itself nor its mirrored twin.  ``nn_stats.json``: the fields above with quantiles of dist in place of the rmse, plus ``space``.
LPIPS space is out of scope: the reference's ``return_lpips=True`` features are about 8 M values per 256 x 256 image, and a training set of
them does not fit on the device.

    python -m style_big_gan_amd.nearest_neighbors exp.config_dir=<dir> exp.config=<file.yaml> --snapshot=<network-snapshot-*.pt> --outdir=<dir> \\
        [--seeds=0-7] [--num=N] [--k=5] [--space=pixel|vgg16] [--detector=<file|dir>] [--res=R] [--data=<folder|zip>] [--mirror=0|1] [--trunc=1] [--class=<idx>] \\
        [--noise-mode=const|random|none] [--device=auto|cuda|cpu] [--batch=64]
"""
import argparse
import json
import os

import numpy as np
import torch

from .tool_support import (STORE_CHUNK_BYTES, add_device_option, add_sampling_options, add_snapshot_option, check_res, checked_features,  # noqa: F401
                           class_label, config_overrides, dataset_features, dataset_kwargs_for, detector_kwargs, device_of, generated_images, load_generator,
                           num_range, open_dataset, reduce_images, reduce_store, require_file, save_png, snapshot_generator_state, tool_device,
                           vgg16_feature_options)
from .torch_utils.ops import knn_manifold, nn_u8, resident_set

SPACES = ('pixel', 'vgg16')
QUANTILES = (0.01, 0.05, 0.25, 0.50, 0.75)
_ROW_BITS = 24                          # nn_u8's row limit: (d2, flip, row) as one int64 key


def item_table(slot, flip, rows):
    """-> int64 [2, rows] on the tables' device: the data set item that is store row r as stored ([0, r]) / mirrored ([1, r]), -1 when the
    data set has no such item"""
    table = torch.full([2, rows], -1, dtype=torch.int64, device=slot.device)
    table[flip.to(torch.int64), slot.to(torch.int64)] = torch.arange(slot.numel(), dtype=torch.int64, device=slot.device)
    return table


def search(queries, store, k, mirrored, exclude=None):
    """the k nearest data set images of every query -> (d2 int64 [Q, k], row int64 [Q, k], flip int64 [Q, k]), ascending by (d2, flip, row).
    `mirrored`: the data set also holds every stored image mirrored, searched as `queries.flip(3)` against the same store."""
    d2, row = nn_u8.topk(queries, store, k, exclude)
    row = row.to(torch.int64)
    if not mirrored:
        return d2, row, torch.zeros_like(row)
    d2f, rowf = nn_u8.topk(queries.flip(3).contiguous(), store, k, exclude)
    key = torch.cat([(d2 << (_ROW_BITS + 1)) | row, (d2f << (_ROW_BITS + 1)) | (1 << _ROW_BITS) | rowf.to(torch.int64)], dim=1)
    key = key.sort(dim=1).values[:, :k]
    return key >> (_ROW_BITS + 1), key & ((1 << _ROW_BITS) - 1), (key >> _ROW_BITS) & 1


def train_to_train(store, mirrored, batch):
    """-> int64 [S] on the store's device: d2 from every stored image to the nearest other image of the data set (its own row is excluded,
    as stored and mirrored)"""
    S = store.shape[0]
    if S < 2:
        raise ValueError('the train_to_train baseline needs at least two stored images')
    out = torch.empty([S], dtype=torch.int64, device=store.device)
    for lo in range(0, S, batch):
        hi = min(lo + batch, S)
        own = torch.arange(lo, hi, dtype=torch.int32, device=store.device)
        out[lo:hi] = search(store[lo:hi], store, 1, mirrored, exclude=own)[0][:, 0]
    return out


def dist_summary(d2, F=1):
    """min, the QUANTILES and the mean of sqrt(d2 / F): the distance, or with F the rmse over the F values of an image"""
    dist = np.sqrt(np.asarray(d2, dtype=np.float64) / F)
    out = dict(min=float(dist.min()), mean=float(dist.mean()))
    out.update({f'p{round(100 * q):02d}': float(v) for q, v in zip(QUANTILES, np.quantile(dist, QUANTILES))})
    return out


def _feature_space(G, dataset, label, seeds, num, k, truncation_psi, noise_mode, batch, outdir, device, max_gib, detector, dataset_kwargs, dataset_name,
                   cache_dir):
    """the --space=vgg16 half of `nearest_training_images`"""
    from .metrics import metric_utils, scores
    from .train_parts.dataloaders import ResidentDataloader
    C, H, W = dataset.image_shape
    opts = vgg16_feature_options(detector, dataset_kwargs, device, cache_dir)
    call_kw = metric_utils.detector_call_kwargs(opts, scores.VGG16, dict(return_features=True))
    detect = metric_utils._detector(opts, scores.VGG16)
    manifold = checked_features(dataset_features(opts, dataset, dataset_name).to(device), 'the data set')
    M, F = manifold.shape
    raw, slot, flip = resident_set.tables(dataset)
    S = len(raw)
    mirrored = bool(flip.any())
    if seeds is not None and M < k:
        raise ValueError(f'--k={k}: the data set holds {M} items')
    fnames = getattr(dataset, '_image_fnames', None)
    result = dict(space='vgg16', F=F, res=dataset.resolution, k=k, mirrored=mirrored)

    def features_of(batch_seeds):
        q = generated_images(G, batch_seeds, label, truncation_psi, noise_mode, device)
        return q, detect(metric_utils._as_rgb(q), **call_kw).to(torch.float32)

    if seeds is not None:
        seeds = [int(s) for s in seeds]
        store = ResidentDataloader(dataset, sampler=(), batch_size=1, device=device, max_gib=max_gib).store
        images, feats = zip(*[features_of([seed]) for seed in seeds])          # one image per call, as generate.py makes them
        d2, item = knn_manifold.topk(checked_features(torch.cat(feats), 'the generated images'), manifold, k)
        d2, item = d2.cpu(), item.cpu().to(torch.int64)
        canvas = torch.zeros([len(seeds) * H, (k + 1) * W, C], dtype=torch.uint8, device=device)
        neighbors = dict()
        for r, seed in enumerate(seeds):
            near = resident_set.gather(store, slot[item[r]].to(device), flip[item[r]].to(device))
            cells = torch.cat([images[r], near]).permute(0, 2, 3, 1)
            canvas[r * H:(r + 1) * H] = cells.permute(1, 0, 2, 3).reshape(H, (k + 1) * W, C)
            neighbors[seed] = [dict(item=i, file=fnames[int(raw[int(slot[i])])] if fnames is not None else None, flip=int(flip[i]), d2=float(d),
                                    dist=float(np.sqrt(d))) for d, i in zip(d2[r].tolist(), item[r].tolist())]
        result.update(neighbors=neighbors, canvas=canvas.cpu().numpy())
        if outdir is not None:
            save_png(result['canvas'], os.path.join(outdir, 'neighbors.png'))
            with open(os.path.join(outdir, 'neighbors.json'), 'w') as f:
                json.dump(dict(space='vgg16', F=F, k=k, seeds={str(s): v for s, v in neighbors.items()}), f, indent=2)

    if num is not None:
        num = int(num)
        if S < 2:
            raise ValueError('the train_to_train baseline needs at least two stored images')
        feats = torch.cat([features_of(list(range(lo, min(lo + batch, num))))[1] for lo in range(0, num, batch)])
        gen = knn_manifold.topk(checked_features(feats, 'the generated images'), manifold, 1)[0][:, 0].cpu().numpy()
        # the baseline: the unmirrored item of every stored image against all items but itself; its mirrored twin is dropped here
        own = item_table(slot, flip, S)
        assert bool((own[0] >= 0).all())
        d2, item = knn_manifold.topk(manifold[own[0].to(device)], manifold, 2 if mirrored else 1, exclude=own[0].to(torch.int32).to(device))
        first = (item[:, 0].cpu().to(torch.int64) == own[1]).to(torch.int64)            # 1 where the nearest is the twin: take the second
        base = d2.cpu().gather(1, first[:, None])[:, 0].numpy()
        p01 = float(np.quantile(base.astype(np.float64), 0.01))
        stats = dict(space='vgg16', F=F, res=dataset.resolution, num=num, stored_images=S, mirrored=mirrored, gen_to_train=dist_summary(gen),
                     train_to_train=dist_summary(base), train_p01_d2=p01, fraction_below_train_p01=float(np.mean(gen <= p01)))
        result.update(gen_to_train=gen, train_to_train=base, stats=stats)
        if outdir is not None:
            np.savez(os.path.join(outdir, 'nn_stats.npz'), gen_to_train=gen, train_to_train=base)
            with open(os.path.join(outdir, 'nn_stats.json'), 'w') as f:
                json.dump(stats, f, indent=2)
    return result


@torch.no_grad()
def nearest_training_images(G, dataset, seeds=None, num=None, k=5, res=None, truncation_psi=1, noise_mode='const', class_idx=None, batch=64,
                            outdir=None, device=None, max_gib=None, space='pixel', detector=None, dataset_kwargs=None, dataset_name='image_folder',
                            cache_dir=None):
    """Nearest training images of G's samples in `dataset` (a train_parts.datasets.Dataset).  -> dict with, for `seeds`, `neighbors`
    ({seed: [{item, file, flip, d2, rmse} x k]}) and `canvas` (uint8 [rows * H, (k + 1) * W, C]); for `num`, `gen_to_train` and
    `train_to_train` (int64 ndarrays) and `stats`.  With `outdir` the files of the module docstring are written.
    `space='vgg16'` searches in the detector's feature space (entries {item, file, flip, d2, dist}, float32 d2 arrays).  `detector` is what
    `MetricOptions.detector` takes -- a callable, a TorchScript file, a dict -- or a directory holding vgg16.pt; `dataset_kwargs` /
    `dataset_name` are what `dataset` was built from (the feature pass builds its own loader from them and keys its cache on them);
    `cache_dir` overrides where features are cached."""
    from .train_parts.dataloaders import ResidentDataloader
    if space not in SPACES:
        raise ValueError(f'--space={space}: must be one of {", ".join(SPACES)}')
    if space == 'vgg16':
        if detector is None:
            raise ValueError('--space=vgg16 needs --detector: a TorchScript vgg16.pt, a directory holding it, or a callable')
        if res is not None:
            raise ValueError('--res cannot be combined with --space=vgg16: the detector sees full-size images')
        if dataset_kwargs is None:
            raise ValueError('--space=vgg16 needs dataset_kwargs: the feature pass builds its own loader of the data set')
    if seeds is None and num is None:
        raise ValueError('one of --seeds and --num is required')
    if num is not None and int(num) < 1:
        raise ValueError(f'--num={num}: must be at least 1')
    batch = int(batch)
    if batch < 1:
        raise ValueError(f'--batch={batch}: must be at least 1')
    device = device_of(G, device)
    C, H, W = dataset.image_shape
    if (G.img_resolution, G.img_resolution) != (H, W) or getattr(G, 'img_channels', C) != C:
        raise ValueError(f'the generator makes {G.img_resolution} x {G.img_resolution} images, the data set holds {C} x {H} x {W}')
    res = check_res(res, dataset.resolution)
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)

    label = class_label(G, class_idx, device)
    if space == 'vgg16':
        return _feature_space(G, dataset, label, seeds, num, k, truncation_psi, noise_mode, batch, outdir, device, max_gib, detector, dataset_kwargs,
                              dataset_name, cache_dir)

    loader = ResidentDataloader(dataset, sampler=(), batch_size=1, device=device, max_gib=max_gib)
    raw, slot, flip = resident_set.tables(dataset)
    store = loader.store
    S = store.shape[0]
    mirrored = bool(flip.any())
    if seeds is not None and S < k:
        raise ValueError(f'--k={k}: the data set holds {S} stored images')
    items = item_table(slot.to(device), flip.to(device), S)
    small = reduce_store(store, res)
    F = small[0].numel()
    fnames = getattr(dataset, '_image_fnames', None)
    result = dict(F=F, res=res if res is not None else dataset.resolution, k=k, mirrored=mirrored)

    def look_up(batch_seeds, kk):
        q = generated_images(G, batch_seeds, label, truncation_psi, noise_mode, device)
        return (q,) + search(reduce_images(q, res), small, kk, mirrored)

    if seeds is not None:
        seeds = [int(s) for s in seeds]
        canvas = torch.zeros([len(seeds) * H, (k + 1) * W, C], dtype=torch.uint8, device=device)
        neighbors = dict()
        for r, seed in enumerate(seeds):                    # one image per call, as generate.py makes them
            q, d2, row, fl = look_up([seed], k)
            near = resident_set.gather(store, row[0].to(torch.int32), fl[0].to(torch.uint8))
            cells = torch.cat([q, near]).permute(0, 2, 3, 1)
            canvas[r * H:(r + 1) * H] = cells.permute(1, 0, 2, 3).reshape(H, (k + 1) * W, C)
            item = items[fl[0], row[0]].cpu().tolist()
            neighbors[seed] = [dict(item=item[t], file=fnames[int(raw[rw])] if fnames is not None else None, flip=int(f), d2=int(d), rmse=float(np.sqrt(d / F)))
                               for t, (d, rw, f) in enumerate(zip(d2[0].cpu().tolist(), row[0].cpu().tolist(), fl[0].cpu().tolist()))]
        result.update(neighbors=neighbors, canvas=canvas.cpu().numpy())
        if outdir is not None:
            save_png(result['canvas'], os.path.join(outdir, 'neighbors.png'))
            with open(os.path.join(outdir, 'neighbors.json'), 'w') as f:
                json.dump(dict(F=F, res=result['res'], k=k, seeds={str(s): v for s, v in neighbors.items()}), f, indent=2)

    if num is not None:
        num = int(num)
        gen = torch.cat([look_up(list(range(lo, min(lo + batch, num))), 1)[1][:, 0] for lo in range(0, num, batch)])
        base = train_to_train(small, mirrored, max(1, min(batch, STORE_CHUNK_BYTES // F)))
        gen, base = gen.cpu().numpy(), base.cpu().numpy()
        p01 = float(np.quantile(base.astype(np.float64), 0.01))
        stats = dict(F=F, res=result['res'], num=num, stored_images=S, mirrored=mirrored, gen_to_train=dist_summary(gen, F),
                     train_to_train=dist_summary(base, F), train_p01_d2=p01, fraction_below_train_p01=float(np.mean(gen <= p01)))
        result.update(gen_to_train=gen, train_to_train=base, stats=stats)
        if outdir is not None:
            np.savez(os.path.join(outdir, 'nn_stats.npz'), gen_to_train=gen, train_to_train=base)
            with open(os.path.join(outdir, 'nn_stats.json'), 'w') as f:
                json.dump(stats, f, indent=2)
    return result


# ---------------------------------------------------------------------------------------------------------------- CLI

def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.nearest_neighbors', description=__doc__.split('\n')[0])
    add_snapshot_option(ap)
    ap.add_argument('--outdir', required=True, help='where to save neighbors.png / neighbors.json / nn_stats.npz / nn_stats.json')
    ap.add_argument('--seeds', type=num_range, help='seeds whose images get a row of neighbours')
    ap.add_argument('--num', type=int, help='distance statistics over the images of seeds 0..N-1')
    ap.add_argument('--k', type=int, default=5, help=f'neighbours per image, 1 to {nn_u8.MAX_K} (default: 5)')
    ap.add_argument('--space', choices=SPACES, default='pixel', help='where distances are taken: pixel bytes, or vgg16.pt features (default: pixel)')
    ap.add_argument('--detector', help='with --space=vgg16: the local TorchScript vgg16.pt, or a directory holding it')
    ap.add_argument('--res', type=int, help='compare box-reduced copies of this resolution (a power of two; default: full size)')
    ap.add_argument('--data', help='data set to search, folder or zip (default: the run\'s data.dataset_path)')
    ap.add_argument('--mirror', type=int, choices=(0, 1), help='whether the data set holds the x-flips (default: the run\'s data.mirror)')
    add_sampling_options(ap)
    add_device_option(ap)
    ap.add_argument('--batch', type=int, default=64, help='images generated and searched at a time with --num (default: 64)')
    args, rest = ap.parse_known_args(argv)
    if args.seeds is None and args.num is None:
        ap.error('one of --seeds and --num is required')
    if args.num is not None and args.num < 1:
        ap.error('--num must be at least 1')
    if not 1 <= args.k <= nn_u8.MAX_K:
        ap.error(f'--k must be between 1 and {nn_u8.MAX_K}')
    if args.res is not None and (args.res < 4 or args.res & (args.res - 1)):
        ap.error('--res must be a power of two, at least 4')
    if args.batch < 1:
        ap.error('--batch must be at least 1')
    if args.space == 'vgg16':
        if args.detector is None:
            ap.error('--space=vgg16 needs --detector: the TorchScript vgg16.pt, or a directory holding it')
        if not os.path.exists(args.detector):
            ap.error(f'--detector={args.detector}: no such TorchScript file or directory (detectors are not downloaded in this build)')
        if args.res is not None:
            ap.error('--res cannot be combined with --space=vgg16: the detector sees full-size images')
    require_file(ap, '--snapshot', args.snapshot)
    args.mirror = None if args.mirror is None else bool(args.mirror)
    return config_overrides(ap, rest), args


def run_nearest_neighbors(argv=None):
    overrides, args = parse_args(argv)
    from . import arguments
    config = arguments.load_config(overrides)
    device = tool_device(args.device)
    G = load_generator(config, args.snapshot, device)
    kw = dataset_kwargs_for(config, G, data=args.data, mirror=args.mirror)
    with open_dataset(config, kw) as dataset:
        feature = dict(space=args.space, detector=args.detector, dataset_kwargs=kw, dataset_name=config.data.dataset) if args.space == 'vgg16' else {}
        result = nearest_training_images(G, dataset, seeds=args.seeds, num=args.num, k=args.k, res=args.res, truncation_psi=args.truncation_psi,
                                         noise_mode=args.noise_mode, class_idx=args.class_idx, batch=args.batch, outdir=args.outdir, device=device,
                                         **feature)
    if 'stats' in result:
        print(json.dumps(result['stats']))
    return result


if __name__ == '__main__':
    run_nearest_neighbors()
