"""Mode coverage: which parts of the data does the generator fail to produce, or over-produce?

The detector-free answer of Richardson & Weiss ("On GANs and GMMs", NeurIPS 2018), the *number of statistically different bins* (NDB): cluster
the training images with k-means, count how many training images and how many generated images fall into each Voronoi cell, run a two-proportion
z-test on every cell, and report the number of significantly different cells and the Jensen-Shannon divergence of the two histograms.  A held-out
split of the data itself calibrates the numbers, and every bin can be shown as pictures.  The reference has no such tool.

* Data: the resident loader's uint8 store (``train_parts/dataloaders.py``), flips off, box-reduced to ``--res`` (``--res=none`` keeps the full
  size; the rules of ``tool_support.check_res``).  ``rng = RandomState(--seed)``; ``P = rng.permutation(len)``; the first
  ``round(holdout * len)`` items of P are held out, the rest are the reference set, which is clustered; ``--holdout=0`` skips the baseline.
* Generated set: the bytes ``generate.py`` writes for the seeds 0 .. ``--num`` - 1 (default: the size of the reference set), reduced the same
  way, produced in batches of ``--batch`` and assigned batch by batch, so only labels and distances are kept.  On a conditional network without
  ``--class`` generated image p takes the label of reference item ``p mod N_ref`` (the class mix of the data); with ``--class=i`` both sets are
  restricted to class i.
* Clustering (``torch_utils/ops/kmeans_u8.py``): k-means++ seeding from the same ``rng``, then Lloyd iterations with byte
  centroids, at most ``--iters``: exact integers on the i8 matrix cores (``nn_u8.topk``) and in ``csrc/kmeans_u8.hip``, the same with
  ``--device=cpu`` and ``cuda``.  ``--bins`` is at most 256 and at most the size of the reference set.
* Statistics per bin, for generated against reference and for held-out against reference (a against b, ``p = n / N``): pooled
  ``P = (n_a + n_b) / (N_a + N_b)``, ``se = sqrt(P (1 - P) (1 / N_a + 1 / N_b))``, ``z = (p_ref - p_other) / se`` (0 where ``se == 0``), two-sided
  ``pvalue = erfc(|z| / sqrt 2)``; the bin is *different* when ``pvalue < alpha``; ``ndb`` counts the different bins, ``ndb_over_k = ndb / K``;
  ``js`` is the Jensen-Shannon divergence of the two histograms in bits, in [0, 1] and 0 for equal histograms.  The held-out pair is the
  calibration: about ``alpha * K`` different bins is what sampling noise alone gives.
* ``modes.json`` (strict JSON): the options, ``N_ref``, ``N_holdout``, ``N_gen``, ``iterations``, ``converged``, the ``inertia`` list (one entry per
  assignment pass, the last for the stored centroids), ``rms`` = sqrt(inertia / (N_ref F)), ``generated: {ndb, ndb_over_k, js}``, ``holdout: {...}``
  (null with ``--holdout=0``) and ``bins``: K entries sorted by z descending (ties by bin), each ``{bin, n_ref, n_gen, n_holdout, z, pvalue, different,
  missing}``; ``missing`` means ``n_gen == 0``.
* ``modes.npz``: ``centroids`` (uint8 [K, F]), ``ref_items``, ``ref_labels``, ``ref_d2``, ``gen_labels``, ``gen_d2``, ``holdout_items``,
  ``holdout_labels``, ``counts_ref``, ``counts_gen``, ``counts_holdout``, ``z``, ``pvalue`` (generated against reference, in bin order), ``res``,
  ``seed``.
* ``modes.png``: one row per shown bin, the ``--show`` most under-produced bins (largest z first) above the ``--show`` most over-produced (most
  negative z first).  A row is the centroid, upscaled by pixel repetition, then the ``--examples`` reference images nearest the centroid, then the
  ``--examples`` generated images nearest it (ties by item / seed), at full resolution; tiles are black where a bin has fewer images.
* ``--from=modes.npz`` reuses the stored centroids, reference labels and counts and scores another snapshot against them; ``res``, the image shape
  and ``seed`` must match, else the run is refused (``iterations``, ``converged`` and ``inertia`` are then null).

Caveats: distances are taken in pixel space; the numbers are not comparable across ``--res``, ``--bins`` or data sets; k-means depends on
``--seed``; the tool is not in the metric registry.

    python -m style_big_gan_amd.modes exp.config_dir=<dir> exp.config=<file.yaml> --snapshot=<network-snapshot-*.pt> --outdir=<dir> \\
        [--bins=100] [--res=32|none] [--num=N] [--holdout=0.2] [--alpha=0.05] [--seed=0] [--iters=30] [--show=6] [--examples=4] \\
        [--data=<folder|zip>] [--trunc=1] [--class=<idx>] [--noise-mode=const|random|none] [--device=auto|cuda|cpu] [--batch=64] [--from=<modes.npz>]
"""
import argparse
import json
import math
import os

import numpy as np
import torch

from .tool_support import (add_device_option, add_sampling_options, add_snapshot_option, check_res, class_label, config_overrides, dataset_kwargs_for,
                           device_of, generated_images, load_generator, open_dataset, reduce_images, reduce_store, require_file, save_png, tool_device)
from .torch_utils.ops import kmeans_u8, resident_set

NPZ_KEYS = ('centroids', 'ref_items', 'ref_labels', 'ref_d2', 'gen_labels', 'gen_d2', 'holdout_items', 'holdout_labels', 'counts_ref', 'counts_gen',
            'counts_holdout', 'z', 'pvalue', 'res', 'seed')


def bin_statistics(n_ref, n_other, alpha):
    """the counts of K bins in the reference set and in another set -> dict(z, pvalue, different: arrays [K]; ndb, ndb_over_k, js)"""
    n_ref, n_other = np.asarray(n_ref, dtype=np.int64), np.asarray(n_other, dtype=np.int64)
    N_ref, N_other = int(n_ref.sum()), int(n_other.sum())
    if n_ref.shape != n_other.shape or n_ref.ndim != 1 or N_ref < 1 or N_other < 1:
        raise ValueError(f'bin_statistics: two non-empty histograms over the same bins are needed, got {n_ref.shape} ({N_ref}) and {n_other.shape} ({N_other})')
    p, q = n_ref / np.float64(N_ref), n_other / np.float64(N_other)
    pooled = (n_ref + n_other) / np.float64(N_ref + N_other)
    se = np.sqrt(pooled * (1 - pooled) * (1 / np.float64(N_ref) + 1 / np.float64(N_other)))
    z = np.where(se > 0, (p - q) / np.where(se > 0, se, 1), 0.0)
    pvalue = np.array([math.erfc(abs(v) / math.sqrt(2)) for v in z.tolist()], dtype=np.float64)
    different = pvalue < alpha
    m = 0.5 * (p + q)

    def half_kl(a):
        return 0.5 * float(sum(x * math.log2(x / y) for x, y in zip(a.tolist(), m.tolist()) if x > 0))

    ndb = int(different.sum())
    return dict(z=z, pvalue=pvalue, different=different, ndb=ndb, ndb_over_k=ndb / len(z), js=min(max(half_kl(p) + half_kl(q), 0.0), 1.0))


def shown_bins(z, show):
    """-> (order, rows): all bins by z descending (ties by bin), and the bins of modes.png: the `show` most under-produced (largest z first), then the
    `show` most over-produced of the others (most negative z first)"""
    order = np.argsort(-np.asarray(z, dtype=np.float64), kind='stable')
    top = order[:max(int(show), 0)]
    rest = order[len(top):]
    return order, [int(b) for b in top] + [int(b) for b in rest[::-1][:max(int(show), 0)]]


def _nearest(labels, d2, b, count):
    """positions of the `count` members of bin b with the smallest d2, ties to the lower position"""
    members = np.nonzero(labels == b)[0]
    return members[np.argsort(d2[members], kind='stable')[:count]]


@torch.no_grad()
def mode_coverage(G, dataset, bins=100, res=32, num=None, holdout=0.2, alpha=0.05, seed=0, iters=30, show=6, examples=4, truncation_psi=1, class_idx=None,
                  noise_mode='const', batch=64, from_file=None, outdir=None, device=None, max_gib=None):
    """The bins of `dataset` (a train_parts.datasets.Dataset without x-flips) and G's samples in them -> dict with `arrays` (what modes.npz holds),
    `stats` (what modes.json holds) and `canvas` (modes.png, uint8 [rows * H, (1 + 2 examples) * W, C]).  With `outdir` the files of the module
    docstring are written.  `res=None` keeps the full size."""
    from .train_parts.dataloaders import ResidentDataloader
    bins, batch, seed, iters, show, examples = int(bins), int(batch), int(seed), int(iters), int(show), int(examples)
    holdout, alpha = float(holdout), float(alpha)
    if batch < 1:
        raise ValueError(f'--batch={batch}: must be at least 1')
    if not 0 <= holdout < 1:
        raise ValueError(f'--holdout={holdout}: must be at least 0 and below 1')
    if not 0 < alpha < 1:
        raise ValueError(f'--alpha={alpha}: must lie between 0 and 1')
    if iters < 1 or show < 0 or examples < 0:
        raise ValueError(f'--iters={iters} must be at least 1, --show={show} and --examples={examples} must not be negative')
    if num is not None and int(num) < 1:
        raise ValueError(f'--num={num}: must be at least 1')
    device = device_of(G, device)
    C, H, W = dataset.image_shape
    if (G.img_resolution, G.img_resolution) != (H, W) or getattr(G, 'img_channels', C) != C:
        raise ValueError(f'the generator makes {G.img_resolution} x {G.img_resolution} images, the data set holds {C} x {H} x {W}')
    res = check_res(res, dataset.resolution)
    r = res if res is not None else dataset.resolution
    F = C * r * r
    raw, slot, flip = resident_set.tables(dataset)
    if bool(flip.any()):
        raise ValueError('the mode coverage tool needs the data set without its x-flips (mirror off): a mirrored copy is not another sample of the data')

    # The items of both sets: every item, or those of the class.
    conditional = G.c_dim != 0
    item_labels = np.stack([dataset.get_label(i) for i in range(len(dataset))]).astype(np.float32).reshape(len(dataset), -1) if conditional else None
    items = np.arange(len(dataset), dtype=np.int64)
    if conditional and class_idx is not None:
        if item_labels.shape[1] != G.c_dim:
            raise ValueError(f'the generator takes {G.c_dim} classes, the data set has labels of width {item_labels.shape[1]}')
        items = items[item_labels.argmax(1) == int(class_idx)]
    if len(items) < 1:
        raise ValueError(f'--class={class_idx}: the data set holds no image of this class')
    rng = np.random.RandomState(seed)
    P = rng.permutation(len(items))
    n_hold = int(round(holdout * len(items)))
    hold_items, ref_items = items[P[:n_hold]], items[P[n_hold:]]

    stored = None
    if from_file is not None:
        with np.load(from_file) as f:
            stored = {k: f[k] for k in NPZ_KEYS}
        cent = stored['centroids']
        if int(stored['res']) != r or cent.ndim != 2 or cent.shape[1] != F or cent.dtype != np.uint8:
            raise ValueError(f'--from={from_file}: centroids {cent.dtype} {cent.shape} at res {int(stored["res"])} do not belong to images of {C} x {r} x {r} '
                             f'(--res={r})')
        if int(stored['seed']) != seed:
            raise ValueError(f'--from={from_file}: stored with --seed={int(stored["seed"])}, this run has --seed={seed}')
        if not (np.array_equal(stored['ref_items'], ref_items) and np.array_equal(stored['holdout_items'], hold_items)):
            raise ValueError(f'--from={from_file}: the stored split ({len(stored["ref_items"])} reference and {len(stored["holdout_items"])} held-out items) '
                             f'is not the split of this data set, --holdout={holdout} and --class={class_idx}')
        bins = cent.shape[0]
    N_ref = len(ref_items)
    if not 1 <= bins <= min(kmeans_u8.MAX_K, N_ref):
        raise ValueError(f'--bins={bins}: must be at least 1, at most {kmeans_u8.MAX_K} and at most the {N_ref} images of the reference set')
    N_gen = int(num) if num is not None else N_ref
    if outdir is not None:
        os.makedirs(outdir, exist_ok=True)

    loader = ResidentDataloader(dataset, sampler=(), batch_size=1, device=device, max_gib=max_gib)
    store = loader.store
    slot = slot.to(device).to(torch.int64)

    def rows_of(item_list):
        """the reduced images of data set items -> uint8 [n, F]"""
        return small[slot[torch.from_numpy(np.ascontiguousarray(item_list)).to(device)]].contiguous()

    small = reduce_store(store, res).reshape(store.shape[0], F)
    if stored is None:
        ref_points = rows_of(ref_items)
        fit = kmeans_u8.lloyd(ref_points, kmeans_u8.seed(ref_points, bins, rng), iters)
        centroids = fit['centroids']
        ref_labels, ref_d2 = fit['labels'].cpu().numpy(), fit['d2'].cpu().numpy()
        counts_ref = fit['counts'].cpu().numpy()
        inertia, iterations, converged = fit['inertia'], fit['iterations'], fit['converged']
        hold_labels = kmeans_u8.assign(rows_of(hold_items), centroids)[0].cpu().numpy() if n_hold else np.zeros([0], dtype=np.int32)
        counts_hold = np.bincount(hold_labels, minlength=bins).astype(np.int64)
        del ref_points
    else:
        centroids = torch.from_numpy(stored['centroids']).to(device)
        ref_labels, ref_d2, counts_ref = stored['ref_labels'], stored['ref_d2'], stored['counts_ref']
        hold_labels, counts_hold = stored['holdout_labels'], stored['counts_holdout']
        inertia, iterations, converged = None, None, None

    # The generated set, batch by batch: only labels and distances are kept.
    one_label = class_label(G, class_idx, device) if not conditional or class_idx is not None else None

    def labels_of(seeds):
        if one_label is not None:
            return one_label
        return torch.from_numpy(item_labels[ref_items[np.asarray(seeds, dtype=np.int64) % N_ref]]).to(device)

    def images_of(seeds):
        return generated_images(G, seeds, labels_of(seeds), truncation_psi, noise_mode, device)

    gen_labels, gen_d2 = [], []
    for lo in range(0, N_gen, batch):
        q = reduce_images(images_of(list(range(lo, min(lo + batch, N_gen)))), res)
        lab, d2 = kmeans_u8.assign(q.reshape(q.shape[0], F), centroids)
        gen_labels.append(lab)
        gen_d2.append(d2)
    gen_labels, gen_d2 = torch.cat(gen_labels).cpu().numpy(), torch.cat(gen_d2).cpu().numpy()
    counts_gen = np.bincount(gen_labels, minlength=bins).astype(np.int64)

    generated = bin_statistics(counts_ref, counts_gen, alpha)
    held = bin_statistics(counts_ref, counts_hold, alpha) if n_hold else None
    order, rows = shown_bins(generated['z'], show)
    arrays = dict(centroids=centroids.cpu().numpy(), ref_items=ref_items, ref_labels=ref_labels, ref_d2=ref_d2, gen_labels=gen_labels, gen_d2=gen_d2,
                  holdout_items=hold_items, holdout_labels=hold_labels, counts_ref=counts_ref, counts_gen=counts_gen, counts_holdout=counts_hold,
                  z=generated['z'], pvalue=generated['pvalue'], res=np.int64(r), seed=np.int64(seed))
    summary = lambda s: dict(ndb=s['ndb'], ndb_over_k=s['ndb_over_k'], js=s['js'])
    stats = dict(options=dict(bins=bins, res=r, num=N_gen, holdout=holdout, alpha=alpha, seed=seed, iters=iters, show=show, examples=examples,
                              trunc=float(truncation_psi), class_idx=None if class_idx is None else int(class_idx), noise_mode=noise_mode, batch=batch,
                              from_file=None if from_file is None else os.path.basename(str(from_file))),
                 N_ref=N_ref, N_holdout=n_hold, N_gen=N_gen, iterations=iterations, converged=converged, inertia=inertia,
                 rms=math.sqrt(int(ref_d2.sum()) / (N_ref * F)), generated=summary(generated), holdout=None if held is None else summary(held),
                 bins=[dict(bin=int(b), n_ref=int(counts_ref[b]), n_gen=int(counts_gen[b]), n_holdout=int(counts_hold[b]), z=float(generated['z'][b]),
                            pvalue=float(generated['pvalue'][b]), different=bool(generated['different'][b]), missing=bool(counts_gen[b] == 0))
                       for b in order.tolist()])

    # The picture: per shown bin the centroid, the nearest reference images and the nearest generated images, at full resolution.
    canvas = np.zeros([len(rows) * H, (1 + 2 * examples) * W, C], dtype=np.uint8)
    picked = [(_nearest(ref_labels, ref_d2, b, examples), _nearest(gen_labels, gen_d2, b, examples)) for b in rows]
    seeds = [int(s) for _, gen in picked for s in gen]
    made = torch.cat([images_of(seeds[lo:lo + batch]) for lo in range(0, len(seeds), batch)]).cpu().numpy() if seeds else None
    at = 0
    for row, (b, (ref, gen)) in enumerate(zip(rows, picked)):
        tiles = [centroids[b].reshape(C, r, r).repeat_interleave(H // r, 1).repeat_interleave(W // r, 2).cpu().numpy()]
        near = store[slot[torch.from_numpy(ref_items[ref]).to(device)]].cpu().numpy() if len(ref) else []
        tiles += list(near) + [None] * (examples - len(ref)) + list(made[at:at + len(gen)] if len(gen) else [])
        at += len(gen)
        for t, tile in enumerate(tiles):
            if tile is not None:
                canvas[row * H:(row + 1) * H, t * W:(t + 1) * W] = tile.transpose(1, 2, 0)
    if outdir is not None:
        np.savez(os.path.join(outdir, 'modes.npz'), **arrays)
        with open(os.path.join(outdir, 'modes.json'), 'w') as f:
            json.dump(stats, f, indent=2, allow_nan=False)
        save_png(canvas, os.path.join(outdir, 'modes.png'))
    return dict(arrays=arrays, stats=stats, canvas=canvas, rows=rows)


# ---------------------------------------------------------------------------------------------------------------- CLI

def res_option(text):
    """'none' -> None (the full size), else the resolution"""
    return None if text == 'none' else int(text)


def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.modes', description=__doc__.split('\n')[0])
    add_snapshot_option(ap)
    ap.add_argument('--outdir', required=True, help='where to save modes.json / modes.npz / modes.png')
    ap.add_argument('--bins', type=int, default=100, help=f'k-means bins, at most {kmeans_u8.MAX_K} and at most the reference set (default: 100)')
    ap.add_argument('--res', type=res_option, default=32, help='cluster box-reduced copies of this resolution, a power of two; none: the full size (default: 32)')
    ap.add_argument('--num', type=int, help='generated images, seeds 0..N-1 (default: the size of the reference set)')
    ap.add_argument('--holdout', type=float, default=0.2, help='share of the data held out as the calibration; 0 skips it (default: 0.2)')
    ap.add_argument('--alpha', type=float, default=0.05, help='significance level of the per-bin test (default: 0.05)')
    ap.add_argument('--seed', type=int, default=0, help='seed of the split and of the k-means++ seeding (default: 0)')
    ap.add_argument('--iters', type=int, default=30, help='Lloyd iterations at most (default: 30)')
    ap.add_argument('--show', type=int, default=6, help='under- and over-produced bins shown in modes.png, each (default: 6)')
    ap.add_argument('--examples', type=int, default=4, help='reference and generated images per shown bin, each (default: 4)')
    ap.add_argument('--data', help='data set to cluster, folder or zip (default: the run\'s data.dataset_path)')
    add_sampling_options(ap)
    add_device_option(ap)
    ap.add_argument('--batch', type=int, default=64, help='images generated and assigned at a time (default: 64)')
    ap.add_argument('--from', dest='from_file', help='a modes.npz: score this snapshot against its stored bins')
    args, rest = ap.parse_known_args(argv)
    if not 1 <= args.bins <= kmeans_u8.MAX_K:
        ap.error(f'--bins must be between 1 and {kmeans_u8.MAX_K}')
    if args.res is not None and (args.res < 4 or args.res & (args.res - 1)):
        ap.error('--res must be a power of two, at least 4, or none')
    if args.num is not None and args.num < 1:
        ap.error('--num must be at least 1')
    if not 0 <= args.holdout < 1:
        ap.error('--holdout must be at least 0 and below 1')
    if not 0 < args.alpha < 1:
        ap.error('--alpha must lie between 0 and 1')
    if args.iters < 1:
        ap.error('--iters must be at least 1')
    if args.show < 0 or args.examples < 0:
        ap.error('--show and --examples must not be negative')
    if args.batch < 1:
        ap.error('--batch must be at least 1')
    require_file(ap, '--snapshot', args.snapshot)
    require_file(ap, '--from', args.from_file)
    return config_overrides(ap, rest), args


def run_modes(argv=None):
    overrides, args = parse_args(argv)
    from . import arguments
    config = arguments.load_config(overrides)
    device = tool_device(args.device)
    G = load_generator(config, args.snapshot, device)
    kw = dataset_kwargs_for(config, G, data=args.data, mirror=False)
    with open_dataset(config, kw) as dataset:
        result = mode_coverage(G, dataset, bins=args.bins, res=args.res, num=args.num, holdout=args.holdout, alpha=args.alpha, seed=args.seed, iters=args.iters,
                               show=args.show, examples=args.examples, truncation_psi=args.truncation_psi, class_idx=args.class_idx,
                               noise_mode=args.noise_mode, batch=args.batch, from_file=args.from_file, outdir=args.outdir, device=device)
    print(json.dumps({k: v for k, v in result['stats'].items() if k != 'bins'}, allow_nan=False))
    return result


if __name__ == '__main__':
    run_modes()
