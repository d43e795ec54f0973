"""The scores computed from feature statistics: Frechet distance (FID), kernel distance (KID), Inception score (IS), improved
precision / recall (PR) and, beyond the reference, density / coverage (PRDC: Naeem et al., "Reliable Fidelity and Diversity Metrics
for Generative Models", ICML 2020).  Arithmetic of the reference's ``stylegan2ada/metrics/{frechet_inception_distance, kernel_inception_distance,
inception_score, precision_recall}.py``; each function cites the lines it follows.  Detector names are the reference's file names; the
files themselves are never fetched (see metric_utils.get_feature_detector)."""
import numpy as np
import scipy.linalg
import torch

from ..torch_utils.ops import knn_manifold
from . import metric_utils

INCEPTION = 'inception-2015-12-05.pt'      # reference: nvlabs-fi-cdn URL / './inception-2015-12-05.pt' (frechet_inception_distance.py:22-23)
VGG16 = 'vgg16.pt'                          # reference: precision_recall.py:37


def frechet_distance(mu_a, sigma_a, mu_b, sigma_b):
    """|mu_a - mu_b|^2 + tr(S_a + S_b - 2 (S_a S_b)^(1/2))   (frechet_inception_distance.py:42-44)"""
    m = np.square(mu_a - mu_b).sum()
    s, _ = scipy.linalg.sqrtm(np.dot(sigma_a, sigma_b), disp=False)
    return float(np.real(m + np.trace(sigma_a + sigma_b - s * 2)))


def compute_fid(opts, max_real, num_gen, dataset_name='image_folder'):
    kw = metric_utils.detector_call_kwargs(opts, INCEPTION, dict(return_features=True))
    mu_real, sigma_real = metric_utils.compute_feature_stats_for_dataset(
        opts=opts, detector_url=INCEPTION, detector_kwargs=kw, rel_lo=0, rel_hi=0, capture_mean_cov=True, max_items=max_real,
        dataset_name=dataset_name).get_mean_cov()
    mu_gen, sigma_gen = metric_utils.compute_feature_stats_for_generator(
        opts=opts, detector_url=INCEPTION, detector_kwargs=kw, rel_lo=0, rel_hi=1, capture_mean_cov=True, max_items=num_gen,
        dataset_name=dataset_name).get_mean_cov()
    if opts.rank != 0:
        return float('nan')
    return frechet_distance(mu_gen, sigma_gen, mu_real, sigma_real)


def kernel_distance(real_features, gen_features, num_subsets, max_subset_size, rng=np.random):
    """unbiased MMD^2 estimate with the cubic polynomial kernel (x.y / n + 1)^3, averaged over random subsets
    (kernel_inception_distance.py:32-43; subsets are drawn generated-first, then real, from `rng`)"""
    n = real_features.shape[1]
    m = min(min(real_features.shape[0], gen_features.shape[0]), max_subset_size)
    t = 0
    for _ in range(num_subsets):
        x = gen_features[rng.choice(gen_features.shape[0], m, replace=False)]
        y = real_features[rng.choice(real_features.shape[0], m, replace=False)]
        a = (x @ x.T / n + 1) ** 3 + (y @ y.T / n + 1) ** 3
        b = (x @ y.T / n + 1) ** 3
        t += (a.sum() - np.diag(a).sum()) / (m - 1) - b.sum() * 2 / m
    return float(t / num_subsets / m)


def compute_kid(opts, max_real, num_gen, num_subsets, max_subset_size, dataset_name='image_folder'):
    kw = metric_utils.detector_call_kwargs(opts, INCEPTION, dict(return_features=True))
    real = metric_utils.compute_feature_stats_for_dataset(opts=opts, dataset_name=dataset_name, detector_url=INCEPTION, detector_kwargs=kw,
                                                          rel_lo=0, rel_hi=0, capture_all=True, max_items=max_real).get_all()
    gen = metric_utils.compute_feature_stats_for_generator(opts=opts, dataset_name=dataset_name, detector_url=INCEPTION, detector_kwargs=kw,
                                                           rel_lo=0, rel_hi=1, capture_all=True, max_items=num_gen).get_all()
    if opts.rank != 0:
        return float('nan')
    return kernel_distance(real, gen, num_subsets, max_subset_size)


def inception_score(gen_probs, num_splits):
    """exp(E_x KL(p(y|x) || p(y))) per split -> (mean, std) over the splits (inception_score.py:30-36)"""
    num_gen = gen_probs.shape[0]
    scores = []
    for i in range(num_splits):
        part = gen_probs[i * num_gen // num_splits:(i + 1) * num_gen // num_splits]
        kl = part * (np.log(part) - np.log(np.mean(part, axis=0, keepdims=True)))
        scores.append(np.exp(np.mean(np.sum(kl, axis=1))))
    return float(np.mean(scores)), float(np.std(scores))


def compute_is(opts, num_gen, num_splits, dataset_name='image_folder'):
    kw = metric_utils.detector_call_kwargs(opts, INCEPTION, dict(no_output_bias=True))
    probs = metric_utils.compute_feature_stats_for_generator(opts=opts, dataset_name=dataset_name, detector_url=INCEPTION, detector_kwargs=kw,
                                                             capture_all=True, max_items=num_gen).get_all()
    if opts.rank != 0:
        return float('nan'), float('nan')
    return inception_score(probs, num_splits)


def pairwise_distances(row_features, col_features, num_gpus, rank, col_batch_size):
    """[rows, cols] Euclidean distances, the column batches dealt round-robin to the ranks and gathered on rank 0
    (precision_recall.py:16-29)"""
    assert 0 <= rank < num_gpus
    num_cols = col_features.shape[0]
    num_batches = ((num_cols - 1) // col_batch_size // num_gpus + 1) * num_gpus
    col_batches = torch.nn.functional.pad(col_features, [0, 0, 0, -num_cols % num_batches]).chunk(num_batches)
    out = []
    for col_batch in col_batches[rank::num_gpus]:
        dist = torch.cdist(row_features.unsqueeze(0), col_batch.unsqueeze(0))[0]
        if num_gpus > 1:
            parts = [torch.empty_like(dist) for _ in range(num_gpus)]
            torch.distributed.all_gather(parts, dist.contiguous())
        else:
            parts = [dist]
        if rank == 0:
            out.extend(p.cpu() for p in parts)
    return torch.cat(out, dim=1)[:, :num_cols] if rank == 0 else None


def precision_recall(real_features, gen_features, nhood_size, row_batch_size, col_batch_size, num_gpus=1, rank=0):
    """precision = share of generated features inside the union of k-NN balls of the real ones; recall = the converse
    (precision_recall.py:48-60).  Features come in as the caller's dtype (the reference casts to fp16 on the device)."""
    results = dict()
    for name, manifold, probes in [('precision', real_features, gen_features), ('recall', gen_features, real_features)]:
        kth = []
        for manifold_batch in manifold.split(row_batch_size):
            dist = pairwise_distances(manifold_batch, manifold, num_gpus, rank, col_batch_size)
            kth.append(dist.to(torch.float32).kthvalue(nhood_size + 1).values.to(manifold.dtype) if rank == 0 else None)
        kth = torch.cat(kth) if rank == 0 else None
        pred = []
        for probes_batch in probes.split(row_batch_size):
            dist = pairwise_distances(probes_batch, manifold, num_gpus, rank, col_batch_size)
            pred.append((dist <= kth).any(dim=1) if rank == 0 else None)
        results[name] = float(torch.cat(pred).to(torch.float32).mean()) if rank == 0 else float('nan')
    return results['precision'], results['recall']


def _rank_share(n, num_gpus, rank):
    """contiguous share [lo, hi) of n rows for `rank`; the shares differ by at most one row"""
    return n * rank // num_gpus, n * (rank + 1) // num_gpus


def precision_recall_fused(real_features, gen_features, nhood_size, row_batch_size, num_gpus=1, rank=0):
    """`precision_recall` on the fused k-NN ops (torch_utils/ops/knn_manifold.py): the distance matrix is never stored and nothing
    crosses to the host but the two counts.  Every rank holds all features; it computes the radii of a contiguous share of the
    manifold rows and the membership of a contiguous share of the probe rows, the radii are exchanged with one all_gather and
    the membership counts with one all_reduce per direction, and every rank returns the numbers."""
    assert 0 <= rank < num_gpus
    results = dict()
    for name, manifold, probes in [('precision', real_features, gen_features), ('recall', gen_features, real_features)]:
        lo, hi = _rank_share(manifold.shape[0], num_gpus, rank)
        kth = [knn_manifold.kth_radius(batch, manifold, nhood_size) for batch in manifold[lo:hi].split(row_batch_size)]
        kth = torch.cat(kth) if kth else torch.empty([0], dtype=torch.float16, device=manifold.device)
        if num_gpus > 1:        # shares differ by at most one row: pad to the largest, gather once, cut the pads
            longest = -(-manifold.shape[0] // num_gpus)
            parts = [torch.empty([longest], dtype=kth.dtype, device=kth.device) for _ in range(num_gpus)]
            torch.distributed.all_gather(parts, torch.nn.functional.pad(kth, [0, longest - kth.shape[0]]))
            kth = torch.cat([part[:b - a] for part, (a, b) in zip(parts, (_rank_share(manifold.shape[0], num_gpus, r) for r in range(num_gpus)))])
        lo, hi = _rank_share(probes.shape[0], num_gpus, rank)
        count = torch.zeros([], dtype=torch.int64, device=probes.device)
        for batch in probes[lo:hi].split(row_batch_size):
            count += knn_manifold.in_manifold(batch, manifold, kth).sum()
        if num_gpus > 1:
            torch.distributed.all_reduce(count)
        results[name] = float(count.to(torch.float32) / probes.shape[0])       # the fp32 mean of the reference's 0 / 1 vector
    return results['precision'], results['recall']


def compute_pr(opts, max_real, num_gen, nhood_size, row_batch_size, col_batch_size, dataset_name='image_folder'):
    kw = metric_utils.detector_call_kwargs(opts, VGG16, dict(return_features=True))
    half = torch.float16 if torch.device(opts.device).type == 'cuda' else torch.float32
    real = metric_utils.compute_feature_stats_for_dataset(opts=opts, dataset_name=dataset_name, detector_url=VGG16, detector_kwargs=kw, rel_lo=0, rel_hi=0,
                                                          capture_all=True, max_items=max_real).get_all_torch().to(half).to(opts.device)
    gen = metric_utils.compute_feature_stats_for_generator(opts=opts, dataset_name=dataset_name, detector_url=VGG16, detector_kwargs=kw, rel_lo=0, rel_hi=1,
                                                           capture_all=True, max_items=num_gen).get_all_torch().to(half).to(opts.device)
    if torch.device(opts.device).type == 'cuda':      # fused HIP kernels; the CPU keeps the reference's cdist / kthvalue structure
        return precision_recall_fused(real, gen, nhood_size, row_batch_size, opts.num_gpus, opts.rank)
    return precision_recall(real, gen, nhood_size, row_batch_size, col_batch_size, opts.num_gpus, opts.rank)


def _radii_fused(features, nhood_size, row_batch_size, num_gpus, rank):
    """k-NN radii of all rows of `features` on every rank: each computes a contiguous share, one all_gather exchanges them"""
    n = features.shape[0]
    lo, hi = _rank_share(n, num_gpus, rank)
    kth = [knn_manifold.kth_radius(batch, features, nhood_size) for batch in features[lo:hi].split(row_batch_size)]
    kth = torch.cat(kth) if kth else torch.empty([0], dtype=torch.float16, device=features.device)
    if num_gpus > 1:        # shares differ by at most one row: pad to the largest, gather once, cut the pads
        longest = -(-n // num_gpus)
        parts = [torch.empty([longest], dtype=kth.dtype, device=kth.device) for _ in range(num_gpus)]
        torch.distributed.all_gather(parts, torch.nn.functional.pad(kth, [0, longest - kth.shape[0]]))
        kth = torch.cat([part[:b - a] for part, (a, b) in zip(parts, (_rank_share(n, num_gpus, r) for r in range(num_gpus)))])
    return kth


def prdc_fused(real_features, gen_features, nhood_size, row_batch_size, num_gpus=1, rank=0):
    """(precision, recall, density, coverage) in the four sweeps that `precision_recall_fused` takes for the first two.  With
    r_X, r_Y the k-NN radii of the real features X [N, F] and the generated ones Y [M, F] (self-distance included), count and nearest
    of `knn_manifold.probe`, (cA, _) = probe(Y, X, r_X) and (cB, nB) = probe(X, Y, r_Y):
        precision = mean(cA > 0)         recall   = mean(cB > 0)         as `precision_recall_fused` for this k, bit for bit
        density   = sum(cA) / (k M)      coverage = mean(nB <= r_X)      the nearest generated point of real i lies within its radius
    All comparisons are `<=` on the fp16 distances, the convention of `in_manifold`; the published code compares with `<`, which
    differs on exact ties only.  Ranks as in `precision_recall_fused`: every rank holds all features, computes the radii of a
    contiguous share (one all_gather per direction) and probes a contiguous share of the rows; the three integer totals of a
    direction (rows with count > 0, sum of counts, rows covered) are int64 and go through one all_reduce; nothing else reaches the
    host, and every rank returns the numbers."""
    assert 0 <= rank < num_gpus
    radius_real = _radii_fused(real_features, nhood_size, row_batch_size, num_gpus, rank)
    radius_gen = _radii_fused(gen_features, nhood_size, row_batch_size, num_gpus, rank)
    totals = []
    for probes, manifold, radius, own_radius in [(gen_features, real_features, radius_real, None), (real_features, gen_features, radius_gen, radius_real)]:
        lo, hi = _rank_share(probes.shape[0], num_gpus, rank)
        total = torch.zeros([3], dtype=torch.int64, device=probes.device)
        for start in range(lo, hi, row_batch_size):
            stop = min(start + row_batch_size, hi)
            count, nearest = knn_manifold.probe(probes[start:stop], manifold, radius)
            total[0] += (count > 0).sum()
            total[1] += count.sum(dtype=torch.int64)
            if own_radius is not None:
                total[2] += (nearest <= own_radius[start:stop]).sum()
        if num_gpus > 1:
            torch.distributed.all_reduce(total)
        totals.append(total.tolist())
    (in_real, balls, _), (in_gen, _, covered) = totals
    num_real, num_gen = real_features.shape[0], gen_features.shape[0]
    precision, recall = (float(np.float32(hits) / np.float32(n)) for hits, n in [(in_real, num_gen), (in_gen, num_real)])   # the fp32 mean of a 0 / 1 vector
    return precision, recall, balls / (nhood_size * num_gen), covered / num_real


def compute_prdc(opts, max_real, num_gen, nhood_size, row_batch_size, dataset_name='image_folder'):
    kw = metric_utils.detector_call_kwargs(opts, VGG16, dict(return_features=True))
    half = torch.float16 if torch.device(opts.device).type == 'cuda' else torch.float32
    real = metric_utils.compute_feature_stats_for_dataset(opts=opts, dataset_name=dataset_name, detector_url=VGG16, detector_kwargs=kw, rel_lo=0, rel_hi=0,
                                                          capture_all=True, max_items=max_real).get_all_torch().to(half).to(opts.device)
    gen = metric_utils.compute_feature_stats_for_generator(opts=opts, dataset_name=dataset_name, detector_url=VGG16, detector_kwargs=kw, rel_lo=0, rel_hi=1,
                                                           capture_all=True, max_items=num_gen).get_all_torch().to(half).to(opts.device)
    return prdc_fused(real, gen, nhood_size, row_batch_size, opts.num_gpus, opts.rank)       # the kernels on the device, the op layer's torch path on the CPU
