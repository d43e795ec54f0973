"""The scores computed from feature statistics: Frechet distance (FID), kernel distance (KID), Inception score (IS), improved
precision / recall (PR) and, beyond the reference, density / coverage (PRDC: Naeem et al., "Reliable Fidelity and Diversity Metrics
for Generative Models", ICML 2020), the per-image realism score of the improved precision / recall paper (`realism_scores`) and the detector-free sliced Wasserstein distance on Laplacian-pyramid patches (SWD: Karras et al.,
"Progressive Growing of GANs", ICLR 2018, section 5; the last part of this file).  Arithmetic of the reference's ``stylegan2ada/metrics/{frechet_inception_distance, kernel_inception_distance,
inception_score, precision_recall}.py``; each function cites the lines it follows.  Detector names are the reference's file names; the
files themselves are never fetched (see metric_utils.get_feature_detector)."""
import numpy as np
import scipy.linalg
import torch

from ..torch_utils.ops import knn_manifold
from ..torch_utils.ops import swd as swd_ops
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


def pruned_radii(radius, keep):
    """fp16 radii [N] -> the same with all but the ceil(keep * N) smallest set to -1: the realism score's pruning of the balls that reach
    too far.  Among equal radii the lower index is kept (a stable sort of the fp16 values)."""
    n = radius.shape[0]
    num_keep = int(np.ceil(keep * n))
    order = torch.sort(radius.to(torch.float32), stable=True).indices
    out = torch.full_like(radius, -1)
    out[order[:num_keep]] = radius[order[:num_keep]]
    return out


def realism_scores(real_features, gen_features, nhood_size=3, keep=0.5, row_batch_size=10000, leave_one_out=False):
    """The realism score of every generated feature (Kynkaanniemi et al., NeurIPS 2019, section 5):
    R(g) = max_r radius_k(r) / |g - r| over the real features whose k-NN radius (self-distance included, as for precision) is among the
    ceil(keep N) smallest.  -> (score fp32 [M], item int32 [M]: the real feature attaining it, radius_kept fp16 [N]: -1 where pruned);
    with `leave_one_out` also (real_score [N], real_item [N]): every real feature against the kept balls of the others, its own
    excluded -- the baseline the generated scores are read against.  One process; `knn_manifold.realism` on either device."""
    radius = realism_radii(real_features, nhood_size, keep, row_batch_size)
    out = realism_sweep(gen_features, real_features, radius, row_batch_size) + (radius,)
    if leave_one_out:
        out = out + realism_sweep(real_features, real_features, radius, row_batch_size, own=True)
    return out


def realism_radii(real_features, nhood_size=3, keep=0.5, row_batch_size=10000):
    """the kept balls of `realism_scores`: fp16 [N], the k-NN radius of every real feature, -1 where pruned"""
    if not 0 < keep <= 1:
        raise ValueError(f'realism_scores: keep = {keep} must lie in (0, 1]')
    return pruned_radii(_radii_fused(real_features, nhood_size, row_batch_size, 1, 0), keep)


def realism_sweep(probes, real_features, radius_kept, row_batch_size=10000, own=False):
    """`knn_manifold.realism` of `probes` in row batches -> (score fp32 [P], item int32 [P]); `own`: probe i is real feature i, whose
    own ball is left out"""
    device = real_features.device
    score, item = [], []
    for lo in range(0, probes.shape[0], row_batch_size):
        hi = min(lo + row_batch_size, probes.shape[0])
        exclude = torch.arange(lo, hi, dtype=torch.int32, device=device) if own else None
        s, i = knn_manifold.realism(probes[lo:hi], real_features, radius_kept, exclude)
        score.append(s)
        item.append(i)
    if not score:
        return torch.empty([0], dtype=torch.float32, device=device), torch.empty([0], dtype=torch.int32, device=device)
    return torch.cat(score), torch.cat(item)


# ------------------------------------------------------------------------------------------------------------------------------
# Sliced Wasserstein distance on Laplacian-pyramid patches.  Constants of the published `swd-16k`.

SWD_NHOOD_SIZE = 7
SWD_NHOODS_PER_IMAGE = 128
SWD_DIR_REPEATS = 4
SWD_DIRS_PER_REPEAT = 128
SWD_MIN_RES = 16
SWD_DIR_CHUNK = 32          # directions projected, sorted and compared at a time: bounds the sort's index tensor at 8 bytes * 32 * M


def swd_resolutions(resolution):
    """level sides R, R/2, ..., 16; a resolution that is not a power of two >= 16 is refused"""
    resolution = int(resolution)
    if resolution < SWD_MIN_RES or resolution & (resolution - 1):
        raise ValueError(f'swd: resolution {resolution} is not a power of two >= {SWD_MIN_RES}')
    return [resolution >> i for i in range(resolution.bit_length() - SWD_MIN_RES.bit_length() + 1)]


def swd_tables(seed, num_images, resolution, channels, nhoods_per_image=SWD_NHOODS_PER_IMAGE, num_dirs=SWD_DIR_REPEATS * SWD_DIRS_PER_REPEAT,
               z_dim=None, num_labels=None):
    """every random number of one evaluation, drawn on the host from ONE numpy.random.RandomState(seed) in this order:
      1. directions   randn(49 C, num_dirs) float64, each column divided by its l2 norm, cast to float32 (columns 128 r .. of repeat r)
      2. centres      per level, largest first: randint(3, S - 3, [N, nhoods_per_image, 2]) = (y, x); image i of BOTH sets uses row i
      3. latents      randn(N, z_dim)                  (when z_dim is given)
      4. label items  randint(num_labels, size=N)      (when num_labels is given): generated image i takes the label of that data-set item
    so nothing depends on the image batch size or on the number of ranks."""
    rs = np.random.RandomState(seed)
    dirs = rs.randn(channels * swd_ops.PP, num_dirs)
    dirs /= np.sqrt(np.sum(np.square(dirs), axis=0, keepdims=True))
    tables = dict(dirs=dirs.astype(np.float32),
                  centres=[rs.randint(3, s - 3, size=[num_images, nhoods_per_image, 2]).astype(np.int32) for s in swd_resolutions(resolution)])
    if z_dim is not None:
        tables['z'] = rs.randn(num_images, z_dim).astype(np.float32)
    if num_labels is not None:
        tables['label_items'] = rs.randint(num_labels, size=num_images)
    return tables


class SwdDescriptors:
    """the descriptor matrices [128 N, 49 C] of one image set, one per pyramid level, filled batch by batch: only they persist"""

    def __init__(self, num_images, resolution, channels, centres, device):
        self.resolutions = swd_resolutions(resolution)
        assert len(centres) == len(self.resolutions) and all(c.shape[0] == num_images and c.shape[2] == 2 for c in centres)
        self.num_images, self.channels, self.device = num_images, channels, torch.device(device)
        self.centres = [torch.as_tensor(c, dtype=torch.int32).to(self.device) for c in centres]
        self.desc = [torch.zeros([num_images * c.shape[1], channels * swd_ops.PP], dtype=torch.float32, device=self.device) for c in self.centres]

    def add(self, start, images):
        """images [B, C, R, R], byte values (uint8 or float), are images start .. start + B - 1 of the set"""
        b = images.shape[0]
        assert 0 <= start and start + b <= self.num_images and tuple(images.shape[1:]) == (self.channels, self.resolutions[0], self.resolutions[0])
        x = images.to(self.device).to(torch.float32).contiguous()
        for level, centres, desc in zip(swd_ops.laplacian_pyramid(x, len(self.resolutions)), self.centres, self.desc):
            swd_ops.gather_descriptors(level, centres[start:start + b].contiguous(), desc, row_offset=start * centres.shape[1])

    def exchange(self, num_gpus):
        """every rank filled the rows of its own images into zeros: one sum per level completes all of them (x + 0 is exact)"""
        if num_gpus > 1:
            for desc in self.desc:
                torch.distributed.all_reduce(desc)
        return self.desc


def swd_normalisation(desc, channels, what='descriptors'):
    """(s, t) fp32 [C] on desc's device with x_hat = fmaf(x, s_c, t_c): s_c = float32(1 / std), t_c = float32(-mean / std), mean and
    population std of channel c over all M * 49 values from the float64 sum and sum of squares of `channel_moments`"""
    sums = swd_ops.channel_moments(desc, channels).cpu().numpy()
    n = float(desc.shape[0] * swd_ops.PP)
    s, t = np.zeros([channels], dtype=np.float32), np.zeros([channels], dtype=np.float32)
    for c in range(channels):
        mean = sums[c, 0] / n
        with np.errstate(all='ignore'):
            std = np.sqrt(sums[c, 1] / n - mean * mean)
        if not np.isfinite(std) or not std > 0 or not np.isfinite(mean):
            raise ValueError(f'swd: {what}, channel {c}: standard deviation {std} (a constant or non-finite channel has no normalised descriptors)')
        s[c], t[c] = np.float32(1.0 / std), np.float32(-mean / std)
    return torch.from_numpy(s).to(desc.device), torch.from_numpy(t).to(desc.device)


def swd_direction_distances(real_desc, fake_desc, dirs, lo=0, hi=None, what='level', dir_chunk=SWD_DIR_CHUNK):
    """D_d = sum_m |sort(p_real[:, d])_m - sort(p_fake[:, d])_m| for the directions lo <= d < hi of dirs fp32 [K, D] -> float64 [hi - lo]
    on the host.  Projection, sort (torch.sort along the contiguous axis of the direction-major projections) and the fixed-order float64
    sum (`sorted_l1`) run in chunks of `dir_chunk` directions; a direction's D_d does not depend on the chunking."""
    assert real_desc.shape == fake_desc.shape and real_desc.device == fake_desc.device
    channels = real_desc.shape[1] // swd_ops.PP
    dirs = torch.as_tensor(dirs, dtype=torch.float32).to(real_desc.device)
    hi = dirs.shape[1] if hi is None else hi
    norm = [swd_normalisation(desc, channels, f'{name} set, {what}') for name, desc in (('real', real_desc), ('generated', fake_desc))]
    out = []
    for a in range(lo, hi, dir_chunk):
        b = min(a + dir_chunk, hi)
        proj = [torch.sort(swd_ops.project(desc, s, t, dirs[:, a:b]), dim=1).values for desc, (s, t) in zip((real_desc, fake_desc), norm)]
        out.append(swd_ops.sorted_l1(proj[0], proj[1]).cpu())
    return torch.cat(out) if out else torch.zeros([0], dtype=torch.float64)


def swd_score(dists, rows, dir_repeats, dirs_per_repeat):
    """1e3 * mean_r(mean_{d in r}(D_d / M)) in float64, the directions of a repeat added left to right, then the repeats left to right"""
    dists = [float(v) for v in dists]
    assert len(dists) == dir_repeats * dirs_per_repeat
    total = 0.0
    for r in range(dir_repeats):
        acc = 0.0
        for d in range(r * dirs_per_repeat, (r + 1) * dirs_per_repeat):
            acc += dists[d] / rows
        total += acc / dirs_per_repeat
    return 1e3 * (total / dir_repeats)


def sliced_wasserstein(real_desc, fake_desc, dirs, dir_repeats=SWD_DIR_REPEATS, dirs_per_repeat=SWD_DIRS_PER_REPEAT, what='level', num_gpus=1, rank=0,
                       dir_chunk=SWD_DIR_CHUNK):
    """the score of one level from its two descriptor matrices [M, 49 C] (every rank holds both).  The directions are dealt to the ranks in
    contiguous shares (`_rank_share`), the D_d exchanged with one all_gather and added in direction order; every rank returns the number."""
    assert 0 <= rank < num_gpus
    num_dirs = dir_repeats * dirs_per_repeat
    lo, hi = _rank_share(num_dirs, num_gpus, rank)
    dists = swd_direction_distances(real_desc, fake_desc, dirs, lo, hi, what=what, dir_chunk=dir_chunk)
    if num_gpus > 1:        # shares differ by at most one direction: pad to the largest, gather once, cut the pads
        longest = -(-num_dirs // num_gpus)
        mine = torch.nn.functional.pad(dists, [0, longest - dists.shape[0]]).to(real_desc.device)
        parts = [torch.empty_like(mine) for _ in range(num_gpus)]
        torch.distributed.all_gather(parts, mine)
        dists = torch.cat([part[:b - a].cpu() for part, (a, b) in zip(parts, (_rank_share(num_dirs, num_gpus, r) for r in range(num_gpus)))])
    return swd_score(dists, real_desc.shape[0], dir_repeats, dirs_per_repeat)


def compute_swd(opts, num_images, dataset_name='image_folder', seed=0, batch_size=64, batch_gen=None, data_loader_kwargs=None,
                nhoods_per_image=SWD_NHOODS_PER_IMAGE, dir_repeats=SWD_DIR_REPEATS, dirs_per_repeat=SWD_DIRS_PER_REPEAT):
    """-> {level side: score}.  N = min(num_images, len(dataset)) real images (items 0 .. N - 1) against N generated ones, quantised to
    uint8 as `compute_feature_stats_for_generator` does, latents and labels from `swd_tables`.  Images stream through in batches; rank r
    renders and reads the images of its contiguous share and the descriptor rows are exchanged once per set."""
    import copy
    from ..train_parts.datasets import datasets
    dataset = datasets[dataset_name](**opts.dataset_kwargs)
    resolution, channels = int(dataset.resolution), int(dataset.num_channels)
    resolutions = swd_resolutions(resolution)
    if channels not in (1, 3):
        raise ValueError(f'swd: {channels} image channels; 1 or 3 are supported')
    n = min(int(num_images), len(dataset))
    if n < 1:
        raise ValueError('swd: the data set is empty')
    G = copy.deepcopy(opts.G).eval().requires_grad_(False).to(opts.device)
    c_dim = G.c_dim or 0
    tables = swd_tables(seed, n, resolution, channels, nhoods_per_image, dir_repeats * dirs_per_repeat, z_dim=G.z_dim, num_labels=len(dataset))
    lo, hi = _rank_share(n, opts.num_gpus, opts.rank)
    if batch_gen is None:
        batch_gen = min(batch_size, 4)
    if data_loader_kwargs is None:
        data_loader_kwargs = dict(pin_memory=(torch.device(opts.device).type == 'cuda'), num_workers=3, prefetch_factor=2)

    real = SwdDescriptors(n, resolution, channels, tables['centres'], opts.device)
    progress = opts.progress.sub(tag='dataset patches', num_items=n, rel_lo=0, rel_hi=0.3)
    start = lo
    if hi > lo:
        for images, _labels in torch.utils.data.DataLoader(dataset=dataset, sampler=range(lo, hi), batch_size=batch_size, **data_loader_kwargs):
            real.add(start, images)
            start += images.shape[0]
            progress.update(start - lo)
    fake = SwdDescriptors(n, resolution, channels, tables['centres'], opts.device)
    progress = opts.progress.sub(tag='generator patches', num_items=n, rel_lo=0.3, rel_hi=0.6)
    with torch.no_grad():
        for start in range(lo, hi, batch_gen):
            stop = min(start + batch_gen, hi)
            z = torch.from_numpy(tables['z'][start:stop]).to(opts.device)
            if c_dim:
                c = torch.from_numpy(np.stack([dataset.get_label(int(i)) for i in tables['label_items'][start:stop]])).to(opts.device)
            else:
                c = torch.zeros([stop - start, 0], device=opts.device)
            img = G(z, c, **opts.G_kwargs)
            fake.add(start, (img * 127.5 + 128).clamp(0, 255).to(torch.uint8))
            progress.update(stop - lo)
    real_desc, fake_desc = real.exchange(opts.num_gpus), fake.exchange(opts.num_gpus)
    results = dict()
    for i, res in enumerate(resolutions):
        results[res] = sliced_wasserstein(real_desc[i], fake_desc[i], tables['dirs'], dir_repeats, dirs_per_repeat, what=f'level {res}x{res}',
                                          num_gpus=opts.num_gpus, rank=opts.rank)
        real_desc[i] = fake_desc[i] = None      # a level's matrices are dropped once it is scored
    return results
