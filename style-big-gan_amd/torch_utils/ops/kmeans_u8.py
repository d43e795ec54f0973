"""k-means on uint8 rows with byte centroids, in exact integers (csrc/kmeans_u8.hip; the clustering behind ``modes.py``).
Every function has ONE definition for both devices: device tensors run the HIP kernels, CPU tensors run the same integer definition in torch --
the results are equal, not close.

    assign(points, centroids)      uint8 [N, F], uint8 [K, F] -> (label int32 [N], d2 int64 [N]): the nearest centre of every row and the exact
                                   squared distance sum_f (points[n, f] - centroids[k, f])^2; a tie goes to the lower centre.  This is
                                   ``nn_u8.topk(points, centroids, 1)`` unpacked (the i8 matrix cores on the device).
    update(points, labels, centroids)
                                   -> (new_centroids uint8 [K, F], counts int64 [K], sums int64 [K, F]): counts[k] = rows with label k,
                                   sums[k, f] = their int64 column sums, new_centroids[k, f] = (2 sums[k, f] + counts[k]) // (2 counts[k]), the
                                   mean rounded half up; an empty cluster keeps its old row and has a sums row of 0.
    seed(points, K, rng)           k-means++ in exact integers -> uint8 [K, F].  Centre 0 is row ``rng.randint(N)``; for each further centre,
                                   best = minimum(best, d2 to the newest centre), total = best.sum() as a Python int,
                                   r = (int(rng.random_sample() * 2**53) * total) >> 53, and the new centre is the first row whose int64
                                   cumsum(best) exceeds r.  total == 0 (fewer than K distinct rows) raises with that count.  ``rng`` is a
                                   ``numpy.random.RandomState``; one host synchronisation per centre.
    lloyd(points, centroids, max_iter)
                                   assign, then update, until the centroids do not change (``converged``) or ``max_iter`` iterations are done; ends
                                   with an assign against the returned centroids (the last iteration's own when it converged) -> dict(centroids,
                                   labels, d2, counts, inertia, iterations, converged).  ``inertia`` lists sum(d2) of every assign made as Python
                                   ints, so its last entry belongs to the returned centroids.  Byte centroids are a deliberate departure from
                                   real-valued k-means: a centre is off by at most half a grey level per value, every distance is an exact integer
                                   and both devices agree; the objective is then not guaranteed to fall monotonically, hence ``max_iter``.

``update`` refuses a wrong dtype, a non-dense tensor, mixed devices, a label outside [0, K) and sizes outside 1 <= N <= 2^24, 1 <= K <= 256,
F a multiple of 16 and at most 3 * 2^20 (on the CPU any F >= 1) with a message that names shapes, dtypes and devices.
"""
import numpy as np
import torch

from ... import _lib
from . import nn_u8

MAX_K = 256                     # csrc/kmeans_u8.hip
MAX_ROWS = nn_u8.MAX_ROWS
MAX_F = nn_u8.MAX_F
_CPU_BYTES = 1 << 26            # int64 work set of one row block of the CPU update


def _describe(**tensors):
    return ", ".join(f"{name} {str(t.dtype).replace('torch.', '')} {tuple(t.shape)} on {t.device}" if isinstance(t, torch.Tensor) else f"{name} {type(t).__name__}"
                     for name, t in tensors.items())


def _check(what, points, centroids, labels=None):
    """-> (N, F, K) of a valid call; anything else raises"""
    given = dict(points=points, centroids=centroids) if labels is None else dict(points=points, labels=labels, centroids=centroids)
    text = _describe(**given)
    if not all(isinstance(t, torch.Tensor) for t in given.values()):
        raise RuntimeError(f"{what}: expects torch tensors, got {text}")
    if points.dtype != torch.uint8 or centroids.dtype != torch.uint8 or points.ndim != 2 or centroids.ndim != 2 or points.shape[1] != centroids.shape[1]:
        raise RuntimeError(f"{what}: expects points uint8 [N, F] and centroids uint8 [K, F], got {text}")
    n, f = points.shape
    k = centroids.shape[0]
    if labels is not None and (labels.dtype != torch.int32 or tuple(labels.shape) != (n,)):
        raise RuntimeError(f"{what}: expects labels int32 [{n}], got {text}")
    if any(t.device != points.device for t in given.values()):
        raise RuntimeError(f"{what}: tensors on different devices: {text}")
    for name, t in given.items():
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be dense (strides {tuple(t.stride())}): {text}")
    if not (1 <= n <= MAX_ROWS and 1 <= k <= MAX_K and 1 <= f <= MAX_F):
        raise RuntimeError(f"{what}: sizes outside 1 <= N <= {MAX_ROWS}, 1 <= K <= {MAX_K}, 1 <= F <= {MAX_F}: {text}")
    if points.device.type == "cuda" and f % 16 != 0:
        raise RuntimeError(f"{what}: the row length {f} must be a multiple of 16 for the device path: {text}")
    return n, f, k


def assign(points, centroids):
    _check("kmeans_u8.assign", points, centroids)
    d2, index = nn_u8.topk(points, centroids, 1)
    return index[:, 0].contiguous(), d2[:, 0].contiguous()


def update(points, labels, centroids):
    what = "kmeans_u8.update"
    n, f, k = _check(what, points, centroids, labels)
    low, high = int(labels.min()), int(labels.max())
    if low < 0 or high >= k:
        raise RuntimeError(f"{what}: labels lie in [{low}, {high}], outside [0, {k}): {_describe(points=points, labels=labels, centroids=centroids)}")
    dev = points.device
    if dev.type != "cuda":
        index = labels.to(torch.int64)
        counts = torch.bincount(index, minlength=k)
        sums = torch.zeros([k, f], dtype=torch.int64)
        rows = max(1, _CPU_BYTES // (8 * f))
        for lo in range(0, n, rows):
            sums.index_add_(0, index[lo:lo + rows], points[lo:lo + rows].to(torch.int64))
        full = counts.clamp(min=1)[:, None]
        mean = torch.div(2 * sums + full, 2 * full, rounding_mode="floor").to(torch.uint8)
        return torch.where((counts > 0)[:, None], mean, centroids), counts, sums
    lib = _lib.load()
    ws = _lib.workspace(lib.sbg_kmeans_u8_update_workspace(n, f, k), dev, "sbg_kmeans_u8_update_workspace")
    new = torch.empty([k, f], dtype=torch.uint8, device=dev)
    sums = torch.empty([k, f], dtype=torch.int64, device=dev)
    counts = torch.empty([k], dtype=torch.int64, device=dev)
    _lib.check(lib.sbg_kmeans_u8_update(points.data_ptr(), labels.data_ptr(), centroids.data_ptr(), new.data_ptr(), sums.data_ptr(), counts.data_ptr(),
                                        ws.data_ptr(), n, f, k, _lib.stream_ptr(dev)), "sbg_kmeans_u8_update")
    return new, counts, sums


def seed(points, K, rng):
    what = "kmeans_u8.seed"
    K = int(K)
    if not isinstance(points, torch.Tensor) or points.dtype != torch.uint8 or points.ndim != 2 or not points.is_contiguous():
        raise RuntimeError(f"{what}: expects dense points uint8 [N, F], got {_describe(points=points)}")
    n = points.shape[0]
    if not 1 <= K <= min(MAX_K, n):
        raise RuntimeError(f"{what}: K = {K} centres, 1 to min({MAX_K}, N) are supported: {_describe(points=points)}")
    if not isinstance(rng, np.random.RandomState):
        raise RuntimeError(f"{what}: rng must be a numpy.random.RandomState, got {type(rng).__name__}")
    rows = [int(rng.randint(n))]
    best = None
    for i in range(1, K):
        d2 = assign(points, points[rows[-1]:rows[-1] + 1])[1]
        best = d2 if best is None else torch.minimum(best, d2)
        total = int(best.sum())
        if total == 0:
            raise RuntimeError(f"{what}: the table {tuple(points.shape)} holds only {i} distinct rows, K = {K} centres need {K}")
        r = (int(rng.random_sample() * 2 ** 53) * total) >> 53
        cum = torch.cumsum(best, 0)
        rows.append(int(torch.searchsorted(cum, torch.tensor([r], dtype=torch.int64, device=points.device), right=True)[0]))
    return points[torch.tensor(rows, dtype=torch.int64, device=points.device)].contiguous()


def lloyd(points, centroids, max_iter):
    what = "kmeans_u8.lloyd"
    _check(what, points, centroids)
    max_iter = int(max_iter)
    if max_iter < 0:
        raise RuntimeError(f"{what}: max_iter = {max_iter} must not be negative")
    k = centroids.shape[0]
    inertia, iterations, converged, labels, d2 = [], 0, False, None, None
    while iterations < max_iter and not converged:
        labels, d2 = assign(points, centroids)
        inertia.append(int(d2.sum()))
        new = update(points, labels, centroids)[0]
        iterations += 1
        converged = torch.equal(new, centroids)
        centroids = new
    if not converged:
        labels, d2 = assign(points, centroids)
        inertia.append(int(d2.sum()))
    counts = torch.bincount(labels.to(torch.int64), minlength=k)
    return dict(centroids=centroids, labels=labels, d2=d2, counts=counts, inertia=inertia, iterations=iterations, converged=converged)
