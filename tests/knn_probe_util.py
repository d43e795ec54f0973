"""numpy oracle of the probe pass (csrc/knn_manifold.hip, torch_utils/ops/knn_manifold.py `probe`) and of the density / coverage metric
built on it (metrics/scores.py `prdc_fused`), on the distances of knn_manifold_util.

    count[i]   = |{ j : d(P[i], M[j]) <= r[j] }|        nearest[i] = min_j d(P[i], M[j])
    r_X = kth_radius(X, X, k), r_Y = kth_radius(Y, Y, k), (cA, _) = probe(Y, X, r_X), (cB, nB) = probe(X, Y, r_Y)
    precision = mean(cA > 0)   recall = mean(cB > 0)   density = sum(cA) / (k M)   coverage = mean(nB <= r_X)
"""
import functools

import numpy as np

import knn_manifold_util as ku

NEAR = 2.0 ** -8            # relative margin inside which fp32 summation order may decide a comparison (the existing membership test's)


def probe(probes, manifold, radius):
    d, _ = ku.distances(probes, manifold)
    return (d <= radius[None, :]).sum(axis=1).astype(np.int32), d.min(axis=1)


def near_pairs(probes, manifold, radius):
    """bool [P, C]: the (probe, ball) pairs whose float64 distance lies within NEAR of the radius, relative to the radius"""
    _, d = ku.distances(probes, manifold)
    r = radius.astype(np.float64)[None, :]
    return np.abs(r - d) / r < NEAR


def undecided_cover(reals, gens, radius_real):
    """bool [N]: the reals whose float64 nearest generated distance lies within NEAR of their own radius"""
    _, d = ku.distances(reals, gens)
    r = radius_real.astype(np.float64)
    return np.abs(r - d.min(axis=1)) / r < NEAR


def prdc(real, gen, k):
    """the four numbers by brute force; precision and recall as the fp32 mean of the 0 / 1 vector (what precision_recall returns)"""
    r_real, r_gen = ku.kth_radius(real, real, k), ku.kth_radius(gen, gen, k)
    c_a, _ = probe(gen, real, r_real)
    c_b, n_b = probe(real, gen, r_gen)
    return (float((c_a > 0).astype(np.float32).mean()), float((c_b > 0).astype(np.float32).mean()),
            int(c_a.sum(dtype=np.int64)) / (k * len(gen)), float(np.mean(n_b <= r_real)))


@functools.lru_cache(maxsize=None)
def exact_probe(R, C, F, k, offset):
    """the oracle's (count, nearest) for the probes of ku.exact_case against its manifold and `radius_all`.  Callers must not modify them."""
    case = ku.exact_case(R, C, F, k, offset)
    return probe(case["probes"], case["manifold"], case["radius_all"])


@functools.lru_cache(maxsize=None)
def multi_tile_probe(R, C, F, k):
    case = ku.multi_tile_case(R, C, F, k)
    return probe(case["probes"], case["manifold"], case["radius"])
