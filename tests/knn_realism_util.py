"""numpy oracle of the realism pass (csrc/knn_manifold.hip mode 4, torch_utils/ops/knn_manifold.py `realism`) and of `scores.realism_scores`
built on it, on the distances of knn_manifold_util (float64 sums, one cast to fp32, fp32 sqrt, fp16):

    eligible(i, j) = r[j] >= 0 and j != exclude[i]
    q(i, j)        = +inf where d(i, j) == 0, else float32(r[j]) / float32(d(i, j))
    score[i]       = max of q(i, j) over the eligible j (0 without one),  index[i] = the lowest eligible j attaining it (-1 without one)
"""
import functools

import numpy as np

import knn_manifold_util as ku

REL = 2.0 ** -9             # one fp16 ulp of d, relative: what fp32 summation order may move a realistic score by (the probe test's `ulps <= 1`)


def ratios(probes, manifold, radius, exclude=None):
    """float32 [P, C]: q(i, j), and -1 where j is not eligible"""
    d = ku.distances(probes, manifold)[0].astype(np.float32)
    r = np.asarray(radius).astype(np.float16).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, np.float32(np.inf), r[None, :] / d).astype(np.float32)
    eligible = np.broadcast_to(r[None, :] >= 0, q.shape)
    if exclude is not None:
        eligible = eligible & (np.arange(len(manifold))[None, :] != np.asarray(exclude)[:, None])
    return np.where(eligible, q, np.float32(-1))


def realism(probes, manifold, radius, exclude=None):
    """-> (score float32 [P], index int32 [P])"""
    q = ratios(probes, manifold, radius, exclude)
    index = q.argmax(axis=1)                                    # numpy's argmax returns the first of equal maxima: the lowest index
    score = q[np.arange(len(q)), index]
    none = score < 0
    return np.where(none, np.float32(0), score).astype(np.float32), np.where(none, -1, index).astype(np.int32)


def tied(probes, manifold, radius, exclude=None):
    """bool [P]: the maximum is attained by more than one eligible j"""
    q = ratios(probes, manifold, radius, exclude)
    best = q.max(axis=1)
    return ((q == best[:, None]).sum(axis=1) > 1) & (best >= 0)


def half_pruned(radius):
    """every second radius (the odd indices) set to -1"""
    r = np.array(radius, dtype=np.float16)
    r[1::2] = -1
    return r


def prune(radius, keep):
    """the radii with all but the ceil(keep * N) smallest set to -1, ties kept at the lower index (`scores.realism_scores`' rule)"""
    r = np.array(radius, dtype=np.float16)
    n_keep = int(np.ceil(keep * len(r)))
    order = np.argsort(r.astype(np.float32), kind="stable")
    out = np.full_like(r, -1)
    out[order[:n_keep]] = r[order[:n_keep]]
    return out


def exclude_for(R, C):
    """an int32 [R] exclusion list that names a manifold row for most probes, -1 for every seventh; probes that are copies of manifold
    points (every fifth, copy of row i / 5 mod C) exclude that very row"""
    ex = (np.arange(R, dtype=np.int64) * 3 + 1) % C
    ex[::5] = np.arange(len(ex[::5])) % C
    ex[::7] = -1
    return ex.astype(np.int32)


@functools.lru_cache(maxsize=None)
def exact_realism(R, C, F, k, offset, pruned=False, excluded=False):
    """the oracle's (score, index, radius, exclude) on ku.exact_case, with half the radii at -1 (`pruned`) and / or an exclusion list
    (`excluded`).  Callers must not modify the arrays."""
    case = ku.exact_case(R, C, F, k, offset)
    radius = half_pruned(case["radius_all"]) if pruned else case["radius_all"]
    exclude = exclude_for(R, C) if excluded else None
    score, index = realism(case["probes"], case["manifold"], radius, exclude)
    return score, index, radius, exclude


@functools.lru_cache(maxsize=None)
def realistic_case(n_real, n_gen, F, seed, k=3, keep=0.5):
    """ku.realistic_features with radii at k, the larger-radius half pruned -> dict(real, gen, radius, score, index, q)"""
    real, gen = ku.realistic_features(n_real, n_gen, F, seed)
    radius = prune(ku.kth_radius(real, real, k), keep)
    q = ratios(gen, real, radius)
    score, index = realism(gen, real, radius)
    return dict(real=real, gen=gen, radius=radius, score=score, index=index, q=q)


def f32_bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


def within_margin(score, index, want_score, want_index, q):
    """the realistic-value conditions: -> (largest relative score difference, share of scores equal in bits, bool [P] index acceptable: the
    oracle's, or one whose oracle ratio is within REL relative of the maximum)"""
    rel = np.abs(score.astype(np.float64) - want_score) / want_score
    equal = np.mean(f32_bits(score) == f32_bits(want_score))
    at = q[np.arange(len(q)), np.maximum(index, 0)].astype(np.float64)
    ok = (index == want_index) | ((index >= 0) & (at >= want_score * (1 - REL)))
    return float(rel.max()), float(equal), ok
