"""numpy oracle and data for the feature-space top-k search (csrc/knn_manifold.hip `topk`, torch_utils/ops/knn_manifold.py).

The oracle: d2 from float64 sums cast to fp32, as in `knn_manifold_util.distances`, then the k smallest by (d2, row).  A non-negative fp32
orders like its bits, so the oracle sorts the integer `bits(d2) << 32 | row` -- a stable sort by d2 in other words.  With integer
features and 4 max n(x) < 2^24 every fp32 sum the kernel forms is exact in any order, so it must reproduce the oracle bit for bit."""
import contextlib
import functools

import numpy as np
import torch

from knn_manifold_util import exact_features, plan, pr_launches, realistic_features  # noqa: F401

TOPK_MODE = 3               # dims[6] of a 'pr' launch record


def d2_f64(queries, manifold):
    """float64 [Q, M]: max((n(x) + n(y)) - 2 s, 0) of the fp16 values"""
    x, y = queries.astype(np.float64), manifold.astype(np.float64)
    return np.maximum(((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :]) - 2.0 * (x @ y.T), 0.0)


def oracle_topk(queries, manifold, k, exclude=None, rows=4096):
    """-> (d2 float32 [Q, k], index int32 [Q, k]) ascending by (d2, row); row exclude[q] is left out when it lies in [0, M)"""
    Q, M = len(queries), len(manifold)
    d2_out, idx_out = np.empty([Q, k], dtype=np.float32), np.empty([Q, k], dtype=np.int32)
    col = np.arange(M, dtype=np.uint64)
    for lo in range(0, Q, rows):
        d2 = d2_f64(queries[lo:lo + rows], manifold).astype(np.float32)
        assert not np.signbit(d2).any()
        key = (d2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | col[None, :]
        if exclude is not None:
            key[col[None, :] == exclude[lo:lo + rows, None].astype(np.int64).astype(np.uint64)] = np.iinfo(np.uint64).max
        key = np.sort(np.partition(key, k - 1, axis=1)[:, :k], axis=1) if M > k else np.sort(key, axis=1)
        assert (key != np.iinfo(np.uint64).max).all()
        d2_out[lo:lo + rows] = (key >> np.uint64(32)).astype(np.uint32).view(np.float32)
        idx_out[lo:lo + rows] = (key & np.uint64(0xffffffff)).astype(np.int32)
    return d2_out, idx_out


def same(got, want):
    """the fp32 bits of d2 and the indices"""
    d2, index = (t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else t for t in got)
    return (d2.dtype == np.float32 and index.dtype == np.int32 and d2.shape == want[0].shape and index.shape == want[1].shape
            and np.array_equal(d2.view(np.uint32), want[0].view(np.uint32)) and np.array_equal(index, want[1]))


@functools.lru_cache(maxsize=None)
def exact_case(Q, M, F, k, far=None):
    """-> (queries [Q, F], manifold [M, F], planted [(a, b)] with manifold[b] a copy of manifold[a], a < b, the oracle's answer).  Every
    third query equals a stored row; with `far` rows j and j + far are identical for a few j.  Computed once per shape; callers must not
    modify the arrays."""
    manifold = exact_features(M, F, seed=M + F + k)
    planted = [(a, b) for a, b in [(0, 3), (0, 5), (1, M - 1), (2, M // 2)] if a < b < M]
    if far is not None:
        planted += [(j, j + far) for j in (7, 120, 131, 1000, 4099) if j + far < M]
    for a, b in planted:
        manifold[b] = manifold[a]
    queries = exact_features(Q, F, seed=7 * Q + 1)
    picks = (np.arange(len(queries[::3])) * 7919) % M
    picks[:len(planted)] = [a for a, _ in planted][:len(picks)]         # queries that equal a planted row: the tie must go to the lower copy
    queries[::3] = manifold[picks]
    return queries, manifold, planted, oracle_topk(queries, manifold, k)


def to_dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


@contextlib.contextmanager
def topk_launches():
    """-> list of (variant name, dims) of the top-k 'pr' launches made inside the block (the norm passes carry no mode and are kept)"""
    with pr_launches() as seen:
        mine = []
        yield mine
    mine.extend((v, d) for v, d in seen if v == "norms" or d[6] == TOPK_MODE)
