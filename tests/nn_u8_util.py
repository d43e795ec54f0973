"""The oracle of the exact uint8 nearest-row search (torch_utils/ops/nn_u8.py) and the data its tests share.

`oracle_topk` is numpy: d2 = n(q) + n(x) - 2 q.x with a float64 GEMM, which is exact because every partial sum is an integer below
F * 65025 < 2^53; then a stable sort by (d2, j) -- only the rows at or below the k-th smallest d2 of a query are sorted, in ascending j."""
import numpy as np
import torch

INT64_MAX = np.iinfo(np.int64).max


def oracle_topk(queries, store, k, exclude=None, block=1024):
    """uint8 ndarrays [Q, F], [M, F]; exclude int [Q] or None -> (d2 int64 [Q, k], index int32 [Q, k]), ascending by (d2, j)"""
    queries, store = np.asarray(queries), np.asarray(store)
    Q, F = queries.shape
    M = store.shape[0]
    assert queries.dtype == np.uint8 and store.dtype == np.uint8 and store.shape[1] == F and F * 65025 < 2 ** 53
    xs = store.astype(np.float64)
    nx = np.einsum("mf,mf->m", xs, xs)
    d2_out = np.empty([Q, k], dtype=np.int64)
    idx_out = np.empty([Q, k], dtype=np.int32)
    for q0 in range(0, Q, block):
        qs = queries[q0:q0 + block].astype(np.float64)
        d2 = (np.einsum("qf,qf->q", qs, qs)[:, None] + nx[None, :] - 2.0 * (qs @ xs.T)).astype(np.int64)
        assert d2.min() >= 0
        if exclude is not None:
            for r in range(d2.shape[0]):
                if 0 <= int(exclude[q0 + r]) < M:
                    d2[r, int(exclude[q0 + r])] = INT64_MAX
        kth = np.partition(d2, k - 1, axis=1)[:, k - 1]
        for r in range(d2.shape[0]):
            cand = np.nonzero(d2[r] <= kth[r])[0]                           # ascending j
            order = cand[np.argsort(d2[r, cand], kind="stable")[:k]]        # stable: ties keep ascending j
            d2_out[q0 + r], idx_out[q0 + r] = d2[r, order], order
    assert d2_out.max() < INT64_MAX, "fewer than k rows are left"
    return d2_out, idx_out


def make_case(Q, M, F, seed, far=None):
    """asymmetric random full-range bytes -> (queries [Q, F], store [M, F], planted pairs [(j, its copy's row)]), uint8 ndarrays with
    * stored rows that are exact copies of EARLIER rows (row j + d = row j for a few j, d = 1 and `far`: a tie goes to the lower index),
    * queries that are stored rows with a few bytes changed (the nearest row is known), some of them rows that have a copy."""
    rng = np.random.RandomState(seed)
    store = rng.randint(0, 256, [M, F], dtype=np.uint8)
    queries = rng.randint(0, 256, [Q, F], dtype=np.uint8)
    planted, used = [], set()
    for d in [1] + ([far] if far else []):
        for j in rng.randint(0, max(M - d, 1), size=min(4, max(M - d, 0))):
            if j + d < M and j not in used and j + d not in used:          # a row takes part in one pair at most
                store[j + d] = store[j]
                planted.append((int(j), int(j + d)))
                used.update((int(j), int(j + d)))
    src = [a for a, _ in planted] + list(rng.randint(0, M, size=3))
    for i, j in zip(range(Q - 1, -1, -2), src):                             # every second query from the end
        queries[i] = store[j]
        pos = rng.randint(0, F, size=min(3, F))
        queries[i, pos] ^= rng.randint(1, 256, size=pos.size).astype(np.uint8)
    return queries, store, planted


def same(got, want):
    """(d2, index) device tensors against the oracle's arrays, bit for bit"""
    d2, idx = got
    return (d2.dtype == torch.int64 and idx.dtype == torch.int32 and np.array_equal(d2.cpu().numpy(), want[0])
            and np.array_equal(idx.cpu().numpy(), want[1]))
