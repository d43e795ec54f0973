"""numpy oracle and data for the k-NN manifold kernels (csrc/knn_manifold.hip, torch_utils/ops/knn_manifold.py).

The oracle: d2 in float64 from the fp16 inputs, cast to fp32, `np.sqrt` in fp32, `.astype(np.float16)`; a sort for the radius, `<=` / `any`
for the membership.  With integer features and 4 max|x|^2 < 2^24 every fp32 sum the kernels form is exact in any order, so they must
reproduce the oracle bit for bit."""
import contextlib
import functools

import numpy as np
import torch


def distances(rows, manifold):
    """fp16 [R, C] distances by the oracle's definition, and the float64 ones"""
    x, y = rows.astype(np.float64), manifold.astype(np.float64)
    d2 = np.maximum(((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :]) - 2.0 * (x @ y.T), 0.0)
    return np.sqrt(d2.astype(np.float32)).astype(np.float16), np.sqrt(d2)


def kth_radius(rows, manifold, k):
    d, _ = distances(rows, manifold)
    return np.sort(d, axis=1)[:, k]


def in_manifold(probes, manifold, radius):
    d, _ = distances(probes, manifold)
    return (d <= radius[None, :]).any(axis=1)


def margins(probes, manifold, radius):
    """float64 deciding margin of every probe: max_j (r_j - d_ij) / r_j"""
    _, d = distances(probes, manifold)
    r = radius.astype(np.float64)[None, :]
    return ((r - d) / r).max(axis=1)


def exact_features(n, F, seed):
    """integer features in fp16 whose sums are exact in fp32: values in [-2, 2] for a narrow F; at F = 4096 forty varying columns with
    integers up to 8 and a constant non-zero pattern in the rest (norms ~1e5, distances ~10: the cancellation case)"""
    rng = np.random.RandomState(seed)
    if F <= 128:
        x = rng.randint(-2, 3, size=[n, F])
    else:
        x = np.tile(4 + np.arange(F) % 3, [n, 1])
        cols = np.random.RandomState(1234).permutation(F)[:40]          # the same columns for every matrix
        x[:, cols] = rng.randint(0, 9, size=[n, 40])
    assert 4 * int((x * x).sum(1).max()) < 2 ** 24
    return x.astype(np.float16)


@functools.lru_cache(maxsize=None)
def exact_case(R, C, F, k, offset):
    """-> manifold [C, F] with duplicate points, rows (a slice of the manifold at `offset` when it fits), probes [R, F] holding copies of
    manifold points, and the oracle's answers.  Computed once per shape; callers must not modify the arrays."""
    manifold = exact_features(C, F, seed=C + F + k)
    for dst, src in [(3, 0), (5, 0), (6, 0), (C - 1, 1), (C // 2, 2)]:      # four copies of point 0 (radius 0 up to k = 3), two pairs
        if dst < C and src < C:
            manifold[dst] = manifold[src]
    rows = manifold[offset:offset + R] if offset + R <= C else exact_features(R, F, seed=7 * R + 1)
    probes = exact_features(R, F, seed=R + 3)
    probes[::5] = manifold[np.arange(len(probes[::5])) % C]                 # every fifth probe equals a manifold point
    radius_rows = kth_radius(rows, manifold, k)
    radius_all = kth_radius(manifold, manifold, k)
    return dict(manifold=manifold, rows=rows, probes=probes, radius_rows=radius_rows, radius_all=radius_all,
                inside=in_manifold(probes, manifold, radius_all))


def plan(R, C):
    """(column tiles, runs per row tile, tiles per run) of a launch: the split rule of csrc/knn_select.h (`plan_runs`), restated"""
    rtiles, ctiles = -(-R // 128), -(-C // 128)
    want = min(max(512 // rtiles, 1), ctiles)
    tiles_per_run = -(-ctiles // want)
    return ctiles, -(-ctiles // tiles_per_run), tiles_per_run


@functools.lru_cache(maxsize=None)
def multi_tile_case(R, C, F, k):
    """a shape whose workgroups walk several manifold tiles each: rows and probes independent of the manifold (every fifth probe a copy of a
    manifold point), radii that vary from point to point around the median nearest-neighbour distance so that both outcomes occur.
    Computed once per shape; callers must not modify the arrays."""
    manifold = exact_features(C, F, seed=C + F + k)
    rows = exact_features(R, F, seed=7 * R + 1)
    probes = exact_features(R, F, seed=R + 3)
    picks = (np.arange(len(probes[::5])) * 7919) % C                         # copies from all over the manifold, the last tile included
    picks[-1] = C - 1
    probes[::5] = manifold[picks]
    d_rows, _ = distances(rows, manifold)
    radius_rows = np.partition(d_rows, k, axis=1)[:, k]
    d, _ = distances(probes, manifold)
    near = np.sort(d[np.arange(R) % 5 != 0].min(axis=1))                     # nearest-neighbour distance of the probes that are no copies
    values = np.unique(d)
    mid = int(np.searchsorted(values, near[len(near) // 2]))
    radius = values[np.clip(mid + (np.arange(C) * 7) % 5 - 2, 0, len(values) - 1)]
    return dict(manifold=manifold, rows=rows, probes=probes, radius_rows=radius_rows, radius=radius, inside=(d <= radius[None, :]).any(axis=1))


def realistic_features(n_real, n_gen, F, seed):
    """low-rank Gaussian features z[., 8] @ A[8, F] + 0.5, the generated z scaled by 0.8"""
    rng = np.random.RandomState(seed)
    A = rng.randn(8, F)
    real = (rng.randn(n_real, 8) @ A + 0.5).astype(np.float16)
    gen = (0.8 * rng.randn(n_gen, 8) @ A + 0.5).astype(np.float16)
    return real, gen


def bits(x):
    return np.ascontiguousarray(x).view(np.uint16)


def to_np(t):
    return t.detach().cpu().numpy()


@contextlib.contextmanager
def pr_launches():
    """-> list of (variant name, dims) of the 'pr' launches made inside the block"""
    from style_big_gan_amd import _lib
    seen = []
    _lib.prof_enable(True)
    _lib.prof_fetch()
    try:
        yield seen
        torch.cuda.synchronize()
        seen.extend((_lib.PR_VARIANTS[r["dims"][0]], r["dims"]) for r in _lib.prof_fetch() if r["kind"] == "pr")
    finally:
        _lib.prof_enable(False)
