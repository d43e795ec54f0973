"""The k-nearest-neighbour arithmetic of the precision / recall metric as fused HIP kernels (csrc/knn_manifold.hip).

``kth_radius`` is the reference's ``dist.kthvalue(nhood_size + 1)`` and ``in_manifold`` its ``(dist <= kth).any(dim=1)``
(stylegan2ada/metrics/precision_recall.py:48-60), both without the distance matrix ever being stored.  ``probe`` returns, per probe, how
many balls hold it and how far its nearest manifold point is: the pass behind density / coverage (Naeem et al., ICML 2020), which the
reference does not have.  One definition for both devices:

    n(x) = sum x_f^2,  s(x, y) = sum x_f y_f        products of the fp16 values, summed in fp32 (any order)
    d2   = max((n(x) + n(y)) - 2 s, 0)               fp32, in that association
    d    = fp16(sqrt_f32(d2))                        selection and comparison happen on these fp16 values

``topk`` is the feature-space search of ``nearest_neighbors.py``: the k nearest manifold rows of every query with their indices, selected
on the fp32 d2 itself.  ``realism`` is the per-probe realism score of the improved precision / recall paper (its section 5): the largest
radius / d over the manifold's kept balls with the index that attains it, on the same fp16 d.

Device tensors must be fp16 and run the kernels; a missing kernel or an unsupported input is an error, never a quiet torch fallback.
CPU tensors run the same definition in torch (float64 sums rounded to fp32, then the steps above), so the metric's plumbing is testable
without a GPU.
"""
import types

import torch

from ... import _lib
from . import _topk_common

MAX_NEIGHBOURS = 8          # k + 1 <= 8 (csrc/knn_manifold.hip)
MAX_TOPK = 8                # topk: 1 <= k <= 8
MAX_ROWS = 1 << 24
_CPU_ROWS = 1024            # rows per block of the CPU path
_TOPK = types.SimpleNamespace(noun="manifold", rows="manifold rows", dtype=torch.float16, d2_dtype=torch.float32, max_k=MAX_TOPK, max_rows=MAX_ROWS,
                              flatten=False, entry="sbg_knn_topk", workspace="sbg_knn_topk_workspace")


def _check(rows, manifold, k):
    if rows.ndim != 2 or manifold.ndim != 2 or rows.shape[1] != manifold.shape[1]:
        raise RuntimeError(f"knn_manifold: expects [R, F] and [C, F], got {tuple(rows.shape)} and {tuple(manifold.shape)}")
    if rows.device != manifold.device:
        raise RuntimeError(f"knn_manifold: tensors on different devices ({rows.device}, {manifold.device})")
    if not 0 <= k < MAX_NEIGHBOURS:
        raise RuntimeError(f"knn_manifold: k + 1 = {k + 1} neighbours, at most {MAX_NEIGHBOURS} are supported")
    if manifold.shape[0] < k + 1:
        raise RuntimeError(f"knn_manifold: the manifold has {manifold.shape[0]} points, the (k + 1)-th neighbour needs {k + 1}")


def _cpu_distances(rows, manifold, n_manifold):
    """[r, C] fp16 distances of a block of rows by the definition above"""
    x = rows.to(torch.float64)
    n_rows = x.square().sum(1).to(torch.float32)
    s = (x @ manifold.to(torch.float64).T).to(torch.float32)
    d2 = ((n_rows[:, None] + n_manifold[None, :]) - 2 * s).clamp_(min=0)
    return d2.sqrt().to(torch.float16)


def _workspace(lib, R, C, k, membership, device):
    nbytes = lib.sbg_knn_workspace(R, C, k, int(membership))
    if nbytes < 0:
        raise RuntimeError(f"knn_manifold: unsupported sizes R={R} C={C} k={k}")
    return _lib.workspace(nbytes, device, "sbg_knn_workspace")


def kth_radius(rows, manifold, k):
    """rows [R, F], manifold [C, F] -> fp16 [R]: the (k + 1)-th smallest distance from each row to the manifold's points.  When
    `rows` is a slice of `manifold` the self-distance takes part, as in the reference."""
    _check(rows, manifold, k)
    R, F = rows.shape
    C = manifold.shape[0]
    if rows.device.type != "cuda":
        n_manifold = manifold.to(torch.float64).square().sum(1).to(torch.float32)
        out = [_cpu_distances(b, manifold, n_manifold).to(torch.float32).kthvalue(k + 1).values.to(torch.float16) for b in rows.split(_CPU_ROWS)]
        return torch.cat(out) if out else torch.empty([0], dtype=torch.float16)
    rows, manifold = (_lib.require_dtype(t, torch.float16, "knn_manifold.kth_radius").contiguous() for t in (rows, manifold))
    out = torch.empty([R], dtype=torch.float16, device=rows.device)
    if R == 0:
        return out
    lib = _lib.load()
    ws = _workspace(lib, R, C, k, False, rows.device)
    _lib.check(lib.sbg_knn_kth_radius(rows.data_ptr(), manifold.data_ptr(), R, C, F, k, out.data_ptr(), ws.data_ptr(), _lib.stream_ptr(rows.device)),
               "sbg_knn_kth_radius")
    return out


def in_manifold(probes, manifold, radius):
    """probes [P, F], manifold [C, F], radius [C] -> bool [P]: does the probe lie inside the ball of some manifold point"""
    _check(probes, manifold, 0)
    P, F = probes.shape
    C = manifold.shape[0]
    if radius.shape != (C,) or radius.device != manifold.device:
        raise RuntimeError(f"knn_manifold.in_manifold: expects one radius per manifold point on its device, got {tuple(radius.shape)} on {radius.device}")
    if probes.device.type != "cuda":
        n_manifold = manifold.to(torch.float64).square().sum(1).to(torch.float32)
        r = radius.to(torch.float16)
        out = [(_cpu_distances(b, manifold, n_manifold) <= r).any(dim=1) for b in probes.split(_CPU_ROWS)]
        return torch.cat(out) if out else torch.empty([0], dtype=torch.bool)
    probes, manifold, radius = (_lib.require_dtype(t, torch.float16, "knn_manifold.in_manifold").contiguous() for t in (probes, manifold, radius))
    out = torch.empty([P], dtype=torch.uint8, device=probes.device)
    if P == 0:
        return out.bool()
    lib = _lib.load()
    ws = _workspace(lib, P, C, 0, True, probes.device)
    _lib.check(lib.sbg_knn_in_manifold(probes.data_ptr(), manifold.data_ptr(), radius.data_ptr(), P, C, F, out.data_ptr(), ws.data_ptr(),
                                       _lib.stream_ptr(probes.device)), "sbg_knn_in_manifold")
    return out.bool()


def probe(probes, manifold, radius):
    """probes [P, F], manifold [C, F], radius [C] -> (count int32 [P], nearest fp16 [P]): the number of manifold points whose ball holds the
    probe (`d <= radius[j]`, so `count > 0` is `in_manifold`) and the distance to the nearest manifold point (`kth_radius(probes, manifold, 0)`)"""
    _check(probes, manifold, 0)
    P, F = probes.shape
    C = manifold.shape[0]
    if radius.shape != (C,) or radius.device != manifold.device:
        raise RuntimeError(f"knn_manifold.probe: expects one radius per manifold point on its device, got {tuple(radius.shape)} on {radius.device}")
    if probes.device.type != "cuda":
        n_manifold = manifold.to(torch.float64).square().sum(1).to(torch.float32)
        r = radius.to(torch.float16)
        count, nearest = [], []
        for b in probes.split(_CPU_ROWS):
            d = _cpu_distances(b, manifold, n_manifold)
            count.append((d <= r).sum(dim=1, dtype=torch.int32))
            nearest.append(d.to(torch.float32).min(dim=1).values.to(torch.float16))
        if not count:
            return torch.empty([0], dtype=torch.int32), torch.empty([0], dtype=torch.float16)
        return torch.cat(count), torch.cat(nearest)
    probes, manifold, radius = (_lib.require_dtype(t, torch.float16, "knn_manifold.probe").contiguous() for t in (probes, manifold, radius))
    count = torch.empty([P], dtype=torch.int32, device=probes.device)
    nearest = torch.empty([P], dtype=torch.float16, device=probes.device)
    if P == 0:
        return count, nearest
    lib = _lib.load()
    nbytes = lib.sbg_knn_probe_workspace(P, C)
    if nbytes < 0:
        raise RuntimeError(f"knn_manifold.probe: unsupported sizes P={P} C={C}")
    ws = _lib.workspace(nbytes, probes.device, "sbg_knn_probe_workspace")
    _lib.check(lib.sbg_knn_probe(probes.data_ptr(), manifold.data_ptr(), radius.data_ptr(), P, C, F, count.data_ptr(), nearest.data_ptr(), ws.data_ptr(),
                                 _lib.stream_ptr(probes.device)), "sbg_knn_probe")
    return count, nearest


def realism(probes, manifold, radius, exclude=None):
    """probes [P, F], manifold [C, F], radius [C] (negative: the point is pruned), exclude int32 [P] or None (a manifold index, or -1)
    -> (score fp32 [P], index int32 [P]): the realism score of Kynkaanniemi et al. (NeurIPS 2019, section 5) on the module's fp16 d.

        eligible(i, j) = radius[j] >= 0 and j != exclude[i]
        q(i, j)        = +inf when d(i, j) == 0 (also at radius 0), else float(radius[j]) / float(d(i, j)), one fp32 division
        score[i]       = max of q(i, j) over the eligible j; 0 when there is none
        index[i]       = the lowest eligible j attaining it; -1 when there is none

    A maximum with ties to the lower index depends on no order, so any cut of the probes into batches gives the same bits; and since q
    is formed from the d that `in_manifold` compares, ``score >= 1`` is `in_manifold(probes, manifold, radius)` when nothing is excluded.
    Device tensors must be fp16 (``exclude`` int32) and run the kernel; anything else raises.  CPU tensors run the definition in torch."""
    what = "knn_manifold.realism"
    _check(probes, manifold, 0)
    P, F = probes.shape
    C = manifold.shape[0]
    if radius.shape != (C,) or radius.device != manifold.device:
        raise RuntimeError(f"{what}: expects one radius per manifold point on its device, got {tuple(radius.shape)} on {radius.device}")
    if exclude is not None:
        if exclude.dtype != torch.int32:
            raise RuntimeError(f"{what}: exclude must be int32, got {exclude.dtype}")
        if exclude.shape != (P,) or exclude.device != probes.device:
            raise RuntimeError(f"{what}: expects one excluded manifold index per probe on its device, got {tuple(exclude.shape)} on {exclude.device}")
    if probes.device.type != "cuda":
        n_manifold = manifold.to(torch.float64).square().sum(1).to(torch.float32)
        r = radius.to(torch.float16).to(torch.float32)
        cols = torch.arange(C)
        score, index = [], []
        for lo in range(0, P, _CPU_ROWS):
            d = _cpu_distances(probes[lo:lo + _CPU_ROWS], manifold, n_manifold).to(torch.float32)
            q = torch.where(d == 0, torch.full_like(d, float("inf")), (r[None, :] / d).abs())      # abs: a radius of -0 counts as +0
            eligible = (r >= 0)[None, :].expand_as(q)
            if exclude is not None:
                eligible = eligible & (cols[None, :] != exclude[lo:lo + _CPU_ROWS, None])
            q = torch.where(eligible, q, torch.full_like(q, -1.0))
            best = q.max(dim=1).values
            first = (q == best[:, None]).to(torch.uint8).argmax(dim=1)          # of equal maxima the first: the lowest index
            none = best < 0
            score.append(torch.where(none, torch.zeros_like(best), best))
            index.append(torch.where(none, torch.full_like(first, -1), first).to(torch.int32))
        if not score:
            return torch.empty([0], dtype=torch.float32), torch.empty([0], dtype=torch.int32)
        return torch.cat(score), torch.cat(index)
    probes, manifold, radius = (_lib.require_dtype(t, torch.float16, what).contiguous() for t in (probes, manifold, radius))
    score = torch.empty([P], dtype=torch.float32, device=probes.device)
    index = torch.empty([P], dtype=torch.int32, device=probes.device)
    if P == 0:
        return score, index
    if F % 8 != 0:
        raise RuntimeError(f"{what}: the feature width {F} must be a multiple of 8 (16-byte pieces) for the device path")
    if exclude is not None:
        exclude = exclude.contiguous()
    lib = _lib.load()
    nbytes = lib.sbg_knn_realism_workspace(P, C)
    if nbytes < 0:
        raise RuntimeError(f"{what}: unsupported sizes P={P} C={C}")
    ws = _lib.workspace(nbytes, probes.device, "sbg_knn_realism_workspace")
    _lib.check(lib.sbg_knn_realism(probes.data_ptr(), manifold.data_ptr(), radius.data_ptr(), P, C, F, None if exclude is None else exclude.data_ptr(),
                                   score.data_ptr(), index.data_ptr(), ws.data_ptr(), _lib.stream_ptr(probes.device)), "sbg_knn_realism")
    return score, index


def topk(queries, manifold, k, exclude=None):
    """queries fp16 [Q, F], manifold fp16 [M, F], exclude int32 [Q] or None -> (d2 float32 [Q, k], index int32 [Q, k]): the k manifold rows
    nearest to every query by the module's d2 (the fp32 value; nothing is rounded to fp16), ascending by (d2, row), so a tie goes to the
    lower row.  Row ``exclude[q]`` is skipped when it lies in [0, M); it is the only row skipped -- a duplicate of it elsewhere is a
    legitimate hit.  Device tensors run the kernel on the current stream (1 <= k <= 8, F a multiple of 8, dense 16-byte aligned rows,
    Q, M <= 2^24 -- anything else raises, nothing falls back to torch); CPU tensors run the same definition in torch with a stable sort.
    Non-finite features are outside the definition: on the device ``fmaxf(NaN, 0)`` is 0, so a NaN distance would rank first; callers
    check their features (``nearest_neighbors.py`` does, once per matrix)."""
    what = "knn_manifold.topk"
    Q, M, F = _topk_common.check(what, _TOPK, queries, manifold, k, exclude)
    if queries.device.type != "cuda":
        n_manifold = manifold.to(torch.float64).square().sum(1).to(torch.float32)
        y = manifold.to(torch.float64).T
        cols = torch.arange(M)
        d2_out = torch.empty([Q, k], dtype=torch.float32)
        idx_out = torch.empty([Q, k], dtype=torch.int32)
        for lo in range(0, Q, _CPU_ROWS):
            x = queries[lo:lo + _CPU_ROWS].to(torch.float64)
            n_rows = x.square().sum(1).to(torch.float32)
            d2 = ((n_rows[:, None] + n_manifold[None, :]) - 2 * (x @ y).to(torch.float32)).clamp_(min=0)
            d2_out[lo:lo + _CPU_ROWS], idx_out[lo:lo + _CPU_ROWS] = _topk_common.select(
                d2, k, None if exclude is None else exclude[lo:lo + _CPU_ROWS], cols, float("inf"))
        return d2_out, idx_out
    if F % 8 != 0:
        raise RuntimeError(f"{what}: the feature width {F} must be a multiple of 8 (16-byte pieces) for the device path")
    return _topk_common.run_device(what, _TOPK, queries, manifold, Q, M, F, k, exclude)
