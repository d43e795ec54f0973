"""Exact nearest rows of a uint8 store for uint8 queries (csrc/nn_u8.hip): the search behind ``nearest_neighbors.py``.

``topk(queries, store, k, exclude=None)`` returns, for every query q, the k rows j of the store with the smallest

    d2(q, j) = sum_f (queries[q, f] - store[j, f])^2          an exact int64 integer

sorted ascending by (d2, j), so a tie goes to the lower row.  Row ``exclude[q]`` is skipped when it lies in [0, M); it is the only row
skipped -- a duplicate of it elsewhere in the store is a legitimate hit.  Trailing dimensions are flattened, so ``[Q, C, H, W]`` against
``[M, C, H, W]`` works.

Device tensors run the kernels (i8 matrix cores, int64 norms and distances); an input outside their limits is an error, never a quiet
torch fallback.  ``topk_reference`` is the same semantics in torch int64 arithmetic, in row blocks; CPU tensors take it, so the tool's
plumbing is testable without a GPU.
"""
import types

import torch

from . import _topk_common

MAX_K = 8                       # csrc/nn_u8.hip
MAX_F = 3 * 1024 * 1024
MAX_ROWS = 1 << 24
_REF_BYTES = 1 << 27            # int64 work set of one block of topk_reference
_KIND = types.SimpleNamespace(noun="store", rows="stored rows", dtype=torch.uint8, d2_dtype=torch.int64, max_k=MAX_K, max_rows=MAX_ROWS,
                              flatten=True, entry="sbg_u8_nn_topk", workspace="sbg_u8_nn_workspace")


def topk_reference(queries, store, k, exclude=None):
    """the semantics of `topk` in torch int64 arithmetic on the tensors' own device, in row blocks -> (d2 int64 [Q, k], index int32 [Q, k])"""
    Q, M, F = _topk_common.check("nn_u8 topk_reference", _KIND, queries, store, k, exclude)
    q = queries.reshape(Q, F)
    s = store.reshape(M, F)
    cols = torch.arange(M, device=store.device)
    qb = max(1, min(Q, 64))
    mb = max(1, min(M, _REF_BYTES // (8 * qb * min(F, 4096))))
    fb = max(1, min(F, _REF_BYTES // (8 * qb * mb)))
    d2_out = torch.empty([Q, k], dtype=torch.int64, device=store.device)
    idx_out = torch.empty([Q, k], dtype=torch.int32, device=store.device)
    for q0 in range(0, Q, qb):
        d2 = torch.zeros([min(qb, Q - q0), M], dtype=torch.int64, device=store.device)
        for m0 in range(0, M, mb):
            for f0 in range(0, F, fb):
                a = q[q0:q0 + qb, None, f0:f0 + fb].to(torch.int64)
                b = s[None, m0:m0 + mb, f0:f0 + fb].to(torch.int64)
                d2[:, m0:m0 + mb] += (a - b).square_().sum(2)
        d2_out[q0:q0 + qb], idx_out[q0:q0 + qb] = _topk_common.select(
            d2, k, None if exclude is None else exclude[q0:q0 + qb], cols, torch.iinfo(torch.int64).max)
    return d2_out, idx_out


def topk(queries, store, k, exclude=None):
    """queries uint8 [Q, ...], store uint8 [M, ...] (the same row length F), exclude int32 [Q] or None -> (d2 int64 [Q, k], index int32 [Q, k]):
    the k nearest rows of every query, ascending by (d2, row).  Device tensors run the kernels on the current stream (F a multiple of 16,
    at most 3 * 2^20; 16-byte aligned; Q, M <= 2^24 -- anything else raises); CPU tensors take `topk_reference`."""
    what = "nn_u8 topk"
    Q, M, F = _topk_common.check(what, _KIND, queries, store, k, exclude)
    if store.device.type != "cuda":
        return topk_reference(queries, store, k, exclude)
    if F % 16 != 0 or F > MAX_F:
        raise RuntimeError(f"{what}: the row length {F} must be a multiple of 16, at most {MAX_F}, for the device path")
    return _topk_common.run_device(what, _KIND, queries, store, Q, M, F, k, exclude)
