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
import torch

from ... import _lib

MAX_K = 8                       # csrc/nn_u8.hip
MAX_F = 3 * 1024 * 1024
MAX_ROWS = 1 << 24
_REF_BYTES = 1 << 27            # int64 work set of one block of topk_reference


def _check(queries, store, k, exclude, what):
    for name, t in (("queries", queries), ("store", store)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{what}: {name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != torch.uint8 or t.ndim < 2:
            raise RuntimeError(f"{what}: {name} must be uint8 with at least 2 dimensions, got {t.dtype} {list(t.shape)}")
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be dense (shape {list(t.shape)}, strides {list(t.stride())}); call .contiguous() first")
    if queries.device != store.device:
        raise RuntimeError(f"{what}: queries are on {queries.device}, the store on {store.device}")
    Q, M = queries.shape[0], store.shape[0]
    if queries.shape[1:].numel() != store.shape[1:].numel():
        raise RuntimeError(f"{what}: queries {list(queries.shape)} and store {list(store.shape)} differ in the row length")
    F = store.shape[1:].numel()
    if not isinstance(k, int) or not 1 <= k <= MAX_K:
        raise RuntimeError(f"{what}: k = {k} neighbours, 1 to {MAX_K} are supported")
    if Q < 1 or M < 1 or F < 1:
        raise RuntimeError(f"{what}: empty queries {list(queries.shape)} or store {list(store.shape)}")
    if exclude is not None:
        if not isinstance(exclude, torch.Tensor):
            raise RuntimeError(f"{what}: exclude must be a torch tensor, got {type(exclude).__name__}")
        if exclude.dtype != torch.int32 or list(exclude.shape) != [Q]:
            raise RuntimeError(f"{what}: exclude must be int32 {[Q]}, got {exclude.dtype} {list(exclude.shape)}")
        if exclude.device != store.device:
            raise RuntimeError(f"{what}: exclude is on {exclude.device}, the store on {store.device}")
        if not exclude.is_contiguous():
            raise RuntimeError(f"{what}: exclude must be dense; call .contiguous() first")
    if M < k:
        raise RuntimeError(f"{what}: the store has {M} rows, {k} neighbours need {k}")
    if exclude is not None and M == k and bool(((exclude >= 0) & (exclude < M)).any()):
        raise RuntimeError(f"{what}: the store has {M} rows and one is excluded, {k} neighbours need {k + 1}")
    return Q, M, F


def topk_reference(queries, store, k, exclude=None):
    """the semantics of `topk` in torch int64 arithmetic on the tensors' own device, in row blocks -> (d2 int64 [Q, k], index int32 [Q, k])"""
    Q, M, F = _check(queries, store, k, exclude, "nn_u8 topk_reference")
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
        if exclude is not None:
            d2 = torch.where(cols[None, :] == exclude[q0:q0 + qb, None].to(torch.int64), torch.iinfo(torch.int64).max, d2)
        order = torch.sort(d2, dim=1, stable=True).indices[:, :k]           # stable: ties go to the lower row
        d2_out[q0:q0 + qb] = d2.gather(1, order)
        idx_out[q0:q0 + qb] = order.to(torch.int32)
    return d2_out, idx_out


def topk(queries, store, k, exclude=None):
    """queries uint8 [Q, ...], store uint8 [M, ...] (the same row length F), exclude int32 [Q] or None -> (d2 int64 [Q, k], index int32 [Q, k]):
    the k nearest rows of every query, ascending by (d2, row).  Device tensors run the kernels on the current stream (F a multiple of 16,
    at most 3 * 2^20; 16-byte aligned; Q, M <= 2^24 -- anything else raises); CPU tensors take `topk_reference`."""
    what = "nn_u8 topk"
    Q, M, F = _check(queries, store, k, exclude, what)
    if store.device.type != "cuda":
        return topk_reference(queries, store, k, exclude)
    if F % 16 != 0 or F > MAX_F:
        raise RuntimeError(f"{what}: the row length {F} must be a multiple of 16, at most {MAX_F}, for the device path")
    if Q > MAX_ROWS or M > MAX_ROWS:
        raise RuntimeError(f"{what}: {Q} queries / {M} stored rows, at most {MAX_ROWS} each for the device path")
    if queries.data_ptr() % 16 or store.data_ptr() % 16:
        raise RuntimeError(f"{what}: queries and store must be 16-byte aligned for the device path")
    if exclude is not None and M == k:
        exclude = None          # _check has seen that no entry lies in [0, M)
    lib = _lib.load()
    nbytes = lib.sbg_u8_nn_workspace(Q, M, k)
    if nbytes < 0:
        raise RuntimeError(f"{what}: unsupported sizes Q={Q} M={M} k={k}")
    ws = _lib.workspace(nbytes, store.device, "sbg_u8_nn_workspace")
    d2 = torch.empty([Q, k], dtype=torch.int64, device=store.device)
    index = torch.empty([Q, k], dtype=torch.int32, device=store.device)
    _lib.check(lib.sbg_u8_nn_topk(queries.data_ptr(), store.data_ptr(), Q, M, F, k, _lib.ptr(exclude), d2.data_ptr(), index.data_ptr(), ws.data_ptr(),
                                  _lib.stream_ptr(store.device)), "sbg_u8_nn_topk")
    return d2, index
