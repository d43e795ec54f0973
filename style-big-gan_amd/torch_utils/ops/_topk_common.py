"""What the two nearest-row searches (`knn_manifold.topk`: fp16 features; `nn_u8.topk`: uint8 rows) share outside the kernels: the
argument validation, the selection of the torch paths, and the checks, the workspace and the call of the device path.  An op describes
itself by a record `kind`: `noun` / `rows` name the searched matrix and its rows in the messages, `dtype` / `d2_dtype` are the rows' and
the distances' types, `max_k` / `max_rows` the limits, `entry` / `workspace` the library's names, and `flatten` says whether rows are
[Q, ...] with trailing dimensions flattened (dense on every path; the uint8 op's message texts) or plain [Q, F]."""
import torch

from ... import _lib


def _require_dense(what, name, t):
    if not t.is_contiguous():
        raise RuntimeError(f"{what}: {name} must be dense (shape {list(t.shape)}, strides {list(t.stride())}); call .contiguous() first")


def check(what, kind, queries, store, k, exclude):
    """-> (Q, M, F) of a valid search; anything else raises"""
    noun, flatten, dtype_name = kind.noun, kind.flatten, str(kind.dtype).replace("torch.", "")
    for name, t in (("queries", queries), (noun, store)):
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{what}: {name} must be a torch tensor, got {type(t).__name__}")
        if flatten:
            if t.dtype != kind.dtype or t.ndim < 2:
                raise RuntimeError(f"{what}: {name} must be {dtype_name} with at least 2 dimensions, got {t.dtype} {list(t.shape)}")
            _require_dense(what, name, t)
    if flatten:
        if queries.device != store.device:
            raise RuntimeError(f"{what}: queries are on {queries.device}, the {noun} on {store.device}")
        if queries.shape[1:].numel() != store.shape[1:].numel():
            raise RuntimeError(f"{what}: queries {list(queries.shape)} and {noun} {list(store.shape)} differ in the row length")
    else:
        if queries.ndim != 2 or store.ndim != 2 or queries.shape[1] != store.shape[1]:
            raise RuntimeError(f"{what}: expects [Q, F] and [M, F], got {tuple(queries.shape)} and {tuple(store.shape)}")
        if queries.device != store.device:
            raise RuntimeError(f"{what}: tensors on different devices ({queries.device}, {store.device})")
        if queries.dtype != kind.dtype or store.dtype != kind.dtype:
            raise RuntimeError(f"{what}: expects {dtype_name}, got {queries.dtype} and {store.dtype}")
    Q, M, F = queries.shape[0], store.shape[0], store.shape[1:].numel()
    if not isinstance(k, int) or not 1 <= k <= kind.max_k:
        raise RuntimeError(f"{what}: k = {k} neighbours, 1 to {kind.max_k} are supported")
    if Q < 1 or F < 1 or (flatten and M < 1):
        raise RuntimeError(f"{what}: empty queries {list(queries.shape)} or {noun} {list(store.shape)}" if flatten else
                           f"{what}: empty queries {tuple(queries.shape)}")
    if exclude is not None:
        if flatten and not isinstance(exclude, torch.Tensor):
            raise RuntimeError(f"{what}: exclude must be a torch tensor, got {type(exclude).__name__}")
        if not isinstance(exclude, torch.Tensor) or exclude.dtype != torch.int32 or list(exclude.shape) != [Q]:
            raise RuntimeError(f"{what}: exclude must be int32 {[Q]}, got {exclude.dtype} {list(exclude.shape)}" if flatten else
                               f"{what}: exclude must be an int32 tensor {[Q]}, got {getattr(exclude, 'dtype', type(exclude).__name__)} "
                               f"{list(getattr(exclude, 'shape', []))}")
        if exclude.device != store.device:
            raise RuntimeError(f"{what}: exclude is on {exclude.device}, the {noun} on {store.device}")
        if not exclude.is_contiguous():
            raise RuntimeError(f"{what}: exclude must be dense; call .contiguous() first")
    if M < k:
        raise RuntimeError(f"{what}: the {noun} has {M} rows, {k} neighbours need {k}")
    if exclude is not None and M == k and bool(((exclude >= 0) & (exclude < M)).any()):
        raise RuntimeError(f"{what}: the {noun} has {M} rows and one is excluded, {k} neighbours need {k + 1}")
    return Q, M, F


def select(d2, k, exclude, cols, worst):
    """d2 [q, M] of a block of queries, exclude [q] or None, cols = arange(M) -> (d2 [q, k], index int32 [q, k]) ascending by (d2, row),
    row exclude[i] left out (its distance replaced by `worst`, which no distance reaches)"""
    key = d2 if exclude is None else torch.where(cols[None, :] == exclude[:, None].to(torch.int64), worst, d2)
    order = torch.sort(key, dim=1, stable=True).indices[:, :k]          # stable: ties go to the lower row
    return d2.gather(1, order), order.to(torch.int32)


def run_device(what, kind, queries, store, Q, M, F, k, exclude):
    """the device path behind `check` and the op's own limits on F: row limit, dense, 16-byte aligned; the workspace; the call"""
    if Q > kind.max_rows or M > kind.max_rows:
        raise RuntimeError(f"{what}: {Q} queries / {M} {kind.rows}, at most {kind.max_rows} each for the device path")
    for name, t in (("queries", queries), (kind.noun, store)):
        _require_dense(what, name, t)
        if t.data_ptr() % 16:
            raise RuntimeError(f"{what}: queries and {kind.noun} must be 16-byte aligned for the device path" if kind.flatten else
                               f"{what}: {name} must be 16-byte aligned for the device path")
    if M == k:
        exclude = None          # `check` has seen that no entry lies in [0, M)
    lib = _lib.load()
    nbytes = getattr(lib, kind.workspace)(Q, M, k)
    if nbytes < 0:
        raise RuntimeError(f"{what}: unsupported sizes Q={Q} M={M} k={k}")
    ws = _lib.workspace(nbytes, store.device, kind.workspace)
    d2 = torch.empty([Q, k], dtype=kind.d2_dtype, device=store.device)
    index = torch.empty([Q, k], dtype=torch.int32, device=store.device)
    _lib.check(getattr(lib, kind.entry)(queries.data_ptr(), store.data_ptr(), Q, M, F, k, _lib.ptr(exclude), d2.data_ptr(), index.data_ptr(), ws.data_ptr(),
                                        _lib.stream_ptr(store.device)), kind.entry)
    return d2, index
