"""Arithmetic of the latent directions tool (csrc/directions.hip; GANSpace: Harkonen et al., NeurIPS 2020; SeFa: Shen & Zhou, CVPR 2021).
Every function has ONE definition for both devices: device tensors run the HIP kernels, CPU tensors run the same arithmetic, in the same
order, in numpy through ``_exact_common`` -- the results are equal bit for bit, not close (DESIGN.md section 25 states the orders).

    column_mean(x)                 fp32 [N, D] -> float64 [D]: float64 column sums in the ``chunked_sum_np`` order (chunks of 1024 rows; lane t of
                                   256 adds the rows t, t + 256, ...; ``block_sum``; the chunk sums merged the same way), divided once by N
    gram(x, mean)                  fp32 [N, D], fp32 [D] | None -> float64 [D, D], in this order, which is the contract:
                                     1. c[n, i] = x[n, i] - mean[i], one fp32 subtraction (``mean=None``: c = x);
                                     2. the rows are cut into chunks of CHUNK_ROWS = 256; a chunk with an odd row count gets one more row of +0.0
                                        (after centring), so the chain always runs over whole 2-row matrix-core steps;
                                     3. per chunk q, P_q[i, j] = the fp32 chain from +0.0 over the rows in ascending order,
                                        acc = fmaf(c[n, i], c[n, j], acc) (on the device: v_mfma_f32_32x32x2_f32, that chain bit for bit);
                                     4. per group g of GROUP_CHUNKS = 16 consecutive chunks, the sequential float64 sum
                                        S_g = ((0 + (double)P_0) + (double)P_1) + ... in chunk order;
                                     5. G[i, j] = the ``strided_sum_np`` (csrc/merge.h, div = 1) sum of the S_g over g.
                                   The order depends on (N, D) alone; G is symmetric bit for bit (fmaf(a, b, .) = fmaf(b, a, .)).
    edit_table(ws, comps, scale, sigmas, layers)
                                   fp32 [S, L, D], [K, D], [K], [T] -> fp32 [S K T, L, D]: row (s K + k) T + t is ws[s] with
                                   fmaf(sigmas[t] * scale[k], comps[k, d], ws[s, l, d]) on the layers in ``layers`` (the step one fp32 product), a
                                   copy on the others.  No truncation.  S K T = 0 gives an empty table.

All three refuse a wrong dtype, non-dense input, tensors on different devices, N < 1 and D outside 1 .. MAX_D with a message that names the shape.
The CPU path of ``gram`` emulates fmaf in numpy (about 110 ns per element of the upper triangle and row): it is meant for small N.
"""
import numpy as np
import torch

from ... import _lib
from ._exact_common import chunked_sum_np, fma32, strided_sum_np

MAX_D = 1024
MEAN_ROWS = 1024            # rows per chunk of column_mean
CHUNK_ROWS = 256            # rows per fp32 chain of gram
GROUP_CHUNKS = 16           # chunks per sequential float64 sum of gram
_CPU_ELEMENTS = 1 << 21     # chains the CPU path of gram advances together (bounds its temporaries)
_MERGE_VALUES = 1 << 14     # values the CPU path of gram merges together (strided_sum_np pads each to 256 lanes)


def _dense_f32(t, what, shape_text, ndim):
    if t.dtype != torch.float32 or t.ndim != ndim or not t.is_contiguous():
        raise RuntimeError(f"{what}: expects a dense float32 {shape_text}, got {t.dtype} of shape {tuple(t.shape)} with strides {t.stride()}")
    return t


def _table(x, what):
    _dense_f32(x, what, "[N, D]", 2)
    n, d = x.shape
    if n < 1 or not 1 <= d <= MAX_D:
        raise RuntimeError(f"{what}: shape {tuple(x.shape)} is not [N >= 1, 1 <= D <= {MAX_D}]")
    return n, d


def column_mean(x):
    n, d = _table(x, "directions.column_mean")
    if x.device.type != "cuda":
        return torch.from_numpy(chunked_sum_np(np.ascontiguousarray(x.numpy().astype(np.float64).T), MEAN_ROWS) / np.float64(n))
    lib = _lib.load()
    ws = _lib.workspace(lib.sbg_directions_mean_workspace(n, d), x.device, "sbg_directions_mean_workspace")
    out = torch.empty([d], dtype=torch.float64, device=x.device)
    _lib.check(lib.sbg_directions_mean(x.data_ptr(), out.data_ptr(), ws.data_ptr(), n, d, _lib.stream_ptr(x.device)), "sbg_directions_mean")
    return out


def _chains(c, iu, ju):
    """c fp32 [Q, R, D] -> fp32 [Q, P]: per chunk and upper-triangle pair p = (iu[p], ju[p]), the fmaf chain from +0.0 over the R rows"""
    q, r, _ = c.shape
    out = np.empty([q, len(iu)], dtype=np.float32)
    step = max(_CPU_ELEMENTS // len(iu), 1)
    for lo in range(0, q, step):
        blk = c[lo:lo + step]
        acc = np.zeros([blk.shape[0], len(iu)], dtype=np.float32)
        for n in range(r):
            acc = fma32(blk[:, n, iu], blk[:, n, ju], acc)
        out[lo:lo + step] = acc
    return out


def _gram_np(x, mean):
    n, d = x.shape
    c = x - mean[None, :] if mean is not None else x
    iu, ju = np.triu_indices(d)
    full = n // CHUNK_ROWS
    parts = []
    if full:
        parts.append(_chains(c[:full * CHUNK_ROWS].reshape(full, CHUNK_ROWS, d), iu, ju))
    tail = n - full * CHUNK_ROWS
    if tail:
        rows = c[full * CHUNK_ROWS:]
        if tail & 1:
            rows = np.concatenate([rows, np.zeros([1, d], dtype=np.float32)])      # the odd-row rule: one row of +0.0 after centring
        parts.append(_chains(rows[None], iu, ju))
    p = np.concatenate(parts).astype(np.float64)           # [chunks, P]
    chunks = p.shape[0]
    groups = -(-chunks // GROUP_CHUNKS)
    s = np.zeros([groups, len(iu)], dtype=np.float64)
    for g in range(groups):
        for q in range(g * GROUP_CHUNKS, min((g + 1) * GROUP_CHUNKS, chunks)):
            s[g] = s[g] + p[q]
    s = np.ascontiguousarray(s.T)
    tri = np.concatenate([strided_sum_np(s[lo:lo + _MERGE_VALUES]) for lo in range(0, len(iu), _MERGE_VALUES)])
    out = np.empty([d, d], dtype=np.float64)
    out[iu, ju] = tri
    out[ju, iu] = tri
    return out


def gram(x, mean=None):
    what = "directions.gram"
    n, d = _table(x, what)
    if mean is not None:
        if mean.dtype != torch.float32 or tuple(mean.shape) != (d,) or not mean.is_contiguous() or mean.device != x.device:
            raise RuntimeError(f"{what}: mean ({mean.dtype} {tuple(mean.shape)} on {mean.device}) must be a dense float32 [{d}] on the device of "
                               f"x {tuple(x.shape)}, {x.device}")
    if x.device.type != "cuda":
        return torch.from_numpy(_gram_np(x.numpy(), None if mean is None else mean.numpy()))
    lib = _lib.load()
    ws = _lib.workspace(lib.sbg_directions_gram_workspace(n, d), x.device, "sbg_directions_gram_workspace")
    out = torch.empty([d, d], dtype=torch.float64, device=x.device)
    _lib.check(lib.sbg_directions_gram(x.data_ptr(), None if mean is None else mean.data_ptr(), out.data_ptr(), ws.data_ptr(), n, d,
                                       _lib.stream_ptr(x.device)), "sbg_directions_gram")
    return out


def edit_table(ws, comps, scale, sigmas, layers):
    what = "directions.edit_table"
    _dense_f32(ws, what, "[S, L, D]", 3)
    s, l, d = ws.shape
    for name, v, ndim in (("comps", comps, 2), ("scale", scale, 1), ("sigmas", sigmas, 1)):
        _dense_f32(v, f"{what} ({name})", "[K, D]" if ndim == 2 else "vector", ndim)
        if v.device != ws.device:
            raise RuntimeError(f"{what}: {name} is on {v.device}, ws {tuple(ws.shape)} on {ws.device}")
    k, t = comps.shape[0], sigmas.shape[0]
    if l < 1 or not 1 <= d <= MAX_D or comps.shape[1] != d or scale.shape[0] != k:
        raise RuntimeError(f"{what}: ws {tuple(ws.shape)}, comps {tuple(comps.shape)}, scale {tuple(scale.shape)}: expects [S, L >= 1, 1 <= D <= {MAX_D}], "
                           "[K, D] and [K]")
    layers = sorted({int(i) for i in layers})
    if not layers or layers[0] < 0 or layers[-1] >= l:
        raise RuntimeError(f"{what}: layers {layers} must be a non-empty set of indices in [0, {l}) for ws {tuple(ws.shape)}")
    rows = s * k * t
    if rows == 0:
        return torch.empty([0, l, d], dtype=torch.float32, device=ws.device)
    if ws.device.type != "cuda":
        wn, cn = ws.numpy(), comps.numpy()
        step = sigmas.numpy()[None, :] * scale.numpy()[:, None]                 # [K, T], one fp32 product
        out = np.broadcast_to(wn[:, None, None], [s, k, t, l, d]).copy()
        shape = [s, k, t, len(layers), d]
        out[:, :, :, layers] = fma32(np.broadcast_to(step[None, :, :, None, None], shape), np.broadcast_to(cn[None, :, None, None, :], shape),
                                     np.broadcast_to(wn[:, None, None, layers], shape))
        return torch.from_numpy(out.reshape(rows, l, d))
    mask = torch.zeros([l], dtype=torch.int32)
    mask[layers] = 1
    mask = mask.to(ws.device)
    out = torch.empty([rows, l, d], dtype=torch.float32, device=ws.device)
    _lib.check(_lib.load().sbg_directions_edit(ws.data_ptr(), comps.data_ptr(), scale.data_ptr(), sigmas.data_ptr(), mask.data_ptr(), out.data_ptr(),
                                               s, l, d, k, t, _lib.stream_ptr(ws.device)), "sbg_directions_edit")
    return out
