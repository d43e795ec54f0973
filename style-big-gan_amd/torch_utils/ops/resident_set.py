"""A training batch out of a device-resident uint8 image store (csrc/resident_set.hip): gather by slot, mirror, normalise through a table.

The store holds every *stored* image of a data set once, uint8 ``[S, C, H, W]``.  Item ``i`` of the data set is ``store[slot[i]]``, mirrored
along x when ``flip[i]`` is set -- the reference's ``Dataset.__getitem__`` (train_parts/datasets.py:78-83) as two small tables, so x-flip
doubling (``data.mirror``) doubles the tables and not the store.  ``gather`` turns ``B`` such items into a batch: uint8 as the ``basic``
loader delivers it, or fp32 through a table of the 256 values a byte can become.  The kernel does no floating-point arithmetic;
``normalisation_table`` evaluates the trainer's own expression ``img.to(torch.float32) / 127.5 - 1`` (reference trainers.py:716) over
0..255 on the device the trainer would have evaluated it on, so a resident-fed run sees the bits a ``basic``-fed run sees whichever way that
device rounds the division.

``gather_reference`` is the same semantics in plain torch indexing; CPU tensors take it (the loader works without a GPU).  On the device an
unsupported input is an error, never a quiet torch fallback.
"""
import numpy as np
import torch

from ... import _lib


def normalisation_table(device):
    """-> fp32 [256] on `device`: the trainer's normalisation of every byte value, evaluated there"""
    return torch.arange(256, dtype=torch.uint8, device=device).to(torch.float32) / 127.5 - 1


def tables(dataset):
    """-> (raw, slot, flip) of a `train_parts.datasets.Dataset`: `raw` int64 ndarray, the sorted distinct stored images the data set uses
    (the store's order); `slot` int32 tensor [len(dataset)], the position of item i's stored image in `raw`; `flip` uint8 tensor
    [len(dataset)], 1 where item i is the mirrored copy.  Mirroring doubles len(dataset), not `raw`."""
    raw_idx = np.asarray(dataset._raw_idx, dtype=np.int64)
    raw = np.unique(raw_idx)
    slot = np.searchsorted(raw, raw_idx).astype(np.int32)
    flip = np.ascontiguousarray(np.asarray(dataset._xflip, dtype=np.uint8))
    return raw, torch.from_numpy(slot), torch.from_numpy(flip)


def _check(store, slot, flip, lut, what):
    for name, t, dtype, ndim in (("store", store, torch.uint8, 4), ("slot", slot, torch.int32, 1), ("flip", flip, torch.uint8, 1), ("lut", lut, torch.float32, 1)):
        if t is None and name in ("flip", "lut"):
            continue
        if not isinstance(t, torch.Tensor):
            raise RuntimeError(f"{what}: {name} must be a torch tensor, got {type(t).__name__}")
        if t.dtype != dtype or t.ndim != ndim:
            raise RuntimeError(f"{what}: {name} must be {str(dtype).replace('torch.', '')} with {ndim} dimension(s), got {t.dtype} {list(t.shape)}")
        if t.device != store.device:
            raise RuntimeError(f"{what}: {name} is on {t.device}, the store on {store.device}")
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: {name} must be dense (shape {list(t.shape)}, strides {list(t.stride())}); call .contiguous() first")
    if store.numel() == 0 or slot.numel() == 0:
        raise RuntimeError(f"{what}: empty store {list(store.shape)} or batch {list(slot.shape)}")
    if flip is not None and flip.shape != slot.shape:
        raise RuntimeError(f"{what}: flip {list(flip.shape)} does not match slot {list(slot.shape)}")
    if lut is not None and lut.numel() != 256:
        raise RuntimeError(f"{what}: the table must hold 256 values, got {lut.numel()}")


def gather_reference(store, slot, flip, lut=None):
    """the semantics of `gather` in torch indexing, on the tensors' own device: uint8 [B, C, H, W] (fp32 through `lut` when given); an
    image whose slot lies outside [0, S) is 0 (NaN)"""
    _check(store, slot, flip, lut, "resident_set gather_reference")
    S = store.shape[0]
    idx = slot.to(torch.int64)
    ok = (idx >= 0) & (idx < S)
    img = store[idx.clamp(0, S - 1)]
    if flip is not None:
        img = torch.where(flip.to(torch.bool)[:, None, None, None], img.flip(3), img)
    if lut is None:
        return torch.where(ok[:, None, None, None], img, torch.zeros_like(img))
    out = lut[img.to(torch.int64)]
    return torch.where(ok[:, None, None, None], out, torch.full_like(out, float("nan")))


def gather(store, slot, flip, lut=None, out=None):
    """-> out[b, c, y, x] = store[slot[b], c, y, flip[b] ? W - 1 - x : x] as uint8 [B, C, H, W], or lut[that byte] as fp32 when `lut`
    (fp32 [256]) is given.  `store` uint8 [S, C, H, W], `slot` int32 [B], `flip` uint8 [B] or None, all dense and on one device.  Device
    tensors run the kernel on the current stream (no allocation besides the result, no synchronisation); CPU tensors take `gather_reference`.
    `out`, when given, is the dense tensor of the result's shape, dtype and device that receives it."""
    what = "resident_set gather"
    _check(store, slot, flip, lut, what)
    S, C, H, W = store.shape
    B = slot.shape[0]
    dtype = torch.uint8 if lut is None else torch.float32
    if out is not None and (not isinstance(out, torch.Tensor) or out.dtype != dtype or list(out.shape) != [B, C, H, W] or out.device != store.device
                            or not out.is_contiguous()):
        raise RuntimeError(f"{what}: out must be a dense {str(dtype).replace('torch.', '')} tensor {[B, C, H, W]} on {store.device}")
    if store.device.type != "cuda":
        ref = gather_reference(store, slot, flip, lut)
        return ref if out is None else out.copy_(ref)
    if C * H * W > 0x7fffffff - 256:
        raise RuntimeError(f"{what}: images of {C} x {H} x {W} values are too large for the device path")
    if out is None:
        out = torch.empty([B, C, H, W], dtype=dtype, device=store.device)
    _lib.check(_lib.load().sbg_u8_gather_images(store.data_ptr(), S, C, H, W, slot.data_ptr(), _lib.ptr(flip), B, out.data_ptr(),
                                                0 if lut is None else 1, _lib.ptr(lut), _lib.stream_ptr(store.device)), "sbg_u8_gather_images")
    return out
