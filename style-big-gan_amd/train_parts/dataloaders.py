"""Data loaders (reference ``train_parts/dataloaders.py:7-12``): stock ``torch.utils.data.DataLoader`` under the name 'basic' with the
reference's defaults (pinned host buffers, 3 workers, prefetch 2); fed by ``misc.InfiniteSampler`` it is an endless stream of
``(uint8 [B, C, H, W], float32 [B, label_dim])`` batches sharded by rank.

'resident' is this build's own: the data set is decoded once into one uint8 tensor on the training device and every batch is one small
index upload and one gather kernel (``torch_utils/ops/resident_set.py``) -- no worker processes, no image traffic over PCIe, no host
work that grows with the resolution."""
import concurrent.futures
import inspect
import itertools

import numpy as np
import torch

from .. import utils
from ..torch_utils.ops import resident_set

dataloaders = utils.ClassRegistry()


@dataloaders.add_to_registry("basic")
class BasicDataloader(torch.utils.data.DataLoader):
    def __init__(self, pin_memory=True, num_workers=3, prefetch_factor=2, **args):
        if num_workers == 0:
            prefetch_factor = None          # torch rejects a prefetch factor without workers
        super().__init__(pin_memory=pin_memory and torch.cuda.is_available(), num_workers=num_workers, prefetch_factor=prefetch_factor, **args)


def free_device_bytes(device):
    """free memory of `device` in bytes, None where there is no figure (the CPU); the resident loader's size rule reads it through this
    module attribute, so the rule can be exercised without a device"""
    device = torch.device(device)
    if device.type != "cuda":
        return None
    return torch.cuda.mem_get_info(device)[0]


def resident_footprint(dataset):
    """-> (store bytes, table bytes) the resident loader allocates for `dataset`: every distinct stored image once as uint8, and per item a
    slot (int32), a flip flag (uint8) and a label row (fp32), plus the 256-entry normalisation table"""
    raw, slot, _ = resident_set.tables(dataset)
    c, h, w = dataset.image_shape
    return len(raw) * c * h * w, slot.numel() * (4 + 1 + 4 * int(dataset.label_dim)) + 256 * 4


def accepts_device(loader_class):
    """whether a registered loader class takes the training device as `device=` (the stock DataLoader does not)"""
    return "device" in inspect.signature(loader_class.__init__).parameters


@dataloaders.add_to_registry("resident")
class ResidentDataloader:
    """The whole training set as one uint8 tensor ``[stored images, C, H, W]`` on `device`, built once in the constructor; an endless
    (as long as `sampler` is) stream of batches gathered from it.

    Build: every stored image the data set uses is decoded exactly once through ``dataset._load_raw_image`` by a pool of `workers`
    threads (PIL releases the GIL while it decodes) into pinned staging chunks of at most ``STAGING_BYTES``, which are copied
    asynchronously into the store in the order of ``resident_set.tables(dataset)[0]``, whatever order the pool finishes in.  Labels
    become one fp32 table ``[len(dataset), label_dim]``.  Before anything is allocated or decoded the store and its tables must fit
    `max_gib` GiB when that is given, else half of the device's free memory; a ``ValueError`` says otherwise and points to the
    'basic' loader.  Images of differing shape are refused as ``Dataset.__getitem__`` refuses them.

    Iteration: ``iter(loader)`` yields ``(uint8 [B, C, H, W], float32 [B, label_dim])`` on `device` -- the 'basic' contract with device
    tensors; ``loader.batches(normalized=True)`` yields the images as fp32 through ``resident_set.normalisation_table(device)``, bit for bit
    ``img.to(torch.float32) / 127.5 - 1`` evaluated on `device`.  Indices come from `sampler`, `batch_size` consecutive ones per batch as
    the stock DataLoader takes them; they go up `index_block` batches at a time from a pinned buffer without blocking, so the sampler
    runs up to `index_block` batches ahead of the consumer.  A step is then one ``index_select`` per table per block and one gather
    kernel per batch; in steady state ``next()`` does not synchronise the host with the device.

    Every rank of a multi-GPU run builds the FULL store on its own device: the rank-sharded sampler deals any index to any rank (its
    windowed reshuffle moves indices between the ranks' streams), so no rank can know a subset it will be asked for."""

    STAGING_BYTES = 64 << 20        # upper bound of one pinned staging chunk (two are in use)

    def __init__(self, dataset, sampler, batch_size, device=None, workers=4, max_gib=None, index_block=64):
        if device is None:
            device = torch.device("cuda", torch.cuda.current_device()) if torch.cuda.is_available() else torch.device("cpu")
        self.dataset, self.sampler, self.batch_size = dataset, sampler, int(batch_size)
        self.device, self.workers, self.index_block = torch.device(device), max(int(workers), 1), max(int(index_block), 1)
        if self.batch_size < 1:
            raise ValueError(f"resident loader: batch_size must be positive, got {batch_size}")
        raw, slot, flip = resident_set.tables(dataset)
        self.store_bytes, self.table_bytes = resident_footprint(dataset)
        need = self.store_bytes + self.table_bytes
        if max_gib is not None:
            limit, rule = int(float(max_gib) * 2 ** 30), f"dataloaders_args.resident.max_gib={max_gib}"
        else:
            free = free_device_bytes(self.device)
            limit, rule = (None, "") if free is None else (int(free) // 2, f"half of the {int(free)} bytes free on {self.device}")
        if limit is not None and need > limit:
            raise ValueError(f"resident loader: the store and its tables need {need} bytes ({need / 2 ** 30:.3f} GiB), more than the {limit} bytes "
                             f"({limit / 2 ** 30:.3f} GiB) allowed by {rule}; use data.dataloader=basic for this data set")
        self._slot, self._flip = slot.to(self.device), flip.to(self.device)
        labels = np.stack([dataset.get_label(i) for i in range(len(dataset))]).astype(np.float32).reshape(len(dataset), -1)
        self._labels = torch.from_numpy(labels).to(self.device)
        self._lut = resident_set.normalisation_table(self.device)
        self.store = self._build(raw)

    def _build(self, raw):
        dataset, dev = self.dataset, self.device
        shape = list(dataset.image_shape)
        image_bytes = int(np.prod(shape))
        per_chunk = max(1, min(self.STAGING_BYTES // image_bytes, len(raw)))
        on_gpu = dev.type == "cuda"
        store = torch.empty([len(raw)] + shape, dtype=torch.uint8, device=dev)
        staging = [torch.empty([per_chunk] + shape, dtype=torch.uint8, pin_memory=on_gpu) for _ in range(2 if len(raw) > per_chunk else 1)]
        copied = [None] * len(staging)                          # per staging chunk, the event behind its last copy into the store

        def decode(dst, raw_idx):
            image = dataset._load_raw_image(raw_idx)
            assert isinstance(image, np.ndarray) and image.dtype == np.uint8 and list(image.shape) == shape, \
                f"stored image {raw_idx} is {getattr(image, 'dtype', type(image))} {list(getattr(image, 'shape', []))}, the data set says uint8 {shape}"
            dst[...] = image

        with concurrent.futures.ThreadPoolExecutor(max_workers=self.workers) as pool:
            for k, lo in enumerate(range(0, len(raw), per_chunk)):
                hi = min(lo + per_chunk, len(raw))
                buf = staging[k % len(staging)]
                if copied[k % len(staging)] is not None:
                    copied[k % len(staging)].synchronize()      # the chunk's previous contents have reached the store
                view = buf.numpy()
                first = 0
                if k == 0:                                      # the first read on this thread: a lazily opened archive is opened once
                    decode(view[0], raw[lo])
                    first = 1
                for _ in pool.map(decode, view[first:hi - lo], raw[lo + first:hi]):     # rows are fixed by position: completion order is irrelevant
                    pass
                store[lo:hi].copy_(buf[:hi - lo], non_blocking=True)
                if on_gpu:
                    copied[k % len(staging)] = torch.cuda.Event()
                    copied[k % len(staging)].record(torch.cuda.current_stream(dev))
        if on_gpu:
            torch.cuda.current_stream(dev).synchronize()        # the pinned chunks are released below
        return store

    def __iter__(self):
        return self.batches(normalized=False)

    def batches(self, normalized=False):
        """endless generator of (images, labels) on the device: uint8 images, or with `normalized` the fp32 images the trainer feeds"""
        B, dev = self.batch_size, self.device
        lut = self._lut if normalized else None
        indices = iter(self.sampler)
        while True:
            block = np.fromiter(itertools.islice(indices, B * self.index_block), dtype=np.int64)
            if block.size == 0:
                return
            host = torch.empty([block.size], dtype=torch.int64, pin_memory=dev.type == "cuda")     # from torch's pinned cache: reused once its upload is done
            host.numpy()[:] = block
            idx = host.to(dev, non_blocking=True)
            slot, flip, labels = self._slot.index_select(0, idx), self._flip.index_select(0, idx), self._labels.index_select(0, idx)
            for lo in range(0, block.size, B):
                yield resident_set.gather(self.store, slot[lo:lo + B], flip[lo:lo + B], lut), labels[lo:lo + B]
            if block.size < B * self.index_block:               # a finite sampler ran out
                return
