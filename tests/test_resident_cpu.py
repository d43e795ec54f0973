"""The device-resident training set loader, host side: the slot / flip / label tables and `gather_reference` against the data set's own
items, the loader against the 'basic' loader batch for batch, what the build promises (one decode per stored image, independence of
the pool and of the staging chunks), the size rule and the configuration surface.  Everything here runs the loader with device='cpu'."""
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import arguments, starter
from style_big_gan_amd.torch_utils import misc
from style_big_gan_amd.torch_utils.ops import resident_set
from style_big_gan_amd.train_parts import dataloaders as DL
import resident_util as R


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("resident")
    return {"dir": R.make_image_folder(str(tmp / "data")), "zip": R.make_image_folder(str(tmp / "dataz"), as_zip=True)}


def _loader(ds, rank=0, replicas=1, cls=DL.ResidentDataloader, **kw):
    return cls(dataset=ds, sampler=misc.InfiniteSampler(ds, rank=rank, num_replicas=replicas, seed=1), batch_size=4, device="cpu", **kw)


@pytest.mark.parametrize("case", list(R.DATASET_CASES))
@pytest.mark.parametrize("source", ["dir", "zip"])
def test_items_equal_the_data_sets(folders, source, case):
    """for every item: the gathered image is the data set's image byte for byte, the label table's row its label; the store holds each
    distinct stored image once, mirrored or not"""
    kw, distinct = R.DATASET_CASES[case]
    ds = R.image_folder_class()(path=folders[source], **kw)
    raw, slot, flip = resident_set.tables(ds)
    assert len(raw) == distinct and np.array_equal(raw, np.unique(ds._raw_idx)) and len(ds) == distinct * (2 if kw.get("xflip") else 1)
    assert slot.dtype == torch.int32 and flip.dtype == torch.uint8 and slot.shape == flip.shape == (len(ds),)
    assert np.array_equal(raw[slot.numpy()], ds._raw_idx) and np.array_equal(flip.numpy(), ds._xflip)
    loader = _loader(ds)
    store = R.numpy_store(ds, raw)
    assert loader.store.dtype == torch.uint8 and torch.equal(loader.store, store)
    assert loader.store_bytes == store.numel() and loader._labels.shape == (len(ds), ds.label_dim) and loader._labels.dtype == torch.float32
    assert ds.label_dim == (4 if kw.get("use_labels") else 0)
    for i in range(len(ds)):
        img, lab = ds[i]
        got = resident_set.gather_reference(store, slot[i:i + 1], flip[i:i + 1])
        assert got.dtype == torch.uint8 and np.array_equal(got[0].numpy(), img), i
        assert torch.equal(resident_set.gather(store, slot[i:i + 1], flip[i:i + 1]), got)       # CPU tensors take the reference
        assert np.array_equal(loader._labels[i].numpy(), lab), i
    ds.close()


def test_batches_equal_the_basic_loader(folders):
    """two ranks of one sampler, past the windowed reshuffle and the wrap: the same uint8 images and labels as the stock DataLoader, and
    the normalised stream is the trainer's expression of them bit for bit"""
    ds = R.image_folder_class()(path=folders["dir"], xflip=True, use_labels=True)
    n = math.ceil(2.5 * len(ds) / 4)
    assert len(ds) == 28 and n == 18
    for rank in (0, 1):
        basic = iter(DL.dataloaders["basic"](dataset=ds, sampler=misc.InfiniteSampler(ds, rank=rank, num_replicas=2, seed=1), batch_size=4, num_workers=0))
        res = _loader(ds, rank, 2, index_block=5)       # 18 batches cross three index blocks
        raw_it, norm_it = iter(res), res.batches(normalized=True)
        for k in range(n):
            img, lab = next(basic)
            rimg, rlab = next(raw_it)
            nimg, nlab = next(norm_it)
            assert rimg.dtype == torch.uint8 and rlab.dtype == torch.float32 and nimg.dtype == torch.float32
            assert torch.equal(rimg, img) and torch.equal(rlab, lab), (rank, k)
            assert torch.equal(nimg, img.to(torch.float32) / 127.5 - 1) and torch.equal(nlab, lab), (rank, k)
    finite = DL.ResidentDataloader(dataset=ds, sampler=list(range(10)), batch_size=4, device="cpu", index_block=2)
    assert [b[0].shape[0] for b in finite] == [4, 4, 2]         # a finite sampler: the stock loader's batches, the last one short


def test_build_decodes_once_and_does_not_depend_on_the_pool_or_the_chunks(folders):
    ds = R.counting_dataset(path=folders["zip"], xflip=True)
    raw, _, _ = resident_set.tables(ds)
    want = R.numpy_store(ds, raw)
    image_bytes = int(np.prod(ds.image_shape))

    class SmallChunks(DL.ResidentDataloader):
        STAGING_BYTES = 3 * image_bytes + 1         # 3 images per chunk: 14 images in 5 chunks over two staging buffers

    class OneImageChunks(DL.ResidentDataloader):
        STAGING_BYTES = 1                           # less than an image: one image per chunk

    for cls, workers in ((DL.ResidentDataloader, 1), (DL.ResidentDataloader, 4), (SmallChunks, 1), (SmallChunks, 4), (OneImageChunks, 3)):
        ds.decoded = []
        loader = _loader(ds, cls=cls, workers=workers)
        assert sorted(ds.decoded) == raw.tolist(), (cls.__name__, workers)       # every stored image exactly once, the mirror costs nothing
        assert torch.equal(loader.store, want), (cls.__name__, workers)
        for _ in zip(range(3), loader):
            pass
        assert len(ds.decoded) == len(raw)                                      # iterating decodes nothing


def test_images_of_another_shape_are_refused(folders):
    ds = R.image_folder_class()(path=folders["dir"])
    ds._raw_shape[2] += 1
    with pytest.raises(AssertionError):
        _loader(ds)


def test_size_rule(folders, monkeypatch):
    ds = R.counting_dataset(path=folders["dir"], xflip=True, use_labels=True)
    store_bytes, table_bytes = DL.resident_footprint(ds)
    assert store_bytes == 14 * 3 * 16 * 16 and table_bytes == 28 * (4 + 1 + 4 * 4) + 1024
    seen = []
    monkeypatch.setattr(DL, "free_device_bytes", lambda device: seen.append(device) or 2 * store_bytes - 1)
    with pytest.raises(ValueError, match=r"data\.dataloader=basic") as err:
        _loader(ds)
    assert str(store_bytes + table_bytes) in str(err.value) and str((2 * store_bytes - 1) // 2) in str(err.value)
    assert ds.decoded == [] and seen == [torch.device("cpu")]                   # refused before any decode
    monkeypatch.setattr(DL, "free_device_bytes", lambda device: 2 * (store_bytes + table_bytes))
    assert _loader(ds).store.shape[0] == 14                                    # exactly half of the free memory is enough
    ds.decoded = []
    with pytest.raises(ValueError, match="max_gib"):                            # max_gib rules, whatever is free
        _loader(ds, max_gib=(store_bytes + table_bytes - 1) / 2 ** 30)
    assert ds.decoded == []
    monkeypatch.setattr(DL, "free_device_bytes", lambda device: 1)
    assert _loader(ds, max_gib=(store_bytes + table_bytes + 1) / 2 ** 30).store.shape[0] == 14


def test_gather_refuses_what_it_does_not_support():
    store = torch.zeros([3, 1, 2, 4], dtype=torch.uint8)
    slot, flip = torch.tensor([0, 2], dtype=torch.int32), torch.tensor([0, 1], dtype=torch.uint8)
    for bad in (dict(store=store.float()), dict(slot=slot.long()), dict(flip=flip.bool()), dict(flip=flip[:1]), dict(lut=torch.zeros(255)),
                dict(store=store[:, :, :, ::2]), dict(lut=torch.zeros(256, dtype=torch.float64)), dict(out=torch.zeros([2, 1, 2, 4]))):
        with pytest.raises(RuntimeError, match="resident_set"):
            resident_set.gather(**dict(dict(store=store, slot=slot, flip=flip), **bad))
    out_of_range = resident_set.gather_reference(store + 7, torch.tensor([-1, 1, 3], dtype=torch.int32), None, torch.arange(256, dtype=torch.float32))
    assert torch.isnan(out_of_range[0]).all() and torch.isnan(out_of_range[2]).all() and bool((out_of_range[1] == 7).all())
    assert not resident_set.gather_reference(store + 7, torch.tensor([-1, 3], dtype=torch.int32), None).any()
    lut = resident_set.normalisation_table("cpu")
    assert lut.dtype == torch.float32 and lut.shape == (256,) and lut[0] == -1 and lut[255] == 1


def test_configuration_surface(folders, tmp_path):
    defaults = arguments.structured_defaults().dataloaders_args.resident
    assert {k: defaults[k] for k in ("device", "workers", "max_gib", "index_block")} == dict(device=None, workers=4, max_gib=None, index_block=64)
    assert arguments.structured_defaults().data.dataloader == "basic"          # no default changes
    argv = R.write_config(tmp_path, R.DCGAN_LIKE, folders["dir"], "data.dataloader=resident", "dataloaders_args.resident.workers=2")
    cfg = arguments.load_config(argv)
    assert cfg.data.dataloader == "resident" and cfg.dataloaders_args.resident.workers == 2 and cfg.dataloaders_args.resident.index_block == 64
    from style_big_gan_amd.train_parts.trainers import trainers
    tr = trainers[cfg.exp.trainer]().setup_arguments(cfg)
    assert tr.data_loader_kwargs == dict(workers=2, max_gib=None, index_block=64)      # the device is the trainer's to pass, not a setting
    with pytest.raises(ValueError, match="device"):
        trainers[cfg.exp.trainer]().setup_arguments(arguments.load_config(argv + ["dataloaders_args.resident.device=cpu"]))
    assert DL.accepts_device(DL.dataloaders["resident"]) and not DL.accepts_device(DL.dataloaders["basic"])


def test_training_through_the_resident_loader(tmp_path):
    """a DCGAN-like trainer over an image folder, two iterations fed by `next_images` from the resident store; the same trainer on 'basic'
    is fed the same bits"""
    path = R.make_image_folder(str(tmp_path / "data"), n=12, res=32)
    runs = {}
    for name in ("resident", "basic"):
        argv = R.write_config(tmp_path, R.DCGAN_LIKE, path, f"data.dataloader={name}", "data.mirror=true", "dataloaders_args.basic.num_workers=0",
                              "dataloaders_args.resident.workers=2")
        t = runs[name] = starter.main(argv, max_iterations=2)
        assert t.engine.batch_idx == 2 and len(t.dataset) == 24 and all(torch.isfinite(p).all() for p in t.engine.G.parameters())
    res, basic = runs["resident"], runs["basic"]
    assert res.training_image_iterator is not None and basic.training_image_iterator is None
    assert res.data_loader_kwargs["device"] == res.device() and "device" not in basic.data_loader_kwargs
    for _ in range(3):
        (a, ca), (b, cb) = res.next_images(8, res.device()), basic.next_images(8, basic.device())
        assert a.dtype == torch.float32 and a.device.type == res.device().type and torch.equal(a, b) and torch.equal(ca, cb)
    img, c = res.next_batch(8, res.device())                                    # next_batch keeps its contract
    assert img.dtype == torch.uint8 and tuple(img.shape) == (8, 3, 32, 32) and tuple(c.shape) == (8, 0)
