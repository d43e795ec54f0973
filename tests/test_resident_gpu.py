"""The device-resident training set loader on the device: the gather kernel against `gather_reference` on the same inputs, bit for bit
(both paths, both output types, mirrors, tables, slots outside the store, offsets past 2^32), the loader's steady state without a host
synchronisation, and a trainer fed by it against the same trainer fed by the 'basic' loader."""
import itertools
import os
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import _lib, starter
from style_big_gan_amd.torch_utils import misc
from style_big_gan_amd.torch_utils.ops import resident_set
from style_big_gan_amd.train_parts import dataloaders as DL
import resident_util as R

pytestmark = pytest.mark.gpu

S = 7


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(torch.int32) if a.dtype == torch.float32 else a, b.view(torch.int32) if b.dtype == torch.float32 else b)


def _paths(fn):
    """run fn with the launch log on -> (its result, the path code of every gather launch it made)"""
    _lib.prof_enable(True)
    try:
        _lib.prof_fetch()
        out = fn()
        return out, [r["dims"] for r in _lib.prof_fetch() if r["kind"] == "resident"]
    finally:
        _lib.prof_enable(False)


def _flips(B, dev):
    mixed = torch.tensor([(i * 3 + 1) % 2 for i in range(B)], dtype=torch.uint8, device=dev)
    return {"none": None, "zeros": torch.zeros(B, dtype=torch.uint8, device=dev), "ones": torch.ones(B, dtype=torch.uint8, device=dev), "mixed": mixed}


@pytest.mark.parametrize("W", [4, 8, 12, 16, 5, 6])
def test_gather_equals_the_reference(dev, W):
    """W = 4, 8, 12 (an odd number of dwords: the middle one mirrors onto itself) and 16 take the dword path, 5 and 6 the byte path; with
    H in {1, 3}, C in {1, 3}, B in {1, 5}: slots out of order, repeated and S - 1; every flip pattern; both output types"""
    gen = torch.Generator().manual_seed(W)
    lut = resident_set.normalisation_table(dev)
    want_path = 1 if W % 4 == 0 else 2
    for H, C, B in itertools.product((1, 3), (1, 3), (1, 5)):
        store = torch.randint(0, 256, [S, C, H, W], dtype=torch.uint8, generator=gen).to(dev)
        slot = torch.tensor([S - 1, 2, 2, 0, 5][:B], dtype=torch.int32, device=dev)
        for name, flip in _flips(B, dev).items():
            for table in (None, lut):
                got, dims = _paths(lambda: resident_set.gather(store, slot, flip, table))
                assert _same_bits(got, resident_set.gather_reference(store, slot, flip, table)), (H, C, B, name, table is not None)
                assert dims == [(B, C, H, W, int(table is not None), 0, want_path)], dims


def test_a_store_one_byte_into_its_allocation_takes_the_byte_path(dev):
    C, H, W, B = 3, 3, 8, 5
    n = S * C * H * W
    buf = torch.randint(0, 256, [n + 4], dtype=torch.uint8, generator=torch.Generator().manual_seed(1)).to(dev)
    store = buf[1:1 + n].view(S, C, H, W)
    assert store.data_ptr() % 4 == 1 and store.is_contiguous()
    slot = torch.tensor([S - 1, 2, 2, 0, 5], dtype=torch.int32, device=dev)
    flip = _flips(B, dev)["mixed"]
    for table in (None, resident_set.normalisation_table(dev)):
        got, dims = _paths(lambda: resident_set.gather(store, slot, flip, table))
        assert _same_bits(got, resident_set.gather_reference(store, slot, flip, table)) and [d[6] for d in dims] == [2]
        aligned, dims = _paths(lambda: resident_set.gather(store.clone(), slot, flip, table))
        assert _same_bits(aligned, got) and [d[6] for d in dims] == [1]


def test_the_table_decides_the_values(dev):
    """all 256 byte values through the normalisation table are the trainer's expression evaluated on the device; an arbitrary table
    (-0.0, infinities, a NaN with a payload) comes back bit for bit"""
    store = torch.arange(256, dtype=torch.uint8, device=dev).view(1, 1, 16, 16).repeat(2, 1, 1, 1)
    store[1] = store[1].flip(1)
    slot = torch.tensor([1, 0, 1], dtype=torch.int32, device=dev)
    flip = torch.tensor([0, 1, 1], dtype=torch.uint8, device=dev)
    raw = resident_set.gather(store, slot, flip)
    assert raw.dtype == torch.uint8 and torch.equal(raw, resident_set.gather_reference(store, slot, flip))
    got = resident_set.gather(store, slot, flip, resident_set.normalisation_table(dev))
    assert _same_bits(got, raw.to(torch.float32) / 127.5 - 1)
    bits = torch.randint(-2 ** 31, 2 ** 31, [256], dtype=torch.int64, generator=torch.Generator().manual_seed(2)).to(torch.int32)
    bits[:4] = torch.tensor([-2 ** 31, 0x7f800000, -0x00800000, 0x7fc12345], dtype=torch.int32)       # -0.0, +inf, -inf, NaN with a payload
    table = bits.to(dev).view(torch.float32)
    got = resident_set.gather(store, slot, flip, table)
    assert torch.equal(got.view(torch.int32), bits.to(dev)[raw.to(torch.int64)])
    assert got.view(torch.int32)[1, 0, 0, 15].item() == -2 ** 31 and got.view(torch.int32)[1, 0, 0, 12].item() == 0x7fc12345


@pytest.mark.parametrize("W", [8, 6])
def test_slots_outside_the_store_and_the_bounds_of_out(dev, W):
    """slots -1 and S give an all-NaN (fp32) or all-0 (uint8) image and leave their neighbours exact; the images in front of and behind
    `out` in one allocation are not touched"""
    C, H, B = 3, 3, 5
    store = torch.randint(1, 256, [S, C, H, W], dtype=torch.uint8, generator=torch.Generator().manual_seed(3)).to(dev)
    slot = torch.tensor([3, -1, S - 1, S, 0], dtype=torch.int32, device=dev)
    flip = _flips(B, dev)["mixed"]
    good = torch.tensor([0, 2, 4], device=dev)
    for table, sentinel in ((None, 0xA5), (resident_set.normalisation_table(dev), 12345.0)):
        whole = torch.full([B + 2, C, H, W], sentinel, dtype=torch.uint8 if table is None else torch.float32, device=dev)
        got = resident_set.gather(store, slot, flip, table, out=whole[1:B + 1])
        assert got.data_ptr() == whole[1].data_ptr()
        assert bool((whole[0] == sentinel).all()) and bool((whole[B + 1] == sentinel).all())
        for b in (1, 3):
            assert bool(torch.isnan(got[b]).all()) if table is not None else not bool(got[b].any())
        assert _same_bits(got[good], resident_set.gather_reference(store, slot[good].contiguous(), flip[good].contiguous(), table))


def test_offsets_past_4_gib(dev):
    """a store of 21846 images of 3 x 256 x 256 bytes is 4 295 098 368 bytes; slot 10922 straddles 2^31 and slot 21845 ends past 2^32"""
    n, C, H, W = 21846, 3, 256, 256
    assert n * C * H * W > 2 ** 32 and 10922 * C * H * W < 2 ** 31 < 10923 * C * H * W
    store = torch.empty([n, C, H, W], dtype=torch.uint8, device=dev)
    picks = [0, 10922, 21845]
    pattern = torch.randint(0, 256, [3, C, H, W], dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(dev)
    for k, s in enumerate(picks):
        store[s].copy_(pattern[k])
    slot = torch.tensor([21845, 0, 10922], dtype=torch.int32, device=dev)
    flip = torch.tensor([1, 0, 1], dtype=torch.uint8, device=dev)
    want = torch.stack([pattern[2].flip(2), pattern[0], pattern[1].flip(2)])
    got = resident_set.gather(store, slot, flip)
    assert torch.equal(got, want) and torch.equal(got, resident_set.gather_reference(store, slot, flip))
    lut = resident_set.normalisation_table(dev)
    assert _same_bits(resident_set.gather(store, slot, flip, lut), want.to(torch.float32) / 127.5 - 1)
    del store


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    """24 labelled PNGs at 32 x 32"""
    return R.make_image_folder(str(tmp_path_factory.mktemp("resident_gpu") / "data"), n=24, res=32)


def test_steady_state_does_not_synchronise(dev, folder):
    ds = R.image_folder_class()(path=folder, xflip=True, use_labels=True)
    loader = DL.ResidentDataloader(dataset=ds, sampler=misc.InfiniteSampler(ds, seed=1), batch_size=4, device=dev, workers=2, index_block=2)
    assert loader.store.device == dev and loader.store.shape == (24, 3, 32, 32)
    raw, slot, flip = resident_set.tables(ds)
    assert torch.equal(loader.store.cpu(), R.numpy_store(ds, raw))
    stream = loader.batches(normalized=True)
    batches = [next(stream), next(stream)]              # warm-up: one index block
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batches += [next(stream), next(stream), next(stream)]       # the second block's upload and the first batch of the third
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    order = list(itertools.islice(iter(misc.InfiniteSampler(ds, seed=1)), 20))
    for k, (img, lab) in enumerate(batches):
        idx = order[4 * k:4 * k + 4]
        want = torch.stack([torch.from_numpy(ds[i][0]) for i in idx]).to(dev).to(torch.float32) / 127.5 - 1      # the trainer's expression, on the device
        assert img.device == dev and _same_bits(img, want), k
        assert torch.equal(lab.cpu(), torch.stack([torch.from_numpy(ds[i][1]) for i in idx])), k


def _trainer(tmp, folder, loader, *more):
    os.makedirs(str(tmp), exist_ok=True)
    argv = R.write_config(tmp, R.SG2_TINY, folder, f"data.dataloader={loader}", "data.mirror=true", "data.cond=true", "dataloaders_args.basic.num_workers=0",
                          "datasets_args.image_folder.use_labels=true", *more)
    return argv


def test_a_trainer_is_fed_the_same_bits_as_by_the_basic_loader(tmp_path, folder):
    fed = {}
    for name in ("basic", "resident"):
        trainer = starter.main(_trainer(tmp_path / name, folder, name), max_iterations=0)
        assert len(trainer.dataset) == 48 and trainer.dataset.label_dim > 0
        seen, step = [], trainer.engine.train_iteration

        def record(img, c, _seen=seen, _step=step):
            _seen.append((img.detach().clone(), c.detach().clone()))
            return _step(img, c)

        trainer.engine.train_iteration = record
        assert trainer.training_loop(max_iterations=8) == 8
        fed[name] = seen
    assert len(fed["basic"]) == len(fed["resident"]) == 8
    for (a, ca), (b, cb) in zip(fed["basic"], fed["resident"]):
        assert a.dtype == b.dtype == torch.float32 and a.is_cuda and b.is_cuda and tuple(a.shape) == (8, 3, 32, 32)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(ca, cb)


def test_a_run_through_the_resident_loader(tmp_path, folder, capsys):
    trainer = starter.main(_trainer(tmp_path / "run", folder, "resident", "log.run_log=on"), max_iterations=2)
    assert trainer.engine.batch_idx == 2
    grads = [p.grad for p in list(trainer.engine.G.parameters()) + list(trainer.engine.D.parameters()) if p.grad is not None]
    assert grads and all(bool(torch.isfinite(g).all()) for g in grads)
    store_gib = 24 * 3 * 32 * 32 / 2 ** 30
    line = f"Data loader:        resident (store {store_gib:.3f} GiB)"
    assert line in capsys.readouterr().out and line in open(os.path.join(str(tmp_path / "run"), "logs", "run", "log.txt")).read()
