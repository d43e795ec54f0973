"""The k-means kernels of the mode coverage tool on the device: `update` equals the op's CPU path exactly (one row, an empty cluster, a partial
row chunk and a partial column tile, the largest K, the production width, four empty clusters, sorted and shuffled labels), the int64 merge
above 2^31, two launches, the launch records, the refusals of the op layer and of the library, `seed` and `lloyd` against their CPU runs, and
the tool with --device=cuda: from a snapshot of this build, and against its own CPU run with the exact stand-in generator."""
import json
import os

import numpy as np
import pytest
import torch

import modes_util as mu
from exact_util import expect_launch
from nearest_util import BankGenerator
from test_calc_metrics_cpu import _run
from style_big_gan_amd import _lib, modes as MD
from style_big_gan_amd.torch_utils.ops import kmeans_u8 as ops
from style_big_gan_amd.train_parts.datasets import ImageFolderDataset

pytestmark = pytest.mark.gpu

CASES = mu.UPDATE_CASES[:3] + [(4099, 7, 272), (1000, 256, 64), (600, 100, 3072)]


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _d(dev, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in arrays]


def _equal(got, want):
    return all(g.dtype == w.dtype and g.shape == w.shape and torch.equal(g.cpu(), w) for g, w in zip(got, want))


@pytest.mark.parametrize("n,k,f", CASES)
def test_update_equals_the_cpu_path(dev, n, k, f):
    case = mu.update_case(n, k, f)
    want = ops.update(*[torch.from_numpy(a) for a in case])
    got = ops.update(*_d(dev, *case))
    assert all(t.device == dev for t in got) and _equal(got, want)
    assert _equal(ops.update(*_d(dev, *case)), want)             # two launches give the same bits


def test_one_label_for_every_row(dev):
    points, _, old = mu.table(300, 5, 80)
    labels = np.full([300], 3, dtype=np.int32)
    want = ops.update(*[torch.from_numpy(a) for a in (points, labels, old)])
    got = ops.update(*_d(dev, points, labels, old))
    assert _equal(got, want) and got[1].tolist() == [0, 0, 0, 300, 0]
    keep = [0, 1, 2, 4]
    assert np.array_equal(got[0].cpu().numpy()[keep], old[keep]) and not got[2].cpu().numpy()[keep].any()


def test_sorted_and_shuffled_labels_give_equal_results(dev):
    points, labels, old = mu.table(5000, 11, 528)
    order = np.argsort(labels, kind="stable")
    shuffled = ops.update(*_d(dev, points, labels, old))
    in_order = ops.update(*_d(dev, points[order], labels[order], old))
    assert (np.diff(labels[order]) >= 0).all() and _equal(in_order, [t.cpu() for t in shuffled])
    assert _equal(shuffled, ops.update(*[torch.from_numpy(a) for a in (points, labels, old)]))


def test_the_int64_merge(dev):
    """8 421 505 rows of 255 in one cluster: 255 N = 2 147 483 775 > 2^31 - 1, more than one i32 partial can hold.  The expected value is arithmetic."""
    n = 8421505
    assert 255 * n == 2147483775 > 2 ** 31 - 1 and n > 1 << 23
    points = torch.full([n, 16], 255, dtype=torch.uint8, device=dev)
    labels = torch.ones([n], dtype=torch.int32, device=dev)
    old = torch.full([2, 16], 7, dtype=torch.uint8, device=dev)
    new, counts, sums = ops.update(points, labels, old)
    assert counts.tolist() == [0, n] and sums[1].tolist() == [2147483775] * 16 and not sums[0].any()
    assert new[1].tolist() == [255] * 16 and new[0].tolist() == [7] * 16


def test_launch_records(dev):
    points, labels, old = _d(dev, *mu.table(4099, 7, 272))
    with expect_launch("kmeans_u8", lambda r: r[:4] == (0, 4099, 272, 7), "accumulate") as log:
        ops.update(points, labels, old)
    recs = [r["dims"] for r in log if r["kind"] == "kmeans_u8"]
    assert [_lib.KMEANS_VARIANTS[r[0]] for r in recs] == ["accumulate", "finish"] and all(r[1:4] == (4099, 272, 7) for r in recs)
    chunks, lanes = recs[0][4], recs[0][5]
    assert recs[1][4:6] == (chunks, lanes) and chunks > 1 and 4099 % -(-4099 // chunks) != 0 and 272 % (16 * lanes) != 0       # partial chunk, partial tile
    assert _lib.load().sbg_kmeans_u8_update_workspace(4099, 272, 7) == 4 * chunks * 7 * 273


def test_refusals_on_the_device(dev):
    p, l, c = _d(dev, *mu.table(8, 3, 16))
    for args, message in [((p.float(), l, c), r"float32 \(8, 16\)"), ((p, l.long(), c), r"labels int64"), ((p[:, ::2], l, c[:, ::2]), "dense"),
                          ((p, l.cpu(), c), r"different devices.*cpu"), ((p, l, c.cpu()), "different devices"),
                          ((p, l, torch.zeros([257, 16], dtype=torch.uint8, device=dev)), r"\(257, 16\)"),
                          ((torch.zeros([4, 24], dtype=torch.uint8, device=dev), l[:4].contiguous(), torch.zeros([3, 24], dtype=torch.uint8, device=dev)),
                           "row length 24 must be a multiple of 16")]:
        with pytest.raises(RuntimeError, match=message):
            ops.update(*args)
    worse = l.clone()
    worse[2] = 3
    with pytest.raises(RuntimeError, match=r"outside \[0, 3\)"):
        ops.update(p, worse, c)
    # the library's own checks, below the op layer's: status 1, the message, and nothing launched
    lib = _lib.load()
    new = torch.full([3, 16], 77, dtype=torch.uint8, device=dev)
    sums, counts = torch.full([3, 16], -7, dtype=torch.int64, device=dev), torch.full([3], -7, dtype=torch.int64, device=dev)
    ws = torch.zeros([1 << 16], device=dev)
    call = lambda points, n, f, k: lib.sbg_kmeans_u8_update(points, l.data_ptr(), c.data_ptr(), new.data_ptr(), sums.data_ptr(), counts.data_ptr(), ws.data_ptr(),
                                                            n, f, k, _lib.stream_ptr(dev))
    for refused, message in [(lambda: call(p.data_ptr(), 8, 16, 257), "N=8 F=16 K=257"), (lambda: call(p.data_ptr(), 8, 24, 3), "N=8 F=24 K=3"),
                             (lambda: call(p.data_ptr(), 0, 16, 3), "N=0 F=16 K=3"), (lambda: call(None, 8, 16, 3), "null or misaligned"),
                             (lambda: call(p.data_ptr() + 1, 8, 16, 3), "null or misaligned")]:
        status = refused()
        assert status == 1 and message in lib.sbg_last_error().decode(), message
    torch.cuda.synchronize()
    assert bool((new == 77).all()) and bool((sums == -7).all()) and bool((counts == -7).all())


def test_a_label_out_of_range_is_skipped_by_the_kernel(dev):
    """the op layer refuses it; the kernel below must not write out of bounds for it: the row is left out"""
    points, labels, old = mu.table(64, 3, 32)
    bad = labels.copy()
    bad[[5, 40]] = [3, -1]
    keep = np.ones([64], dtype=bool)
    keep[[5, 40]] = False
    want = mu.scalar_update(points[keep], labels[keep], old)
    p, l, c = _d(dev, points, bad, old)
    new = torch.empty_like(c)
    sums, counts = torch.empty([3, 32], dtype=torch.int64, device=dev), torch.empty([3], dtype=torch.int64, device=dev)
    lib = _lib.load()
    ws = _lib.workspace(lib.sbg_kmeans_u8_update_workspace(64, 32, 3), dev, "sbg_kmeans_u8_update_workspace")
    guard = torch.full([4096], 5, dtype=torch.int32, device=dev)                                  # allocated next: an overrun would likely land here
    _lib.check(lib.sbg_kmeans_u8_update(p.data_ptr(), l.data_ptr(), c.data_ptr(), new.data_ptr(), sums.data_ptr(), counts.data_ptr(), ws.data_ptr(), 64, 32, 3,
                                        _lib.stream_ptr(dev)), "sbg_kmeans_u8_update")
    assert mu.same_update((new, counts, sums), want) and bool((guard == 5).all())


@pytest.mark.parametrize("name", ["planted", "random"])
def test_seed_and_lloyd_equal_their_cpu_runs(dev, name):
    points, k = (mu.planted_table()[0], 4) if name == "planted" else (mu.table(700, 1, 48, seed=3)[0], 9)
    host, device = torch.from_numpy(points), torch.from_numpy(points).to(dev)
    c0, c1 = ops.seed(host, k, np.random.RandomState(1)), ops.seed(device, k, np.random.RandomState(1))
    assert c1.device == dev and torch.equal(c0, c1.cpu())
    a, b = ops.lloyd(host, c0, 30), ops.lloyd(device, c1, 30)
    assert a["inertia"] == b["inertia"] and (a["iterations"], a["converged"]) == (b["iterations"], b["converged"])
    assert all(torch.equal(a[key], b[key].cpu()) and b[key].device == dev for key in ("centroids", "labels", "d2", "counts"))
    if name == "random":
        assert a["iterations"] > 3                               # several updates ran on the device


def test_the_tool_from_a_snapshot_of_this_build(dev, tmp_path, capsys):
    _, overrides, snap, data = _run(tmp_path)
    out = tmp_path / "out"
    result = MD.run_modes(overrides + [f"--snapshot={snap}", f"--outdir={out}", "--device=cuda", "--bins=3", "--res=8", "--holdout=0.25", "--num=40", "--show=2",
                                       "--examples=2", "--batch=16"])
    assert sorted(os.listdir(out)) == ["modes.json", "modes.npz", "modes.png"]
    stats = json.loads(open(out / "modes.json").read(), parse_constant=lambda name: pytest.fail(f"modes.json holds {name}"))
    assert stats == result["stats"] and (stats["N_ref"], stats["N_holdout"], stats["N_gen"]) == (15, 5, 40)         # the run's mirror is switched off
    assert len(stats["bins"]) == 3 and sum(b["n_gen"] for b in stats["bins"]) == 40 and sum(b["n_ref"] for b in stats["bins"]) == 15
    assert 0 <= stats["generated"]["js"] <= 1 and 0 <= stats["generated"]["ndb"] <= 3
    npz = np.load(out / "modes.npz")
    assert npz["centroids"].shape == (3, 192) and npz["gen_labels"].shape == (40,) and result["canvas"].shape == (3 * 16, 5 * 16, 3)
    # the stored labels are the exact nearest centroids of the stored items
    dataset = ImageFolderDataset(path=data)
    small = MD.reduce_images(torch.from_numpy(np.stack([dataset[int(i)][0] for i in npz["ref_items"]])), 8).reshape(15, -1)
    labels, d2 = ops.assign(small, torch.from_numpy(npz["centroids"]))
    assert np.array_equal(labels.numpy(), npz["ref_labels"]) and np.array_equal(d2.numpy(), npz["ref_d2"])


def test_the_tool_on_the_device_equals_its_cpu_run(dev, tmp_path):
    """the stand-in generator returns the same bytes on both devices and everything after it is integer arithmetic: every file is the same"""
    images, mode = mu.mode_images()
    root = mu.write_folder(str(tmp_path / "data"), images)
    runs = {}
    for name, device in (("cpu", torch.device("cpu")), ("cuda", dev)):
        dataset = ImageFolderDataset(path=root)
        G = BankGenerator(images[mode != 2]).to(device)
        runs[name] = MD.mode_coverage(G, dataset, bins=7, res=8, holdout=0.25, show=2, examples=3, batch=50, iters=8, outdir=str(tmp_path / name), device=device)
    assert sorted(os.listdir(tmp_path / "cpu")) == sorted(os.listdir(tmp_path / "cuda")) == ["modes.json", "modes.npz", "modes.png"]
    a, b = np.load(tmp_path / "cpu" / "modes.npz"), np.load(tmp_path / "cuda" / "modes.npz")
    assert sorted(a.files) == sorted(b.files) == sorted(MD.NPZ_KEYS)
    assert all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes() for k in a.files)
    for name in ("modes.json", "modes.png"):
        assert open(tmp_path / "cpu" / name, "rb").read() == open(tmp_path / "cuda" / name, "rb").read()
    assert runs["cuda"]["stats"]["bins"][0]["missing"] and runs["cuda"]["stats"]["iterations"] >= 1
