"""The uint8 resampling kernels and the data set tool on the device: `resize` against the reference tool's transforms
(tests/golden/dataset_tool.npz) and against the integer restatement on the CPU, bit for bit -- odd pitches, boxes at odd byte offsets,
views, the sizes a data set conversion runs -- the launch log, the refusals, and the tool with --device cuda against --device cpu."""
import contextlib
import os
import sys

import numpy as np
import PIL.Image
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import _lib, dataset_tool
from style_big_gan_amd.torch_utils.ops import resample_u8
import dataset_tool_util as du
from test_dataset_tool_cpu import apply_plan, check_against_fixture, fixture_inputs, run_tool

pytestmark = pytest.mark.gpu

DWORD, BYTES = 1, 2         # dims[6] of a resample/v launch record


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "these tests need a ROCm device"
    return torch.device("cuda:0")


@contextlib.contextmanager
def launches():
    """-> list of (variant name, dims) of every resample launch inside the block"""
    _lib.prof_enable(True)
    _lib.prof_fetch()
    seen = []
    try:
        yield seen
    finally:
        torch.cuda.synchronize()
        recs = _lib.prof_fetch()
        _lib.prof_enable(False)
        seen.extend((_lib.RESAMPLE_VARIANTS[r["dims"][0]], r["dims"]) for r in recs if r["kind"] == "resample")


def batch(seed, shape):
    """striped uint8 [N, H, W, C], every image different"""
    x = np.stack([du.striped(seed + n, shape[1:]) for n in range(shape[0])])
    return torch.from_numpy(x)


def test_resize_equals_the_fixture_for_every_case(dev):
    g = du.fixture()
    for case in g.meta["transforms"]:
        y = apply_plan(g.npz[case["key"] + "/x"], case, lambda t, *a, **kw: resample_u8.resize(t.to(dev), *a, **kw))
        if case["dropped"]:
            assert y is None, case
        else:
            ref = g.npz[case["key"] + "/y"]
            assert y.shape == ref.shape and np.array_equal(y, ref), case


@pytest.mark.parametrize("filter", ["lanczos", "box"])
@pytest.mark.parametrize("shape", [(2, 40, 57, 3), (3, 33, 47, 1), (1, 64, 64, 3), (2, 17, 23, 3), (1, 300, 451, 3)])
def test_odd_pitches_and_scalings_are_exact(dev, filter, shape):
    """widths whose byte pitch is not a multiple of 4, down, up, non-integer, one axis only, one pixel"""
    x = batch(3, shape)
    H, W = shape[1:3]
    for w, h in [(W // 2, H // 2), (2 * W + 1, 2 * H - 1), (31, 29), (W, 19), (30, H), (1, 1), (W - 1, H + 1), (270, 7)]:
        got = resample_u8.resize(x.to(dev), w, h, filter)
        assert got.shape == (shape[0], h, w, shape[3]) and got.is_contiguous()
        assert torch.equal(got.cpu(), resample_u8.resize_reference(x, w, h, filter)), (shape, w, h)


def test_ranks_boxes_and_views(dev):
    x = batch(11, (3, 50, 71, 3))
    d = x.to(dev)
    for box in [(1, 0, 70, 50), (3, 5, 64, 44), (7, 1, 8, 50), (0, 13, 71, 14), (5, 5, 37, 37)]:       # left * 3 bytes: odd offsets
        for w, h in [(16, 16), (box[2] - box[0], 9), (40, box[3] - box[1]), (box[2] - box[0], box[3] - box[1])]:
            got = resample_u8.resize(d, w, h, "lanczos", box=box)
            assert torch.equal(got.cpu(), resample_u8.resize_reference(x, w, h, "lanczos", box=box)), (box, w, h)
    # [H, W] and [H, W, C]
    assert torch.equal(resample_u8.resize(d[0, :, :, 1].contiguous(), 20, 30, "box").cpu(), resample_u8.resize_reference(x[0, :, :, 1], 20, 30, "box"))
    assert torch.equal(resample_u8.resize(d[1], 20, 30, "lanczos").cpu(), resample_u8.resize_reference(x[1], 20, 30, "lanczos"))
    # views with dense pixels: a window of a larger batch (row pitch and image stride larger than the shape, odd base), every other image
    for view in (lambda t: t[:, 3:41, 2:69], lambda t: t[::2], lambda t: t[1:, 1::1, 5:6]):
        for w, h in [(24, 24), (view(x).shape[2], 10)]:
            assert torch.equal(resample_u8.resize(view(d), w, h, "lanczos").cpu(), resample_u8.resize_reference(view(x).contiguous(), w, h, "lanczos"))
    # anything else is refused, never copied behind the caller's back or sent to torch
    for bad in (d[:, :, ::2], d.permute(0, 2, 1, 3), d[:, :, :, :1], d[:1, :1].expand(1, 8, 71, 3)):
        with pytest.raises(RuntimeError, match="dense rows"):
            resample_u8.resize(bad, 8, 8, "box")


def test_launch_log_shows_the_passes_that_ran(dev):
    x = batch(5, (2, 48, 64, 3)).to(dev)
    with launches() as seen:
        resample_u8.resize(x, 32, 24, "lanczos")
    assert [s[0] for s in seen] == ["h", "v"]
    assert seen[0][1][1:6] == (2, 48, 64, 32, 3) and seen[0][1][6] == 32                   # rows = the input's: the horizontal pass runs first
    assert seen[1][1][1:5] == (2, 96, 48, 24) and seen[1][1][6] == DWORD
    with launches() as seen:
        resample_u8.resize(x, 64, 24, "lanczos")                                            # width unchanged
        resample_u8.resize(x, 31, 48, "box")                                                # height unchanged
        resample_u8.resize(x, 64, 48, "box")                                                # nothing to do
        resample_u8.resize(x, 63, 20, "box", box=(1, 0, 64, 48))                            # vertical only, from an odd byte offset
    assert [s[0] for s in seen] == ["v", "h", "v"]
    assert seen[0][1][6] == DWORD and seen[2][1][6] == BYTES and seen[2][1][2] == 63 * 3
    with launches() as seen:
        resample_u8.resize(batch(6, (1, 8, 4000, 1)).to(dev), 40, 8, "box")                 # a span of 100 input pixels per output pixel
    assert [s[0] for s in seen] == ["h"] and seen[0][1][6] == 64


@pytest.mark.parametrize("filter", ["lanczos", "box"])
def test_data_set_sizes_are_exact(dev, filter):
    x = batch(21, (16, 1024, 1024, 3))
    with launches() as seen:
        got = resample_u8.resize(x.to(dev), 256, 256, filter)
    assert [s[0] for s in seen] == ["h", "v"] and seen[0][1][6] == 256
    assert torch.equal(got.cpu(), resample_u8.resize_reference(x, 256, 256, filter))
    ref = np.array(PIL.Image.fromarray(x[5].numpy()).resize((256, 256), {"lanczos": PIL.Image.LANCZOS, "box": PIL.Image.BOX}[filter]))
    assert np.array_equal(got[5].cpu().numpy(), ref)
    x = batch(22, (4, 1080, 1920, 3))
    box = dataset_tool.plan_transform("center-crop", 512, 512, x.shape[1:])[0]
    assert box == (420, 0, 1500, 1080)
    got = resample_u8.resize(x.to(dev), 512, 512, filter, box=box)
    assert torch.equal(got.cpu(), resample_u8.resize_reference(x, 512, 512, filter, box=box))


def test_bad_device_inputs_raise(dev):
    x = torch.zeros([2, 16, 16, 3], dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="uint8"):
        resample_u8.resize(x.float(), 8, 8, "box")
    with pytest.raises(RuntimeError, match="C = 1 or 3"):
        resample_u8.resize(torch.zeros([2, 16, 16, 4], dtype=torch.uint8, device=dev), 8, 8, "box")
    with pytest.raises(RuntimeError, match="unknown filter"):
        resample_u8.resize(x, 8, 8, "nearest")
    with pytest.raises(RuntimeError, match="box"):
        resample_u8.resize(x, 8, 8, "box", box=(4, 0, 4, 16))
    with pytest.raises(RuntimeError, match="LDS"):
        resample_u8.resize(torch.zeros([1, 2, 70000, 3], dtype=torch.uint8, device=dev), 16, 2, "lanczos")
    lib = _lib.load()
    t = torch.zeros([64], dtype=torch.int32, device=dev)
    o = torch.zeros([2, 16, 24], dtype=torch.uint8, device=dev)
    h = lambda *tail: lib.sbg_u8_resample_h(x.data_ptr(), 768, 48, o.data_ptr(), 384, 24, 2, 16, 16, 8, *tail, None)     # noqa: E731
    assert h(2, t.data_ptr(), t.data_ptr(), 3, 16, 16) != 0 and b"C must be 1 or 3" in lib.sbg_last_error()
    assert h(3, t.data_ptr(), t.data_ptr(), 3, 24, 16) != 0 and b"power of two" in lib.sbg_last_error()
    assert h(3, t.data_ptr(), t.data_ptr(), 3, 16, 17) != 0 and b"span" in lib.sbg_last_error()
    assert h(3, None, t.data_ptr(), 3, 16, 16) != 0 and b"null pointer" in lib.sbg_last_error()
    v = lambda dst, pitch: lib.sbg_u8_resample_v(x.data_ptr(), 768, 48, dst, 8 * pitch, pitch, 2, 48, 16, 8, t.data_ptr(), t.data_ptr(), 3, None)  # noqa: E731
    assert v(o.data_ptr() + 1, 48) != 0 and b"multiples of 4" in lib.sbg_last_error()
    assert v(o.data_ptr(), 46) != 0 and b"multiples of 4" in lib.sbg_last_error()


@pytest.mark.parametrize("name", ["folder", "zip", "wide"])
def test_tool_on_the_device_reproduces_the_reference_archive(dev, tmp_path, name):
    g = du.fixture()
    src = du.build_source(name, fixture_inputs(g, name), str(tmp_path))
    dest = du.dest_path(name, str(tmp_path))
    with launches() as seen:
        stats = dataset_tool.convert_dataset(src, dest, device="cuda", **_options(du.RUNS[name]["args"]))
    assert stats["device"] == "cuda" and seen and {s[0] for s in seen} <= {"h", "v"}
    check_against_fixture(g, name, dest)


def _options(args):
    kw = {}
    for a in args:
        k, v = a[2:].split("=")
        kw[k.replace("-", "_")] = int(v) if v.isdigit() else v
    return kw


def test_tool_writes_the_same_archive_on_both_devices(dev, tmp_path):
    """a generated folder of mixed sizes: runs of equal shape longer than one device batch, single images, a grey-free RGB set"""
    shapes = [(72, 96, 3)] * 19 + [(96, 72, 3)] + [(64, 64, 3)] * 3 + [(72, 96, 3)] * 2 + [(130, 67, 3)]
    src = tmp_path / "src"
    src.mkdir()
    for i, shape in enumerate(shapes):
        PIL.Image.fromarray(du.striped(300 + i, shape)).save(src / f"i{i:03d}.png")
    out = run_tool(f"--source={src}", f"--dest={tmp_path / 'gpu.zip'}", "--device=cuda", "--transform=center-crop", "--width=64", "--height=64").stdout
    assert "images written on cuda" in out
    run_tool(f"--source={src}", f"--dest={tmp_path / 'cpu.zip'}", "--device=cpu", "--transform=center-crop", "--width=64", "--height=64", "--workers=2")
    (n1, p1, j1), (n2, p2, j2) = du.read_archive(str(tmp_path / "gpu.zip")), du.read_archive(str(tmp_path / "cpu.zip"))
    assert n1 == n2 and j1 == j2 and len(p1) == len(shapes) and all(np.array_equal(p1[n], p2[n]) for n in p1)
    with launches() as seen:
        dataset_tool.convert_dataset(str(src), str(tmp_path / "again.zip"), transform="center-crop", width=64, height=64, device="cuda")
    assert [s[1][1] for s in seen if s[0] == "h"] == [16, 3, 1, 2, 1]            # the batches: 19 = 16 + 3; 64 x 64 images are left as they are
