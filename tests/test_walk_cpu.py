"""The latent walk tool without a device: `walk_weights` (frame positions, key frames, the weights' sum before rounding, the folds, loop wrap,
slerp), the CPU paths of `blend_table` and `pair_sqdiff` against restatements written here, every refusal before any library call, the ABI, and the
tool end to end with the exact stand-in generator: every file, the animations read back byte for byte, the contact sheet, key frames against
`generated_images`, walk.json, the table rebuilt from walk.npz, the grid's deal, the refusals."""
import importlib
import json
import os
import types

import numpy as np
import PIL.Image
import pytest
import torch

import walk_util as wu
from style_big_gan_amd import _lib, interpolate as IP, tool_support
from style_big_gan_amd.torch_utils.ops import walk as ops

CPU = torch.device("cpu")


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).copy())


# ---------------------------------------------------------------------------------------------------------------- walk_weights

@pytest.mark.parametrize("n", [1, 2, 3, 7, 30, 60])
@pytest.mark.parametrize("k", [2, 3, 5])
def test_frame_positions_and_key_frames(k, n):
    for loop in (False, True):
        for method in ("linear", "cubic"):
            index, w64, segment, tau = ops.walk_weights64(method, k, n, loop)
            _, w32, _, _ = ops.walk_weights(method, k, n, loop)
            T = k * n if loop else (k - 1) * n + 1
            assert index.shape == (T, 4) and index.dtype == np.int32 and w32.shape == (T, 4) and w32.dtype == np.float32
            assert segment.shape == (T,) and segment.dtype == np.int32 and tau.shape == (T,) and tau.dtype == np.float64 and w64.dtype == np.float64
            for f in range(T):
                u = np.float64(f) / np.float64(n)
                s = int(np.floor(u)) if loop else min(int(np.floor(u)), k - 2)
                assert segment[f] == s and tau[f] == u - s
            if not loop:
                assert segment[-1] == k - 2 and tau[-1] == 1.0
            assert np.abs(w64.sum(axis=1) - 1).max() <= 1e-15                      # before the one rounding
            assert wu.same_bits(w32, w64.astype(np.float32))
            on_key = tau == 0
            assert on_key.sum() == (k if loop else k - 1) and (w64[on_key] == [0, 1, 0, 0]).all() and (w32[on_key] == [0, 1, 0, 0]).all()
            assert (index[on_key, 1] == segment[on_key]).all()
            if not loop:
                assert (w32[-1] == [0, 0, 1, 0]).all() and index[-1, 2] == k - 1
            assert index.min() >= 0 and index.max() < k


def test_cubic_is_catmull_rom_with_reflected_ends():
    index, w, segment, tau = ops.walk_weights64("cubic", 4, 4, False)
    t = 0.25
    inner = [(-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2, (t ** 3 - t ** 2) / 2]
    assert index[5].tolist() == [0, 1, 2, 3] and w[5].tolist() == inner                            # s = 1: all four neighbours exist
    assert index[1].tolist() == [0, 0, 1, 2] and w[1].tolist() == [0, inner[1] + 2 * inner[0], inner[2] - inner[0], inner[3]]
    assert index[9].tolist() == [1, 2, 3, 2] and w[9].tolist() == [inner[0], inner[1] - inner[3], inner[2] + 2 * inner[3], 0]
    # two keys: both folds, which is the straight line
    for n in (1, 2, 3, 7, 10, 30, 60):
        ci, cw, _, _ = ops.walk_weights("cubic", 2, n, False)
        li, lw, _, _ = ops.walk_weights("linear", 2, n, False)
        assert wu.same_bits(cw, lw) and np.array_equal(ci, li)
    c64 = ops.walk_weights64("cubic", 2, 10, False)[1][3]
    assert c64[0] == 0 and c64[3] == 0 and abs(c64[1] - 0.7) < 1e-15 and abs(c64[2] - 0.3) < 1e-15


def test_loop_indices_wrap():
    index, _, segment, _ = ops.walk_weights("cubic", 5, 2, True)
    assert index.shape == (10, 4)
    assert index[0].tolist() == [4, 0, 1, 2] and index[1].tolist() == [4, 0, 1, 2] and index[6].tolist() == [2, 3, 4, 0] and index[9].tolist() == [3, 4, 0, 1]
    index, weight, _, _ = ops.walk_weights("linear", 3, 2, True)
    assert index[5].tolist() == [2, 2, 0, 2] and weight[5].tolist() == [0, 0.5, 0.5, 0]


def test_slerp_weights():
    omega = np.array([0.9, 0.0, 2.5])
    index, w64, segment, tau = ops.walk_weights64("slerp", 4, 5, False, omega)
    _, w32, _, _ = ops.walk_weights("slerp", 4, 5, False, omega)
    on_key = tau == 0
    assert (w32[on_key][:, 1:3] == [1, 0]).all() and (w32[-1, 1:3] == [0, 1]).all() and not w32[:, 0].any() and not w32[:, 3].any()
    assert (index[:, 0] == segment).all() and (index[:, 3] == segment).all() and (index[:, 2] == segment + 1).all()
    f = 2                                                                   # segment 0, tau = 0.4
    assert tau[f] == 2 / 5 and w64[f, 1] == np.sin((1 - tau[f]) * 0.9) / np.sin(0.9) and w64[f, 2] == np.sin(tau[f] * 0.9) / np.sin(0.9)
    assert w64[f, 1] + w64[f, 2] > 1
    lin = ops.walk_weights64("linear", 4, 5, False)[1]
    assert wu.same_bits(w64[5:10], lin[5:10])                               # a repeated key (omega = 0): the linear weights
    assert wu.same_bits(ops.walk_weights64("slerp", 2, 4, False, [5e-7])[1], ops.walk_weights64("linear", 2, 4, False)[1])
    for bad in (None, [0.5], [0.5] * 4):
        with pytest.raises(ValueError, match="--method=slerp"):
            ops.walk_weights("slerp", 4, 5, False, bad)
    assert ops.walk_weights("slerp", 4, 5, True, [0.5] * 4)[0].shape == (20, 4)
    for args, message in [(("cubic", 1, 5, False), "at least 2 keys"), (("cubic", 3, 0, False), "--frames-per-key=0"), (("spline", 3, 2, False), "--method=spline")]:
        with pytest.raises(ValueError, match=message):
            ops.walk_weights(*args)


# ---------------------------------------------------------------------------------------------------------------- blend_table

@pytest.mark.parametrize("k,l,d,t,loop", wu.SHAPES[:3])
def test_blend_table_equals_the_scalar_restatement(k, l, d, t, loop):
    keys = wu.key_table(k, l, d)
    index, weight, hold = wu.taps(k, t, loop)
    assert index.shape == (t, 4)
    got = wu.cpu_table(k, l, d, t, loop, False)
    assert got.dtype == np.float32 and wu.same_bits(got, wu.restate_blend(keys, index, weight))
    if loop:
        assert (index[:, 0] > index[:, 1]).any() and (index[:, 3] < index[:, 2]).any()          # both wraps are among the frames
    if l > 1:
        layers = wu.odd_layers(l)
        masked = wu.cpu_table(k, l, d, t, loop, True)
        assert wu.same_bits(masked, wu.restate_blend(keys, index, weight, layers, hold))
        held = [i for i in range(l) if i not in layers]
        assert wu.same_bits(masked[:, held], keys[hold][:, held]) and wu.same_bits(masked[:, layers], got[:, layers])
        assert np.signbit(keys[hold][:, held][keys[hold][:, held] == 0]).any()                      # -0.0 is among the copies


def test_rows_on_keys_equal_the_keys():
    keys = wu.key_table(5, 14, 40)
    for method, loop in (("linear", False), ("cubic", False), ("cubic", True), ("slerp", True)):
        index, weight, segment, tau = ops.walk_weights(method, 5, 3, loop, [0.7] * 5 if method == "slerp" else None)
        out = ops.blend_table(_t(keys), _t(index), _t(weight)).numpy()
        on_key = np.flatnonzero(tau == 0)
        assert len(on_key) == (5 if loop else 4)
        assert np.array_equal(out[on_key], keys[segment[on_key]])                                   # the values; -0.0 may come back as +0.0
        nonzero = keys[segment[on_key]] != 0
        assert wu.same_bits(out[on_key][nonzero], keys[segment[on_key]][nonzero])
        if not loop:
            assert np.array_equal(out[-1], keys[4])
    empty = ops.blend_table(_t(keys), torch.zeros([0, 4], dtype=torch.int32), torch.zeros([0, 4]))
    assert empty.shape == (0, 14, 40) and empty.dtype == torch.float32


def test_blend_table_refusals(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a refusal must come before any library call"))
    keys, index, weight, hold = torch.zeros([3, 4, 8]), torch.zeros([5, 4], dtype=torch.int32), torch.zeros([5, 4]), torch.zeros([5], dtype=torch.int32)
    out_of_range, negative, bad_hold = index.clone(), index.clone(), hold.clone()
    out_of_range[4, 3], negative[0, 0], bad_hold[2] = 3, -1, 3
    for args, kw, message in [
            ((keys.double(), index, weight), {}, r"float64 \(3, 4, 8\)"), ((keys, index.long(), weight), {}, r"int64 \(5, 4\)"),
            ((keys, index, weight.double()), {}, r"float64 \(5, 4\)"), ((keys, index, weight), dict(layers=[0], hold=hold.long()), r"int64 \(5,\)"),
            ((keys.transpose(0, 1), index, weight), {}, r"\(4, 3, 8\) strides"), ((keys, index.t().contiguous().t(), weight), {}, r"strides \(1, 5\)"),
            ((keys, index, torch.zeros([5, 8])[:, ::2]), {}, r"strides \(8, 2\)"),
            ((keys, index.to("meta"), weight), {}, "meta"), ((keys, index, weight.to("meta")), {}, "meta"),
            ((keys, index, weight), dict(layers=[0], hold=hold.to("meta")), "meta"),
            ((torch.zeros([3, 4, 1025]), index, weight), {}, r"\(3, 4, 1025\)"), ((torch.zeros([3, 4, 0]), index, weight), {}, r"\(3, 4, 0\)"),
            ((keys, torch.zeros([5, 3], dtype=torch.int32), weight), {}, r"\(5, 3\)"), ((keys, index, torch.zeros([4, 4])), {}, r"\(4, 4\)"),
            ((torch.zeros([1, 2048, 1024]), torch.zeros([1024, 4], dtype=torch.int32), torch.zeros([1024, 4])), {}, r"1024 x 2048 x 1024 = 2147483648.*\(1, 2048, 1024\)"),
            ((keys, out_of_range, weight), {}, r"outside \[0, K = 3\).*\(3, 4, 8\)"), ((keys, negative, weight), {}, r"outside \[0, K = 3\)"),
            ((keys, index, weight), dict(layers=[1], hold=bad_hold), r"outside \[0, K = 3\)"),
            ((keys, index, weight), dict(layers=[1]), "hold is required exactly"), ((keys, index, weight), dict(hold=hold), "hold is required exactly"),
            ((keys, index, weight), dict(layers=[0, 1, 2, 3], hold=hold), "hold is required exactly"),
            ((keys, index, weight), dict(layers=[4], hold=hold), r"layers \[4\]"), ((keys, index, weight), dict(layers=[], hold=hold), r"layers \[\]")]:
        with pytest.raises(RuntimeError, match=message):
            ops.blend_table(*args, **kw)
    assert ops.blend_table(torch.zeros([1, 1, 1024]), index[:1], weight[:1]).shape == (1, 1, 1024)      # the largest D
    assert ops.blend_table(keys, index, weight, layers=[0, 1, 2, 3]).shape == (5, 4, 8)                # every layer: no hold


# ---------------------------------------------------------------------------------------------------------------- pair_sqdiff

@pytest.mark.parametrize("f", [1, 15, 4096])
def test_pair_sqdiff_equals_numpy(f):
    a, b = wu.byte_rows(4, f, 0), wu.byte_rows(4, f, 1)
    got = ops.pair_sqdiff(_t(a), _t(b))
    assert got.dtype == torch.int64 and got.shape == (4,) and np.array_equal(got.numpy(), wu.sqdiff_np(a, b))
    ones, zeros = torch.full([2, f], 255, dtype=torch.uint8), torch.zeros([2, f], dtype=torch.uint8)
    assert ops.pair_sqdiff(ones, zeros).tolist() == [65025 * f] * 2 and ops.pair_sqdiff(zeros, ones).tolist() == [65025 * f] * 2
    x = _t(wu.byte_rows(6, f, 2))
    assert np.array_equal(ops.pair_sqdiff(x[:-2], x[2:]).numpy(), wu.sqdiff_np(x.numpy()[:-2], x.numpy()[2:]))    # slices along dimension 0


def test_pair_sqdiff_refusals(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a refusal must come before any library call"))
    a = torch.zeros([4, 16], dtype=torch.uint8)
    for x, y, message in [(a.int(), a.int(), r"int32 \(4, 16\)"), (a, a.float(), "float32"), (a[:, ::2], a[:, ::2], r"strides \(16, 2\)"), (a.t(), a.t(), r"\(16, 4\)"),
                          (a, a[:3], r"\(3, 16\)"), (a, a.to("meta"), "meta"), (a[0], a[0], r"\(16,\)"), (a[:, :0], a[:, :0], r"\[4, 0\]"),
                          (torch.zeros([1, (1 << 26) + 1], dtype=torch.uint8, device="meta"),) * 2 + (r"\[1, 67108865\]",),
                          (torch.zeros([(1 << 24) + 1, 1], dtype=torch.uint8, device="meta"),) * 2 + (r"\[16777217, 1\]",)]:
        with pytest.raises(RuntimeError, match=message):
            ops.pair_sqdiff(x, y)
    empty = ops.pair_sqdiff(a[:0], a[:0])
    assert empty.shape == (0,) and empty.dtype == torch.int64


# ---------------------------------------------------------------------------------------------------------------- ABI

def test_abi_symbols_resolve():
    lib = _lib.load()
    for name in ("sbg_walk_blend", "sbg_walk_sqdiff_splits", "sbg_walk_sqdiff_workspace", "sbg_walk_sqdiff"):
        assert getattr(lib, name) is not None
    assert _lib.KERNEL_KINDS[32] == "walk" and _lib.WALK_VARIANTS == {0: "blend", 1: "sqdiff", 2: "merge"}
    assert len(lib.sbg_walk_blend.argtypes) == 11 and len(lib.sbg_walk_sqdiff.argtypes) == 7
    assert lib.sbg_walk_sqdiff_splits.restype is _lib.ctypes.c_int64 and lib.sbg_walk_sqdiff_workspace.restype is _lib.ctypes.c_int64
    for n, f, splits in [(1, 1, 1), (3, 15, 1), (5, 16384, 1), (5, 16385, 2), (2, 3 << 20, 192), (1 << 24, 1 << 26, 4096)]:
        assert lib.sbg_walk_sqdiff_splits(n, f) == splits == ops.sqdiff_splits(n, f)
        assert lib.sbg_walk_sqdiff_workspace(n, f) == (0 if splits == 1 else 8 * n * splits)
    for n, f in [(0, 8), (8, 0), ((1 << 24) + 1, 8), (8, (1 << 26) + 1), (-1, 8)]:
        assert lib.sbg_walk_sqdiff_splits(n, f) == -1 and lib.sbg_walk_sqdiff_workspace(n, f) == -1
    # refused in the library too, below the op layer: nothing is launched (no device is touched here)
    for refused, message in [(lambda: lib.sbg_walk_blend(None, None, None, None, None, None, 2, 3, 1, 1025, None), "D=1025"),
                             (lambda: lib.sbg_walk_blend(None, None, None, None, None, None, 2, 1 << 20, 2048, 1024, None), "too large"),
                             (lambda: lib.sbg_walk_blend(None, None, None, None, None, None, 2, 3, 1, 8, None), "null or misaligned"),
                             (lambda: lib.sbg_walk_sqdiff(None, None, None, None, 0, 8, None), "[0, 8]"),
                             (lambda: lib.sbg_walk_sqdiff(None, None, None, None, 2, 8, None), "null or misaligned")]:
        assert refused() == 1 and message in lib.sbg_last_error().decode(), message
    assert lib.sbg_walk_blend(None, None, None, None, None, None, 2, 0, 1, 8, None) == 0            # T = 0: nothing to do


# ---------------------------------------------------------------------------------------------------------------- the tool

SEEDS = [3, 1, 4, 15, 9, 2]


@pytest.fixture(scope="module")
def walk_run(tmp_path_factory):
    """one open cubic walk of the stand-in generator, 2 x 1 cells of 3 keys: (outdir, result)"""
    out = tmp_path_factory.mktemp("walk") / "out"
    result = IP.interpolate(wu.ExactGenerator(), str(out), seeds=SEEDS, grid="2x1", frames_per_key=4, truncation_psi=0.5, batch=5, strip=4, save_frames=True,
                            device=CPU)
    return out, result


def test_every_file_exists_and_the_apng_holds_the_frames(walk_run):
    out, result = walk_run
    frames = result["frames"]
    assert frames.shape == (9, 8, 16, 3) and frames.dtype == np.uint8 and len(np.unique(frames)) > 8
    assert sorted(os.listdir(out)) == ["frames", "walk.apng", "walk.json", "walk.npz", "walk.png"]
    assert sorted(os.listdir(out / "frames")) == [f"frame{t:05d}.png" for t in range(9)]
    assert np.array_equal(wu.read_animation(out / "walk.apng", 30, 9), frames)
    assert PIL.Image.open(out / "walk.apng").info["loop"] == 0
    for t in (0, 5, 8):
        assert np.array_equal(np.array(PIL.Image.open(out / "frames" / f"frame{t:05d}.png")), frames[t])


@pytest.mark.parametrize("fmt", ["webp", "gif", "none"])
def test_the_other_formats(walk_run, tmp_path, fmt):
    _, first = walk_run
    result = IP.interpolate(wu.ExactGenerator(), str(tmp_path), fmt=fmt, fps=25, seeds=SEEDS, grid="2x1", frames_per_key=4, truncation_psi=0.5, batch=16, device=CPU)
    assert np.array_equal(result["frames"], first["frames"]) and np.array_equal(result["d2"], first["d2"])          # the batch changes nothing
    assert sorted(os.listdir(tmp_path)) == sorted(([] if fmt == "none" else [f"walk.{fmt}"]) + ["walk.json", "walk.npz", "walk.png"])
    if fmt == "webp":
        assert np.array_equal(wu.read_animation(tmp_path / "walk.webp", 25, 9), result["frames"])
    if fmt == "gif":                                                # palette-quantised: the size and the expanded count only
        assert wu.read_animation(tmp_path / "walk.gif", 25, 9).shape == (9, 8, 16, 3)


def test_one_channel_is_written_as_l(tmp_path):
    frames = np.random.RandomState(0).randint(0, 256, [4, 8, 8, 1], dtype=np.uint8)
    frames[2] = frames[1]
    for fmt in ("apng", "webp"):
        tool_support.save_animation(frames, str(tmp_path / f"a.{fmt}"), fmt, 10)
        assert np.array_equal(wu.read_animation(tmp_path / f"a.{fmt}", 10, 4, "L"), frames[:, :, :, 0])
    assert PIL.Image.open(tmp_path / "a.apng").mode == "L" and PIL.Image.open(tmp_path / "a.apng").n_frames == 3    # the repeated frame is merged
    for bad, message in [(("mp4", 10), "--format=mp4"), (("gif", 0), "--fps=0")]:
        with pytest.raises(ValueError, match=message):
            tool_support.save_animation(frames, str(tmp_path / "b"), *bad)


def test_the_contact_sheet_and_the_grid_deal(walk_run):
    out, result = walk_run
    frames = result["frames"]
    sheet = np.array(PIL.Image.open(out / "walk.png"))
    assert IP.strip_frames(9, 4) == [0, 3, 5, 8] and IP.strip_frames(3, 8) == [0, 1, 2] and IP.strip_frames(9, 1) == [0] and IP.strip_frames(601, 8)[-1] == 600
    assert sheet.shape == (2 * 8, 4 * 8, 3) and np.array_equal(sheet, result["sheet"])
    for c in range(2):
        for j, t in enumerate([0, 3, 5, 8]):
            assert np.array_equal(sheet[8 * c:8 * c + 8, 8 * j:8 * j + 8], frames[t, :, 8 * c:8 * c + 8]), (c, j)
    # key k of cell c is seed k * cells + c; a frame on a key is the image generate.py writes for the seed at the same psi
    G = wu.ExactGenerator()
    for k in range(3):
        for c in range(2):
            want = tool_support.generated_images(G, [SEEDS[2 * k + c]], tool_support.class_label(G, None, CPU), 0.5, "const", CPU)[0].permute(1, 2, 0).numpy()
            assert np.array_equal(frames[4 * k, :, 8 * c:8 * c + 8], want), (k, c)
    assert (result["d2"] > 0).all() and result["d2"].shape == (2, 8) and result["d2"].dtype == np.int64


def test_walk_json_and_npz(walk_run):
    out, result = walk_run
    stats = json.loads(open(out / "walk.json").read(), parse_constant=lambda name: pytest.fail(f"walk.json holds {name}"))
    assert stats == result["stats"] and (stats["frames"], stats["steps"], stats["keys_per_cell"]) == (9, 8, 3)
    opts = stats["options"]
    assert (opts["seeds"], opts["grid"], opts["space"], opts["method"], opts["layers"], opts["format"], opts["fps"], opts["strip"]) == \
        (SEEDS, [2, 1], "w", "cubic", [0, 1, 2, 3, 4, 5], "apng", 30.0, 4)
    npz = np.load(out / "walk.npz")
    assert sorted(npz.files) == ["classes", "d2", "grid", "hold", "index", "keys", "layers", "method", "omega", "seeds", "segment", "space", "tau", "weight"]
    assert npz["keys"].shape == (6, 6, 24) and npz["index"].shape == (18, 4) and npz["weight"].dtype == np.float32 and npz["d2"].dtype == np.int64
    assert npz["seeds"].tolist() == SEEDS and npz["omega"].size == 0 and npz["classes"].size == 0 and str(npz["space"]) == "w" and npz["grid"].tolist() == [2, 1]
    assert npz["index"][1::2].min() == 3 and npz["index"][::2].max() == 2                            # cell 1's taps are offset by K
    rmse = np.sqrt(npz["d2"].astype(np.float64) / (3 * 8 * 8))
    assert len(stats["cells"]) == 2
    for c, cell in enumerate(stats["cells"]):
        assert cell == dict(rmse_mean=float(rmse[c].mean()), rmse_median=float(np.median(rmse[c])), rmse_max=float(rmse[c].max()),
                            argmax_frame=int(np.argmax(rmse[c])), jerk=float(rmse[c].max() / np.median(rmse[c])))
    assert stats["overall"]["rmse_max"] == float(rmse.max()) and stats["overall"]["rmse_mean"] == float(rmse.reshape(-1).mean())
    # the table is not stored: it is rebuilt from the file bit for bit, and so are the frames
    table = IP.table_from_arrays(npz)
    assert table.shape == (18, 6, 24)
    img = wu.ExactGenerator().synthesis(table)
    again = tool_support.image_export.quantize(img, "clamp").numpy().reshape(9, 2, 8, 8, 3).transpose(0, 2, 1, 3, 4).reshape(9, 8, 16, 3)
    assert np.array_equal(again, result["frames"])


def test_a_constant_walk(tmp_path):
    result = IP.interpolate(wu.ExactGenerator(), str(tmp_path), seeds=[7, 7, 7], frames_per_key=3, device=CPU)
    stats = json.loads(open(tmp_path / "walk.json").read(), parse_constant=lambda name: pytest.fail(f"walk.json holds {name}"))
    assert not result["d2"].any() and result["d2"].shape == (1, 6) and stats["cells"][0]["jerk"] is None and stats["overall"]["jerk"] is None
    assert stats["cells"][0]["rmse_max"] == 0
    im = PIL.Image.open(tmp_path / "walk.apng")
    assert getattr(im, "n_frames", 1) == 1                          # all frames identical: one long frame
    assert np.array_equal(wu.read_animation(tmp_path / "walk.apng", 30, 7), result["frames"])


def test_layers_loop_and_z_space(walk_run, tmp_path):
    _, first = walk_run
    G = wu.ExactGenerator()
    part = IP.render_walk(G, seeds=SEEDS, grid=(2, 1), frames_per_key=4, layers="0-2", truncation_psi=0.5, device=CPU)
    table = IP.table_from_arrays(part["arrays"]).numpy().reshape(9, 2, 6, 24)
    keys = part["arrays"]["keys"].reshape(2, 3, 6, 24)
    assert wu.same_bits(table[:, :, 3:], np.broadcast_to(keys[None, :, 0, 3:], [9, 2, 3, 24]))     # the other layers hold the cell's key 0
    assert np.array_equal(part["frames"][0], first["frames"][0]) and not np.array_equal(part["frames"][4], first["frames"][4])
    assert part["arrays"]["layers"].tolist() == [0, 1, 2] and part["arrays"]["hold"].tolist() == [0, 3] * 9
    loop = IP.render_walk(G, seeds=[0, 1, 2], space="z", loop=True, frames_per_key=4, truncation_psi=0.5, batch=7, device=CPU)
    arrays = loop["arrays"]
    assert loop["frames"].shape == (12, 8, 8, 3) and loop["d2"].shape == (1, 12) and str(arrays["method"]) == "slerp" and arrays["keys"].shape == (3, 1, 12)
    z = tool_support.seed_latents(G, [0, 1, 2])
    unit = z / np.linalg.norm(z, axis=1, keepdims=True)
    want = np.arccos([unit[0] @ unit[1], unit[1] @ unit[2], unit[2] @ unit[0]])
    assert arrays["omega"].shape == (1, 3) and np.allclose(arrays["omega"][0], want, rtol=0, atol=1e-12)
    for k in range(3):
        want = tool_support.generated_images(G, [k], tool_support.class_label(G, None, CPU), 0.5, "const", CPU)[0].permute(1, 2, 0).numpy()
        assert np.array_equal(loop["frames"][4 * k], want), k
    last_to_first = wu.sqdiff_np(loop["frames"][-1].reshape(1, -1), loop["frames"][0].reshape(1, -1))
    assert loop["d2"][0, -1] == last_to_first[0] and loop["d2"][0, 0] == wu.sqdiff_np(loop["frames"][0].reshape(1, -1), loop["frames"][1].reshape(1, -1))[0]
    # projected rows are keys as they are; --trunc is ignored with a warning
    w = G.mapping(torch.from_numpy(tool_support.seed_latents(G, SEEDS)), None, truncation_psi=0.5).numpy()
    np.savez(tmp_path / "projected_w.npz", w=w)
    proj = IP.render_walk(G, projected_w=str(tmp_path / "projected_w.npz"), grid="2x1", frames_per_key=4, device=CPU)
    assert np.array_equal(proj["frames"], first["frames"]) and proj["arrays"]["seeds"].size == 0


def test_trunc_with_projected_w_warns(capsys):
    G = wu.ExactGenerator()
    w = G.mapping(torch.from_numpy(tool_support.seed_latents(G, [0, 1])), None).numpy()
    a = IP.render_walk(G, projected_w=w, frames_per_key=2, truncation_psi=0.5, device=CPU)
    assert "warn: --trunc is ignored when using --projected-w" in capsys.readouterr().out
    b = IP.render_walk(G, projected_w=w, frames_per_key=2, device=CPU)
    assert "warn" not in capsys.readouterr().out and np.array_equal(a["frames"], b["frames"])


def test_cli_run_on_the_cpu(walk_run, tmp_path, capsys, monkeypatch):
    from test_calc_metrics_cpu import _run
    _, first = walk_run
    _, overrides, snap, _ = _run(tmp_path)
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", lambda config, state, device: wu.ExactGenerator().to(device))
    out = tmp_path / "out"
    result = IP.run_interpolate(overrides + [f"--snapshot={snap}", f"--outdir={out}", "--seeds=3,1,4,15,9,2", "--grid=2x1", "--frames-per-key=4", "--trunc=0.5",
                                             "--batch=5", "--strip=4", "--device=cpu"])
    assert np.array_equal(result["frames"], first["frames"]) and sorted(os.listdir(out)) == ["walk.apng", "walk.json", "walk.npz", "walk.png"]
    printed = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert printed == result["stats"] and printed["frames"] == 9


def test_option_parsing_and_refusals(tmp_path, capsys):
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    ok = [f"--snapshot={snap}", f"--outdir={tmp_path / 'out'}"]
    overrides, args = IP.parse_args(["exp.config=a.yaml"] + ok + ["--seeds=0-3"])
    assert overrides == ["exp.config=a.yaml"] and args.seeds == [0, 1, 2, 3]
    assert (args.projected_w, args.grid, args.space, args.method, args.frames_per_key, args.loop, args.layers, args.classes) == (None, "1x1", "w", None, 30, False, None, None)
    assert (args.truncation_psi, args.class_idx, args.noise_mode, args.fmt, args.fps, args.strip, args.save_frames, args.batch, args.device) == \
        (1, None, "const", "apng", 30, 8, False, 16, "auto")
    _, args = IP.parse_args(ok + ["--seeds=0,1", "--space=z", "--method=linear", "--loop", "--format=webp", "--fps=12.5", "--save-frames", "--grid=1x1", "--class=3"])
    assert (args.space, args.method, args.loop, args.fmt, args.fps, args.save_frames, args.class_idx) == ("z", "linear", True, "webp", 12.5, True, 3)
    np.savez(tmp_path / "projected_w.npz", w=np.zeros([2, 6, 24], dtype=np.float32))
    pw = f"--projected-w={tmp_path / 'projected_w.npz'}"
    for bad, message in [(ok, "exactly one of --seeds and --projected-w"), (ok + ["--seeds=0,1", pw], "exactly one of --seeds and --projected-w"),
                         (ok + ["--seeds=0,1", "--grid=2"], "--grid=2: expects GWxGH"), (ok + ["--seeds=0,1", "--grid=0x1"], "--grid=0x1"),
                         (ok + ["--seeds=0,1", "--method=slerp"], "--method=slerp is for --space=z only"), (ok + [pw, "--space=z"], "--projected-w is refused with --space=z"),
                         (ok + ["--seeds=0,1", "--space=z", "--layers=0-2"], "--layers is refused with --space=z"),
                         (ok + ["--seeds=0,1", "--space=z", "--classes=0,1"], "--classes is refused with --space=z"),
                         (ok + ["--seeds=0,1", "--classes=0,1", "--class=1"], "exclude one another"), (ok + ["--seeds=0,1", "--frames-per-key=0"], "--frames-per-key=0"),
                         (ok + ["--seeds=0,1", "--strip=0"], "--strip=0"), (ok + ["--seeds=0,1", "--batch=0"], "--batch=0"), (ok + ["--seeds=0,1", "--fps=0"], "--fps=0"),
                         (ok + ["--seeds=0,1", "--format=mp4"], "invalid choice"), (ok + ["--seeds=0,1", "--space=y"], "invalid choice"),
                         ([f"--snapshot={tmp_path / 'absent.pt'}", ok[1], "--seeds=0,1"], "no such file"), (ok + [f"--projected-w={tmp_path / 'absent.npz'}"], "no such file"),
                         (ok[:1] + ["--seeds=0,1"], "--outdir"), (ok + ["--seeds=0,1", "--frobnicate"], "unrecognised")]:
        with pytest.raises(SystemExit):
            IP.parse_args(bad)
        assert message in capsys.readouterr().err, bad
    G = wu.ExactGenerator()
    two = dict(seeds=[0, 1])
    for kw, message in [(dict(seeds=[0, 1, 2], grid="2x1"), r"--seeds: 3 keys do not deal into --grid=2x1"), (dict(seeds=[0, 1], grid="2x1"), "K >= 2"),
                        (dict(seeds=[0]), "K >= 2"), (dict(projected_w=np.zeros([3, 6, 24], dtype=np.float32), grid="2x1"), "--projected-w: 3 keys"),
                        (dict(projected_w=np.zeros([2, 5, 24], dtype=np.float32)), r"--projected-w: w of shape \(2, 5, 24\)"),
                        (dict(), "exactly one of --seeds and --projected-w"), (dict(two, projected_w=np.zeros([2, 6, 24])), "exactly one of"),
                        (dict(two, method="slerp"), "--method=slerp is for --space=z only"), (dict(two, method="spline"), "--method=spline"),
                        (dict(two, space="y"), "--space=y"), (dict(projected_w=np.zeros([2, 6, 24], dtype=np.float32), space="z"), "--projected-w is refused with --space=z"),
                        (dict(two, space="z", layers="0-2"), "--layers is refused with --space=z"), (dict(two, space="z", classes=[0, 1]), "--classes is refused with --space=z"),
                        (dict(two, classes=[0, 1]), "--classes: one class per key is for conditional networks only"), (dict(two, layers="6"), "--layers=6"),
                        (dict(two, grid="3"), "--grid=3"), (dict(two, batch=0), "--batch=0"), (dict(two, frames_per_key=0), "--frames-per-key=0")]:
        with pytest.raises(ValueError, match=message):
            IP.render_walk(G, **dict(dict(device=CPU), **kw))
    for kw, message in [(dict(fmt="mp4"), "--format=mp4"), (dict(fps=0), "--fps=0"), (dict(strip=0), "--strip=0")]:
        with pytest.raises(ValueError, match=message):
            IP.interpolate(G, str(tmp_path / "never"), seeds=[0, 1], device=CPU, **kw)
    assert not os.path.exists(tmp_path / "never")
    # a conditional network needs --class or --classes, as class_label says; --classes deals one class per key
    cond = wu.ExactGenerator()
    cond.c_dim = 4
    with pytest.raises(ValueError, match="Must specify class label"):
        IP.render_walk(cond, seeds=[0, 1], device=CPU)
    with pytest.raises(ValueError, match=r"--classes: expects one class in \[0, 4\) per seed, 2 of them"):
        IP.render_walk(cond, seeds=[0, 1], classes=[0, 1, 2], device=CPU)
    with pytest.raises(ValueError, match=r"--classes: expects one class in \[0, 4\)"):
        IP.render_walk(cond, seeds=[0, 1], classes=[0, 4], device=CPU)
    assert IP.render_walk(cond, seeds=[0, 1], classes=[0, 3], frames_per_key=2, device=CPU)["arrays"]["classes"].tolist() == [0, 3]
    # more frames than the encoder can hold as a list: refused with both numbers before anything is rendered
    big = wu.ExactGenerator(res=1024)
    with pytest.raises(ValueError, match=r"--frames-per-key=400: 401 frames of 12582912 bytes are 5045747712 bytes, above the 2147483648"):
        IP.render_walk(big, seeds=[0, 1, 2, 3, 4, 5, 6, 7], grid="2x2", frames_per_key=400, device=CPU)
    for other in (torch.nn.Linear(2, 2), types.SimpleNamespace(synthesis=None)):                  # BigGAN, DCGAN: no W space
        with pytest.raises(ValueError, match="mapping and synthesis"):
            IP.render_walk(other, seeds=[0, 1], device=CPU)


def test_the_tool_imports_no_other_tool():
    from test_tool_support_cpu import TOOLS
    mod = importlib.import_module("style_big_gan_amd.interpolate")
    others = {f"style_big_gan_amd.{t}" for t in tuple(TOOLS) + ("diversity", "realism", "directions", "modes", "style_mixing", "generate")}
    held = {v.__name__ if isinstance(v, types.ModuleType) else getattr(v, "__module__", None) for v in vars(mod).values()}
    assert not held & others, held & others
    assert IP.parse_layers is tool_support.parse_layers and "interpolate" in tool_support.__doc__ and "eleven" in tool_support.__doc__
