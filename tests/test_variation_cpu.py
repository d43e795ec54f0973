"""The variation tool without a device: the numpy paths of `accumulate`, `numerator` and `render` against restatements in Python ints, the stated
overflow bounds, the split rule, every refusal before any library call, the ABI, which noise a synthesis layer hands to its convolution with and
without `noise_input`, the `noise_inputs` context, and the tool end to end with `--device=cpu`: from a snapshot of this build under the CPU
restatement of its generator, and with the exact stand-in generator."""
import json
import os

import numpy as np
import pytest
import torch

import moments_util as mu
from test_calc_metrics_cpu import _run
from style_big_gan_amd import _lib, arguments, tool_support, variation as V
from style_big_gan_amd.torch_utils.ops import moments_u8 as ops
from style_big_gan_amd.train_parts import generators as GEN

CPU = torch.device("cpu")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x).copy())


# ---------------------------------------------------------------------------------------------------------------- the ops

@pytest.mark.parametrize("kind", mu.KINDS)
@pytest.mark.parametrize("n", [0, 1, 2, 255])
@pytest.mark.parametrize("g,f", [(1, 1), (3, 15), (1, 3072), (3, 3072)])
def test_accumulate_equals_the_python_int_restatement(g, f, n, kind):
    images = mu.byte_images(g, n, f, kind)
    total, squares = (v.tolist() for v in mu.cpu_moments(g, n, f, kind))
    want = mu.restate_accumulate(images)
    assert total == want[0] and squares == want[1]
    if kind == "full":
        assert total == [[255 * n] * f] * g and squares == [[65025 * n] * f] * g


@pytest.mark.parametrize("g,n,f", [(1, 2, 1), (3, 255, 15), (1, 7, 3072)])
def test_two_partial_accumulations_equal_one(g, n, f):
    images = _t(mu.byte_images(g, n, f))
    total, squares = torch.zeros([g, f], dtype=torch.int64), torch.zeros([g, f], dtype=torch.int64)
    cut = n // 2
    ops.accumulate(images[:, :cut], total, squares)              # slices along N: the rows keep their strides
    ops.accumulate(images[:, cut:], total, squares)
    assert np.array_equal(total.numpy(), mu.cpu_moments(g, n, f)[0]) and np.array_equal(squares.numpy(), mu.cpu_moments(g, n, f)[1])
    before = total.clone()
    assert ops.accumulate(images[:, :0], total, squares)[0] is total and torch.equal(total, before)      # N = 0 changes nothing
    # running sums that are not zero, past 2^32
    total2, squares2 = torch.full([g, f], 1 << 40, dtype=torch.int64), torch.full([g, f], -5, dtype=torch.int64)
    ops.accumulate(images, total2, squares2)
    assert torch.equal(total2, before + (1 << 40)) and torch.equal(squares2, squares - 5)


@pytest.mark.parametrize("g,c,p,n", [(1, 1, 1, 2), (3, 3, 5, 255), (1, 3, 1024, 7)])
def test_numerator_equals_the_python_int_restatement(g, c, p, n):
    total, squares = mu.cpu_moments(g, n, c * p)
    got = ops.numerator(_t(total).reshape(g, c, p), _t(squares).reshape(g, c, p), n)
    assert got.dtype == torch.int64 and got.shape == (g, p)
    assert got.tolist() == mu.restate_numerator(total.reshape(g, c, p).tolist(), squares.reshape(g, c, p).tolist(), n)
    assert int(got.min()) >= 0


def test_numerator_of_identical_images_and_of_black_and_white():
    same = torch.from_numpy(np.repeat(mu.byte_images(1, 1, 48), 9, axis=1))
    total, squares = torch.zeros([1, 48], dtype=torch.int64), torch.zeros([1, 48], dtype=torch.int64)
    ops.accumulate(same, total, squares)
    assert ops.numerator(total.reshape(1, 3, 16), squares.reshape(1, 3, 16), 9).tolist() == [[0] * 16]
    pair = torch.tensor([0, 255], dtype=torch.uint8).reshape(1, 2, 1).repeat(1, 1, 3)
    total, squares = torch.zeros([1, 3], dtype=torch.int64), torch.zeros([1, 3], dtype=torch.int64)
    ops.accumulate(pair, total, squares)
    num = ops.numerator(total.reshape(1, 3, 1), squares.reshape(1, 3, 1), 2)
    assert num.tolist() == [[3 * 65025]]                                        # per channel 2 * 65025 - 255^2
    assert ops.pixel_std(num.numpy(), 3, 2).tolist() == [[np.sqrt(65025 / 2)]]    # the textbook unbiased variance of {0, 255}: 255^2 / 2
    assert ops.pixel_std(num.numpy(), 3, 1).tolist() == [[0.0]]


def test_render_thresholds_at_equality_ties_and_zero_groups():
    num = np.array([[0, 5, 9, 9, 0, 7], [0, 5, 10, 9, 0, 2], [0, 4, 10, 1, 0, 7]], dtype=np.int64)
    thresholds = np.sort(np.concatenate([[5, 9, 10], np.full(252, 1 << 40)])).astype(np.int64)
    table = mu.colour_table()
    heat, dominant = ops.render(_t(num), thresholds, table)
    assert heat.dtype == torch.uint8 and heat.shape == (3, 3, 6) and dominant.dtype == torch.uint8 and dominant.shape == (6,)
    level = np.array([[0, 1, 2, 2, 0, 1], [0, 1, 3, 2, 0, 0], [0, 0, 3, 0, 0, 1]])           # a value equal to a threshold has reached it
    assert np.array_equal(heat.numpy(), table[level].transpose(0, 2, 1))
    assert dominant.tolist() == [255, 0, 1, 0, 255, 0]                          # all zero: 255; equal values: the lower group
    want = mu.restate_render(num.tolist(), thresholds.tolist(), table.tolist())
    assert heat.tolist() == want[0] and dominant.tolist() == want[1]


@pytest.mark.parametrize("g,p", [(1, 1), (3, 15), (2, 1024)])
def test_render_equals_the_python_int_restatement(g, p):
    total, squares = mu.cpu_moments(g, 7, 3 * p)
    num = ops.numerator(_t(total).reshape(g, 3, p), _t(squares).reshape(g, 3, p), 7)
    thresholds = mu.thresholds_for(num.numpy())
    heat, dominant = ops.render(num, thresholds, mu.colour_table())
    want = mu.restate_render(num.tolist(), thresholds.tolist(), mu.colour_table().tolist())
    assert heat.tolist() == want[0] and dominant.tolist() == want[1]
    assert len(np.unique(heat.numpy())) > 2 or p == 1


def test_std_thresholds_are_a_scale():
    thr = ops.std_thresholds(10.0, 3, 100)
    assert thr.dtype == np.int64 and thr.shape == (255,) and (np.diff(thr) >= 0).all() and thr[0] >= 1
    assert thr[-1] == 10 * 10 * 3 * 100 * 99                                    # level 255 begins at std = max_std
    std = ops.pixel_std(thr, 3, 100)
    assert np.abs(std - np.arange(1, 256) * 10.0 / 255).max() < 1e-3 and (std >= np.arange(1, 256) * 10.0 / 255 - 1e-12).all()
    assert (ops.std_thresholds(0.0, 3, 100) == 1).all()                         # nothing varies: zero is level 0, anything else the top


# ---------------------------------------------------------------------------------------------------------------- bounds, split rule, refusals

def test_the_stated_overflow_bounds():
    assert ops.MAX_N == 32768 and 255 * 255 * ops.MAX_N < 1 << 32 and 255 * ops.MAX_N < 1 << 32            # a work-item's 32-bit partials
    assert 255 * 255 * 66051 < 1 << 32 <= 255 * 255 * 66052                                                   # the bound the header names
    for c in (1, 3, 1024):
        n = ops.numerator_max_n(c)
        assert n * n * 65025 * c < 1 << 63 <= (n + 1) * (n + 1) * 65025 * c
        total, squares = torch.full([1, c, 1], 255 * n, dtype=torch.int64), torch.full([1, c, 1], 65025 * n, dtype=torch.int64)
        assert ops.numerator(total, squares, n).tolist() == [[0]]                                             # n * 65025 n - (255 n)^2 in every channel
        half = torch.full([1, c, 1], 65025 * (n // 2), dtype=torch.int64)                                     # half the images white, half black
        want = c * (n * 65025 * (n // 2) - (255 * (n // 2)) ** 2)
        assert 0 < want < 1 << 63 and ops.numerator(torch.full([1, c, 1], 255 * (n // 2), dtype=torch.int64), half, n).tolist() == [[want]]
        with pytest.raises(RuntimeError, match=f"n = {n + 1} is not within"):
            ops.numerator(total, squares, n + 1)
    assert ops.numerator_max_n(1) == 11909805 and ops.numerator_max_n(3) == 6876129
    # more rows than one call takes are fed in several: every byte 255 at the largest N and one above
    for n in (ops.MAX_N, ops.MAX_N + 1):
        total, squares = torch.zeros([1, 2], dtype=torch.int64), torch.zeros([1, 2], dtype=torch.int64)
        ops.accumulate(torch.full([1, n, 2], 255, dtype=torch.uint8), total, squares)
        assert total.tolist() == [[255 * n] * 2] and squares.tolist() == [[65025 * n] * 2]


def test_the_split_rule():
    rule = ops.accumulate_splits
    assert rule(1, 0, 3072) == 0 and rule(1, 1, 3072) == 1 and rule(1, 16, 3072) == 1 and rule(1, 17, 3072) == 2
    assert rule(1, 100, 3072) == 7 and rule(1, 32, 196608) == 2 and rule(1, 32768, 48) == 1024
    assert rule(3, 255, 15) == 16 and rule(1, 64, 4096 * 1024) == 1 and rule(1, 64, 4096 * 512) == 2 and rule(3, 255, 4097) == 16
    for g, n, f in [(1, 100, 3072), (3, 255, 15), (2, 33, 5000), (1, 32768, 48), (7, 1000, 70000)]:
        splits = rule(g, n, f)
        rows = -(-n // splits)
        assert (splits - 1) * rows < n <= splits * rows                         # no empty split
    x = torch.zeros([2, 8, 48], dtype=torch.uint8)
    assert ops.load_width(x) == 16 and ops.load_width(x[:, :, :47]) == 16 and ops.load_width(torch.zeros([2, 8, 20], dtype=torch.uint8)) == 4
    assert ops.load_width(torch.zeros([2, 8, 15], dtype=torch.uint8)) == 1 and ops.load_width(torch.zeros([1, 8, 32], dtype=torch.uint8)[:, :, 1:]) == 16


def test_refusals_happen_before_any_library_call(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("a refused call reached the library"))
    images, total, squares = torch.zeros([2, 4, 8], dtype=torch.uint8), torch.zeros([2, 8], dtype=torch.int64), torch.zeros([2, 8], dtype=torch.int64)
    for args, message in [((images.int(), total, squares), "uint8"), ((images[0], total, squares), r"\[G, N, F\]"),
                          ((images, total[:1], squares), r"\(1, 8\)"), ((images, total.int(), squares), "int32"), ((images, total, total), "two tensors"),
                          ((images[:, :, ::2], total[:, :4].contiguous(), squares[:, :4].contiguous()), "dense along F"),
                          ((torch.zeros([2, 1, 8], dtype=torch.uint8).expand(2, 4, 8), total, squares), "overlap"),
                          ((torch.zeros([2, 4, 0], dtype=torch.uint8), total[:, :0], squares[:, :0]), "1 <= F")]:
        with pytest.raises(RuntimeError, match=message):
            ops.accumulate(*args)
    m = torch.zeros([2, 3, 4], dtype=torch.int64)
    for args, message in [((m.int(), m.int(), 2), "int64"), ((m, m[:1], 2), "one shape"), ((m, m, -1), "n = -1"), ((m[:, :, ::2], m[:, :, ::2], 2), "dense"),
                          ((torch.zeros([1, 1025, 1], dtype=torch.int64),) * 2 + (2,), "C <= 1024")]:
        with pytest.raises(RuntimeError, match=message):
            ops.numerator(*args)
    num, thr, table = torch.zeros([2, 4], dtype=torch.int64), np.arange(1, 256, dtype=np.int64), mu.colour_table()
    for args, message in [((num.int(), thr, table), "int64"), ((num, thr[::-1], table), "ascending"), ((num, thr[:254], table), "255"),
                          ((num, thr.astype(np.int32), table), "int64"), ((num, thr, table[:255]), r"\[256, 3\]"),
                          ((torch.zeros([256, 4], dtype=torch.int64), thr, table), "G <= 255")]:
        with pytest.raises(RuntimeError, match=message):
            ops.render(*args)


def test_the_abi():
    header = open(os.path.join(ROOT, "include", "sbg_hip.h")).read()
    names = ["sbg_moments_accumulate_max_n", "sbg_moments_accumulate_splits", "sbg_moments_accumulate_workspace", "sbg_moments_accumulate",
             "sbg_moments_numerator_max_n", "sbg_moments_numerator", "sbg_moments_render"]
    declared = {name for name, _, _ in _lib.SYMBOLS}
    lib = _lib.load()                                                           # every symbol resolves, or the load fails
    for name in names:
        assert f" {name}(" in header and name in declared and hasattr(lib, name)
    assert "SBG_K_MOMENTS = 33" in header and _lib.KERNEL_KINDS[33] == "moments"
    assert _lib.MOMENTS_VARIANTS == {0: "accumulate", 1: "merge", 2: "numerator", 3: "render"}
    # the host side of the library states the same limits and the same rule as the op
    assert lib.sbg_moments_accumulate_max_n() == ops.MAX_N
    for g, n, f in [(1, 0, 8), (1, 1, 1), (1, 100, 3072), (3, 255, 15), (1, 32, 196608), (1, 32768, 48), (2, 33, 5000), (65535, 3, 7)]:
        splits = ops.accumulate_splits(g, n, f)
        assert lib.sbg_moments_accumulate_splits(g, n, f) == splits
        assert lib.sbg_moments_accumulate_workspace(g, n, f) == (0 if splits <= 1 else 16 * splits * g * f)
    for g, n, f in [(0, 1, 8), (65536, 1, 8), (1, -1, 8), (1, 32769, 8), (1, 1, 0), (1, 1, (1 << 26) + 1)]:
        assert lib.sbg_moments_accumulate_splits(g, n, f) == -1 and lib.sbg_moments_accumulate_workspace(g, n, f) == -1
    for c in (1, 3, 1024):
        assert lib.sbg_moments_numerator_max_n(c) == ops.numerator_max_n(c)
    assert lib.sbg_moments_numerator_max_n(0) == -1 and lib.sbg_moments_numerator_max_n(1025) == -1


# ---------------------------------------------------------------------------------------------------------------- noise_input

def _layer_noise(monkeypatch, layer, mode, n=2):
    """the noise a SynthesisLayer hands to its convolution (the package's convolutions run only on the device)"""
    seen = []
    monkeypatch.setattr(GEN, "modulated_conv2d", lambda x, weight, styles, noise=None, **kw: seen.append(noise) or x.new_zeros([x.shape[0], weight.shape[0], layer.resolution, layer.resolution]))
    monkeypatch.setattr(GEN.bias_act, "bias_act", lambda x, b, **kw: x)
    with torch.no_grad():
        layer(torch.zeros([n, 4, layer.resolution, layer.resolution]), torch.zeros([n, 8]), noise_mode=mode, styles=torch.ones([n, 4]))
    return seen[0]


def test_a_layer_uses_its_noise_input_in_the_random_and_const_modes_only(monkeypatch):
    torch.manual_seed(1)
    layer = GEN.SynthesisLayer(in_channels=4, out_channels=4, w_dim=8, resolution=8).eval().requires_grad_(False)
    layer.noise_strength.fill_(0.75)
    assert GEN.SynthesisLayer.noise_input is None and layer.noise_input is None and "noise_input" not in layer.state_dict()
    # unset: what the layer always did
    assert _layer_noise(monkeypatch, layer, "none") is None
    const = _layer_noise(monkeypatch, layer, "const")
    assert mu.same_bits(const.numpy(), (layer.noise_const * layer.noise_strength).numpy()) and const.shape == (8, 8)
    torch.manual_seed(7)
    drawn = _layer_noise(monkeypatch, layer, "random")
    torch.manual_seed(7)
    assert mu.same_bits(drawn.numpy(), (torch.randn([2, 1, 8, 8]) * layer.noise_strength).numpy())
    # set: both noisy modes use it, 'none' stays none
    given = torch.randn([2, 1, 8, 8])
    layer.noise_input = given
    for mode in ("random", "const"):
        assert mu.same_bits(_layer_noise(monkeypatch, layer, mode).numpy(), (given * layer.noise_strength).numpy())
    assert _layer_noise(monkeypatch, layer, "none") is None
    layer.noise_input = layer.noise_const.expand(2, 1, 8, 8).contiguous()
    assert mu.same_bits(_layer_noise(monkeypatch, layer, "const").numpy(), const.expand(2, 1, 8, 8).contiguous().numpy())     # noise_const itself: the same bits
    layer.noise_input = torch.zeros([3, 1, 8, 8])
    with pytest.raises(AssertionError, match="dimension 0"):
        _layer_noise(monkeypatch, layer, "const")
    layer.noise_input = None
    assert mu.same_bits(_layer_noise(monkeypatch, layer, "const").numpy(), const.numpy())
    silent = GEN.SynthesisLayer(in_channels=4, out_channels=4, w_dim=8, resolution=8, use_noise=False).eval()
    silent.noise_input = given
    assert _layer_noise(monkeypatch, silent, "random") is None


def _package_generator():
    return GEN.generators["sg2_classic"](z_dim=16, c_dim=0, w_dim=16, img_resolution=16, img_channels=3, mapping_kwargs=dict(num_layers=2),
                                         synthesis_kwargs=dict(channel_base=256, channel_max=16))


def test_noise_layers_and_the_noise_inputs_context():
    G = _package_generator()
    layers = tool_support.noise_layers(G)
    assert layers == [("b4.conv1", 4), ("b8.conv0", 8), ("b8.conv1", 8), ("b16.conv0", 16), ("b16.conv1", 16)]
    assert V.ws_resolutions(G) == [4, 8, 8, 16, 16, 16] and len(V.ws_resolutions(G)) == G.num_ws
    noise = {"b8.conv0": torch.zeros([2, 1, 8, 8]), "b16.conv1": torch.ones([2, 1, 16, 16])}
    with tool_support.noise_inputs(G, noise):
        assert G.synthesis.b8.conv0.noise_input is noise["b8.conv0"] and G.synthesis.b16.conv1.noise_input is noise["b16.conv1"]
        assert G.synthesis.b4.conv1.noise_input is None and G.synthesis.b8.conv1.noise_input is None
    assert all(getattr(getattr(G.synthesis, f"b{r}"), n).noise_input is None for r, n in [(8, "conv0"), (16, "conv1")])
    with pytest.raises(KeyError):
        with tool_support.noise_inputs(G, noise):
            raise KeyError("inside")
    assert all(m.noise_input is None for m in G.synthesis.modules() if isinstance(m, GEN.SynthesisLayer))           # cleared on an exception too
    for bad, message in [({"b8.conv2": noise["b8.conv0"]}, "not a noise layer"), ({"b8.conv0": torch.zeros([2, 1, 4, 4])}, r"\[N, 1, 8, 8\]"),
                         ({"b8.conv0": torch.zeros([2, 1, 8, 8], dtype=torch.float64)}, "fp32")]:
        with pytest.raises(ValueError, match=message):
            with tool_support.noise_inputs(G, bad):
                pass
    assert all(m.noise_input is None for m in G.synthesis.modules() if isinstance(m, GEN.SynthesisLayer))

    class Plain(torch.nn.Module):
        z_dim, c_dim = 4, 0
    for other in (Plain(), GEN.generators["cnn32_dcgan"](z_dim=8, c_dim=0, img_resolution=32)):
        with pytest.raises(ValueError, match="no synthesis network"):
            tool_support.noise_layers(other)
        with pytest.raises(ValueError, match="mapping and synthesis"):
            V.measure_variation(other, seeds=[0], device=CPU)


# ---------------------------------------------------------------------------------------------------------------- the tool

def test_option_parsing_groups_and_the_draw_order(tmp_path, capsys):
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    ok = [f"--snapshot={snap}", f"--outdir={tmp_path / 'out'}"]
    overrides, args = V.parse_args(["exp.config=a.yaml"] + ok + ["--seeds=0-3"])
    assert overrides == ["exp.config=a.yaml"] and args.seeds == [0, 1, 2, 3] and args.vary == "noise,noise-layers,styles" and args.draws == 100
    assert (args.seed, args.groups, args.truncation_psi, args.class_idx, args.batch, args.max_std, args.device) == (0, None, 1, None, 32, None, "auto")
    for bad, message in [(ok, "exactly one of"), (ok + ["--seeds=1", "--vary=noise,colour"], "a list of"), (ok + ["--seeds=1", "--draws=1"], "at least 2"),
                         (ok + ["--seeds=1", "--batch=0"], "at least 1"), (ok + ["--seeds=1", "--max-std=0"], "positive"),
                         ([f"--snapshot={tmp_path / 'absent.pt'}", "--outdir=o", "--seeds=1"], "no such file"), (ok + ["--seeds=1", "--frobnicate"], "unrecognised")]:
        with pytest.raises(SystemExit):
            V.parse_args(bad)
        assert message in capsys.readouterr().err, bad
    G = _package_generator()
    assert V.parse_groups(None, G) == [("coarse", [0, 1, 2]), ("middle", [3, 4, 5])]                                # no 64 x 64 block: no fine group
    assert V.parse_groups("fine,coarse", G) == [("coarse", [0, 1, 2])]
    assert V.parse_groups("0-1,2-5", G) == [("0-1", [0, 1]), ("2-5", [2, 3, 4, 5])]
    for bad in ("0-9", "pose", "fine", "0-1,0-1"):
        with pytest.raises(ValueError):
            V.parse_groups(bad, G)
    plan = V.plan_sources(G, ["styles", "noise", "noise-layers"], None)
    assert [p[0] for p in plan] == ["noise"] + [f"noise:{n}" for n, _ in tool_support.noise_layers(G)] + ["styles:coarse", "styles:middle"]
    # draw by draw, layer by layer
    layers = [("b4.conv1", 4), ("b8.conv0", 8)]
    got = V.draw_noise(np.random.RandomState(3), layers, 2)
    rng = np.random.RandomState(3)
    for d in range(2):
        for name, res in layers:
            assert mu.same_bits(got[name][d, 0].numpy(), rng.randn(res, res).astype(np.float32))


def _tool_run(tmp_path, monkeypatch, strength):
    _, overrides, snap, _ = _run(tmp_path)
    mu.set_noise_strength(snap, strength)
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", mu.oracle_variation_generator)
    return overrides, snap


def test_the_tool_from_a_snapshot_of_this_build_on_the_cpu(tmp_path, monkeypatch, capsys):
    overrides, snap = _tool_run(tmp_path, monkeypatch, 1.0)
    argv = overrides + [f"--snapshot={snap}", "--device=cpu", "--seeds=0,3", "--draws=6", "--seed=2"]
    result = V.run_variation(argv + [f"--outdir={tmp_path / 'a'}", "--batch=3"])
    assert sorted(os.listdir(tmp_path / "a")) == mu.FILES
    stats = json.loads(open(tmp_path / "a" / "variation.json").read(), parse_constant=lambda name: pytest.fail(f"variation.json holds {name}"))
    assert stats == result["stats"] and json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == stats
    names = ["noise"] + [f"noise:b{r}.{c}" for r, c in [(4, "conv1"), (8, "conv0"), (8, "conv1"), (16, "conv0"), (16, "conv1")]] + ["styles:coarse", "styles:middle"]
    assert stats["sources"] == names and stats["competing"] == names[1:] and stats["options"]["draws"] == 6 and stats["options"]["seeds"] == [0, 3]
    arrays = np.load(tmp_path / "a" / "variation.npz")
    num, mean = arrays["num"], arrays["mean"]
    assert num.shape == (2, 8, 16, 16) and num.dtype == np.int64 and mean.shape == (2, 8, 3, 16, 16) and mean.dtype == np.float32
    assert arrays["sources"].tolist() == names and arrays["layers"].tolist() == [n[6:] for n in names[1:6]] and int(arrays["draws"]) == 6
    assert arrays["groups"].tolist() == ["coarse=0,1,2", "middle=3,4,5"] and arrays["seeds"].tolist() == [0, 3] and int(arrays["seed"]) == 2
    assert (num >= 0).all() and all((num[:, s] > 0).any() for s in range(8))                  # with noise_strength 1 every source moves pixels
    std = ops.pixel_std(num, 3, 6)
    assert stats["largest_std"] == stats["max_std"] == float(std.max()) == float(arrays["max_std"]) > 0
    assert np.array_equal(arrays["thresholds"], ops.std_thresholds(float(std.max()), 3, 6))
    for b in range(2):
        per = stats["bases"][b]
        assert per["noise_unused"] is False and per["noise_additivity"] > 0
        for s, name in enumerate(names):
            assert per["sources"][name]["max"] == float(std[b, s].max()) and per["sources"][name]["rms_std"] == float(np.sqrt((std[b, s] ** 2).mean()))
        assert abs(sum(per["sources"][n]["share"] for n in names[1:6]) - 1) < 1e-12 and per["sources"]["noise"]["share"] == 1.0
        assert abs(sum(per["sources"][n]["share"] for n in names[6:]) - 1) < 1e-12
        assert abs(sum(per["sources"][n]["dominant_fraction"] for n in names[1:]) + float((arrays["dominant"][b] == 255).mean()) - 1) < 1e-12
        assert per["sources"]["noise"]["dominant_fraction"] is None
    # the sheet: the unvaried image, the heat maps, the dominant map
    import PIL.Image
    sheet = np.array(PIL.Image.open(tmp_path / "a" / "variation.png"))
    assert sheet.shape == (2 * 16, 10 * 16, 3) and np.array_equal(sheet, result["sheet"])
    G = mu.oracle_variation_generator(arguments.load_config(overrides), tool_support.snapshot_generator_state(snap), "cpu")
    base = torch.cat([tool_support.generated_images(G, [s], torch.zeros([1, 0]), 1, "const", CPU) for s in (0, 3)]).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(arrays["base"], base) and np.array_equal(sheet[:16, :16], base[0]) and np.array_equal(sheet[16:, :16], base[1])
    level = np.searchsorted(arrays["thresholds"], num, side="right")
    assert np.array_equal(sheet[16:, 16 * 3:16 * 4], V.heat_table()[level[1, 2]]) and level.max() == 255
    # two runs, and a different batch, write the same files (batches of two and more: the CPU backend convolves a single image on another path,
    # which moves the last bits of the restatement's activations; the draws themselves never depend on the batch)
    V.run_variation(argv + [f"--outdir={tmp_path / 'b'}", "--batch=3"])
    V.run_variation(argv + [f"--outdir={tmp_path / 'c'}", "--batch=2"])
    assert mu.same_outputs(tmp_path / "a", tmp_path / "b")
    assert mu.same_outputs(tmp_path / "a", tmp_path / "c")
    # a shared scale
    shared = V.run_variation(argv + [f"--outdir={tmp_path / 'd'}", "--batch=6", "--max-std=40", "--vary=styles", "--groups=0-1,5-5"])
    assert shared["stats"]["max_std"] == 40.0 and shared["stats"]["sources"] == ["styles:0-1", "styles:5-5"] and shared["stats"]["bases"][0]["noise_unused"] is None
    assert np.array_equal(shared["arrays"]["thresholds"], ops.std_thresholds(40.0, 3, 6))


def test_a_network_that_ignores_its_noise(tmp_path, monkeypatch):
    overrides, snap = _tool_run(tmp_path, monkeypatch, 0.0)
    result = V.run_variation(overrides + [f"--snapshot={snap}", "--device=cpu", "--seeds=1", "--draws=3", "--batch=2", f"--outdir={tmp_path / 'out'}"])
    num, stats = result["arrays"]["num"], result["stats"]
    assert (num[:, :6] == 0).all() and (num[:, 6] > 0).any() and (num[:, 7] > 0).any()           # every noise map is zero, the styles maps are not
    assert stats["overall"]["noise_unused"] is True and stats["bases"][0]["noise_unused"] is True and stats["overall"]["noise_additivity"] is None
    assert stats["overall"]["sources"]["noise"]["share"] is None and stats["overall"]["sources"]["noise"]["rms_std"] == 0.0
    base = result["arrays"]["base"][0].transpose(2, 0, 1).astype(np.float32)
    assert all(np.array_equal(result["arrays"]["mean"][0, s], base) for s in range(6))          # the mean of a source that changes nothing: the image
    json.loads(open(tmp_path / "out" / "variation.json").read(), parse_constant=lambda name: pytest.fail(f"variation.json holds {name}"))


def test_the_tool_with_the_exact_generator_on_the_cpu(tmp_path):
    G = mu.ExactVariationGenerator()
    kept = {}
    result = V.variation(G, str(tmp_path / "a"), seeds=[4, 9], draws=6, seed=1, batch=4, truncation_psi=0.5, device=CPU,
                         on_images=lambda b, name, lo, images: kept.setdefault((b, name), []).append(images.clone()))
    names = result["stats"]["sources"]
    assert names == ["noise", "noise:b4.conv1", "noise:b8.conv0", "noise:b8.conv1", "styles:coarse"]
    num = result["arrays"]["num"]
    assert num.shape == (2, 5, 8, 8) and all((num[:, s] > 0).any() for s in range(5))
    # the maps are those of the images the tool made, by the restatement
    for b in range(2):
        for s, name in enumerate(names):
            images = torch.cat(kept[(b, name)]).numpy()
            assert images.shape == (6, 8, 8, 3)
            planar = images.transpose(0, 3, 1, 2).reshape(1, 6, 3 * 64)
            total, squares = mu.restate_accumulate(planar)
            want = mu.restate_numerator([np.array(total[0]).reshape(3, 64).tolist()], [np.array(squares[0]).reshape(3, 64).tolist()], 6)
            assert num[b, s].reshape(-1).tolist() == want[0]
            assert np.array_equal(result["arrays"]["mean"][b, s], (np.array(total[0], dtype=np.float64) / 6).astype(np.float32).reshape(3, 8, 8))
    # the noise group's images are those of the documented draws
    rng = np.random.RandomState(1)
    noise = V.draw_noise(rng, tool_support.noise_layers(G), 6)
    with tool_support.noise_inputs(G, noise):
        want = tool_support.generated_images(G, [4] * 6, torch.zeros([1, 0]), 0.5, "const", CPU)
    assert np.array_equal(torch.cat(kept[(0, "noise")]).numpy(), want.permute(0, 2, 3, 1).numpy())
    V.variation(G, str(tmp_path / "b"), seeds=[4, 9], draws=6, seed=1, batch=6, truncation_psi=0.5, device=CPU)
    assert mu.same_outputs(tmp_path / "a", tmp_path / "b")
    other = V.variation(G, str(tmp_path / "c"), seeds=[4, 9], draws=6, seed=2, batch=6, truncation_psi=0.5, device=CPU)
    assert not np.array_equal(other["arrays"]["num"], num)
    with pytest.raises(ValueError, match="at least 2"):
        V.measure_variation(G, seeds=[0], draws=1, device=CPU)
    with pytest.raises(ValueError, match="exactly one"):
        V.measure_variation(G, device=CPU)
    w = G.mapping(torch.from_numpy(tool_support.seed_latents(G, [4, 9])), None, truncation_psi=0.5).numpy()
    proj = V.measure_variation(G, projected_w=w, draws=6, seed=1, batch=4, vary="noise,noise-layers", device=CPU)
    assert np.array_equal(proj["arrays"]["num"][0], num[0, :4])                 # the first base latent's noise draws come first in the stream
