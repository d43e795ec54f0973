"""The variation kernels on the device: `accumulate`, `numerator` and `render` equal the op's CPU path bit for bit (one byte, odd base offsets and
row strides larger than F, every load width, partial first and last vectors, the N-split with its merge launch, running sums that are not zero,
the largest N of a call with every byte 255, a sum past 2^32), the launch records against the split rule of the header, refusals that launch
nothing, `noise_input` on the package's synthesis network, and the tool with --device=cuda: against its own CPU run with the exact stand-in
generator, and from a snapshot of this build."""
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

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def _records(fn):
    """the `moments` launch records of one call"""
    torch.cuda.synchronize()
    _lib.prof_enable(True)
    _lib.prof_fetch()
    try:
        fn()
        torch.cuda.synchronize()
        return [r["dims"] for r in _lib.prof_fetch() if r["kind"] == "moments"]
    finally:
        _lib.prof_enable(False)


def _placed(images, pad, offset, dev):
    """uint8 [G, N, F] on the device as a view of a larger buffer: rows F + pad bytes apart, the first byte `offset` bytes into the allocation"""
    g, n, f = images.shape
    buffer = torch.full([offset + g * n * (f + pad)], 77, dtype=torch.uint8, device=dev)            # 77: bytes between the rows are never read
    view = buffer[offset:].reshape(g, n, f + pad)[:, :, :f]
    view.copy_(torch.from_numpy(images.copy()).to(dev))
    assert view.data_ptr() % 16 == offset % 16 and view.stride(1) == f + pad
    return view


# (G, N, F, pad, offset, load width): one byte; byte loads from an odd base with rows 17 apart and the N-split; the low-resolution image with the
# N-split; N = 1; one whole tile; dword loads with partial vectors; 16-byte loads from a base 3 bytes off; a second tile begun, from a base 9 bytes off;
# the split past one tile
CASES = [(1, 1, 1, 0, 0, 1), (3, 255, 15, 2, 1, 1), (1, 255, 3072, 0, 0, 16), (3, 1, 3072, 0, 0, 16), (1, 5, 4096, 0, 0, 16), (3, 7, 4097, 3, 4, 4),
         (1, 16, 3072, 16, 3, 16), (3, 2, 4100, 12, 9, 16), (2, 40, 70000, 0, 0, 16)]


@pytest.mark.parametrize("g,n,f,pad,offset,width", CASES)
def test_accumulate_equals_the_cpu_path_and_logs_the_split_rule(dev, g, n, f, pad, offset, width):
    images = _placed(mu.byte_images(g, n, f), pad, offset, dev)
    start = (torch.arange(g * f, dtype=torch.int64).reshape(g, f) * 1000003) % (1 << 36) - (1 << 20)         # running sums that are not zero, some past 2^32
    total, squares = start.clone().to(dev), (start * 3 + 1).to(dev)
    recs = _records(lambda: ops.accumulate(images, total, squares))
    want_sum, want_sq = mu.cpu_moments(g, n, f)
    assert torch.equal(total.cpu(), start + torch.from_numpy(want_sum.copy())) and torch.equal(squares.cpu(), start * 3 + 1 + torch.from_numpy(want_sq.copy()))
    splits = ops.accumulate_splits(g, n, f)
    assert ops.load_width(images) == width
    want = [(0, g, n, f, splits, width)] + ([(1, g, n, f, splits)] if splits > 1 else [])
    assert [r[:len(w)] for r, w in zip(recs, want)] == want and len(recs) == len(want)
    assert _lib.load().sbg_moments_accumulate_splits(g, n, f) == splits
    again_sum, again_sq = torch.zeros_like(total), torch.zeros_like(squares)
    ops.accumulate(images, again_sum, again_sq)
    assert np.array_equal(again_sum.cpu().numpy(), want_sum) and np.array_equal(again_sq.cpu().numpy(), want_sq)


def test_the_cases_take_every_path():
    splits = [ops.accumulate_splits(g, n, f) for g, n, f, _, _, _ in CASES]
    assert 1 in splits and max(splits) == 16 and splits[-1] == 3 and CASES[-1][2] > ops.TILE          # direct, split, split across tiles


def test_the_largest_call_with_every_byte_255(dev):
    n = ops.MAX_N
    # one work-item sums all the rows of its columns: G * tiles = 1024 workgroups leave N unsplit
    images = torch.full([1024, n, 16], 255, dtype=torch.uint8, device=dev)
    assert ops.accumulate_splits(1024, n, 16) == 1
    total, squares = torch.zeros([1024, 16], dtype=torch.int64, device=dev), torch.zeros([1024, 16], dtype=torch.int64, device=dev)
    for call in (1, 2, 3):
        ops.accumulate(images, total, squares)
        assert bool((total == 255 * n * call).all()) and bool((squares == 65025 * n * call).all())
    assert 65025 * n * 3 > 1 << 32 > 65025 * n                                   # the running sum is past 2^32, a call's partial is not
    del images
    # the same rows split over 1024 workgroups and merged
    images = torch.full([1, n, 48], 255, dtype=torch.uint8, device=dev)
    assert ops.accumulate_splits(1, n, 48) == 1024
    total, squares = torch.zeros([1, 48], dtype=torch.int64, device=dev), torch.zeros([1, 48], dtype=torch.int64, device=dev)
    ops.accumulate(images, total, squares)
    assert total.tolist() == [[255 * n] * 48] and squares.tolist() == [[65025 * n] * 48]
    # more rows than a call takes: the op feeds them in two
    more = torch.full([1, n + 3, 48], 255, dtype=torch.uint8, device=dev)
    recs = _records(lambda: ops.accumulate(more, total, squares))
    assert [r[0] for r in recs] == [0, 1, 0] and [r[2] for r in recs] == [n, n, 3]
    assert total.tolist() == [[255 * (2 * n + 3)] * 48] and squares.tolist() == [[65025 * (2 * n + 3)] * 48]


def test_nothing_is_launched_for_no_rows_or_a_refused_shape(dev):
    total, squares = torch.ones([2, 8], dtype=torch.int64, device=dev), torch.ones([2, 8], dtype=torch.int64, device=dev)
    assert _records(lambda: ops.accumulate(torch.zeros([2, 0, 8], dtype=torch.uint8, device=dev), total, squares)) == []
    assert bool((total == 1).all()) and bool((squares == 1).all())
    lib, stream = _lib.load(), _lib.stream_ptr(dev)
    images = torch.zeros([2, 4, 8], dtype=torch.uint8, device=dev)
    status = []
    # the library's own checks: N = 0 is fine and silent; too many rows, overlapping rows, a misaligned sum and a count above the bound are refused
    calls = [lambda: lib.sbg_moments_accumulate(images.data_ptr(), 8, 32, total.data_ptr(), squares.data_ptr(), None, 2, 0, 8, stream),
             lambda: lib.sbg_moments_accumulate(images.data_ptr(), 8, 32, total.data_ptr(), squares.data_ptr(), None, 2, ops.MAX_N + 1, 8, stream),
             lambda: lib.sbg_moments_accumulate(images.data_ptr(), 7, 32, total.data_ptr(), squares.data_ptr(), None, 2, 4, 8, stream),
             lambda: lib.sbg_moments_accumulate(images.data_ptr(), 8, 32, total.data_ptr() + 4, squares.data_ptr(), None, 2, 4, 8, stream),
             lambda: lib.sbg_moments_numerator(total.data_ptr(), squares.data_ptr(), total.data_ptr(), 1, 2, 4, ops.numerator_max_n(2) + 1, stream),
             lambda: lib.sbg_moments_render(total.data_ptr(), total.data_ptr(), images.data_ptr(), images.data_ptr(), images.data_ptr(), 256, 4, stream)]

    def run():
        for call in calls:
            code = call()
            status.append((code, (lib.sbg_last_error() or b"").decode() if code else ""))
    assert _records(run) == []
    assert status[0] == (0, "") and all(code != 0 for code, _ in status[1:])
    assert "[2, 32769, 8]" in status[1][1] and "[2, 4, 8]" in status[2][1] and "7" in status[2][1] and "[2, 4, 8]" in status[3][1]
    assert str(ops.numerator_max_n(2) + 1) in status[4][1] and "[1, 2, 4]" in status[4][1] and "[256, 4]" in status[5][1]
    assert bool((total == 1).all()) and bool((squares == 1).all())
    for args, message in [((images.cpu(), total, squares), "cpu"), ((images, total.cpu(), squares), "cpu"), ((images, total[:, :4], squares), "dense int64")]:
        with pytest.raises(RuntimeError, match=message):
            ops.accumulate(*args)


@pytest.mark.parametrize("g,c,p,n", [(1, 1, 1, 2), (3, 3, 15, 255), (2, 3, 1024, 7), (1, 3, 4101, 5)])
def test_numerator_and_render_equal_the_cpu_path(dev, g, c, p, n):
    total, squares = mu.cpu_moments(g, n, c * p)
    t, q = torch.from_numpy(total.copy()).reshape(g, c, p), torch.from_numpy(squares.copy()).reshape(g, c, p)
    want = ops.numerator(t, q, n)
    out = []
    recs = _records(lambda: out.append(ops.numerator(t.to(dev), q.to(dev), n)))
    got = out[0]
    assert got.device == dev and got.dtype == torch.int64 and torch.equal(got.cpu(), want) and [r[:4] for r in recs] == [(2, g, c, p)]
    thresholds, table = mu.thresholds_for(want.numpy()), mu.colour_table()
    heat, dominant = ops.render(want, thresholds, table)
    out = []
    recs = _records(lambda: out.append(ops.render(got, thresholds, table)))
    assert [r[:3] for r in recs] == [(3, g, p)]
    assert out[0][0].dtype == torch.uint8 and torch.equal(out[0][0].cpu(), heat) and torch.equal(out[0][1].cpu(), dominant)
    # ties and all-zero pixels
    num = want.clone()
    num[:, 0] = 0
    if g > 1 and p > 2:
        num[1, 1] = num[0, 1]
        num[0, 2] = num[1:, 2].max()
    heat, dominant = ops.render(num, thresholds, table)
    heat_d, dominant_d = ops.render(num.to(dev), thresholds, table)
    assert torch.equal(heat_d.cpu(), heat) and torch.equal(dominant_d.cpu(), dominant) and int(dominant[0]) == 255


def test_the_largest_count_of_the_numerator(dev):
    for c in (1, 3):
        n = ops.numerator_max_n(c)
        half = n // 2
        total, squares = torch.full([1, c, 5], 255 * half, dtype=torch.int64, device=dev), torch.full([1, c, 5], 65025 * half, dtype=torch.int64, device=dev)
        want = c * (n * 65025 * half - (255 * half) ** 2)
        assert want < 1 << 63 and ops.numerator(total, squares, n).tolist() == [[want] * 5]
        with pytest.raises(RuntimeError, match="is not within"):
            ops.numerator(total, squares, n + 1)


# ---------------------------------------------------------------------------------------------------------------- noise_input

@pytest.mark.parametrize("num_fp16_res", [0, 2])
def test_noise_inputs_on_the_synthesis_network(dev, num_fp16_res):
    torch.manual_seed(3)
    G = GEN.generators["sg2_classic"](z_dim=16, c_dim=0, w_dim=24, img_resolution=16, img_channels=3, mapping_kwargs=dict(num_layers=2),
                                      synthesis_kwargs=dict(channel_base=256, channel_max=32, num_fp16_res=num_fp16_res)).eval().requires_grad_(False).to(dev)
    layers = tool_support.noise_layers(G)
    for name, _ in layers:
        block, layer = name.split(".")
        getattr(getattr(G.synthesis, block), layer).noise_strength.fill_(0.5)
    ws = G.mapping(torch.randn([3, 16], device=dev), torch.zeros([3, 0], device=dev))
    with torch.no_grad():
        G.synthesis(ws, noise_mode="const")             # a network's first pass packs its weights and sizes its workspaces; the comparisons start after it
        plain = {mode: G.synthesis(ws, noise_mode=mode) for mode in ("const", "none")}
        torch.manual_seed(11)
        plain["random"] = G.synthesis(ws, noise_mode="random")
        torch.manual_seed(11)
        drawn = {name: torch.randn([3, 1, res, res], device=dev) for name, res in layers}         # the layers draw in synthesis order
        const = {name: getattr(getattr(G.synthesis, name.split(".")[0]), name.split(".")[1]).noise_const.expand(3, 1, -1, -1).contiguous() for name, _ in layers}
        with tool_support.noise_inputs(G, const):
            as_const = {mode: G.synthesis(ws, noise_mode=mode) for mode in ("const", "random", "none")}
        with tool_support.noise_inputs(G, drawn):
            as_drawn = {mode: G.synthesis(ws, noise_mode=mode) for mode in ("const", "random")}
        after = G.synthesis(ws, noise_mode="const")
    bits = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    gap = lambda a, b: float((a.double() - b.double()).abs().max())
    print({"const input / const": gap(as_const["const"], plain["const"]), "const input, random / const": gap(as_const["random"], as_const["const"]),
           "none": gap(as_const["none"], plain["none"]), "drawn input / random": gap(as_drawn["random"], plain["random"]),
           "drawn input, const / random": gap(as_drawn["const"], plain["random"]), "after / const": gap(after, plain["const"]),
           "largest value": float(plain["const"].abs().max())})
    # the same tensors through the same kernels: the same bits
    assert bits(as_drawn["random"], plain["random"]) and bits(as_drawn["const"], plain["random"])       # the input stands for the drawn noise, in both modes
    assert bits(as_const["random"], as_const["const"]) and bits(as_const["none"], plain["none"])         # 'none' stays none
    assert bits(after, plain["const"]) and not bits(plain["const"], plain["none"]) and not bits(plain["const"], plain["random"])      # cleared: as before
    if num_fp16_res == 0:
        # noise_const handed in per sample takes the kernels' per-sample noise operand, not the shared one: the same values, but the two forms of a
        # fused tail need not add noise and bias in one order, so the comparison is the fp32 bound smoke() holds the HIP path to (1e-4 of the
        # largest value), not bits; the noise the layer hands over IS the same bits (tests/test_variation_cpu.py)
        assert gap(as_const["const"], plain["const"]) <= 1e-4 * float(plain["const"].abs().max())


def test_noise_inputs_follow_the_blocks_that_run_over_slices_of_the_batch(dev):
    torch.manual_seed(5)
    G = GEN.generators["sg2_classic"](z_dim=16, c_dim=0, w_dim=24, img_resolution=16, img_channels=3, mapping_kwargs=dict(num_layers=2),
                                      synthesis_kwargs=dict(channel_base=256, channel_max=32)).eval().requires_grad_(False).to(dev)
    layers = tool_support.noise_layers(G)
    for name, _ in layers:
        block, layer = name.split(".")
        getattr(getattr(G.synthesis, block), layer).noise_strength.fill_(0.5)
    ws = G.mapping(torch.randn([4, 16], device=dev), torch.zeros([4, 0], device=dev))
    noise = {name: torch.randn([4, 1, res, res], device=dev) for name, res in layers}
    with torch.no_grad():
        G.synthesis(ws, noise_mode="const")
        with tool_support.noise_inputs(G, noise):
            whole = G.synthesis(ws, noise_mode="const")
        G.synthesis.pass_bytes_limit = 200000           # the 16 x 16 block's largest tensor is 55 488 bytes a sample: it runs over two slices of two
        assert G.synthesis.pass_plan(4) == (1, 2)
        with tool_support.noise_inputs(G, noise):
            sliced = G.synthesis(ws, noise_mode="const")
            assert all(getattr(getattr(G.synthesis, n.split(".")[0]), n.split(".")[1]).noise_input is noise[n] for n, _ in layers)      # put back whole
        swapped = dict(noise, **{"b16.conv1": noise["b16.conv1"].flip(0)})
        with tool_support.noise_inputs(G, swapped):
            other = G.synthesis(ws, noise_mode="const")
    gap = lambda a, b: float((a.double() - b.double()).abs().max())
    scale = float(whole.abs().max())
    print({"sliced / whole": gap(sliced, whole), "other rows / whole": gap(other, whole), "largest value": scale})
    # a slice of the batch may take other kernels than the whole batch: smoke()'s fp32 bound, not bits; the wrong rows of the noise are far outside it
    assert gap(sliced, whole) <= 1e-4 * scale < 1e-3 * scale < gap(other, whole)


# ---------------------------------------------------------------------------------------------------------------- the tool

def test_the_tool_on_the_device_equals_its_cpu_run(dev, tmp_path):
    """the stand-in generator's bytes are an integer function of ws and the noise inputs, so every file is the same"""
    runs = {}
    for name, device in (("cpu", torch.device("cpu")), ("cuda", dev)):
        runs[name] = V.variation(mu.ExactVariationGenerator().to(device), str(tmp_path / name), seeds=[4, 9, 2], draws=20, seed=1, batch=7, truncation_psi=0.5,
                                 device=device)
    assert mu.same_outputs(tmp_path / "cpu", tmp_path / "cuda")
    num = runs["cuda"]["arrays"]["num"]
    assert num.shape == (3, 5, 8, 8) and all((num[:, s] > 0).any() for s in range(5)) and np.array_equal(runs["cuda"]["sheet"], runs["cpu"]["sheet"])


def test_the_tool_from_a_snapshot_of_this_build(dev, tmp_path):
    _, overrides, snap, _ = _run(tmp_path)
    mu.set_noise_strength(snap, 1.0, silent=("b8.conv0",))
    G = tool_support.load_generator(arguments.load_config(overrides), snap, dev, announce=False)
    kept = {}
    result = V.variation(G, str(tmp_path / "out"), seeds=[5], draws=3, seed=4, batch=1, device=dev,
                         on_images=lambda b, name, lo, images: kept.setdefault(name, []).append(images.clone()))
    assert sorted(os.listdir(tmp_path / "out")) == mu.FILES
    stats = json.loads(open(tmp_path / "out" / "variation.json").read(), parse_constant=lambda name: pytest.fail(f"variation.json holds {name}"))
    names = stats["sources"]
    assert stats == result["stats"] and names[:3] == ["noise", "noise:b4.conv1", "noise:b8.conv0"] and len(names) == 8
    arrays = np.load(tmp_path / "out" / "variation.npz")
    num, mean, base = arrays["num"], arrays["mean"], arrays["base"]
    label = torch.zeros([1, 0], device=dev)
    assert np.array_equal(base[0], tool_support.generated_images(G, [5], label, 1, "const", dev)[0].permute(1, 2, 0).cpu().numpy())
    # a layer whose noise_strength is 0 changes nothing: its map is exactly 0 and its mean is the unvaried image
    silent = names.index("noise:b8.conv0")
    assert (num[0, silent] == 0).all() and np.array_equal(mean[0, silent], base[0].transpose(2, 0, 1).astype(np.float32))
    assert all((num[0, s] > 0).any() for s in range(8) if s != silent) and stats["bases"][0]["noise_unused"] is False
    assert stats["bases"][0]["sources"]["noise:b8.conv0"]["rms_std"] == 0.0 and stats["bases"][0]["sources"]["noise:b8.conv0"]["share"] == 0.0
    # the images of the noise group: the documented draws, set through noise_inputs
    layers = tool_support.noise_layers(G)
    noise = V.draw_noise(np.random.RandomState(4), layers, 3)
    got = torch.cat(kept["noise"])
    assert got.shape == (3, 16, 16, 3) and got.dtype == torch.uint8
    for d in range(3):
        with tool_support.noise_inputs(G, {k: v[d:d + 1].to(dev) for k, v in noise.items()}):
            want = tool_support.generated_images(G, [5], label, 1, "const", dev)
        assert torch.equal(got[d], want[0].permute(1, 2, 0)), d
    assert not torch.equal(got[0], got[1])
    # and the maps are the moments of those images
    images = got.cpu().numpy().transpose(0, 3, 1, 2).reshape(1, 3, 3 * 256)
    total, squares = mu.restate_accumulate(images)
    want = mu.restate_numerator([np.array(total[0]).reshape(3, 256).tolist()], [np.array(squares[0]).reshape(3, 256).tolist()], 3)
    assert num[0, 0].reshape(-1).tolist() == want[0]
