"""The latent directions tool without a device: the op's numpy path against the scalar restatement of directions_util bit for bit, the
properties of the Gram matrix (exactly rounded products, symmetry, constant columns, the float64 bound), planted structure through the
eigen-decomposition, `edit_table`, and the tool end to end on a snapshot the trainer wrote, with the CPU restatement of the generator."""
import importlib
import json
import os
import types

import numpy as np
import PIL.Image
import pytest
import torch

import directions_util as du
from test_calc_metrics_cpu import _CpuGenerator, _run
from style_big_gan_amd import _lib, directions as DR, generate, tool_support
from style_big_gan_amd.torch_utils.ops import directions as ops

CPU = torch.device("cpu")
_BUILD = tool_support.build_generator


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x).copy())


def _centred(x, mean):
    return x - mean[None, :] if mean is not None else x


# ---------------------------------------------------------------------------------------------------------------- the op

@pytest.mark.parametrize("with_mean", [False, True])
@pytest.mark.parametrize("n,d", [(1, 4), (2, 5), (3, 8), (257, 4), (4097, 3)])
def test_cpu_path_equals_the_scalar_restatement(n, d, with_mean):
    x = du.table(n, d)
    mean64 = ops.column_mean(_t(x)).numpy()
    assert du.same_bits(mean64, du.restate_mean(x))
    mean = mean64.astype(np.float32) if with_mean else None
    got = ops.gram(_t(x), _t(mean)).numpy()
    assert got.dtype == np.float64 and du.same_bits(got, du.restate_gram(x, mean))


def test_one_row_gives_the_exactly_rounded_product():
    x = du.table(1, 8)
    got = ops.gram(_t(x)).numpy()
    want = (x[0].astype(np.float64)[:, None] * x[0].astype(np.float64)[None, :]).astype(np.float32).astype(np.float64)       # fl(c_i c_j)
    assert du.same_bits(got, want)


@pytest.mark.parametrize("n,d", [(257, 32), (300, 96)])
def test_symmetric_bit_for_bit(n, d):
    _, plain, centred = du.cpu_results(n, d)
    assert du.same_bits(plain, plain.T) and du.same_bits(centred, centred.T)


def test_a_constant_column_gives_an_exactly_zero_row_and_column():
    mean, _, centred = du.cpu_results(257, 32, "constant")
    assert mean[1] == np.float64(np.float32(1.7))               # 257 equal terms and one division: exact
    assert not centred[1].any() and not centred[:, 1].any() and centred[0, 0] > 0


@pytest.mark.parametrize("n,d", [(130, 512), (257, 32), (300, 96), (4097, 32)])
def test_float64_bound(n, d):
    """|G - G64| <= gamma sum_n |c_i c_j| elementwise, gamma = 256 u / (1 - 256 u), u = 2^-24: the bound of a 256-term fp32 chain; the float64
    stages add at most (groups + chunks) 2^-53 relative, which the slack between a chain's real error and its bound covers many times."""
    x = du.table(n, d)
    mean, plain, centred = du.cpu_results(n, d)
    u = 2.0 ** -24
    gamma = 256 * u / (1 - 256 * u)
    for got, m in ((plain, None), (centred, mean.astype(np.float32))):
        c = _centred(x, m).astype(np.float64)
        want, budget = c.T @ c, np.abs(c).T @ np.abs(c)
        err = np.abs(got - want)
        print(f"({n}, {d}) mean {m is not None}: max err / max |G| = {err.max() / np.abs(want).max():.3e}, max err / bound = {(err / (gamma * budget + 1e-300)).max():.3e}")
        assert (err <= gamma * budget).all()
        assert err.max() <= 5.1e-7 * np.abs(want).max()


def _planted():
    rng = np.random.RandomState(0)
    scales = np.array([8, 4, 2] + [0.25] * 61)
    base = rng.randn(2000, 64)
    q, _ = np.linalg.qr(rng.randn(64, 64))
    x = ((base * scales) @ q.T + 5).astype(np.float32)
    return x, q, scales


@pytest.fixture(scope="module")
def planted():
    x, q, scales = _planted()
    xt = _t(x)
    mean = ops.column_mean(xt)
    matrix = ops.gram(xt, mean.to(torch.float32)).numpy() / (len(x) - 1)
    return matrix, q, scales


def test_planted_structure_is_recovered(planted):
    matrix, q, scales = planted
    comps, values, stdev = DR.eigen(matrix, 3)
    for k in range(3):
        cos = abs(float(comps[k].astype(np.float64) @ q[:, k]))
        print(f"component {k}: |cos| {cos:.5f}, stdev {stdev[k]:.3f}")
        assert cos >= 0.999
        assert abs(float(stdev[k]) - scales[k]) <= 0.05 * scales[k]


def test_eigen_decomposition(planted):
    matrix = planted[0]
    comps, values, stdev = DR.eigen(matrix, 8)
    assert comps.dtype == stdev.dtype == np.float32 and values.dtype == np.float64 and comps.shape == (8, 64) and values.shape == (64,) and stdev.shape == (8,)
    assert (np.diff(values) <= 0).all()
    assert du.same_bits(stdev, np.sqrt(np.maximum(values[:8], 0)).astype(np.float32))
    vectors = np.linalg.eigh(matrix)[1][:, ::-1].T
    for k in range(8):
        top = int(np.argmax(np.abs(comps[k])))
        assert comps[k, top] > 0
        v = vectors[k] if vectors[k][np.argmax(np.abs(vectors[k]))] > 0 else -vectors[k]
        assert du.same_bits(comps[k], v.astype(np.float32))
        assert np.linalg.norm(matrix @ v - values[k] * v) <= 1e-10 * np.linalg.norm(matrix)
    # ties in magnitude go to the lowest index; negative eigenvalues give a zero stdev
    comps, values, stdev = DR.eigen(np.array([[0.0, -1.0], [-1.0, 0.0]]), 2)
    assert np.allclose(values, [1, -1]) and abs(stdev[0] - 1) < 1e-6 and stdev[1] == 0 and (comps[:, 0] > 0).all()


def _edit_case(s, l, d, k, t, seed=3):
    rng = np.random.RandomState(seed)
    sig = DR.sigma_table(2.0, t) if t % 2 else rng.randn(t).astype(np.float32)
    return (rng.randn(s, l, d).astype(np.float32), rng.randn(k, d).astype(np.float32), (rng.rand(k) + 0.5).astype(np.float32), sig)


def test_edit_table():
    ws, comps, scale, sigmas = _edit_case(2, 3, 5, 2, 3)
    layers = [0, 2]
    got = ops.edit_table(_t(ws), _t(comps), _t(scale), _t(sigmas), layers).numpy()
    assert got.shape == (12, 3, 5) and du.same_bits(got, du.restate_edit(ws, comps, scale, sigmas, layers))
    cells = got.reshape(2, 2, 3, 3, 5)
    assert sigmas[1] == 0 and sigmas[0] == -sigmas[2] == -2
    for k in range(2):
        assert np.array_equal(cells[:, k, 1], ws)                # the centre column is the base latent
    assert du.same_bits(cells[:, :, :, 1], np.broadcast_to(ws[:, None, None, 1], [2, 2, 3, 5]))          # the unselected layer is a copy
    assert not np.array_equal(cells[:, :, 0, 0], cells[:, :, 2, 0])
    with pytest.raises(RuntimeError, match=r"non-empty.*\(2, 3, 5\)"):
        ops.edit_table(_t(ws), _t(comps), _t(scale), _t(sigmas), [])
    with pytest.raises(RuntimeError, match="layers"):
        ops.edit_table(_t(ws), _t(comps), _t(scale), _t(sigmas), [3])
    for s, k, t in [(0, 2, 3), (2, 0, 3), (2, 2, 0)]:
        w2, c2, s2, g2 = _edit_case(s, 3, 5, k, t)
        empty = ops.edit_table(_t(w2), _t(c2), _t(s2), _t(g2), [0])
        assert empty.shape == (0, 3, 5) and empty.dtype == torch.float32


def test_refusals():
    x = torch.zeros([4, 8])
    for fn in (ops.column_mean, ops.gram):
        for bad, message in [(x.double(), r"float64.*\(4, 8\)"), (x.t(), r"\(8, 4\)"), (x[:, ::2], r"\(4, 4\)"), (x[0], r"\(8,\)"), (x[:0], r"\(0, 8\)"),
                             (torch.zeros([2, 0]), r"\(2, 0\)"), (torch.zeros([1, 1025]), r"\(1, 1025\)")]:
            with pytest.raises(RuntimeError, match=message):
                fn(bad)
    assert ops.column_mean(torch.zeros([1, 1024])).shape == (1024,) and ops._table(torch.zeros([1, 1024]), "gram") == (1, 1024)
    for mean, message in [(torch.zeros([8], dtype=torch.float64), "float64"), (torch.zeros([7]), r"\(7,\)"), (torch.zeros([16])[::2], r"\(8,\)"),
                          (torch.zeros([8], device="meta"), "meta")]:
        with pytest.raises(RuntimeError, match=message):
            ops.gram(x, mean)
    ws, comps, scale, sigmas = (_t(v) for v in _edit_case(2, 3, 5, 2, 3))
    for args, message in [((ws.double(), comps, scale, sigmas), "float64"), ((ws, comps[:, :4].contiguous(), scale, sigmas), r"\(2, 3, 5\)"),
                          ((ws, comps, scale[:1], sigmas), r"\(1,\)"), ((ws, comps.to("meta"), scale, sigmas), "meta"),
                          ((ws.transpose(0, 1), comps, scale, sigmas), "strides"), ((torch.zeros([2, 3, 1025]), torch.zeros([2, 1025]), scale, sigmas), "1025")]:
        with pytest.raises(RuntimeError, match=message):
            ops.edit_table(*args, [0])


def test_prototypes_are_in_the_binding_table():
    lib = _lib.load()
    assert _lib.KERNEL_KINDS[30] == "directions" and _lib.DIRECTIONS_VARIANTS == {0: "mean", 1: "gram", 2: "merge", 3: "edit"}
    assert len(lib.sbg_directions_gram.argtypes) == 7 and len(lib.sbg_directions_edit.argtypes) == 12
    for n, d in [(1, 1), (4096, 512), (4097, 512), (65536, 512), (300, 1024)]:
        assert lib.sbg_directions_gram_workspace(n, d) == 8 * -(-n // (ops.CHUNK_ROWS * ops.GROUP_CHUNKS)) * d * d
        assert lib.sbg_directions_mean_workspace(n, d) == 8 * -(-n // ops.MEAN_ROWS) * d
    for n, d in [(0, 8), (8, 0), (8, 1025), (-1, 8)]:
        assert lib.sbg_directions_gram_workspace(n, d) == -1 and lib.sbg_directions_mean_workspace(n, d) == -1


# ---------------------------------------------------------------------------------------------------------------- the tool

def test_sigmas_and_layers():
    s = DR.sigma_table(2, 5)
    assert s.dtype == np.float32 and s.tolist() == [-2.0, -1.0, 0.0, 1.0, 2.0]
    s = DR.sigma_table(3, 7)
    assert s[3] == 0 and np.array_equal(s, -s[::-1]) and du.same_bits(s, (np.float64(3) * (2 * np.arange(7.0) - 6) / 6).astype(np.float32))
    assert DR.sigma_table(3, 1).tolist() == [0.0]
    for steps in (0, 2, 4, -1):
        with pytest.raises(ValueError, match="--steps"):
            DR.sigma_table(2, steps)
    assert DR.parse_layers("all", 6) == DR.parse_layers(None, 6) == [0, 1, 2, 3, 4, 5]
    assert DR.parse_layers("1-3", 6) == [1, 2, 3] and DR.parse_layers("4,0,4", 6) == [0, 4]
    with pytest.raises(ValueError, match="0 to 5"):
        DR.parse_layers("2-6", 6)


class _ToolGenerator(_CpuGenerator):
    """the CPU restatement of the snapshot's generator with the surface the tool uses on top of `project()`'s: `w_dim`, a mapping that takes
    `truncation_psi` (1 only) and `synthesis.style_slots()` of the package's own network built on the host from the same weights"""

    def __init__(self, m, state, real):
        super().__init__(m, state)
        self.w_dim, self.num_ws = m["w_dim"], self.mapping.num_ws
        object.__setattr__(self, "real", real)
        self.synthesis.style_slots = real.synthesis.style_slots

    def _mapping(self, z, c, truncation_psi=1, truncation_cutoff=None):
        assert truncation_psi == 1 and truncation_cutoff is None
        return super()._mapping(z, c)


def _tool_generator(config, state, device):
    assert torch.device(device).type == "cpu"
    m = dict(z_dim=16, w_dim=16, img_resolution=16, channel_base=256, channel_max=16, mapping_layers=2, conv_clamp=256)
    return _ToolGenerator(m, state, _BUILD(config, state, "cpu")).eval().requires_grad_(False)


@pytest.fixture(scope="module")
def tool_run(tmp_path_factory):
    """one pca run of the CLI on a snapshot the trainer wrote: (overrides, snapshot, outdir, result, generator)"""
    tmp_path = tmp_path_factory.mktemp("directions")
    _, overrides, snap, _ = _run(tmp_path)
    out = tmp_path / "out"
    mp = pytest.MonkeyPatch()
    mp.setattr("style_big_gan_amd.tool_support.build_generator", _tool_generator)
    try:
        result = DR.run_directions(overrides + [f"--snapshot={snap}", f"--outdir={out}", "--device=cpu", "--num=300", "--components=3", "--seeds=0,1", "--steps=3"])
        from style_big_gan_amd import arguments
        G = tool_support.load_generator(arguments.load_config(overrides), snap, CPU, announce=False)
        yield overrides, snap, out, result, G
    finally:
        mp.undo()


def test_the_tool_on_a_snapshot(tool_run, capsys):
    overrides, snap, out, result, G = tool_run
    assert sorted(os.listdir(out)) == ["directions.json", "directions.npz", "seed0000.png", "seed0001.png"]
    npz = np.load(out / "directions.npz")
    assert sorted(npz.files) == ["components", "eigenvalues", "layers", "mean", "method", "num", "seed", "sigmas", "stdev", "total_variance"]
    assert str(npz["method"]) == "pca" and int(npz["num"]) == 300 and int(npz["seed"]) == 0 and npz["layers"].tolist() == list(range(6))
    assert npz["components"].shape == (3, 16) and npz["components"].dtype == np.float32 and npz["stdev"].shape == (3,) and npz["stdev"].dtype == np.float32
    assert npz["eigenvalues"].shape == (16,) and npz["eigenvalues"].dtype == np.float64 and npz["mean"].shape == (16,) and npz["mean"].dtype == np.float64
    assert npz["sigmas"].tolist() == [-2.0, 0.0, 2.0] and float(npz["total_variance"]) == float(npz["eigenvalues"].sum())
    # the analysis is the op's on the mapped latents (w_dim = 16: the partial-tile path)
    x = DR.mapped_latents(G, 300, 0, torch.zeros([1, 0]), 64, CPU)
    mean = ops.column_mean(x)
    comps, values, stdev = DR.eigen(ops.gram(x, mean.to(torch.float32)).numpy() / 299, 3)
    assert du.same_bits(npz["components"], comps) and du.same_bits(npz["eigenvalues"], values) and du.same_bits(npz["stdev"], stdev)
    assert du.same_bits(npz["mean"], mean.numpy())
    stats = json.loads(open(out / "directions.json").read(), parse_constant=lambda name: pytest.fail(f"directions.json holds {name}"))
    assert stats == result["stats"]
    assert set(stats) == {"method", "num", "w_dim", "num_ws", "layers", "sigmas", "components", "effective_dim"}
    assert (stats["method"], stats["num"], stats["w_dim"], stats["num_ws"], stats["sigmas"]) == ("pca", 300, 16, 6, [-2.0, 0.0, 2.0])
    assert len(stats["components"]) == 3 and all(set(c) == {"eigenvalue", "stdev", "explained", "cumulative"} for c in stats["components"])
    explained = [c["explained"] for c in stats["components"]]
    assert all(e > 0 for e in explained) and sum(explained) <= 1 and explained == sorted(explained, reverse=True)
    assert abs(stats["components"][-1]["cumulative"] - sum(explained)) < 1e-12 and 1 <= stats["effective_dim"] <= 16
    # the pictures: 3 components x 3 sigmas of 16 x 16 images; the centre column is the image generate.py writes for the seed
    for i, seed in enumerate((0, 1)):
        png = np.array(PIL.Image.open(out / f"seed{seed:04d}.png"))
        assert png.shape == (48, 48, 3) and np.array_equal(png, result["grids"][f"seed{seed:04d}.png"])
        want = generate.generate_images(G, seeds=[seed], device=CPU)[0]
        for k in range(3):
            assert np.array_equal(png[16 * k:16 * k + 16, 16:32], want), (seed, k)
        assert not np.array_equal(png[:16, :16], png[:16, 32:])


def test_a_run_from_the_stored_analysis_writes_the_same_pictures(tool_run, tmp_path, monkeypatch):
    overrides, snap, out, result, G = tool_run
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", _tool_generator)
    monkeypatch.setattr(ops, "gram", lambda *a, **k: pytest.fail("--from must not analyse"))
    again = tmp_path / "again"
    DR.run_directions(overrides + [f"--snapshot={snap}", f"--outdir={again}", "--device=cpu", f"--from={out / 'directions.npz'}", "--seeds=0,1", "--steps=3"])
    assert sorted(os.listdir(again)) == sorted(os.listdir(out))
    for name in ("seed0000.png", "seed0001.png"):
        assert open(again / name, "rb").read() == open(out / name, "rb").read()
    a, b = np.load(again / "directions.npz"), np.load(out / "directions.npz")
    assert all(du.same_bits(a[k], b[k]) for k in b.files)
    # other layers, a projected latent
    w = G.mapping(torch.from_numpy(tool_support.seed_latents(G, [0])), None).numpy()
    np.savez(tmp_path / "projected_w.npz", w=w)
    res = DR.latent_directions(G, from_file=str(out / "directions.npz"), layers="0-1", projected_w=str(tmp_path / "projected_w.npz"), steps=3, device=CPU,
                               outdir=str(tmp_path / "proj"))
    assert sorted(os.listdir(tmp_path / "proj")) == ["directions.json", "directions.npz", "w00.png"] and res["stats"]["layers"] == [0, 1]
    assert np.array_equal(res["grids"]["w00.png"][:, 16:32], result["grids"]["seed0000.png"][:, 16:32])
    assert not np.array_equal(res["grids"]["w00.png"], result["grids"]["seed0000.png"])


def test_sefa_uses_the_convolutions_style_affines(tool_run, tmp_path):
    overrides, snap, out, result, G = tool_run
    slots = list(G.real.synthesis.style_slots())
    assert [(name, idx) for name, _, idx in slots] == [("b4.conv1", 0), ("b4.torgb", 1), ("b8.conv0", 1), ("b8.conv1", 2), ("b8.torgb", 3), ("b16.conv0", 3),
                                                      ("b16.conv1", 4), ("b16.torgb", 5)]
    assert all(affine is G.real.synthesis.get_submodule(name).affine for name, affine, _ in slots)
    with pytest.raises(ValueError, match="ToRGB"):
        DR.latent_directions(G, method="sefa", layers="5", components=3, device=CPU)
    picked = [affine.weight.detach().double().numpy() for name, affine, idx in slots if name in ("b4.conv1", "b8.conv0", "b8.conv1")]
    rows = np.concatenate(picked)
    rows = (rows / np.sqrt((rows * rows).sum(axis=1, keepdims=True))).astype(np.float32)
    assert rows.shape == (48, 16) and du.same_bits(DR.sefa_rows(G, [0, 1, 2]), rows)
    res = DR.latent_directions(G, method="sefa", layers="0-2", components=3, seeds=[0], steps=3, device=CPU, outdir=str(tmp_path / "sefa"))
    comps, values, stdev = DR.eigen(ops.gram(_t(rows)).numpy(), 3)
    arrays = res["arrays"]
    assert du.same_bits(arrays["components"], comps) and du.same_bits(arrays["eigenvalues"], values) and not arrays["mean"].any()
    assert (str(arrays["method"]), int(arrays["num"]), int(arrays["seed"]), arrays["layers"].tolist()) == ("sefa", 48, -1, [0, 1, 2])
    assert arrays["sigmas"].tolist() == [-3.0, 0.0, 3.0]         # the default range of sefa; scale 1: plain distances in W
    assert abs(float(values.sum()) - 48) < 1e-4                  # unit rows: the trace is their number
    assert sorted(os.listdir(tmp_path / "sefa")) == ["directions.json", "directions.npz", "seed0000.png"]
    # scale = 1: the edited latents are w + sigma * component on the layers 0..2
    w = G.mapping(torch.from_numpy(tool_support.seed_latents(G, [0])), None)
    table = ops.edit_table(w, _t(comps), torch.ones([3]), _t(arrays["sigmas"]), [0, 1, 2])
    canvas = tool_support.image_export.tile(G.synthesis(table, noise_mode="const"), (3, 3), "clamp").numpy()
    assert np.array_equal(canvas, res["grids"]["seed0000.png"])


def test_option_parsing_and_refusals(tmp_path, capsys):
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    ok = [f"--snapshot={snap}", f"--outdir={tmp_path / 'out'}"]
    overrides, args = DR.parse_args(["exp.config=a.yaml"] + ok)
    assert overrides == ["exp.config=a.yaml"]
    assert (args.method, args.num, args.seed, args.components, args.layers, args.from_file, args.seeds, args.projected_w, args.extent, args.steps) == \
        ("pca", 65536, 0, 8, None, None, None, None, None, 5)
    assert (args.truncation_psi, args.class_idx, args.noise_mode, args.device, args.batch) == (1, None, "const", "auto", 64)
    _, args = DR.parse_args(ok + ["--method=sefa", "--layers=0-2", "--seeds=0-3", "--range=1.5", "--steps=7", "--components=4", "--trunc=0.7", "--device=cpu"])
    assert (args.method, args.layers, args.seeds, args.extent, args.steps, args.components) == ("sefa", "0-2", [0, 1, 2, 3], 1.5, 7, 4)
    np.savez(tmp_path / "projected_w.npz", w=np.zeros([1, 6, 16], dtype=np.float32))
    for bad, message in [(ok + ["--seeds=0-3", f"--projected-w={tmp_path / 'projected_w.npz'}"], "exclude one another"), (ok + ["--steps=4"], "--steps=4: must be odd"),
                         (ok + ["--steps=0"], "--steps=0"), (ok + ["--components=0"], "--components=0"), (ok + ["--num=1"], "--num=1"),
                         (ok + ["--batch=0"], "--batch=0"), (ok + ["--range=-1"], "--range=-1"), (ok + ["--method=ica"], "invalid choice"),
                         ([f"--snapshot={tmp_path / 'absent.pt'}", ok[1]], "no such file"), (ok[:1], "--outdir"), (ok[1:], "--snapshot"),
                         (ok + [f"--from={tmp_path / 'absent.npz'}"], "no such file"), (ok + [f"--projected-w={tmp_path / 'absent.npz'}"], "no such file"),
                         (ok + ["--frobnicate"], "unrecognised")]:
        with pytest.raises(SystemExit):
            DR.parse_args(bad)
        assert message in capsys.readouterr().err, bad
    G = du.ExactGenerator()
    for more, message in [(dict(components=25), "--components=25: must be between 1 and w_dim = 24"), (dict(components=0), "--components=0"),
                          (dict(seeds=[0], projected_w=np.zeros([1, 6, 24])), "exclude one another"), (dict(steps=4), "--steps=4"),
                          (dict(layers="6"), "--layers=6"), (dict(num=1), "--num=1"), (dict(method="ica"), "--method=ica"), (dict(batch=0), "--batch=0"),
                          (dict(projected_w=np.zeros([1, 5, 24], dtype=np.float32)), "--projected-w")]:
        with pytest.raises(ValueError, match=message):
            DR.latent_directions(G, **dict(dict(num=40, device=CPU), **more))
    for other in (torch.nn.Linear(2, 2), types.SimpleNamespace(synthesis=None)):              # BigGAN, DCGAN: no W space
        with pytest.raises(ValueError, match="mapping and synthesis"):
            DR.latent_directions(other, num=40, device=CPU)


def test_the_stand_in_generator_end_to_end(tmp_path):
    """no seeds: the analysis alone; --trunc reaches the base latents; the batch size changes nothing"""
    G = du.ExactGenerator()
    res = DR.latent_directions(G, num=50, components=4, device=CPU, outdir=str(tmp_path / "a"))
    assert sorted(os.listdir(tmp_path / "a")) == ["directions.json", "directions.npz"] and res["grids"] == {}
    one = DR.latent_directions(G, num=50, components=4, seeds=[3], truncation_psi=0.5, batch=64, device=CPU)
    two = DR.latent_directions(G, num=50, components=4, seeds=[3], truncation_psi=0.5, batch=7, device=CPU)
    assert one["grids"]["seed0003.png"].shape == (4 * 8, 5 * 8, 3) and np.array_equal(one["grids"]["seed0003.png"], two["grids"]["seed0003.png"])
    z = torch.from_numpy(tool_support.seed_latents(G, [3]))
    want = tool_support.to_uint8(G(z, None, truncation_psi=0.5))[0]
    assert np.array_equal(one["grids"]["seed0003.png"][8:16, 16:24], want)
    assert all(du.same_bits(one["arrays"][k], two["arrays"][k]) for k in one["arrays"])


def test_the_tool_imports_no_other_tool():
    from test_tool_support_cpu import TOOLS
    mod = importlib.import_module("style_big_gan_amd.directions")
    others = {f"style_big_gan_amd.{t}" for t in tuple(TOOLS) + ("diversity", "realism", "style_mixing", "generate")}
    held = {v.__name__ if isinstance(v, types.ModuleType) else getattr(v, "__module__", None) for v in vars(mod).values()}
    assert not held & others, held & others
