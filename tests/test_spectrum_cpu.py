"""The average power spectrum on the CPU (torch_utils/ops/spectrum.py, avg_spectra.py): the exact patterns, the
value graph against numpy's float64 transform under the derived bound, the invariance of the float64 chain, the host arithmetic, every
refusal, and the tool end to end."""
import json
import os

import numpy as np
import PIL.Image
import pytest
import torch

import spectrum_util as SU
from style_big_gan_amd import _lib, avg_spectra as AS
from style_big_gan_amd.torch_utils.ops import spectrum
from style_big_gan_amd.train_parts.datasets import ImageFolderDataset
from test_calc_metrics_cpu import _run

CPU = torch.device("cpu")


@pytest.mark.parametrize("R", [16, 64])
def test_exact_patterns(R):
    """bit reversal, the transposition, which axis is which, and the half that is kept: the whole half-spectrum, zeros included"""
    window, twiddle = SU.pattern_tables(R)
    for name, (image, want) in SU.patterns(R).items():
        acc = torch.zeros([R // 2 + 1, R], dtype=torch.float64)
        out = spectrum.accumulate(acc, torch.from_numpy(image.astype(np.float32))[None, None], 1.0, 0.0, window, twiddle)
        assert out is acc and np.array_equal(acc.numpy(), want), (name, np.argwhere(acc.numpy() != want)[:4])


def test_tables():
    window, twiddle = spectrum.tables(16, 64)
    assert window.dtype == twiddle.dtype == torch.float32 and tuple(window.shape) == (16,) and tuple(twiddle.shape) == (32, 2)
    k = np.kaiser(16, 8.0)
    assert np.array_equal(window.numpy(), (k / np.sqrt((k * k).sum())).astype(np.float32))
    assert abs(float((window.double() ** 2).sum()) - 1) < 1e-6
    ang = 2 * np.pi * np.arange(32) / 64
    assert np.array_equal(twiddle.numpy(), np.stack([np.cos(ang), -np.sin(ang)], axis=1).astype(np.float32))
    assert twiddle[0].tolist() == [1.0, 0.0] and twiddle[16, 1] == -1.0
    assert spectrum.scale_shift(100.0, 50.0) == (float(np.float32(1 / 50.0)), float(np.float32(-2.0)))


@pytest.mark.parametrize("R,P", [(16, 1), (16, 4), (32, 1), (64, 2)])
def test_accuracy_against_float64(R, P):
    """per image-channel ||Y^ - Y||_2 <= tau ||Y||_2, and the accumulated power within (2 tau + tau^2) sum ||Y||^2 (1 + N C 2^-52)"""
    B, C, S = 3, 2, R * P
    images, s, t, window, twiddle, acc = SU.case("float", B, C, R, P)
    got = spectrum.transform(images, s, t, window, twiddle).to(torch.complex128).numpy()
    ref = SU.restatement(images.numpy(), s, t, window.numpy(), S)
    assert got.shape == ref.shape == (B, C, S // 2 + 1, S)
    tau = SU.tau(S)
    err = np.sqrt((np.abs(got - ref) ** 2).sum((2, 3)))
    norm = np.sqrt((np.abs(ref) ** 2).sum((2, 3)))
    print(f"R={R} P={P}: max relative error {float((err / norm).max()):.3e}, tau {tau:.3e}, ratio {float((err / norm).max() / tau):.4f}")
    assert (err <= tau * norm).all()
    spectrum.accumulate(acc, images, s, t, window, twiddle)
    power = (np.abs(ref) ** 2)
    bound = (2 * tau + tau * tau) * power.sum() * (1 + B * C * 2.0 ** -52)
    assert np.abs(acc.numpy() - power.sum((0, 1))).sum() <= bound
    # and the accumulator is the float64 chain over the transform's power, image-channels in order
    chain = np.zeros([S // 2 + 1, S])
    for y in spectrum.transform(images, s, t, window, twiddle).reshape(B * C, S // 2 + 1, S):
        re, im = y.real.double().numpy(), y.imag.double().numpy()
        chain += re * re + im * im
    assert np.array_equal(acc.numpy(), chain)


@pytest.mark.parametrize("kind", ["float", "bytes"])
def test_batch_invariance(kind):
    images, s, t, window, twiddle, acc = SU.case(kind, 5, 3, 16, 2)
    start = torch.from_numpy(np.random.RandomState(3).rand(*acc.shape) * 1e-3)
    one = spectrum.accumulate(start.clone(), images, s, t, window, twiddle)
    two = spectrum.accumulate(start.clone(), images[:2], s, t, window, twiddle)
    spectrum.accumulate(two, images[2:], s, t, window, twiddle)
    each = spectrum.accumulate(start.clone(), images, s, t, window, twiddle, max_workspace_bytes=1)      # every image-channel its own piece
    assert SU.same_bits(one, two) and SU.same_bits(one, each)
    zero = spectrum.accumulate(acc, images, s, t, window, twiddle)
    assert not SU.same_bits(one, zero)                          # a non-zero accumulator continues its chain
    assert np.allclose((one - start).numpy(), zero.numpy(), rtol=1e-9, atol=1e-12)
    assert spectrum.accumulate(start.clone(), images[:0], s, t, window, twiddle).equal(start)
    if kind == "bytes":                                         # bytes as uint8 and as fp32 are one input
        assert SU.same_bits(zero, spectrum.accumulate(torch.zeros_like(acc), images.float(), s, t, window, twiddle))


def test_full_spectrum_symmetry():
    images, s, t, window, twiddle, acc = SU.case("float", 2, 1, 16, 2)
    spectrum.accumulate(acc, images, s, t, window, twiddle)
    S = 32
    full = spectrum.full_spectrum(acc, 2)
    assert full.dtype == np.float64 and full.shape == (S, S)
    assert np.array_equal(full[:, :S // 2 + 1], acc.numpy().T / 2)
    k = np.arange(S)
    assert np.array_equal(full, full[(S - k) % S][:, (S - k) % S])
    whole = np.fft.fft2((images.double().numpy() * np.float32(s) + np.float64(np.float32(t))) * window.double().numpy()[None, None, None, :]
                        * window.double().numpy()[None, None, :, None], s=(S, S))
    assert np.allclose(full, (np.abs(whole) ** 2).mean((0, 1)), rtol=1e-4, atol=1e-9)
    assert np.array_equal(spectrum.full_from_half(spectrum.half_spectrum(acc, 2)), full)


def test_radial_profile_slices_and_compare_by_hand():
    """S = 4: frequencies 0, 1, 2, -1 per axis; r = floor(sqrt(fy^2 + fx^2) + 0.5)"""
    full = np.arange(16, dtype=np.float64).reshape(4, 4)
    # r by (ky, kx): [[0,1,2,1],[1,1,2,1],[2,2,3,2],[1,1,2,1]]  (sqrt 2 -> 1, sqrt 5 -> 2, sqrt 8 -> 3: outside 0..S/2)
    bins = {0: [0], 1: [1, 3, 4, 5, 7, 12, 13, 15], 2: [2, 6, 8, 9, 11, 14]}
    want = np.array([np.mean(bins[r]) for r in range(3)])
    assert np.array_equal(spectrum.radial_profile(full), want)
    s0, s45 = spectrum.slices(full)
    assert s0.tolist() == [0.0, 1.0, 2.0] and s45.tolist() == [0.0, 5.0, 10.0]
    assert spectrum.to_db(np.array([0.0, 1.0, 100.0])).tolist() == [-300.0, 0.0, 20.0]
    # S = 8: ten times the energy in every bin with r > S/4 = 2 is +10 dB there and nothing below
    S = 8
    k = np.arange(S)
    f = np.where(k <= S // 2, k, k - S)
    r = np.floor(np.sqrt(f[:, None] ** 2.0 + f[None, :] ** 2.0) + 0.5)
    real = np.full([S, S], 2.0)
    gen = np.where(r > 2, 20.0, 2.0)
    out = spectrum.compare(real, gen)
    assert abs(out["hf_excess_db"] - 10.0) < 1e-12 and abs(out["lsd_db"] - np.sqrt(100.0 * 2 / 4)) < 1e-12
    assert spectrum.compare(real, real) == dict(lsd_db=0.0, hf_excess_db=0.0)
    assert spectrum.compare(gen, real)["hf_excess_db"] < 0


def test_normalisation():
    rng = np.random.RandomState(5)
    b = rng.randint(0, 256, [7, 3, 16, 16], dtype=np.uint8)
    total, total_sq, count = AS.byte_moments([torch.from_numpy(b[:3]), torch.from_numpy(b[3:])])
    v = b.astype(np.int64)
    assert (total, total_sq, count) == (int(v.sum()), int((v * v).sum()), b.size)
    mean, std = spectrum.normalisation(total, total_sq, count)
    assert abs(mean - b.astype(np.float64).mean()) < 1e-12 and abs(std - b.astype(np.float64).std()) < 1e-10
    with pytest.raises(ValueError, match="std of the real set is 0"):
        spectrum.normalisation(7 * 100, 7 * 100 * 100, 7)
    with pytest.raises(OverflowError, match="int64"):
        spectrum.normalisation(0, 0, 1 << 48)
    with pytest.raises(ValueError, match="must be positive"):
        spectrum.scale_shift(1.0, 0.0)


def test_refusals():
    images, s, t, window, twiddle, acc = SU.case("float", 1, 1, 16, 2)
    ok = dict(acc=acc, images=images, s=s, t=t, window=window, twiddle=twiddle)

    def refuses(exc, message, **change):
        with pytest.raises(exc, match=message):
            spectrum.accumulate(**{**ok, **change})

    z = lambda *shape: torch.zeros(shape)
    refuses(ValueError, r"R=24 must be a power of two", images=z(1, 1, 24, 24))
    refuses(ValueError, r"R=8 must be a power of two in \[16, 1024\]", images=z(1, 1, 8, 8))
    refuses(ValueError, r"R=2048", images=z(1, 1, 2048, 2048))
    refuses(ValueError, r"S=128 must be P \* R with the padding factor P in \(1, 2, 4\)", twiddle=z(64, 2))
    refuses(ValueError, r"S=48", twiddle=z(24, 2))
    refuses(ValueError, r"square \[B, C, R, R\], got \(1, 1, 16, 32\)", images=z(1, 1, 16, 32))
    refuses(ValueError, r"square", images=z(1, 16, 16))
    refuses(ValueError, r"1\.\.4 channels", images=z(1, 5, 16, 16))
    refuses(RuntimeError, r"uint8 or float32", images=z(1, 1, 16, 16).double())
    refuses(ValueError, r"window must be float32 \[16\].*\(32,\)", window=z(32))
    refuses(ValueError, r"window must be float32", window=window.double())
    refuses(ValueError, r"twiddle must be float32 \[S/2, 2\]", twiddle=z(32))
    refuses(ValueError, r"acc must be a dense float64 \[17, 32\].*\(32, 17\)", acc=torch.zeros([32, 17], dtype=torch.float64))
    refuses(ValueError, r"acc must be a dense float64.*float32", acc=z(17, 32))
    refuses(ValueError, r"window is on meta, images on cpu", window=window.to("meta"))
    refuses(ValueError, r"twiddle is on meta", twiddle=twiddle.to("meta"))
    refuses(ValueError, r"acc is on meta", acc=acc.to("meta"))
    refuses(ValueError, r"max_workspace_bytes", max_workspace_bytes=0)
    refuses(RuntimeError, r"must be a torch tensor", images=images.numpy())
    for R, S in [(24, 24), (8, 8), (2048, 2048), (16, 128), (16, 24)]:
        with pytest.raises(ValueError, match=f"R={R}|S={S}"):
            spectrum.tables(R, S)
    with pytest.raises(ValueError, match=r"float64 \[S, S\]"):
        spectrum.radial_profile(np.zeros([4, 6]))
    with pytest.raises(ValueError, match="different sides"):
        spectrum.compare(np.ones([4, 4]), np.ones([8, 8]))
    with pytest.raises(ValueError, match=r"float64 \[S/2 \+ 1, S\]"):
        spectrum.full_spectrum(np.zeros([4, 4]), 1)
    with pytest.raises(ValueError, match="count=0"):
        spectrum.full_spectrum(np.zeros([3, 4]), 0)


def test_abi_symbols_resolve():
    lib = _lib.load()
    for name in ("sbg_spectrum_workspace", "sbg_spectrum_rows", "sbg_spectrum_cols"):
        assert getattr(lib, name) is not None
    assert _lib.KERNEL_KINDS[28] == "spectrum" and _lib.SPECTRUM_VARIANTS == {0: "rows", 1: "cols"}
    assert lib.sbg_spectrum_workspace(6, 16, 64) == 6 * 33 * 16 * 8 and lib.sbg_spectrum_workspace(1, 1024, 4096) == 2049 * 1024 * 8
    for bc, R, S in [(0, 16, 16), (1, 8, 8), (1, 24, 24), (1, 2048, 2048), (1, 16, 128), (1, 32, 16), (1 << 40, 1024, 1024)]:
        assert lib.sbg_spectrum_workspace(bc, R, S) == -1, (bc, R, S)


# ------------------------------------------------------------------------------------------------ the tool

def test_option_parsing_and_failures(tmp_path, capsys):
    snap = tmp_path / "network-snapshot-000000.pt"
    snap.write_bytes(b"")
    npz = tmp_path / "spectrum_real.npz"
    npz.write_bytes(b"")
    overrides, args = AS.parse_args(["exp.config=a.yaml", f"--outdir={tmp_path}"])
    assert overrides == ["exp.config=a.yaml"] and args.snapshot is None and args.num == 16384 and args.interp == 1 and args.batch == 64
    assert args.against is None and args.data is None and args.db_range is None and args.device == "auto" and args.noise_mode == "const"
    _, args = AS.parse_args([f"--outdir={tmp_path}", f"--snapshot={snap}", f"--against={npz}", "--num=100", "--interp=4", "--trunc=0.5", "--class=2",
                             "--noise-mode=random", "--device=cpu", "--batch=16", "--db-range=-60,20"])
    assert (args.num, args.interp, args.truncation_psi, args.class_idx, args.noise_mode, args.device, args.batch, args.db_range) == \
        (100, 4, 0.5, 2, "random", "cpu", 16, (-60.0, 20.0))
    ok = [f"--outdir={tmp_path}"]
    for bad, message in [([], "--outdir"), (ok + ["--num=0"], "at least 1"), (ok + ["--batch=0"], "at least 1"), (ok + ["--interp=3"], "invalid choice"),
                         (ok + [f"--snapshot={tmp_path / 'absent.pt'}"], "no such file"), (ok + [f"--against={tmp_path / 'absent.npz'}"], "no such file"),
                         (ok + [f"--against={npz}"], "needs --snapshot"), (ok + [f"--snapshot={snap}", f"--against={npz}", "--data=/d"], "exclude each other"),
                         (ok + ["--db-range=3"], "lo,hi"), (ok + ["--db-range=3,1"], "above lo"), (ok + ["--frobnicate"], "unrecognised")]:
        with pytest.raises(SystemExit):
            AS.parse_args(bad)
        assert message in capsys.readouterr().err, bad


def test_tool_end_to_end(tmp_path, monkeypatch, capsys):
    """a 16 x 16 data set of 24 images; generators that look their images up in a table"""
    _, overrides, snap, _ = _run(tmp_path)
    data, items = SU.tool_dataset(tmp_path)
    bank = [items]
    monkeypatch.setattr("style_big_gan_amd.tool_support.build_generator", lambda config, state, device: SU.OrderedGenerator(bank[0]).to(device))
    common = overrides + [f"--data={data}", "--device=cpu", "--batch=7", "--interp=2"]

    # the data set alone
    alone = tmp_path / "alone"
    AS.run_avg_spectra(common + [f"--outdir={alone}", "--num=100"])
    assert sorted(os.listdir(alone)) == ["spectrum_real.npz"]
    real = np.load(alone / "spectrum_real.npz")
    assert sorted(real.files) == sorted(AS.NPZ_KEYS)
    assert real["spectrum"].dtype == np.float64 and real["spectrum"].shape == (32, 17)
    assert (int(real["image_size"]), int(real["interp"]), int(real["channels"]), int(real["num_images"])) == (16, 2, 3, 24)
    assert abs(float(real["mean"]) - items.astype(np.float64).mean()) < 1e-12 and abs(float(real["std"]) - items.astype(np.float64).std()) < 1e-10
    window, twiddle = spectrum.tables(16, 32)
    s, t = spectrum.scale_shift(float(real["mean"]), float(real["std"]))
    acc = spectrum.accumulate(torch.zeros([17, 32], dtype=torch.float64), torch.from_numpy(items), s, t, window, twiddle)
    assert np.array_equal(real["spectrum"], acc.numpy().T / 72)

    # the generator returns the data set's own items in order: the two spectra are one
    out = tmp_path / "out"
    capsys.readouterr()
    result = AS.run_avg_spectra(common + [f"--outdir={out}", f"--snapshot={snap}", "--num=24"])
    assert sorted(os.listdir(out)) == ["spectrum.json", "spectrum.png", "spectrum_gen.npz", "spectrum_real.npz"]
    gen = np.load(out / "spectrum_gen.npz")
    assert sorted(gen.files) == sorted(AS.NPZ_KEYS) and np.array_equal(gen["spectrum"], real["spectrum"]) and int(gen["num_images"]) == 24
    assert np.array_equal(np.load(out / "spectrum_real.npz")["spectrum"], real["spectrum"])
    stats = json.load(open(out / "spectrum.json"))
    assert stats["lsd_db"] == 0 and stats["hf_excess_db"] == 0 and stats == json.loads(json.dumps(result["stats"]))
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["lsd_db"] == 0
    assert set(stats) == {"image_size", "interp", "channels", "num_real", "num_gen", "mean", "std", "lsd_db", "hf_excess_db", "frequency", "frequency_45",
                          "real", "gen", "options"}
    assert stats["frequency"] == [r / 2 for r in range(17)] and (stats["num_real"], stats["num_gen"]) == (24, 24)
    full = spectrum.full_from_half(real["spectrum"])
    for which in ("real", "gen"):
        assert set(stats[which]) == {"radial_db", "slice_0_db", "slice_45_db"}
        assert stats[which]["radial_db"] == spectrum.to_db(spectrum.radial_profile(full)).tolist()
        assert stats[which]["slice_0_db"] == spectrum.to_db(full[0, :17]).tolist()
        assert stats[which]["slice_45_db"] == spectrum.to_db(full[np.arange(17), np.arange(17)]).tolist()
    png = np.array(PIL.Image.open(out / "spectrum.png"))
    assert png.shape == (32, 64) and png.dtype == np.uint8 and np.array_equal(png[:, :32], png[:, 32:])
    db = spectrum.to_db(full)
    hi = float(np.ceil(db.max()))
    assert stats["options"]["db_range"] == [hi - 80, hi]
    assert np.array_equal(png[:, :32], np.floor(255 * np.clip((np.fft.fftshift(db) - (hi - 80)) / 80, 0, 1) + 0.5).astype(np.uint8))

    # --against the run's own spectrum_real.npz reproduces spectrum.json without reading the data set
    again = tmp_path / "again"
    AS.run_avg_spectra(overrides + ["--device=cpu", "--batch=5", "--interp=2", f"--outdir={again}", f"--snapshot={snap}", "--num=24",
                                    f"--against={out / 'spectrum_real.npz'}"])
    assert sorted(os.listdir(again)) == ["spectrum.json", "spectrum.png", "spectrum_gen.npz"]
    stats_again = json.load(open(again / "spectrum.json"))
    assert stats_again["options"].pop("batch") == 5 and stats["options"].pop("batch") == 7 and stats_again == stats
    assert np.array_equal(np.load(again / "spectrum_gen.npz")["spectrum"], gen["spectrum"])

    # a checkerboard of +-8 on the generated bytes is excess energy in the outer band.  The corner (S/2, S/2) lies at radius S / sqrt 2,
    # outside the radial profile: the band sees it through the window's main lobe only (on this smooth set; on white noise not at all),
    # the 45 degree slice sees it directly.  Stripes (-1)^x land inside the band, at r = S/2.
    yy, xx = np.meshgrid(np.arange(16), np.arange(16), indexing="ij")
    bank[0] = (items.astype(np.int64) + (8 * (-1) ** (xx + yy))[None, None]).astype(np.uint8)
    board = AS.run_avg_spectra(overrides + ["--device=cpu", "--interp=2", f"--outdir={tmp_path / 'board'}", f"--snapshot={snap}", "--num=24",
                                            f"--against={out / 'spectrum_real.npz'}", "--db-range=-40,30"])["stats"]
    print(f"checkerboard: hf_excess_db {board['hf_excess_db']!r}, lsd_db {board['lsd_db']!r}")
    assert board["hf_excess_db"] > 0 and board["lsd_db"] > 0 and board["options"]["db_range"] == [-40.0, 30.0]
    assert board["gen"]["slice_45_db"][16] > board["real"]["slice_45_db"][16] + 20             # the Nyquist corner
    bank[0] = (items.astype(np.int64) + (8 * (-1) ** xx)[None, None]).astype(np.uint8)
    stripes = AS.run_avg_spectra(overrides + ["--device=cpu", "--interp=2", f"--outdir={tmp_path / 'stripes'}", f"--snapshot={snap}", "--num=24",
                                              f"--against={out / 'spectrum_real.npz'}"])["stats"]
    print(f"stripes: hf_excess_db {stripes['hf_excess_db']!r}")
    assert stripes["hf_excess_db"] > board["hf_excess_db"] and stripes["gen"]["slice_0_db"][16] > stripes["real"]["slice_0_db"][16] + 20

    # a file that describes other images is refused by name
    for flag, field in (("--interp=4", "interp"), ("--interp=1", "interp")):
        with pytest.raises(ValueError, match=f"its {field} is 2"):
            AS.run_avg_spectra(overrides + ["--device=cpu", flag, f"--outdir={tmp_path / 'no'}", f"--snapshot={snap}", f"--against={out / 'spectrum_real.npz'}"])
    AS.save_npz(tmp_path / "other.npz", np.zeros([64, 33]), 1.0, 1.0, 32, 2, 3, 5)
    with pytest.raises(ValueError, match="its image_size is 32, this run has image_size=16"):
        AS.run_avg_spectra(overrides + ["--device=cpu", "--interp=2", f"--outdir={tmp_path / 'no'}", f"--snapshot={snap}", f"--against={tmp_path / 'other.npz'}"])
    AS.save_npz(tmp_path / "grey.npz", np.zeros([32, 17]), 1.0, 1.0, 16, 2, 1, 5)
    with pytest.raises(ValueError, match="its channels is 1, this run has channels=3"):
        AS.run_avg_spectra(overrides + ["--device=cpu", "--interp=2", f"--outdir={tmp_path / 'no'}", f"--snapshot={snap}", f"--against={tmp_path / 'grey.npz'}"])


def test_tool_function_refusals(tmp_path):
    data, items = SU.tool_dataset(tmp_path)
    dataset = ImageFolderDataset(path=data, xflip=True)        # mirrored copies are never measured
    G = SU.OrderedGenerator(items)
    result = AS.average_spectra(G, dataset, num=1000, device=CPU)
    assert result["num_real"] == 24 and result["stats"]["lsd_db"] == 0 and result["real"].shape == (16, 9)
    for kw, message in [(dict(num=0), "--num=0"), (dict(batch=0), "--batch=0"), (dict(interp=3), "--interp=3"), (dict(db_range=(1, 1)), "hi must be above lo")]:
        with pytest.raises(ValueError, match=message):
            AS.average_spectra(G, dataset, device=CPU, **kw)
    with pytest.raises(ValueError, match="one of a data set and --against"):
        AS.average_spectra(G, None, device=CPU)
    with pytest.raises(ValueError, match="the generator makes 3 x 32 x 32 images, the data set holds 3 x 16 x 16"):
        AS.average_spectra(SU.OrderedGenerator(np.zeros([2, 3, 32, 32], dtype=np.uint8)), dataset, device=CPU)
    flat = ImageFolderDataset(path=data)
    flat._load_raw_image = lambda i: np.full([3, 16, 16], 9, dtype=np.uint8)
    with pytest.raises(ValueError, match="std of the real set is 0"):
        AS.average_spectra(None, flat, device=CPU)
    dataset.close()
