"""Generate tests/golden/image_export.npz by running the REFERENCE's image writers on CPU.

Needs the reference checkout (SBG_REFERENCE, see make_golden.py) and no GPU:

    python tests/golden/make_golden_image_export.py

* ``setup_snapshot_image_grid`` and ``save_image_grid`` are called from the reference itself (stylegan2ada/training/training_loop.py
  :30-85, the same two functions as train_parts/trainers.py:63-118).  The module imports ``wandb``, which is not needed here: an empty
  stand-in module takes its place.  The data sets are the seeded toy sets of tests/image_export_util.py (a labelled RGB one and an
  unlabelled grey one); the indices the reference asks them for are recorded, the written PNG is read back and stored as an array.
* ``save_image_grid`` on float images with drange [-1, 1], and on the tie vectors (tests/image_export_util.tie_vector).
* The reference generator (stylegan2ada.training.networks.Generator, fp32) through the statements of stylegan2ada/generate.py:92-99
  (projected w), :105-121 (seeds, label, truncation) and stylegan2ada/style_mixing.py:69-110.  The two command-line tools cannot be
  called: they hard-code torch.device('cuda') and load a pickle.  ``generate()`` and ``style_mix()`` below restate those statements for
  the CPU, one for one, and keep the float images as well.
Nets: ``g16`` (unconditional 16x16, channel_base 256) and ``c16`` (3 classes), weights and noise buffers stored; w_avg is set to a
seeded non-zero vector so that truncation does something.
"""
import os
import sys
import tempfile
import types

import numpy as np
import PIL.Image
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))                        # tests/: the toy data sets and the tie vectors
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))       # the repository root (image_export_util imports the oracle)
from make_golden import R_net, dnnlib, _import_train_parts, npy, save         # noqa: E402
import image_export_util as iu                            # noqa: E402

NETS = dict(g16=dict(seed=730, c_dim=0), c16=dict(seed=731, c_dim=3))
NET_COMMON = dict(z_dim=16, w_dim=16, res=16, channel_base=256, channel_max=16, mapping_layers=2, conv_clamp=256)
GEN_CASES = [dict(tag="plain", net="g16", seeds=[0, 5, 85], psi=1, class_idx=None), dict(tag="trunc", net="g16", seeds=[5, 1234], psi=0.7, class_idx=None),
             dict(tag="cond", net="c16", seeds=[3, 4], psi=0.5, class_idx=1)]
MIX = dict(net="g16", rows=[85, 100, 75], cols=[55, 821, 100], styles=[0, 1, 2], psi=0.7)


def make_G(seed, c_dim):
    torch.manual_seed(seed)
    G = R_net.Generator(z_dim=NET_COMMON["z_dim"], c_dim=c_dim, w_dim=NET_COMMON["w_dim"], img_resolution=NET_COMMON["res"], img_channels=3,
                        mapping_kwargs=dnnlib.EasyDict(num_layers=NET_COMMON["mapping_layers"]),
                        synthesis_kwargs=dnnlib.EasyDict(channel_base=NET_COMMON["channel_base"], channel_max=NET_COMMON["channel_max"],
                                                         num_fp16_res=0, conv_clamp=NET_COMMON["conv_clamp"]))
    with torch.no_grad():
        for name, p in G.named_parameters():
            if name.endswith("noise_strength"):
                p.fill_(0.3)
            if name.endswith(".bias") and "affine" not in name and "mapping" not in name:
                p.copy_(torch.randn_like(p) * 0.1)
        G.mapping.w_avg.copy_(torch.randn_like(G.mapping.w_avg) * 0.5)
    return G.eval().requires_grad_(False)


def read_png(path):
    return np.array(PIL.Image.open(path)), PIL.Image.open(path).mode


def generate(G, seeds, truncation_psi, noise_mode, class_idx, device):
    """generate.py:105-121 -> (float images [N, C, H, W], uint8 [N, H, W, C])"""
    label = torch.zeros([1, G.c_dim], device=device)                                                    # :106
    if G.c_dim != 0:
        label[:, class_idx] = 1                                                                         # :110
    floats, bytes_ = [], []
    for seed in seeds:                                                                                  # :116
        z = torch.from_numpy(np.random.RandomState(seed).randn(1, G.z_dim)).to(device)                  # :118
        img = G(z, label, truncation_psi=truncation_psi, noise_mode=noise_mode)                         # :119
        floats.append(img)
        img = (img.permute(0, 2, 3, 1) * 127.5 + 128).clamp(0, 255).to(torch.uint8)                     # :120
        bytes_.append(img[0].cpu().numpy())
    return torch.cat(floats).numpy(), np.stack(bytes_)


def generate_projected(G, ws, noise_mode, device):
    """generate.py:94-99"""
    ws = torch.tensor(ws, device=device)                                                                # :94
    assert ws.shape[1:] == (G.num_ws, G.w_dim)                                                          # :95
    floats, bytes_ = [], []
    for idx, w in enumerate(ws):                                                                        # :96
        img = G.synthesis(w.unsqueeze(0), noise_mode=noise_mode)                                        # :97
        floats.append(img)
        img = (img.permute(0, 2, 3, 1) * 127.5 + 128).clamp(0, 255).to(torch.uint8)                     # :98
        bytes_.append(img[0].cpu().numpy())
    return torch.cat(floats).numpy(), np.stack(bytes_)


def style_mix(G, row_seeds, col_seeds, col_styles, truncation_psi, noise_mode, outdir, device):
    """style_mixing.py:69-110 -> (all_seeds, image_dict, float image dict, grid.png read back)"""
    all_seeds = list(set(row_seeds + col_seeds))                                                        # :70
    all_z = np.stack([np.random.RandomState(seed).randn(G.z_dim) for seed in all_seeds])                # :71
    all_w = G.mapping(torch.from_numpy(all_z).to(device), None)                                         # :72
    w_avg = G.mapping.w_avg                                                                             # :73
    all_w = w_avg + (all_w - w_avg) * truncation_psi                                                    # :74
    w_dict = {seed: w for seed, w in zip(all_seeds, list(all_w))}                                       # :75
    all_images = G.synthesis(all_w, noise_mode=noise_mode)                                              # :78
    float_dict = {(seed, seed): image.numpy() for seed, image in zip(all_seeds, list(all_images))}
    all_images = (all_images.permute(0, 2, 3, 1) * 127.5 + 128).clamp(0, 255).to(torch.uint8).cpu().numpy()     # :79
    image_dict = {(seed, seed): image for seed, image in zip(all_seeds, list(all_images))}             # :80
    for row_seed in row_seeds:                                                                          # :83
        for col_seed in col_seeds:
            w = w_dict[row_seed].clone()                                                                # :85
            w[col_styles] = w_dict[col_seed][col_styles]                                                # :86
            image = G.synthesis(w[np.newaxis], noise_mode=noise_mode)                                   # :87
            float_dict[(row_seed, col_seed)] = image[0].numpy()
            image = (image.permute(0, 2, 3, 1) * 127.5 + 128).clamp(0, 255).to(torch.uint8)             # :88
            image_dict[(row_seed, col_seed)] = image[0].cpu().numpy()                                   # :89
    for (row_seed, col_seed), image in image_dict.items():                                              # :93
        PIL.Image.fromarray(image, 'RGB').save(f'{outdir}/{row_seed}-{col_seed}.png')                   # :94
    W = G.img_resolution                                                                                # :97
    H = G.img_resolution
    canvas = PIL.Image.new('RGB', (W * (len(col_seeds) + 1), H * (len(row_seeds) + 1)), 'black')        # :99
    for row_idx, row_seed in enumerate([0] + row_seeds):                                                # :100
        for col_idx, col_seed in enumerate([0] + col_seeds):
            if row_idx == 0 and col_idx == 0:
                continue
            key = (row_seed, col_seed)
            if row_idx == 0:
                key = (col_seed, col_seed)
            if col_idx == 0:
                key = (row_seed, row_seed)
            canvas.paste(PIL.Image.fromarray(image_dict[key], 'RGB'), (W * col_idx, H * row_idx))       # :109
    canvas.save(f'{outdir}/grid.png')                                                                   # :110
    return all_seeds, image_dict, float_dict, read_png(f'{outdir}/grid.png')[0]


def main():
    _import_train_parts()           # the omegaconf stand-in: training_loop reaches train_parts through the metrics package
    sys.modules.setdefault("wandb", types.ModuleType("wandb"))
    from stylegan2ada.training import training_loop as R_loop

    arrays, meta = {}, dict(nets={}, gen=[], toy={})
    tmp = tempfile.mkdtemp()
    device = torch.device("cpu")

    # -- grids of real images: setup_snapshot_image_grid + save_image_grid(drange=[0, 255]) from the reference
    for name, kw in iu.TOY_SETS.items():
        ds = iu.ToyDataset(**kw)
        (gw, gh), images, labels = R_loop.setup_snapshot_image_grid(training_set=ds)
        R_loop.save_image_grid(images, os.path.join(tmp, f"{name}.png"), drange=[0, 255], grid_size=(gw, gh))
        png, mode = read_png(os.path.join(tmp, f"{name}.png"))
        arrays[f"toy/{name}/indices"] = np.asarray(ds.asked, dtype=np.int64)
        arrays[f"toy/{name}/labels"] = labels.astype(np.float32)
        arrays[f"toy/{name}/reals_png"] = png
        meta["toy"][name] = dict(grid_size=[int(gw), int(gh)], mode=mode)

    # -- save_image_grid on float images, drange [-1, 1]: random RGB and grey batches, and the tie vectors
    rng = np.random.RandomState(40)
    for name, shape, grid in [("rgb", (6, 3, 5, 8), (3, 2)), ("grey", (4, 1, 6, 7), (2, 2)), ("ties", None, (1, 1))]:
        x = iu.tie_vector() if shape is None else (rng.rand(*shape) * 2.4 - 1.2).astype(np.float32)
        R_loop.save_image_grid(x, os.path.join(tmp, f"f_{name}.png"), drange=[-1, 1], grid_size=grid)
        png, mode = read_png(os.path.join(tmp, f"f_{name}.png"))
        arrays[f"grid/{name}/x"] = x
        arrays[f"grid/{name}/png"] = png
        meta.setdefault("grid", {})[name] = dict(grid_size=list(grid), mode=mode)
    # the clamp rule (generate.py:120) on the same float batches
    for name in ("rgb", "grey", "ties"):
        img = torch.from_numpy(arrays[f"grid/{name}/x"])
        arrays[f"clamp/{name}"] = (img.permute(0, 2, 3, 1) * 127.5 + 128).clamp(0, 255).to(torch.uint8).numpy()

    # -- the generators
    nets = {}
    for tag, kw in NETS.items():
        nets[tag] = make_G(kw["seed"], kw["c_dim"])
        arrays.update({f"{tag}/G/{k}": npy(v) for k, v in nets[tag].state_dict().items()})
        meta["nets"][tag] = dict(NET_COMMON, c_dim=kw["c_dim"], num_ws=int(nets[tag].num_ws))
    for case in GEN_CASES:
        f, b = generate(nets[case["net"]], case["seeds"], case["psi"], "const", case["class_idx"], device)
        arrays[f"gen/{case['tag']}/float"], arrays[f"gen/{case['tag']}/uint8"] = f, b
        meta["gen"].append(case)
    G = nets["g16"]
    z = torch.from_numpy(np.random.RandomState(77).randn(2, G.z_dim))
    ws = (G.mapping(z, None) + 0.1 * torch.from_numpy(np.random.RandomState(78).randn(2, G.num_ws, G.w_dim)).float()).numpy()
    f, b = generate_projected(G, ws, "const", device)
    arrays["proj/ws"], arrays["proj/float"], arrays["proj/uint8"] = ws.astype(np.float32), f, b

    # -- the style matrix
    mixdir = os.path.join(tmp, "mix")
    os.makedirs(mixdir)
    all_seeds, image_dict, float_dict, grid = style_mix(nets[MIX["net"]], MIX["rows"], MIX["cols"], MIX["styles"], MIX["psi"], "const", mixdir, device)
    keys = list(image_dict.keys())
    arrays["mix/keys"] = np.asarray(keys, dtype=np.int64)
    arrays["mix/uint8"] = np.stack([image_dict[k] for k in keys])
    arrays["mix/float"] = np.stack([float_dict[k] for k in keys])
    arrays["mix/grid_png"] = grid
    meta["mix"] = dict(MIX, all_seeds=[int(s) for s in all_seeds], files=sorted(os.listdir(mixdir)))
    save("image_export", arrays, meta)


if __name__ == "__main__":
    main()
