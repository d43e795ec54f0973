"""What the thirteen snapshot tools (the eleven up to the walk tool: generate, style_mixing, projector, calc_metrics, nearest_neighbors, avg_spectra, diversity,
realism, directions, modes, interpolate; then variation and network_summary) share,
each piece once: a generator built from the run's config and a ``network-snapshot-*.pt`` of this build (written by ``BaseTrainer.save_snapshot``), the
discriminator of the same file (network_summary is the one tool that loads it), the
``key=value`` config overrides ``starter`` takes, the options several tools declare alike, the device and the data set of a run, the class label, the
seeded latents, the ws indices of ``--layers``, the noise layers of a synthesis network and the context that hands them noise realisations, the bytes of
generated images, the box reduction behind ``--res``, the ``vgg16.pt`` features of a data set and
the two image writers (one frame, many frames).  What a tool validates
and the options whose help differs per tool stay in the tool."""
import contextlib
import os
import re

import numpy as np
import torch

from .torch_utils.ops import image_export, resample_u8

NOISE_MODES = ('const', 'random', 'none')
STORE_CHUNK_BYTES = 256 << 20           # full-size store bytes reduced (--res) or searched as queries (nearest_neighbors' baseline) at a time
SNAPSHOT_HELP = 'network-snapshot-*.pt of this build (G_ema, or G when there is no EMA)'


def num_range(s):
    """a comma separated list of numbers 'a,b,c' or a range 'a-c' -> list of ints (the reference's option type, generate.py :25-33)"""
    m = re.match(r'^(\d+)-(\d+)$', s)
    return list(range(int(m.group(1)), int(m.group(2)) + 1)) if m else [int(x) for x in s.split(',')]


def parse_layers(text, num_ws):
    """'all' | 'a-b' | 'a,b,c' -> sorted ws indices, all below `num_ws`"""
    layers = list(range(num_ws)) if text in (None, 'all') else sorted(set(num_range(text)))
    if not layers or layers[-1] >= num_ws:
        raise ValueError(f'--layers={text}: the generator has the ws indices 0 to {num_ws - 1}')
    return layers


def add_snapshot_option(ap, required=True, help=SNAPSHOT_HELP):
    ap.add_argument('--snapshot', required=required, help=help)


def add_sampling_options(ap, class_idx=True):
    """--trunc, --class (unless `class_idx` is off) and --noise-mode, in this order"""
    ap.add_argument('--trunc', dest='truncation_psi', type=float, default=1, help='truncation psi (default: 1)')
    if class_idx:
        ap.add_argument('--class', dest='class_idx', type=int, help='class label (unconditional if not specified)')
    ap.add_argument('--noise-mode', choices=NOISE_MODES, default='const', help='noise mode (default: const)')


def add_device_option(ap):
    ap.add_argument('--device', choices=('auto', 'cuda', 'cpu'), default='auto', help='where to run (default: auto)')


def require_file(ap, flag, path):
    """an option that was given must name a file"""
    if path is not None and not os.path.isfile(path):
        ap.error(f'{flag}={path}: no such file')


def config_overrides(parser, rest):
    """the arguments an argparse parser did not recognise must all be `key=value` config overrides -> the list, or the parser's error"""
    bad = [r for r in rest if '=' not in r or r.startswith('-')]
    if bad:
        parser.error(f'unrecognised arguments: {" ".join(bad)}')
    return rest


def resolve_device(name):
    return name if name != 'auto' else 'cuda' if torch.cuda.is_available() else 'cpu'


def tool_device(name):
    """'auto' | 'cuda' | 'cpu' -> the torch.device a one-process tool runs on"""
    return torch.device('cuda', torch.cuda.current_device()) if resolve_device(name) == 'cuda' else torch.device('cpu')


def device_of(G, device):
    """the given device, or the generator's"""
    return torch.device(device) if device is not None else next(iter(G.buffers())).device


def generator_common_kwargs(state):
    """c_dim, img_resolution and img_channels of a generator, read from its state dict (the CLI has no data set to ask)"""
    res = [int(m.group(1)) for k in state for m in [re.match(r'synthesis\.b(\d+)\.', k)] if m]
    if not res:
        raise RuntimeError('the snapshot holds no mapping/synthesis generator')
    img_resolution = max(res)
    torgb = state.get(f'synthesis.b{img_resolution}.torgb.weight')
    embed = state.get('mapping.embed.weight')
    return dict(c_dim=int(embed.shape[1]) if embed is not None else 0, img_resolution=img_resolution,
                img_channels=int(torgb.shape[0]) if torgb is not None else 3)


def dcgan_common_kwargs(state):
    """the same three numbers for the state dict of a DCGAN generator (`main.*` layers: a first transposed convolution [z_dim, 1024, M, M],
    four stride-2 ones, the last to the image channels): no labels, resolution 16 M"""
    first = state['main.0.weight']
    last = [v for k, v in state.items() if re.match(r'main\.\d+\.weight$', k) and v.ndim == 4][-1]
    return dict(c_dim=0, img_resolution=16 * int(first.shape[2]), img_channels=int(last.shape[1]))


def build_generator(config, state, device):
    """G through the `generators` registry with the config's gens_args, weights from `state` (strict)"""
    from .train_parts.generators import generators
    from .train_parts.trainers import BaseTrainer
    name = config.gen.generator
    dcgan = 'main.0.weight' in state and not any(k.startswith('synthesis.') for k in state)
    kw = BaseTrainer._model_kwargs(config.gens_args[name], dcgan_common_kwargs(state) if dcgan else generator_common_kwargs(state))
    G = generators[name](**kw)
    G.load_state_dict(state, strict=True)
    return G.eval().requires_grad_(False).to(device)


def snapshot_generator_state(path):
    """G_ema of a network-snapshot-*.pt, or G when the run kept no average"""
    snap = torch.load(path, map_location='cpu', weights_only=True)
    key = 'G_ema' if snap.get('G_ema') is not None else 'G'
    if key not in snap:
        raise RuntimeError(f'{path} holds neither G_ema nor G')
    return snap[key]


def load_generator(config, snapshot, device, announce=True):
    """G of the snapshot file on `device`; `build_generator` is looked up when called, so a stand-in set on this module is used"""
    if announce:
        print(f'Loading networks from "{snapshot}"...')
    return build_generator(config, snapshot_generator_state(snapshot), device)


def snapshot_discriminator_state(path):
    """D of a network-snapshot-*.pt; a snapshot written without it (a tool's own, or one stripped for release) is refused by name"""
    snap = torch.load(path, map_location='cpu', weights_only=True)
    if snap.get('D') is None:
        raise RuntimeError(f'{path} holds no discriminator (no "D" entry; it holds {", ".join(sorted(snap)) or "nothing"}): '
                           'only a snapshot written by a training run can be summarised with --networks=D')
    return snap['D']


def build_discriminator(config, state, G, device):
    """D through the `discriminators` registry with the config's discs_args; c_dim, img_resolution and img_channels are the generator's;
    weights from `state` (strict); eval mode, no gradients"""
    from .train_parts.discriminators import discriminators
    from .train_parts.trainers import BaseTrainer
    name = config.gen.discriminator
    common = dict(c_dim=int(getattr(G, 'c_dim', 0) or 0), img_resolution=int(G.img_resolution), img_channels=int(getattr(G, 'img_channels', 3)))
    D = discriminators[name](**BaseTrainer._model_kwargs(config.discs_args[name], common))
    D.load_state_dict(state, strict=True)
    return D.eval().requires_grad_(False).to(device)


def load_discriminator(config, snapshot, G, device):
    """D of the snapshot file on `device`, shaped after `G`; `build_discriminator` is looked up when called, so a stand-in set on this module is used"""
    return build_discriminator(config, snapshot_discriminator_state(snapshot), G, device)


def dataset_kwargs_for(config, G, data=None, mirror=None):
    """the data set kwargs of the run, with the tool's overrides: --data the path, --mirror the flips; the labels follow the network"""
    from .train_parts.trainers import training_set_kwargs_from_config
    return training_set_kwargs_from_config(config, seed=config.gen.seed, path=data, mirror=mirror, use_labels=G.c_dim != 0)


@contextlib.contextmanager
def open_dataset(config, kwargs):
    """the run's data set built from `kwargs`, closed on exit"""
    from .train_parts.datasets import datasets
    print('Dataset options:', kwargs)
    dataset = datasets[config.data.dataset](**kwargs)
    try:
        yield dataset
    finally:
        dataset.close()


def detector_kwargs(detector):
    """a callable or a TorchScript file -> MetricOptions(detector=...), a directory -> MetricOptions(detector_dir=...)"""
    if callable(detector) or isinstance(detector, dict) or (isinstance(detector, str) and os.path.isfile(detector)):
        return dict(detector=detector, detector_dir=None)
    if isinstance(detector, str) and os.path.isdir(detector):
        return dict(detector=None, detector_dir=detector)
    raise ValueError(f'--detector={detector}: no such TorchScript file or directory (detectors are not downloaded in this build)')


def vgg16_feature_options(detector, dataset_kwargs, device, cache_dir=None):
    """MetricOptions for the `vgg16.pt` features of a data set and of images (nearest_neighbors --space=vgg16, realism).  A directory is
    resolved to the file here: the process-wide detector cache and the feature cache key on what they are given, and the bare name
    `vgg16.pt` would stand for whichever directory was loaded first.  Features are cached only when the detector is a file."""
    from .metrics import metric_utils, scores
    if isinstance(detector, str) and os.path.isdir(detector):
        if not os.path.isfile(os.path.join(detector, scores.VGG16)):
            raise ValueError(f'--detector={detector}: the directory does not hold {scores.VGG16}')
        detector = os.path.join(detector, scores.VGG16)
    opts = metric_utils.MetricOptions(dataset_kwargs=dataset_kwargs, device=device, cache_dir=cache_dir, **detector_kwargs(detector))
    opts.cache = not callable(metric_utils.detector_source(opts, scores.VGG16))
    return opts


def checked_features(features, what, option='--space=vgg16'):
    """float features [N, F] -> fp16 on their device, finite and of a width the kernel takes"""
    features = features.to(torch.float16)
    if features.ndim != 2 or features.shape[1] % 8 != 0:
        raise ValueError(f'{option}: the detector returns features of shape {list(features.shape[1:])} for {what}; the search needs a vector per '
                         'image whose width is a multiple of 8')
    if not bool(torch.isfinite(features).all()):
        raise ValueError(f'{option}: the features of {what} are not all finite in fp16')
    return features.contiguous()


def dataset_features(opts, dataset, dataset_name, option='--space=vgg16'):
    """the detector's feature of every item of `dataset`, in item order -> float32 tensor [len(dataset), F] on the host"""
    from .metrics import metric_utils, scores
    kw = metric_utils.detector_call_kwargs(opts, scores.VGG16, dict(return_features=True))
    stats = metric_utils.compute_feature_stats_for_dataset(opts, scores.VGG16, kw, dataset_name=dataset_name, capture_all=True)
    if opts.cache and stats.num_items != len(dataset):      # a stale cache file (its name does not key on the row count): not used
        opts.cache = False
        stats = metric_utils.compute_feature_stats_for_dataset(opts, scores.VGG16, kw, dataset_name=dataset_name, capture_all=True)
    if stats.num_items != len(dataset):
        raise ValueError(f'{option}: dataset_kwargs describe a data set of {stats.num_items} items, the data set searched holds {len(dataset)}')
    return stats.get_all_torch()


def class_label(G, class_idx, device):
    """-> one-hot [1, c_dim] on `device`; a conditional network needs a class, an unconditional one ignores it with a warning"""
    label = torch.zeros([1, G.c_dim], device=device)
    if G.c_dim != 0:
        if class_idx is None:
            raise ValueError('Must specify class label with --class when using a conditional network')
        label[:, class_idx] = 1
    elif class_idx is not None:
        print('warn: --class=lbl ignored when running on an unconditional network')
    return label


def seed_latents(G, seeds):
    """-> float64 [len(seeds), z_dim], every row from a generator of its own seed (the reference's `randn(1, z_dim)` draws the same numbers)"""
    return np.stack([np.random.RandomState(seed).randn(G.z_dim) for seed in seeds])


def noise_layers(G):
    """-> [(layer name, resolution)] of the synthesis layers with `use_noise`, in synthesis order ('b4.conv1', 'b8.conv0', ...); a generator
    without a synthesis network of such layers (DCGAN, BigGAN) is refused"""
    synthesis = getattr(G, 'synthesis', None)
    if synthesis is None or not hasattr(synthesis, 'block_resolutions'):
        raise ValueError('the generator has no synthesis network with per-layer noise inputs (a mapping/synthesis generator is needed)')
    found = []
    for res in synthesis.block_resolutions:
        block = getattr(synthesis, f'b{res}')
        for name in ('conv0', 'conv1'):
            layer = getattr(block, name, None)
            if layer is not None and getattr(layer, 'use_noise', False):
                found.append((f'b{res}.{name}', int(layer.resolution)))
    return found


@contextlib.contextmanager
def noise_inputs(G, inputs):
    """while the context is open the named noise layers (`noise_layers`) use the given realisation, fp32 [N, 1, res, res], instead of drawing one
    (noise mode 'random') or reading `noise_const` ('const'); every layer is cleared on exit, an exception included"""
    known = dict(noise_layers(G))
    layers = {}
    for name, noise in inputs.items():
        if name not in known:
            raise ValueError(f'noise_inputs: {name} is not a noise layer of the generator (it has {", ".join(known)})')
        if noise.dtype != torch.float32 or noise.ndim != 4 or tuple(noise.shape[1:]) != (1, known[name], known[name]):
            raise ValueError(f'noise_inputs: {name} expects fp32 [N, 1, {known[name]}, {known[name]}], got {noise.dtype} {tuple(noise.shape)}')
        block, layer = name.split('.')
        layers[name] = getattr(getattr(G.synthesis, block), layer)
    try:
        for name, layer in layers.items():
            layer.noise_input = inputs[name]
        yield
    finally:
        for layer in layers.values():
            layer.noise_input = None


def to_uint8(img):
    """synthesis output [N, C, H, W] -> uint8 [N, H, W, C] on the host (the reference's generate.py :98, :120)"""
    return image_export.quantize(img.to(torch.float32), 'clamp').cpu().numpy()


def generated_images(G, seeds, label, truncation_psi, noise_mode, device):
    """the images of `seeds` in one batch, as the bytes generate.py writes -> uint8 [N, C, H, W] on `device`"""
    z = torch.from_numpy(seed_latents(G, seeds)).to(device)
    img = G(z, label.expand(len(seeds), -1), truncation_psi=truncation_psi, noise_mode=noise_mode)
    return image_export.quantize(img.to(torch.float32), 'clamp').permute(0, 3, 1, 2).contiguous()


def check_res(res, resolution):
    """--res: a power of two in [4, the data resolution]; None keeps the full size"""
    if res is None:
        return None
    res = int(res)
    if res < 4 or res & (res - 1) or res > resolution:
        raise ValueError(f'--res={res}: must be a power of two, at least 4 and at most the data resolution {resolution}')
    return None if res == resolution else res


def reduce_images(images, res):
    """uint8 [N, C, H, W] -> its box-reduced copy [N, C, res, res] (the exact uint8 box filter of resample_u8)"""
    if res is None:
        return images
    out = resample_u8.resize(images.permute(0, 2, 3, 1).contiguous(), res, res, 'box')
    return out.permute(0, 3, 1, 2).contiguous()


def reduce_store(store, res):
    """the whole store reduced once, in chunks of at most STORE_CHUNK_BYTES"""
    if res is None:
        return store
    rows = max(1, STORE_CHUNK_BYTES // max(store[0].numel(), 1))
    return torch.cat([reduce_images(store[lo:lo + rows], res) for lo in range(0, store.shape[0], rows)])


def save_png(img, path):
    """uint8 [H, W, C] -> PNG: mode 'L' for one channel, 'RGB' for three (the way the reference's tools write every image)"""
    import PIL.Image
    img = np.ascontiguousarray(img)
    assert img.ndim == 3 and img.shape[2] in [1, 3]
    (PIL.Image.fromarray(img[:, :, 0], 'L') if img.shape[2] == 1 else PIL.Image.fromarray(img, 'RGB')).save(path)


ANIMATION_FORMATS = {'apng': 'PNG', 'gif': 'GIF', 'webp': 'WEBP'}


def save_animation(frames, path, fmt, fps):
    """uint8 [T, H, W, C] -> an animated PNG ('apng'), GIF ('gif') or lossless WebP ('webp') that plays `fps` frames a second for ever; mode 'L'
    for one channel, 'RGB' for three.  Pillow gets the frames as a list (from a generator its PNG writer keeps the first frame alone); its writers
    merge identical consecutive frames into one of a longer duration, and a file whose frames are all equal holds one still image: a reader
    expands every frame by duration / (1000 / fps) and a still image to the number of frames it expects."""
    import PIL.Image
    frames = np.ascontiguousarray(frames)
    assert frames.ndim == 4 and frames.shape[0] >= 1 and frames.shape[3] in [1, 3] and frames.dtype == np.uint8
    if fmt not in ANIMATION_FORMATS:
        raise ValueError(f'--format={fmt}: one of {", ".join(ANIMATION_FORMATS)}')
    if not float(fps) > 0:
        raise ValueError(f'--fps={fps}: must be positive')
    images = [PIL.Image.fromarray(f[:, :, 0], 'L') if f.shape[2] == 1 else PIL.Image.fromarray(f, 'RGB') for f in frames]
    more = dict(lossless=True) if fmt == 'webp' else {}
    images[0].save(path, format=ANIMATION_FORMATS[fmt], save_all=True, append_images=images[1:], duration=1000 / float(fps), loop=0, **more)
