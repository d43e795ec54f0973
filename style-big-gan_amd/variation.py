"""What does each input of a trained generator decide?  Per-pixel variance by generator input.

The measurements behind figures 4 and 5 of the StyleGAN paper, as numbers and maps: the per-pixel standard deviation over many noise
realisations of one latent, the same per noise layer, and the same over replaced coarse, middle and fine styles.  They show whether the noise
inputs are used at all (a fresh network has ``noise_strength = 0``, a collapsed one keeps it there), which layer draws texture and which
draws nothing, and whether "fine" styles leak into pose.  The reference has no such tool.  One arithmetic is stated once and both devices
follow it bit for bit (``torch_utils/ops/moments_u8.py``).

* Base latents: ``G.mapping(z, label, truncation_psi=--trunc)`` of every seed, one call per seed as ``generate.py`` makes it, or the rows of
  ``w`` in ``--projected-w`` as they are (then ``--trunc`` is ignored with a warning).
* Sources (``--vary``), one group of ``--draws`` images each per base latent:
  ``noise``         every noise layer gets a fresh realisation; the styles are fixed.
  ``noise-layers``  one group per noise layer (``noise:b4.conv1``, ``noise:b8.conv0``, ...): that layer gets fresh realisations, the others
                    keep ``noise_const``.
  ``styles``        one group per entry of ``--groups``: the ws indices of the group are replaced by those of ``--draws`` other latents, the
                    noise stays ``const``.  Default groups by resolution as in the paper: ``coarse`` up to 8 x 8, ``middle`` 16 x 16 and
                    32 x 32, ``fine`` from 64 x 64 (a group without layers at the network's resolution is left out); or ``a-b,c-d,...``,
                    each a range of ws indices.
* The draws are made on the host from ``RandomState(--seed)`` in a fixed order -- base latent, then source, then draw, then layer: a noise
  draw is ``randn(res, res)`` per layer of the source in synthesis order, a style draw is ``randn(z_dim)``, mapped with the label and psi of
  the base -- rounded once to fp32 and uploaded, so the draws follow from the options alone and are the same on both devices and for every
  ``--batch``; the files are the same wherever the generator's image of a latent does not depend on what else is in its batch.  Noise reaches
  the layers through ``tool_support.noise_inputs``.
* Images are synthesised ``--batch`` at a time, quantised with the ``clamp`` rule of ``generate.py`` and added to the running integer sums
  ``sum`` and ``sumsq`` of their group by ``moments_u8.accumulate``; they are never kept.  ``num = sum_c (n sumsq - sum^2)`` is an exact integer
  map (``moments_u8.numerator``); the per-pixel std in byte units is ``sqrt(num / (C n (n - 1)))``, float64 on the host.
* ``variation.npz``: ``num`` int64 [B, G, H, W], ``mean`` fp32 [B, G, C, H, W] (sum / n), ``base`` uint8 [B, H, W, C] (the unvaried images),
  ``dominant`` uint8 [B, H, W], ``sources``, ``layers`` (the noise layers), ``groups`` (``name=i,j,...``), ``draws``, ``seed``, ``seeds``,
  ``thresholds``, ``max_std``.
* ``variation.json`` (strict JSON): the options, ``max_std``, then per base latent and overall, per source: ``rms_std`` (byte units), ``p50``,
  ``p99`` and ``max`` of the per-pixel std, ``share`` (the source's part of the summed variance of its family: ``noise``, the noise layers,
  the style groups), ``dominant_fraction``; ``noise_additivity`` = the layers' summed variance over that of ``noise`` when both were asked for
  (far from 1: the layers interact); ``noise_unused``: true when every noise map is zero.
* ``variation.png``: one row per base latent: the unvaried image, one heat map per source (256 levels from 0 to ``--max-std``, default the
  largest per-pixel std of the run, written to the json so that two runs can share a scale) and the dominant-source map in a fixed palette
  (black: nothing varies).  The dominant source is taken among the noise layers and style groups; ``noise`` competes only when
  ``noise-layers`` was not asked for, since it is their total.

    python -m style_big_gan_amd.variation exp.config_dir=<dir> exp.config=<file.yaml> --snapshot=<network-snapshot-*.pt> --outdir=<dir> \\
        (--seeds=0-3 | --projected-w=<projected_w.npz>) [--vary=noise,noise-layers,styles] [--draws=100] [--seed=0] \\
        [--groups=coarse,middle,fine | a-b,c-d,...] [--trunc=1] [--class=<idx>] [--batch=32] [--max-std=<S>] [--device=auto|cuda|cpu]
"""
import argparse
import json
import os

import numpy as np
import torch

from .tool_support import (add_device_option, add_snapshot_option, class_label, config_overrides, device_of, load_generator, noise_inputs, noise_layers,
                           num_range, parse_layers, require_file, save_png, seed_latents, tool_device)
from .torch_utils.ops import image_export, moments_u8 as ops

SOURCES = ('noise', 'noise-layers', 'styles')
NAMED_GROUPS = ('coarse', 'middle', 'fine')
BLACK = (0, 0, 0)


def heat_table():
    """uint8 [256, 3]: black - red - yellow - white, every channel an integer ramp"""
    level = np.arange(256, dtype=np.int64)
    return np.stack([np.clip(level * 3, 0, 255), np.clip(level * 3 - 255, 0, 255), np.clip(level * 3 - 510, 0, 255)], axis=1).astype(np.uint8)


def source_palette(count):
    """uint8 [count, 3]: the fixed colours of the dominant-source map, source i of the competing ones gets colour i (a 12-colour cycle, dimmed
    on every further round)"""
    base = np.array([[230, 25, 75], [60, 180, 75], [0, 130, 200], [255, 225, 25], [245, 130, 48], [145, 30, 180], [70, 240, 240], [240, 50, 230],
                     [210, 245, 60], [0, 128, 128], [170, 110, 40], [128, 128, 128]], dtype=np.int64)
    return np.stack([base[i % 12] * (4 - min(i // 12, 3)) // 4 for i in range(count)]).astype(np.uint8) if count else np.zeros([0, 3], dtype=np.uint8)


def ws_resolutions(G):
    """-> the resolution of the block every ws index feeds (the last block's ToRGB index belongs to the last block)"""
    out = []
    for res in G.synthesis.block_resolutions:
        out += [int(res)] * int(getattr(G.synthesis, f'b{res}').num_conv)
    last = G.synthesis.block_resolutions[-1]
    out += [int(last)] * int(getattr(G.synthesis, f'b{last}').num_torgb)
    return out


def parse_groups(text, G):
    """--groups -> [(name, sorted ws indices)]: 'coarse,middle,fine' (any subset; a named group the network has no layers for is left out) or
    'a-b,c-d,...' ranges of ws indices"""
    num_ws = int(G.mapping.num_ws)
    items = [t for t in str(text if text is not None else ','.join(NAMED_GROUPS)).split(',') if t]
    if not items:
        raise ValueError(f'--groups={text}: names a group ({", ".join(NAMED_GROUPS)}) or ranges a-b of ws indices')
    res = ws_resolutions(G)
    if len(res) != num_ws:
        raise ValueError(f'the synthesis network reads {len(res)} ws indices, the mapping network makes {num_ws}')
    groups = []
    for item in items:
        if item in NAMED_GROUPS:
            lo, hi = dict(coarse=(0, 8), middle=(16, 32), fine=(64, 1 << 30))[item]
            idx = [i for i, r in enumerate(res) if lo <= r <= hi]
            if idx:
                groups.append((item, idx))
        else:
            try:
                groups.append((item, parse_layers(item, num_ws)))
            except (ValueError, AttributeError):
                raise ValueError(f'--groups={text}: {item} is neither one of {", ".join(NAMED_GROUPS)} nor a range a-b of the ws indices 0 to {num_ws - 1}')
    if not groups:
        raise ValueError(f'--groups={text}: no group has a layer in this generator')
    if len({name for name, _ in groups}) != len(groups):
        raise ValueError(f'--groups={text}: a group is named twice')
    return groups


def draw_noise(rng, layers, count):
    """`count` draws for the noise layers `layers` [(name, res)] from `rng`, draw by draw and layer by layer -> {name: fp32 [count, 1, res, res]}"""
    out = {name: np.empty([count, 1, res, res], dtype=np.float32) for name, res in layers}
    for d in range(count):
        for name, res in layers:
            out[name][d, 0] = rng.randn(res, res)
    return {name: torch.from_numpy(v) for name, v in out.items()}


def plan_sources(G, vary, groups):
    """-> [(source name, family, noise layers that get draws, ws indices that are replaced)] in the order of SOURCES"""
    layers = noise_layers(G)
    vary = [v for v in SOURCES if v in set(vary)]
    if not vary:
        raise ValueError(f'--vary: at least one of {", ".join(SOURCES)}')
    if ('noise' in vary or 'noise-layers' in vary) and not layers:
        raise ValueError('--vary=noise: the generator has no layer with a noise input')
    plan = []
    if 'noise' in vary:
        plan.append(('noise', 'noise', layers, []))
    if 'noise-layers' in vary:
        plan += [(f'noise:{name}', 'noise-layers', [(name, res)], []) for name, res in layers]
    if 'styles' in vary:
        plan += [(f'styles:{name}', 'styles', [], idx) for name, idx in parse_groups(groups, G)]
    if len(plan) > ops.MAX_RENDER_G:
        raise ValueError(f'--vary: {len(plan)} sources, at most {ops.MAX_RENDER_G} can be rendered')
    return plan


def _base_latents(G, seeds, projected_w, label, truncation_psi, device):
    num_ws, w_dim = int(G.mapping.num_ws), int(G.w_dim)
    if projected_w is not None:
        if isinstance(projected_w, (str, os.PathLike)):
            projected_w = np.load(projected_w)['w']
        ws = torch.as_tensor(projected_w).to(device).to(torch.float32).contiguous()
        if ws.ndim != 3 or tuple(ws.shape[1:]) != (num_ws, w_dim) or ws.shape[0] < 1:
            raise ValueError(f'--projected-w: w of shape {tuple(ws.shape)} does not belong to a generator with {num_ws} x {w_dim} latents')
        if truncation_psi != 1:
            print('warn: --trunc is ignored when using --projected-w')
        return ws
    z = seed_latents(G, seeds)
    return torch.cat([G.mapping(torch.from_numpy(z[i:i + 1]).to(device), label, truncation_psi=truncation_psi) for i in range(len(seeds))]).to(torch.float32)


def _bytes(G, ws, noise):
    """the images of `ws` with the noise layers in `noise` fed from it and the others constant -> uint8 [N, H, W, C]"""
    with noise_inputs(G, noise):
        img = G.synthesis(ws, noise_mode='const')
    return image_export.quantize(img.to(torch.float32), 'clamp')


def _source_stats(std):
    """float64 per-pixel std of any shape -> the figures of one source"""
    flat = std.reshape(-1)
    return dict(rms_std=float(np.sqrt((flat * flat).mean())), p50=float(np.percentile(flat, 50)), p99=float(np.percentile(flat, 99)), max=float(flat.max()))


def _stats(num, dominant, plan, compete, C, draws):
    """num int64 [B, G, H, W], dominant uint8 [B, H, W] (index into `compete`) -> (per base list, overall dict) of variation.json"""
    std = ops.pixel_std(num, C, draws)
    S = len(plan)
    names, families = [p[0] for p in plan], [p[1] for p in plan]

    def block(std_s, dom):
        """std_s float64 [G, pixels], dom uint8 [pixels]"""
        total = (std_s * std_s).sum(axis=1)                                 # summed variance per source
        family_total = {f: sum(total[i] for i in range(S) if families[i] == f) for f in set(families)}
        sources = {}
        for i, name in enumerate(names):
            stats = _source_stats(std_s[i])
            stats['share'] = float(total[i] / family_total[families[i]]) if family_total[families[i]] > 0 else None
            stats['dominant_fraction'] = float((dom == compete.index(i)).mean()) if i in compete else None
            sources[name] = stats
        out = dict(sources=sources, noise_additivity=None, noise_unused=None)
        noise_rows = [i for i in range(S) if families[i] in ('noise', 'noise-layers')]
        if noise_rows:
            out['noise_unused'] = bool(all(total[i] == 0 for i in noise_rows))
        if 'noise' in families and 'noise-layers' in families and family_total['noise'] > 0:
            out['noise_additivity'] = float(family_total['noise-layers'] / family_total['noise'])
        return out

    per_base = [block(std[b].reshape(S, -1), dominant[b].reshape(-1)) for b in range(num.shape[0])]
    return per_base, block(np.moveaxis(std, 1, 0).reshape(S, -1), dominant.reshape(-1))


@torch.no_grad()
def measure_variation(G, seeds=None, projected_w=None, vary=SOURCES, draws=100, seed=0, groups=None, truncation_psi=1, class_idx=None, batch=32,
                      max_std=None, device=None, on_images=None):
    """Everything but the files -> dict with `arrays` (what variation.npz holds), `stats` (what variation.json holds without the options) and
    `sheet` (uint8 [B H, (G + 2) W, 3], what variation.png holds).  `on_images(base, source name, first draw, uint8 [n, H, W, C])` sees every
    batch of a group before it is dropped."""
    if not (hasattr(G, 'mapping') and hasattr(G, 'synthesis')):
        raise ValueError('the variation tool needs a generator with mapping and synthesis networks (DCGAN and BigGAN generators have no per-layer inputs)')
    device = device_of(G, device)
    draws, batch, seed = int(draws), int(batch), int(seed)
    if draws < 2:
        raise ValueError(f'--draws={draws}: a variance needs at least 2')
    if batch < 1:
        raise ValueError(f'--batch={batch}: must be at least 1')
    if (seeds is None) == (projected_w is None):
        raise ValueError('exactly one of --seeds and --projected-w is needed')
    if max_std is not None and not float(max_std) > 0:
        raise ValueError(f'--max-std={max_std}: must be positive')
    vary = [v for v in (vary.split(',') if isinstance(vary, str) else vary) if v]
    if any(v not in SOURCES for v in vary):
        raise ValueError(f'--vary={",".join(vary)}: a list of {", ".join(SOURCES)}')
    plan = plan_sources(G, vary, groups)
    seeds = None if seeds is None else [int(s) for s in seeds]
    if seeds is not None and not seeds:
        raise ValueError('--seeds: at least one seed is needed')
    label = class_label(G, class_idx, device)
    base_ws = _base_latents(G, seeds, projected_w, label, truncation_psi, device)
    psi = 1 if projected_w is not None else truncation_psi          # the replacement latents of projected rows are not truncated either
    B, S = int(base_ws.shape[0]), len(plan)
    C, H, W = int(G.img_channels), int(G.img_resolution), int(G.img_resolution)
    if C not in (1, 3):
        raise ValueError(f'the variation tool writes images of 1 or 3 channels, the generator has {C}')
    P, F = H * W, H * W * C
    if draws > ops.numerator_max_n(C):
        raise ValueError(f'--draws={draws}: above {ops.numerator_max_n(C)}, the largest count the exact numerator holds for {C} channels')

    rng = np.random.RandomState(seed)
    num = np.empty([B, S, H, W], dtype=np.int64)
    mean = np.empty([B, S, C, H, W], dtype=np.float32)
    base_images = np.empty([B, H, W, C], dtype=np.uint8)
    sums_d, nums_d = [], []
    for b in range(B):
        w0 = base_ws[b:b + 1]
        base_images[b] = _bytes(G, w0, {})[0].cpu().numpy()
        sums = torch.zeros([2, S, F], dtype=torch.int64, device=device)         # the bytes' own order: (pixel, channel)
        for s, (name, family, layers, replaced) in enumerate(plan):
            for lo in range(0, draws, batch):
                n = min(batch, draws - lo)
                ws = w0.repeat(n, 1, 1)
                if replaced:
                    z = rng.randn(n, G.z_dim)
                    other = torch.cat([G.mapping(torch.from_numpy(z[i:i + 1]).to(device), label, truncation_psi=psi) for i in range(n)]).to(torch.float32)
                    ws[:, replaced] = other[:, replaced]
                noise = {k: v.to(device) for k, v in draw_noise(rng, layers, n).items()}
                images = _bytes(G, ws, noise)
                if on_images is not None:
                    on_images(b, name, lo, images)
                ops.accumulate(images.reshape(1, n, F), sums[0, s:s + 1], sums[1, s:s + 1])
        # (pixel, channel) -> (channel, pixel): the small sums are transposed once, the images never
        planar = sums.reshape(2, S, P, C).permute(0, 1, 3, 2).contiguous()
        num_d = ops.numerator(planar[0], planar[1], draws)
        nums_d.append(num_d)
        num[b] = num_d.cpu().numpy().reshape(S, H, W)
        mean[b] = (planar[0].cpu().numpy().astype(np.float64) / np.float64(draws)).astype(np.float32).reshape(S, C, H, W)

    # the scale, the heat maps and the dominant source
    compete = [i for i, p in enumerate(plan) if not (p[1] == 'noise' and 'noise-layers' in vary)]
    std_max = float(ops.pixel_std(num, C, draws).max())
    scale = float(max_std) if max_std is not None else std_max
    thresholds = ops.std_thresholds(scale, C, draws)
    table, palette = heat_table(), source_palette(len(compete))
    dominant = np.empty([B, H, W], dtype=np.uint8)
    cols = S + 2
    sheet = torch.zeros([B * H, cols * W, 3], dtype=torch.uint8, device=device)
    for b in range(B):
        heat, dom = ops.render(nums_d[b], thresholds, table)
        if len(compete) != S:
            _, dom = ops.render(nums_d[b][compete].contiguous(), thresholds, table)
        dominant[b] = dom.cpu().numpy().reshape(H, W)
        colours = np.concatenate([palette, np.tile(np.asarray(BLACK, dtype=np.uint8), [256 - len(palette), 1])])[dominant[b]]     # [H, W, 3]
        first = torch.from_numpy(base_images[b]).to(device).permute(2, 0, 1).expand(3, H, W)
        last = torch.from_numpy(colours).to(device).permute(2, 0, 1)
        cells = torch.cat([first[None], heat.reshape(S, 3, H, W), last[None]]).to(torch.float32).contiguous()
        image_export.tile(cells, (cols, B), 'grid', drange=(0, 255), canvas=sheet, cell0=b * cols)

    per_base, overall = _stats(num, dominant, plan, compete, C, draws)
    names = [p[0] for p in plan]
    group_text = [f'{p[0].split(":", 1)[1]}={",".join(str(i) for i in p[3])}' for p in plan if p[1] == 'styles']
    arrays = dict(num=num, mean=mean, base=base_images, dominant=dominant, sources=np.array(names), layers=np.array([n for n, _ in noise_layers(G)]),
                  groups=np.array(group_text), draws=np.int64(draws), seed=np.int64(seed),
                  seeds=np.asarray(seeds if seeds is not None else [], dtype=np.int64), thresholds=thresholds, max_std=np.float64(scale))
    stats = dict(sources=names, competing=[names[i] for i in compete], max_std=scale, largest_std=std_max, bases=per_base, overall=overall)
    return dict(arrays=arrays, stats=stats, sheet=sheet.cpu().numpy())


def variation(G, outdir, **options):
    """`measure_variation` and the files of the module docstring -> its dict, with `stats` as variation.json holds it"""
    result = measure_variation(G, **options)
    shown = {k: v for k, v in options.items() if k not in ('device', 'projected_w', 'on_images', 'vary', 'batch')}     # what decides the numbers
    vary = options.get('vary', SOURCES)
    shown.update(projected_w=options.get('projected_w') is not None, vary=[v for v in SOURCES if v in (vary.split(',') if isinstance(vary, str) else vary)])
    result['stats'] = dict(options=shown, **result['stats'])
    os.makedirs(outdir, exist_ok=True)
    save_png(result['sheet'], os.path.join(outdir, 'variation.png'))
    np.savez(os.path.join(outdir, 'variation.npz'), **result['arrays'])
    with open(os.path.join(outdir, 'variation.json'), 'w') as f:
        json.dump(result['stats'], f, indent=2, allow_nan=False)
    return result


# ---------------------------------------------------------------------------------------------------------------- CLI

def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.variation', description=__doc__.split('\n')[0])
    add_snapshot_option(ap)
    ap.add_argument('--outdir', required=True, help='where to save variation.png, variation.npz and variation.json')
    ap.add_argument('--seeds', type=num_range, help='the base latents: list of random seeds')
    ap.add_argument('--projected-w', help='the base latents are the rows of w in this projected_w.npz of the projector (no truncation)')
    ap.add_argument('--vary', default=','.join(SOURCES), help=f'what is varied: a list of {", ".join(SOURCES)} (default: all)')
    ap.add_argument('--draws', type=int, default=100, help='images per source and base latent (default: 100)')
    ap.add_argument('--seed', type=int, default=0, help='seed of the noise realisations and replacement latents (default: 0)')
    ap.add_argument('--groups', help='style groups: coarse,middle,fine (by resolution, default) or ranges of ws indices a-b,c-d,...')
    ap.add_argument('--trunc', dest='truncation_psi', type=float, default=1, help='truncation psi (default: 1)')
    ap.add_argument('--class', dest='class_idx', type=int, help='class label (unconditional if not specified)')
    ap.add_argument('--batch', type=int, default=32, help='images synthesised at a time (default: 32)')
    ap.add_argument('--max-std', type=float, help='the std, in byte units, of the top of the heat-map scale (default: the largest of the run)')
    add_device_option(ap)
    args, rest = ap.parse_known_args(argv)
    if (args.seeds is None) == (args.projected_w is None):
        ap.error('exactly one of --seeds and --projected-w is needed')
    if any(v not in SOURCES for v in args.vary.split(',')):
        ap.error(f'--vary={args.vary}: a list of {", ".join(SOURCES)}')
    if args.draws < 2:
        ap.error(f'--draws={args.draws}: a variance needs at least 2')
    if args.batch < 1:
        ap.error(f'--batch={args.batch}: must be at least 1')
    if args.max_std is not None and not args.max_std > 0:
        ap.error(f'--max-std={args.max_std}: must be positive')
    require_file(ap, '--snapshot', args.snapshot)
    require_file(ap, '--projected-w', args.projected_w)
    return config_overrides(ap, rest), args


def run_variation(argv=None):
    overrides, args = parse_args(argv)
    from . import arguments
    config = arguments.load_config(overrides)
    device = tool_device(args.device)
    G = load_generator(config, args.snapshot, device)
    result = variation(G, args.outdir, seeds=args.seeds, projected_w=args.projected_w, vary=args.vary, draws=args.draws, seed=args.seed, groups=args.groups,
                       truncation_psi=args.truncation_psi, class_idx=args.class_idx, batch=args.batch, max_std=args.max_std, device=device)
    print(json.dumps(result['stats'], allow_nan=False))
    return result


if __name__ == '__main__':
    run_variation()
