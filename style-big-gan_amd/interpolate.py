"""Latent walks of a trained generator: what lies between two images, and is the way there smooth?

The other snapshot tools judge or edit single latents; this one moves through a list of key latents and writes the frames as an animation, the
cheapest visual check of what the ``ppl_*`` metrics measure: jumps, stuck textures and dead regions show within seconds.  The reference has no
such tool.  One arithmetic is stated once and both devices follow it bit for bit (``torch_utils/ops/walk.py``).

* Keys and grid.  ``--grid=GWxGH`` plays ``cells = GW GH`` walks side by side; the number of ``--seeds`` (or of rows of ``w`` in ``--projected-w``)
  must be ``cells K`` with ``K >= 2`` keys per walk; key k of cell c is entry ``k cells + c``.
* ``--space=w`` (default): the keys are ``G.mapping(z, label, truncation_psi=--trunc)`` of each seed, or the projected rows as they are (then
  ``--trunc`` is ignored with a warning).  The table of all frames of all cells is one ``blend_table`` launch: four taps per frame, the fp32 chain
  ``acc = w0 k0; acc = fmaf(wj, kj, acc)``.  ``--layers`` restricts the walk to those ws indices; the others hold the cell's key 0 (coarse-only or
  fine-only walks).
* ``--space=z``: the keys are the seed latents as fp32; the table is blended the same way and every frame goes through ``G.mapping`` with ``--trunc``.
  ``--layers``, ``--classes`` and ``--projected-w`` are refused there.
* ``--method``: ``linear``; ``cubic`` (default in W), the uniform Catmull-Rom spline through the keys, on an open walk with the missing neighbour
  reflected -- local and C1, not the global C2 spline of other video scripts, because four taps per frame is what makes the table one gather
  kernel; ``slerp`` (default and only in Z), ``sin((1 - tau) w) / sin w`` and ``sin(tau w) / sin w`` with ``w`` the angle between the normalised
  keys of the segment, computed in float64 on the host, the linear weights when ``sin w < 1e-6``.  All weights are float64 rounded once to fp32.
  With ``n = --frames-per-key`` an open walk has ``(K - 1) n + 1`` frames, ``--loop`` closes it and has ``K n``.  A frame on a key is the key's image.
* ``--classes=i,j,...`` gives one class per key (conditional networks only; same count and order as the seeds), ``--class`` one for all.
* Frames are synthesised ``--batch`` table rows at a time, quantised with the ``clamp`` rule and tiled into the frame canvases on the device; the
  squared difference of every cell's consecutive frames is ``pair_sqdiff`` (exact integers); canvases reach the host through two pinned buffers
  without a synchronisation per frame; the animation is encoded on the host afterwards.  Pillow needs the frames as a list, so a walk whose
  frames exceed 2 GiB is refused.
* ``walk.<apng|gif|webp>`` (``--format``; ``none`` writes no animation): ``--fps`` frames a second, endless; APNG and lossless WebP hold the frames'
  bytes exactly (identical consecutive frames merged into one of a longer duration), GIF is palette-quantised.
* ``walk.png``: a contact sheet, rows cells, columns ``--strip`` frames evenly spaced, first and last included.  ``frames/frame%05d.png`` with
  ``--save-frames``.
* ``walk.npz``: ``keys`` (row ``c K + k``), ``index`` and ``weight`` (row ``t cells + c``, the cell's offset ``c K`` included), ``hold``, ``segment``,
  ``tau``, ``omega`` (empty unless slerp), ``seeds``, ``classes``, ``layers``, ``grid``, ``space``, ``method``, ``d2`` (int64 [cells, steps]).  The table is
  ``blend_table(keys, index, weight, layers, hold)`` bit for bit on the CPU path, so it is not stored.
* ``walk.json`` (strict JSON): the options, ``frames``, ``steps``; per cell and overall ``rmse_mean``, ``rmse_median``, ``rmse_max``, ``argmax_frame``
  (the frame the largest step starts from) and ``jerk = rmse_max / rmse_median`` (``null`` when the median is 0) of ``rmse = sqrt(d2 / (C H W))``:
  a walk with one step far above the others has a discontinuity there.

    python -m style_big_gan_amd.interpolate exp.config_dir=<dir> exp.config=<file.yaml> --snapshot=<network-snapshot-*.pt> --outdir=<dir> \\
        (--seeds=a,b,c | a-c  |  --projected-w=<projected_w.npz>) [--grid=1x1] [--space=w|z] [--method=cubic|linear|slerp] [--frames-per-key=30] \\
        [--loop] [--layers=all|a-b|a,b,c] [--classes=i,j,...] [--trunc=1] [--class=<idx>] [--noise-mode=const|random|none] \\
        [--format=apng|gif|webp|none] [--fps=30] [--strip=8] [--save-frames] [--batch=16] [--device=auto|cuda|cpu]
"""
import argparse
import json
import os
import re

import numpy as np
import torch

from .tool_support import (ANIMATION_FORMATS, add_device_option, add_sampling_options, add_snapshot_option, class_label, config_overrides, device_of,
                           load_generator, num_range, parse_layers, require_file, save_animation, save_png, seed_latents, tool_device)
from .torch_utils.ops import image_export, walk as ops

SPACES = ('w', 'z')
FORMATS = tuple(ANIMATION_FORMATS) + ('none',)
MAX_FRAME_BYTES = 2 << 30


def parse_grid(text):
    """'GWxGH' -> (gw, gh), both at least 1"""
    m = re.match(r'^(\d+)x(\d+)$', str(text))
    if not m or int(m.group(1)) < 1 or int(m.group(2)) < 1:
        raise ValueError(f'--grid={text}: expects GWxGH with both at least 1, as in 2x1')
    return int(m.group(1)), int(m.group(2))


def segment_angles(z, cells, K, loop):
    """float64 seed latents [cells K, z_dim] in key order (row c K + k) -> float64 [cells, segments]: the angle between the normalised keys of
    every segment (segment s joins the keys s and s + 1, mod K on a loop)"""
    unit = z / np.sqrt((z * z).sum(axis=1, keepdims=True))
    unit = unit.reshape(cells, K, -1)
    nxt = np.roll(unit, -1, axis=1) if loop else unit[:, 1:]
    cur = unit if loop else unit[:, :-1]
    return np.arccos(np.clip((cur * nxt).sum(axis=2), -1.0, 1.0))


def walk_stats(d2, pixels):
    """int64 [cells, steps] -> (the per cell list, the overall dict) of walk.json"""
    rmse = np.sqrt(d2.astype(np.float64) / np.float64(pixels))

    def one(r, argmax):
        median = float(np.median(r))
        return dict(rmse_mean=float(r.mean()), rmse_median=median, rmse_max=float(r.max()), argmax_frame=int(argmax),
                    jerk=float(r.max()) / median if median > 0 else None)
    return [one(r, np.argmax(r)) for r in rmse], one(rmse.reshape(-1), np.argmax(rmse.max(axis=0)))


def strip_frames(T, strip):
    """the `strip` frames of the contact sheet: evenly spaced, first and last included, capped at T"""
    strip = min(int(strip), T)
    return [0] if strip == 1 else [(j * (T - 1) + (strip - 1) // 2) // (strip - 1) for j in range(strip)]


def contact_sheet(frames, grid, picks):
    """uint8 [T, GH H, GW W, C] -> uint8 [cells H, len(picks) W, C]: row c, column j is cell c of frame picks[j]"""
    gw, gh = grid
    H, W = frames.shape[1] // gh, frames.shape[2] // gw
    sheet = np.empty([gw * gh * H, len(picks) * W, frames.shape[3]], dtype=np.uint8)
    for c in range(gw * gh):
        gy, gx = divmod(c, gw)
        for j, t in enumerate(picks):
            sheet[c * H:(c + 1) * H, j * W:(j + 1) * W] = frames[t, gy * H:(gy + 1) * H, gx * W:(gx + 1) * W]
    return sheet


def _walk_keys(G, seeds, projected_w, classes, class_idx, space, truncation_psi, device):
    """-> (entries fp32 [n, L, D] on `device` in the order given, float64 seed latents or None, label of every entry [n, c_dim])"""
    num_ws, w_dim = int(G.mapping.num_ws), int(G.w_dim)
    if projected_w is not None:
        if isinstance(projected_w, (str, os.PathLike)):
            projected_w = np.load(projected_w)['w']
        entries = torch.as_tensor(projected_w).to(device).to(torch.float32).contiguous()
        if entries.ndim != 3 or tuple(entries.shape[1:]) != (num_ws, w_dim):
            raise ValueError(f'--projected-w: w of shape {tuple(entries.shape)} does not belong to a generator with {num_ws} x {w_dim} latents')
        if truncation_psi != 1:
            print('warn: --trunc is ignored when using --projected-w')
        return entries, None, None
    n = len(seeds)
    if classes is not None:
        if G.c_dim == 0:
            raise ValueError('--classes: one class per key is for conditional networks only')
        if len(classes) != n or any(not 0 <= int(c) < G.c_dim for c in classes):
            raise ValueError(f'--classes: expects one class in [0, {G.c_dim}) per seed, {n} of them in the seeds\' order, got {list(classes)}')
        labels = torch.zeros([n, G.c_dim], device=device)
        labels[torch.arange(n), torch.as_tensor([int(c) for c in classes])] = 1
    else:
        labels = class_label(G, class_idx, device).expand(n, -1)
    z = seed_latents(G, seeds)
    if space == 'z':
        return torch.from_numpy(z.astype(np.float32)).to(device)[:, None].contiguous(), z, labels
    rows = [G.mapping(torch.from_numpy(z[i:i + 1]).to(device), labels[i:i + 1], truncation_psi=truncation_psi) for i in range(n)]
    return torch.cat(rows).to(torch.float32).contiguous(), z, labels


class _HostFrames:
    """canvases -> the host array, through at most two pinned buffers in flight on a device (a plain copy on the host)"""

    def __init__(self, frames, slots, device):
        self.frames, self.cuda, self.turn = frames, device.type == 'cuda', 0
        if self.cuda:
            self.pinned = [torch.empty([slots] + list(frames.shape[1:]), dtype=torch.uint8).pin_memory() for _ in range(2)]
            self.pending = [None, None]

    def _land(self, i):
        if self.pending[i] is not None:
            event, first, count = self.pending[i]
            event.synchronize()
            self.frames[first:first + count] = self.pinned[i][:count].numpy()
            self.pending[i] = None

    def put(self, canvases, first):
        count = canvases.shape[0]
        if count == 0:
            return
        if not self.cuda:
            self.frames[first:first + count] = canvases.numpy()
            return
        i, self.turn = self.turn, self.turn ^ 1
        self._land(i)                                   # the copy issued two batches ago
        self.pinned[i][:count].copy_(canvases, non_blocking=True)
        event = torch.cuda.Event()
        event.record()
        self.pending[i] = (event, first, count)

    def finish(self):
        if self.cuda:
            self._land(self.turn)
            self._land(self.turn ^ 1)


@torch.no_grad()
def render_walk(G, seeds=None, projected_w=None, grid=(1, 1), space='w', method=None, frames_per_key=30, loop=False, layers=None, classes=None,
                truncation_psi=1, class_idx=None, noise_mode='const', batch=16, device=None):
    """Everything but the files -> dict with `frames` (uint8 [T, GH H, GW W, C] on the host), `d2` (int64 [cells, steps]), `arrays` (what walk.npz
    holds) and `stats` (what walk.json holds without the options)."""
    if not (hasattr(G, 'mapping') and hasattr(G, 'synthesis')):
        raise ValueError('the interpolate tool needs a generator with mapping and synthesis networks')
    device = device_of(G, device)
    gw, gh = parse_grid(grid) if isinstance(grid, str) else (int(grid[0]), int(grid[1]))
    cells, batch, n_key, loop = gw * gh, int(batch), int(frames_per_key), bool(loop)
    if cells < 1:
        raise ValueError(f'--grid={gw}x{gh}: both must be at least 1')
    if batch < 1:
        raise ValueError(f'--batch={batch}: must be at least 1')
    if n_key < 1:
        raise ValueError(f'--frames-per-key={n_key}: must be at least 1')
    if space not in SPACES:
        raise ValueError(f'--space={space}: one of {", ".join(SPACES)}')
    if (seeds is None) == (projected_w is None):
        raise ValueError('exactly one of --seeds and --projected-w is needed')
    method = method if method is not None else 'cubic' if space == 'w' else 'slerp'
    if method not in ops.METHODS:
        raise ValueError(f'--method={method}: one of {", ".join(ops.METHODS)}')
    if method == 'slerp' and space == 'w':
        raise ValueError('--method=slerp is for --space=z only (W is not a sphere)')
    if space == 'z':
        for flag, given in (('--projected-w', projected_w is not None), ('--layers', layers not in (None, 'all')), ('--classes', classes is not None)):
            if given:
                raise ValueError(f'{flag} is refused with --space=z')
    num_ws = int(G.mapping.num_ws)
    layer_list = [0]                                    # the one layer of a Z table
    if space == 'w':
        layer_list = sorted({int(i) for i in layers}) if isinstance(layers, (list, tuple)) else parse_layers(layers, num_ws)
        if not layer_list or layer_list[0] < 0 or layer_list[-1] >= num_ws:
            raise ValueError(f'--layers={layers}: the generator has the ws indices 0 to {num_ws - 1}')
    seeds = None if seeds is None else [int(s) for s in seeds]
    entries, z, labels = _walk_keys(G, seeds, projected_w, classes, class_idx, space, truncation_psi, device)
    count = entries.shape[0]
    K = count // cells
    if K < 2 or K * cells != count:
        raise ValueError(f'{"--seeds" if seeds is not None else "--projected-w"}: {count} keys do not deal into --grid={gw}x{gh}: it needs '
                         f'cells x K = {cells} x K of them with K >= 2')
    # key k of cell c is entry k cells + c; the key table holds it in row c K + k
    order = torch.arange(count).reshape(K, cells).t().reshape(-1)
    keys = entries[order.to(device)].contiguous()
    omega = segment_angles(z[order.numpy()], cells, K, loop) if method == 'slerp' else np.zeros([0], dtype=np.float64)

    walks = [ops.walk_weights(method, K, n_key, loop, omega[c] if method == 'slerp' else None) for c in range(cells if method == 'slerp' else 1)]
    _, _, segment, tau = walks[0]
    T = len(tau)
    index = np.stack([walks[c % len(walks)][0] + np.int32(c * K) for c in range(cells)], axis=1).reshape(T * cells, 4)
    weight = np.ascontiguousarray(np.stack([walks[c % len(walks)][1] for c in range(cells)], axis=1).reshape(T * cells, 4))
    hold = np.tile(np.arange(cells, dtype=np.int32) * np.int32(K), T)
    partial = len(layer_list) < keys.shape[1]

    C, H, W = int(G.img_channels), int(G.img_resolution), int(G.img_resolution)
    canvas_bytes = gh * H * gw * W * C
    if T * canvas_bytes > MAX_FRAME_BYTES:
        raise ValueError(f'--frames-per-key={n_key}: {T} frames of {canvas_bytes} bytes are {T * canvas_bytes} bytes, above the {MAX_FRAME_BYTES} the '
                         'encoder can hold as a list; fewer frames, a smaller --grid, or several walks')

    table = ops.blend_table(keys, torch.from_numpy(index).to(device), torch.from_numpy(weight).to(device), layer_list if partial else None,
                            torch.from_numpy(hold).to(device) if partial else None)

    frames = np.empty([T, gh * H, gw * W, C], dtype=np.uint8)
    slots = batch // cells + 2                          # frames a batch of rows can touch
    canvases = torch.zeros([slots, gh * H, gw * W, C], dtype=torch.uint8, device=device)
    host = _HostFrames(frames, slots, device)
    rows, carry, first_rows, d2 = T * cells, None, [], []
    for lo in range(0, rows, batch):
        hi = min(lo + batch, rows)
        latents = table[lo:hi]
        if space == 'z':
            latents = G.mapping(latents[:, 0], labels[:1].expand(hi - lo, -1), truncation_psi=truncation_psi)
        img = G.synthesis(latents, noise_mode=noise_mode).to(torch.float32)
        # the bytes of every (frame, cell) row, for the differences of consecutive frames; the last frame's rows are carried on the device
        q = image_export.quantize(img, 'clamp').reshape(hi - lo, -1)
        if lo < cells:
            first_rows.append(q[:cells - lo])
        x = q if carry is None else torch.cat([carry, q])
        if x.shape[0] > cells:
            d2.append(ops.pair_sqdiff(x[:-cells], x[cells:]))
        carry = x[-cells:]
        # the canvases: slot j holds frame f0 + j; a frame the previous batch left unfinished waits in slot 0
        f0, done = lo // cells, hi // cells
        for f in range(f0, (hi - 1) // cells + 1):
            r0, r1 = max(lo, f * cells), min(hi, (f + 1) * cells)
            image_export.tile(img[r0 - lo:r1 - lo], (gw, gh), 'clamp', canvas=canvases[f - f0], cell0=r0 - f * cells)
        host.put(canvases[:done - f0], f0)
        if hi % cells != 0 and done > f0:
            canvases[0].copy_(canvases[done - f0])
    if loop:
        d2.append(ops.pair_sqdiff(carry, torch.cat(first_rows)))
    host.finish()
    steps = T if loop else T - 1
    d2 = torch.cat(d2).reshape(steps, cells).t().contiguous().cpu().numpy() if steps else np.zeros([cells, 0], dtype=np.int64)

    arrays = dict(keys=keys.cpu().numpy(), index=index, weight=weight, hold=hold, segment=segment, tau=tau, omega=omega,
                  seeds=np.asarray(seeds if seeds is not None else [], dtype=np.int64),
                  classes=np.asarray([int(c) for c in classes] if classes is not None else [], dtype=np.int64),
                  layers=np.asarray(layer_list, dtype=np.int64), grid=np.asarray([gw, gh], dtype=np.int64), space=np.array(space),
                  method=np.array(method), d2=d2)
    per_cell, overall = walk_stats(d2, C * H * W) if steps else ([], None)
    stats = dict(frames=T, steps=steps, keys_per_cell=K, cells=per_cell, overall=overall)
    return dict(frames=frames, d2=d2, arrays=arrays, stats=stats)


def table_from_arrays(arrays):
    """the latent table of a walk.npz, on the CPU path: fp32 [T cells, L, D]"""
    keys = torch.from_numpy(np.ascontiguousarray(arrays['keys']))
    layers = [int(i) for i in arrays['layers']]
    partial = str(arrays['space']) == 'w' and len(layers) < keys.shape[1]
    return ops.blend_table(keys, torch.from_numpy(np.ascontiguousarray(arrays['index'])), torch.from_numpy(np.ascontiguousarray(arrays['weight'])),
                           layers if partial else None, torch.from_numpy(np.ascontiguousarray(arrays['hold'])) if partial else None)


def interpolate(G, outdir, fmt='apng', fps=30, strip=8, save_frames=False, **options):
    """`render_walk` and the files of the module docstring -> its dict, with `stats` as walk.json holds it"""
    if fmt not in FORMATS:
        raise ValueError(f'--format={fmt}: one of {", ".join(FORMATS)}')
    if not float(fps) > 0:
        raise ValueError(f'--fps={fps}: must be positive')
    if int(strip) < 1:
        raise ValueError(f'--strip={strip}: must be at least 1')
    result = render_walk(G, **options)
    frames, arrays = result['frames'], result['arrays']
    shown = {k: v for k, v in options.items() if k not in ('device', 'projected_w')}
    shown.update(projected_w=options.get('projected_w') is not None, format=fmt, fps=float(fps), strip=int(strip), save_frames=bool(save_frames),
                 space=str(arrays['space']), method=str(arrays['method']), layers=[int(i) for i in arrays['layers']],
                 grid=[int(i) for i in arrays['grid']])
    result['stats'] = dict(options=shown, **result['stats'])
    os.makedirs(outdir, exist_ok=True)
    if fmt != 'none':
        save_animation(frames, os.path.join(outdir, f'walk.{fmt}'), fmt, fps)
    result['sheet'] = contact_sheet(frames, tuple(int(i) for i in arrays['grid']), strip_frames(frames.shape[0], strip))
    save_png(result['sheet'], os.path.join(outdir, 'walk.png'))
    if save_frames:
        os.makedirs(os.path.join(outdir, 'frames'), exist_ok=True)
        for t, frame in enumerate(frames):
            save_png(frame, os.path.join(outdir, 'frames', f'frame{t:05d}.png'))
    np.savez(os.path.join(outdir, 'walk.npz'), **arrays)
    with open(os.path.join(outdir, 'walk.json'), 'w') as f:
        json.dump(result['stats'], f, indent=2, allow_nan=False)
    return result


# ---------------------------------------------------------------------------------------------------------------- CLI

def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.interpolate', description=__doc__.split('\n')[0])
    add_snapshot_option(ap)
    ap.add_argument('--outdir', required=True, help='where to save walk.<format>, walk.png, walk.npz and walk.json')
    ap.add_argument('--seeds', type=num_range, help='the keys: cells x K seeds, key k of cell c is entry k * cells + c')
    ap.add_argument('--projected-w', help='the keys are the rows of w in this projected_w.npz of the projector (no truncation)')
    ap.add_argument('--grid', default='1x1', help='GWxGH walks side by side (default: 1x1)')
    ap.add_argument('--space', choices=SPACES, default='w', help='where the walk is blended (default: w)')
    ap.add_argument('--method', choices=('cubic', 'linear', 'slerp'), help='cubic: Catmull-Rom through the keys; linear; slerp: --space=z only '
                    '(default: cubic in w, slerp in z)')
    ap.add_argument('--frames-per-key', type=int, default=30, help='frames from one key to the next (default: 30)')
    ap.add_argument('--loop', action='store_true', help='close the walk: the last key leads back to the first')
    ap.add_argument('--layers', help='ws indices that walk, the others hold key 0: all | a-b | a,b,c (default: all)')
    ap.add_argument('--classes', type=num_range, help='one class per key, in the seeds\' order (conditional networks)')
    add_sampling_options(ap)
    ap.add_argument('--format', dest='fmt', choices=FORMATS, default='apng', help='the animation written; none: no animation (default: apng)')
    ap.add_argument('--fps', type=float, default=30, help='frames per second of the animation (default: 30)')
    ap.add_argument('--strip', type=int, default=8, help='frames of the contact sheet walk.png, evenly spaced (default: 8)')
    ap.add_argument('--save-frames', action='store_true', help='also write frames/frame%%05d.png')
    ap.add_argument('--batch', type=int, default=16, help='table rows synthesised at a time (default: 16)')
    add_device_option(ap)
    args, rest = ap.parse_known_args(argv)
    if (args.seeds is None) == (args.projected_w is None):
        ap.error('exactly one of --seeds and --projected-w is needed')
    try:
        parse_grid(args.grid)
    except ValueError as e:
        ap.error(str(e))
    method = args.method or ('cubic' if args.space == 'w' else 'slerp')
    if method == 'slerp' and args.space == 'w':
        ap.error('--method=slerp is for --space=z only (W is not a sphere)')
    if args.space == 'z':
        for flag, given in (('--projected-w', args.projected_w is not None), ('--layers', args.layers not in (None, 'all')), ('--classes', args.classes is not None)):
            if given:
                ap.error(f'{flag} is refused with --space=z')
    if args.classes is not None and args.class_idx is not None:
        ap.error('--classes and --class exclude one another')
    for flag, value in (('--frames-per-key', args.frames_per_key), ('--strip', args.strip), ('--batch', args.batch)):
        if value < 1:
            ap.error(f'{flag}={value}: must be at least 1')
    if not args.fps > 0:
        ap.error(f'--fps={args.fps}: must be positive')
    require_file(ap, '--snapshot', args.snapshot)
    require_file(ap, '--projected-w', args.projected_w)
    return config_overrides(ap, rest), args


def run_interpolate(argv=None):
    overrides, args = parse_args(argv)
    from . import arguments
    config = arguments.load_config(overrides)
    device = tool_device(args.device)
    G = load_generator(config, args.snapshot, device)
    result = interpolate(G, args.outdir, fmt=args.fmt, fps=args.fps, strip=args.strip, save_frames=args.save_frames, seeds=args.seeds,
                         projected_w=args.projected_w, grid=args.grid, space=args.space, method=args.method, frames_per_key=args.frames_per_key,
                         loop=args.loop, layers=args.layers, classes=args.classes, truncation_psi=args.truncation_psi, class_idx=args.class_idx,
                         noise_mode=args.noise_mode, batch=args.batch, device=device)
    print(json.dumps(result['stats'], allow_nan=False))
    return result


if __name__ == '__main__':
    run_interpolate()
