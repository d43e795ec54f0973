"""What is inside a snapshot, layer by layer?  The reference's module table for G and D, with activation statistics.

The reference prints a per-layer table of G and D before it trains (``misc.print_module_summary``: parameters, buffers, output shape,
datatype).  This tool prints the same table for the networks of a snapshot and appends what the table cannot show: the numerics of every
layer's output over a set of samples -- which layers sit at the clamp, which would overflow or go subnormal in fp16, which channels are dead,
where a NaN first appears.  The run log reports the health of the gradients; this reports the activations.  The measurements are exact: one
arithmetic is stated once and both devices follow it bit for bit, whatever ``--batch`` (``torch_utils/ops/act_stats.py``).

* Networks (``--networks``, default ``G,D``): ``G`` is ``G_ema`` of the snapshot (``G`` when the run kept no average), ``D`` its
  discriminator (``tool_support.load_discriminator``; a snapshot without ``D`` is refused by name).
* Inputs: G gets the latents ``generate.py`` makes for ``--seeds`` (one ``RandomState`` per seed), with ``--trunc``, ``--class`` and
  ``--noise-mode``.  D gets the generator's float images -- entry set ``D(fake)`` -- and, with ``--data``, the items ``0 .. len(seeds) - 1`` of
  the data set, flips off, normalised as the trainer normalises (``x / 127.5 - 1``) with their labels: entry set ``D(real)``.
* Per network the table of ``print_module_summary`` is printed once for a batch of ``--batch`` (``--max-nesting`` as there).  Then the samples
  run ``--batch`` at a time with forward hooks on the same entries: every floating-point output of rank 2 or 4 goes through ``act_stats.planes``
  the moment its module returns it -- the tensor itself, in its own dtype and memory layout, no ``.float()`` and no ``.contiguous()`` copy -- and
  ``act_stats.fold`` adds the records to the entry's running per-channel records in sample order.  The files do not depend on ``--batch``
  wherever a sample's activations do not depend on what else is in its batch: this package's device kernels keep that; torch's CPU layers
  (the DCGAN networks) do not, so on the CPU the statistics pass forwards one sample at a time.
* The tensors are the ones this build's modules return.  With the inference fusions on, a layer may hand a pre-modulated tensor to its reader
  (``SynthesisBlock``'s conv0 applies conv1's style modulation in its tail); ``SBG_PREMODULATE=0`` restores the reference's tensors.
* Columns appended to the table (``act_stats.derive``, float64 on the host): ``rms``; ``absmax``; ``fp16 bits`` = log2(65504 / absmax), the
  headroom to fp16's largest value (negative: it overflows); ``zero %``; ``peak %`` = the share of elements ON the largest magnitude (a clamped
  layer shows here, whatever clamp and gain produced the value); ``nonfinite`` (count); ``dead ch`` = channels whose every element was zero.
* ``summary.txt``: the printed tables.  ``summary.json`` (strict JSON): the options and, per network and entry, name, parameters, buffers,
  shape, dtype, memory format and the derived numbers (with the fp16 overflow / subnormal shares, by binade), and ``first_nonfinite``: the first
  entry in execution order with a NaN or an infinity.  ``summary.npz``: per entry the running ``counts`` [C, 70] and ``values`` [C, 4], so
  everything can be derived again.  ``exponents.png``: one row per entry, the 64 binades 2^-32 .. 2^31 as columns, grey by share, red marks at
  fp16's limits (2^-14, below which fp16 is subnormal, and 2^16, where it overflows).
* Two precisions are compared with the ordinary overrides, e.g. ``gens_args.sg2_classic.synthesis_kwargs.num_fp16_res=4``.

    python -m style_big_gan_amd.network_summary exp.config_dir=<dir> exp.config=<file.yaml> --snapshot=<network-snapshot-*.pt> --outdir=<dir> \\
        [--networks=G,D] [--seeds=0-63] [--data=<folder|zip>] [--max-nesting=3] [--trunc=1] [--class=<idx>] [--noise-mode=const|random|none] \\
        [--batch=16] [--device=auto|cuda|cpu]
"""
import argparse
import contextlib
import io
import json
import os

import numpy as np
import torch

from .tool_support import (add_device_option, add_sampling_options, add_snapshot_option, class_label, config_overrides, dataset_kwargs_for, load_discriminator,
                           load_generator, num_range, open_dataset, require_file, save_png, seed_latents, tool_device)
from .torch_utils import misc
from .torch_utils.ops import act_stats

NETWORKS = ('G', 'D')
NUMERIC_COLUMNS = ('rms', 'absmax', 'fp16 bits', 'zero %', 'peak %', 'nonfinite', 'dead ch')
CELL = 6                                        # pixels per binade and per entry in exponents.png


def memory_format(t):
    if t.is_contiguous():
        return 'contiguous'
    if t.ndim == 4 and t.is_contiguous(memory_format=torch.channels_last):
        return 'channels_last'
    return 'strided'


def measured(t):
    """the outputs that get statistics: floating point, rank 2 or 4, not empty"""
    return t.dtype in (torch.float16, torch.bfloat16, torch.float32) and t.ndim in (2, 4) and t.numel() > 0


class EntrySet:
    """the entries of one network under one kind of input (`G`, `D(fake)`, `D(real)`): the table's entries and, per measured output, the running
    records.  `table(inputs)` runs the table pass, `measure(inputs)` one batch of the statistics pass."""

    def __init__(self, key, net, max_nesting, on_output=None):
        self.key, self.net, self.max_nesting, self.on_output = key, net, max_nesting, on_output
        self.entries = None                     # all entries of the table pass, the redundant ones included: index = order of return
        self.running = {}                       # (entry index, output index) -> (counts [C, 70], values [C, 4])
        self.samples = 0

    def table(self, inputs):
        self.entries, outputs = misc.module_summary(self.net, inputs, max_nesting=self.max_nesting, skip_redundant=False)
        for e in self.entries:
            e.shapes = [tuple(t.shape) for t in e.outputs]
            e.dtypes = [str(t.dtype).split('.')[-1] for t in e.outputs]
            e.formats = [memory_format(t) for t in e.outputs]
            e.outputs = [torch.empty(t.shape, dtype=t.dtype, device='meta') for t in e.outputs]       # what the table needs of them; the activations go
            e.new_outputs = e.new_outputs and [None] * len(e.new_outputs)
        return outputs

    @property
    def kept(self):
        return [(i, e) for i, e in enumerate(self.entries) if not e.redundant]

    def measure(self, inputs):
        wanted = {i for i, _ in self.kept}

        def visit(index, entry):
            if index >= len(self.entries) or entry.module is not self.entries[index].module:
                raise RuntimeError(f'{self.key}: the forward pass took another path than the table pass (call {index}: {entry.name})')
            if index not in wanted:
                return
            for j, t in enumerate(entry.outputs):
                if not measured(t):
                    continue
                if self.on_output is not None:
                    self.on_output(self.key, entry.labels()[j], t)
                counts, values = act_stats.planes(t)
                if (index, j) not in self.running:
                    self.running[index, j] = act_stats.empty(t.shape[1], t.device)
                act_stats.fold(counts, values, *self.running[index, j])

        _, outputs = misc.module_summary(self.net, inputs, max_nesting=self.max_nesting, skip_redundant=False, visit=visit)
        self.samples += int(inputs[0].shape[0])
        return outputs

    def rows(self):
        """-> (cells of the table with the numerics columns appended, one dict per row for summary.json, {npz key: array})"""
        kept = [e for _, e in self.kept]
        cells = misc.summary_rows(self.net, kept)
        cells[0] = cells[0] + list(NUMERIC_COLUMNS)
        report, arrays, at = [], {}, 2
        for i, e in self.kept:
            labels = e.labels()
            for j in range(max(len(e.outputs), 1)):
                row = dict(name=labels[j] if e.outputs else e.name, parameters=e.params if j == 0 else 0, buffers=e.buffers if j == 0 else 0,
                           shape=list(e.shapes[j]) if e.outputs else None, dtype=e.dtypes[j] if e.outputs else None,
                           memory_format=e.formats[j] if e.outputs else None, stats=None)
                numbers = ['-'] * len(NUMERIC_COLUMNS)
                if (i, j) in self.running:
                    counts, values = (t.cpu().numpy() for t in self.running[i, j])
                    d = act_stats.derive(counts, values)
                    d.pop('channels')
                    row['stats'] = d
                    arrays[f'{self.key}.{len(report):03d}.{row["name"]}.counts'] = counts
                    arrays[f'{self.key}.{len(report):03d}.{row["name"]}.values'] = values
                    fmt = lambda v, spec: '-' if v is None else format(v, spec)
                    numbers = [fmt(d['rms'], '.4g'), fmt(d['absmax'], '.4g'), fmt(d['fp16_headroom_bits'], '.1f'),
                               fmt(None if d['zero_share'] is None else 100 * d['zero_share'], '.2f'),
                               fmt(None if d['peak_share'] is None else 100 * d['peak_share'], '.2f'), str(d['nonfinite']), str(len(d['dead_channels']))]
                cells[at] = cells[at] + numbers
                at += 1
                report.append(row)
        cells[1] = cells[1] + ['---'] * len(NUMERIC_COLUMNS)
        cells[at] = cells[at] + ['---'] * len(NUMERIC_COLUMNS)
        cells[at + 1] = cells[at + 1] + ['-'] * len(NUMERIC_COLUMNS)
        return cells, report, arrays


def exponent_image(reports):
    """[(key, rows)] -> uint8 [rows * CELL, 64 * CELL, 3]: per measured row the share of the finite non-zero elements per binade, white (none) to
    black (all) on a square-root scale; red lines left of binade -14 (fp16's smallest normal) and of binade 16 (fp16 overflows)"""
    hists = [np.asarray(r['stats']['hist'], dtype=np.float64) for _, rows in reports for r in rows if r['stats'] is not None]
    img = np.full([max(len(hists), 1) * CELL, act_stats.BINS * CELL, 3], 255, dtype=np.uint8)
    for y, h in enumerate(hists):
        share = h / h.sum() if h.sum() > 0 else h
        grey = np.rint(255 * (1 - np.sqrt(share))).astype(np.uint8)
        img[y * CELL:(y + 1) * CELL] = np.repeat(grey, CELL)[None, :, None]
    for b in (act_stats.FP16_SUBNORMAL_BIN, act_stats.FP16_OVERFLOW_BIN):
        img[:, b * CELL] = (255, 0, 0)
    return img


def _generator_images(G, z, label, truncation_psi, noise_mode):
    """the inputs of one generator batch, as generate.py hands them over"""
    c = label.expand(z.shape[0], -1)
    if hasattr(G, 'mapping') and hasattr(G, 'synthesis'):
        return [z, c], dict(truncation_psi=truncation_psi, noise_mode=noise_mode)
    return [z.to(torch.float32), c], {}             # the DCGAN and BigGAN generators take (z, c) alone


def _bound(net, kwargs):
    """while open, `net(*inputs)` passes `kwargs` on as well: `module_summary` hands positional inputs over alone"""
    if not kwargs:
        return contextlib.nullcontext()

    @contextlib.contextmanager
    def bind():
        forward = net.forward
        net.forward = lambda *a: forward(*a, **kwargs)
        try:
            yield
        finally:
            del net.forward
    return bind()


@torch.no_grad()
def measure_networks(G, D=None, networks=NETWORKS, seeds=range(64), dataset=None, max_nesting=3, truncation_psi=1, class_idx=None, noise_mode='const',
                     batch=16, device=None, on_output=None):
    """Everything but the files -> dict with `text` (summary.txt), `report` (summary.json without the options), `arrays` (summary.npz) and
    `image` (exponents.png).  `dataset`, when given, supplies the real images of `D(real)`.  `on_output(entry set, row name, tensor)` sees
    every tensor just before it is measured."""
    networks = [n for n in NETWORKS if n in set(networks)]
    seeds = [int(s) for s in seeds]
    batch = int(batch)
    if not networks:
        raise ValueError(f'--networks: at least one of {", ".join(NETWORKS)}')
    if not seeds:
        raise ValueError('--seeds: at least one seed is needed')
    if batch < 1:
        raise ValueError(f'--batch={batch}: must be at least 1')
    if 'D' in networks and D is None:
        raise ValueError('--networks=D: no discriminator was loaded')
    if dataset is not None and len(dataset) < len(seeds):
        raise ValueError(f'--data: the data set holds {len(dataset)} items, {len(seeds)} are needed (one per seed)')
    device = torch.device(device) if device is not None else next(iter(G.parameters())).device
    label = class_label(G, class_idx, device)
    z_all = torch.from_numpy(seed_latents(G, seeds)).to(device)
    sets = {}
    if 'G' in networks:
        sets['G'] = EntrySet('G', G, max_nesting, on_output)
    if 'D' in networks:
        sets['D(fake)'] = EntrySet('D(fake)', D, max_nesting, on_output)
        if dataset is not None:
            sets['D(real)'] = EntrySet('D(real)', D, max_nesting, on_output)

    def real_batch(lo, hi):
        items = [dataset[i] for i in range(lo, hi)]
        img = torch.from_numpy(np.stack([it[0] for it in items])).to(device).to(torch.float32) / 127.5 - 1
        return [img, torch.from_numpy(np.stack([it[1] for it in items])).to(device)]

    text = io.StringIO()

    def say(lines):
        for line in lines:
            print(line)
            text.write(line + '\n')

    def run_pass(table, step):
        """one pass over the samples, `step` at a time: the table pass stops after the first batch"""
        for lo in range(0, len(seeds), step):
            z = z_all[lo:lo + step]
            inputs, kwargs = _generator_images(G, z, label, truncation_psi, noise_mode)
            with _bound(G, kwargs):
                if 'G' in sets:
                    img = sets['G'].table(inputs) if table else sets['G'].measure(inputs)
                else:
                    img = G(*inputs)
            if table and 'G' in sets:
                say([''] + misc.format_table(misc.summary_rows(G, [e for _, e in sets['G'].kept])) + [''])
            if 'D(fake)' in sets:
                d_inputs = [img.to(torch.float32), label.expand(z.shape[0], -1)]
                sets['D(fake)'].table(d_inputs) if table else sets['D(fake)'].measure(d_inputs)
                if table:
                    say([''] + misc.format_table(misc.summary_rows(D, [e for _, e in sets['D(fake)'].kept])) + [''])
            if 'D(real)' in sets:
                r_inputs = real_batch(lo, min(lo + step, len(seeds)))
                sets['D(real)'].table(r_inputs) if table else sets['D(real)'].measure(r_inputs)
            if table:
                return

    run_pass(table=True, step=batch)
    # On the CPU (the torch.nn layers of the DCGAN networks) the statistics pass forwards ONE sample at a time: torch's CPU convolutions and GEMMs
    # pick their blocking by the batch size, so a sample's activations would depend on what else is in its batch and the files on --batch.
    run_pass(table=False, step=batch if device.type == 'cuda' else 1)

    report, arrays, reports = {}, {}, []
    for key, s in sets.items():
        cells, rows, arr = s.rows()
        say([f'{key}: activation statistics over {s.samples} samples', ''] + misc.format_table(cells) + [''])
        first = next((r['name'] for r in rows if r['stats'] is not None and r['stats']['nonfinite'] > 0), None)
        report[key] = dict(samples=s.samples, parameters=sum(r['parameters'] for r in rows), buffers=sum(r['buffers'] for r in rows),
                           first_nonfinite=first, entries=rows)
        arrays.update(arr)
        reports.append((key, rows))
        if first is not None:
            say([f'{key}: the first entry with a NaN or an infinity is {first}', ''])
    return dict(text=text.getvalue(), report=report, arrays=arrays, image=exponent_image(reports))


def network_summary(G, outdir, D=None, **options):
    """`measure_networks` and the files of the module docstring -> its dict, with `report` as summary.json holds it"""
    result = measure_networks(G, D=D, **options)
    shown = {k: (list(v) if isinstance(v, range) else v) for k, v in options.items() if k not in ('device', 'dataset', 'on_output')}
    shown['data'] = options.get('dataset') is not None
    result['report'] = dict(options=shown, networks=result['report'])
    os.makedirs(outdir, exist_ok=True)
    with open(os.path.join(outdir, 'summary.txt'), 'w') as f:
        f.write(result['text'])
    with open(os.path.join(outdir, 'summary.json'), 'w') as f:
        json.dump(result['report'], f, indent=2, allow_nan=False)
    np.savez(os.path.join(outdir, 'summary.npz'), **result['arrays'])
    save_png(result['image'], os.path.join(outdir, 'exponents.png'))
    return result


# ---------------------------------------------------------------------------------------------------------------- CLI

def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.network_summary', description=__doc__.split('\n')[0])
    add_snapshot_option(ap, help='network-snapshot-*.pt of this build (G_ema, or G when there is no EMA; D for --networks=D)')
    ap.add_argument('--outdir', required=True, help='where to save summary.txt, summary.json, summary.npz and exponents.png')
    ap.add_argument('--networks', default=','.join(NETWORKS), help=f'which networks: a list of {", ".join(NETWORKS)} (default: both)')
    ap.add_argument('--seeds', type=num_range, default=list(range(64)), help='the samples: list of random seeds (default: 0-63)')
    ap.add_argument('--data', help='data set (folder or zip) whose first items D also sees: entry set D(real)')
    ap.add_argument('--max-nesting', type=int, default=3, help='deepest module nesting shown (default: 3)')
    add_sampling_options(ap)
    ap.add_argument('--batch', type=int, default=16, help='samples per forward pass (default: 16)')
    add_device_option(ap)
    args, rest = ap.parse_known_args(argv)
    args.networks = [n for n in args.networks.split(',') if n]
    if not args.networks or any(n not in NETWORKS for n in args.networks):
        ap.error(f'--networks={",".join(args.networks)}: a list of {", ".join(NETWORKS)}')
    if not args.seeds:
        ap.error('--seeds: at least one seed is needed')
    if args.batch < 1:
        ap.error(f'--batch={args.batch}: must be at least 1')
    if args.max_nesting < 0:
        ap.error(f'--max-nesting={args.max_nesting}: must not be negative')
    require_file(ap, '--snapshot', args.snapshot)
    if args.data is not None and not os.path.exists(args.data):
        ap.error(f'--data={args.data}: no such file or folder')
    return config_overrides(ap, rest), args


def run_network_summary(argv=None):
    overrides, args = parse_args(argv)
    from . import arguments
    config = arguments.load_config(overrides)
    device = tool_device(args.device)
    G = load_generator(config, args.snapshot, device)
    D = load_discriminator(config, args.snapshot, G, device) if 'D' in args.networks else None
    options = dict(networks=args.networks, seeds=args.seeds, max_nesting=args.max_nesting, truncation_psi=args.truncation_psi, class_idx=args.class_idx,
                   noise_mode=args.noise_mode, batch=args.batch, device=device)
    if args.data is not None and D is not None:
        with open_dataset(config, dataset_kwargs_for(config, G, data=args.data, mirror=False)) as dataset:
            return network_summary(G, args.outdir, D=D, dataset=dataset, **options)
    return network_summary(G, args.outdir, D=D, **options)


if __name__ == '__main__':
    run_network_summary()
