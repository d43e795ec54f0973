"""Calculate quality metrics for a snapshot on disk.

Counterpart of the reference's ``stylegan2ada/calc_metrics.py`` (``subprocess_fn`` :27-81, ``calc_metrics`` :100-186): same options, same
metric names, one ``report_metric`` JSON line per metric, appended to ``metric-<name>.jsonl`` when ``training_options.json`` sits next to
the snapshot (the reference's run-dir rule, :170-176).  Differences:
* the CLI builds G from the run's config (the ``key=value`` list ``starter`` takes) and loads a ``network-snapshot-*.pt`` of this build;
  the data set options come from that config too (snapshots of this build hold no ``training_set_kwargs``), through the helper the
  trainer itself uses; ``--data`` overrides the path, ``--mirror`` the flips, and the labels follow ``G.c_dim``;
* detectors are local: ``--detector`` names a TorchScript file or a directory holding the reference's file names; nothing is fetched;
  it may be left out when no metric asked for needs one (``swd16k``, the sliced Wasserstein distance on Laplacian-pyramid patches);
* on a GPU the precision / recall metrics run on the fused k-NN kernels (metrics/scores.py, ``precision_recall_fused``), and so does
  ``prdc50k5_full`` (precision / recall / density / coverage, ``prdc_fused``), a metric the reference does not have;
* ``calc_metrics()`` is a function of a generator for callers that already hold one.

    python -m style_big_gan_amd.calc_metrics exp.config_dir=<dir> exp.config=<file.yaml> --snapshot=<network-snapshot-*.pt> \\
        [--metrics=fid50k_full,pr50k3_full | none] [--data=<folder|zip>] [--mirror=0|1] [--gpus=1] [--detector=<TorchScript file | directory>] \\
        [--verbose=1] [--device=auto|cuda|cpu]
"""
import argparse
import os
import tempfile

import torch

from .metrics import metric_main, metric_utils, perceptual_path_length
from .tool_support import (add_device_option, add_snapshot_option, config_overrides, dataset_kwargs_for, detector_kwargs, load_generator, require_file,
                           resolve_device)

MAX_GPUS = 16


def comma_list(s):
    """'a,b,c' -> ['a', 'b', 'c']; '' and 'none' -> [] (the reference's CommaSeparatedList, :86-96)"""
    if s is None or s.lower() == 'none' or s == '':
        return []
    return s.split(',')


def needs_detector(metrics):
    """whether any of `metrics` computes on detector features (metric_main.needs_detector); unknown names count: they fail on their own"""
    return any(metric_main.needs_detector(m) for m in metrics)


def check_metrics(metrics, G=None, detector=None):
    """unknown names fail with the list of valid ones; the perceptual-path-length metrics keep the checks the trainer makes at setup:
    the LPIPS detector must be present and G needs `mapping` / `synthesis`"""
    bad = [m for m in metrics if not metric_main.is_valid_metric(m)]
    if bad:
        raise ValueError('--metrics: unknown ' + ', '.join(bad) + '; valid: ' + ', '.join(metric_main.list_valid_metrics()))
    ppl = [m for m in metrics if m.startswith(('ppl_', 'ppl2_'))]
    if not ppl:
        return
    if isinstance(detector, str):
        if os.path.isdir(detector):
            if not os.path.isfile(os.path.join(detector, perceptual_path_length.VGG16)):
                raise ValueError(f'--metrics={",".join(ppl)} needs the LPIPS detector {perceptual_path_length.VGG16}: --detector={detector} does not hold it')
        elif metric_utils.get_feature_detector_name(detector) != metric_utils.get_feature_detector_name(perceptual_path_length.VGG16):
            raise ValueError(f'--metrics={",".join(ppl)} needs the LPIPS detector {perceptual_path_length.VGG16}; --detector={detector} is another '
                             'detector (pass a directory holding vgg16.pt)')
    if G is not None and not (hasattr(G, 'mapping') and hasattr(G, 'synthesis')):
        raise ValueError(f'--metrics={",".join(ppl)} needs a generator with mapping and synthesis networks')


def calc_metrics(G, metrics, dataset_kwargs, detector, num_gpus=1, rank=0, device=None, run_dir=None, snapshot=None, dataset_name='image_folder',
                 verbose=False):
    """every metric of `metrics` on G against the data set; rank 0 reports (one JSON line each, and metric-<name>.jsonl under `run_dir`).
    With num_gpus > 1 the caller has initialised torch.distributed.  -> {metric: result dict}"""
    device = torch.device(device) if device is not None else next(iter(G.parameters())).device
    check_metrics(metrics, G, detector)
    kw = detector_kwargs(detector) if detector is not None or needs_detector(metrics) else dict(detector=None, detector_dir=None)
    out = dict()
    for metric in metrics:
        if rank == 0 and verbose:
            print(f'Calculating {metric}...')
        progress = metric_utils.ProgressMonitor(verbose=verbose)
        result = metric_main.calc_metric(metric=metric, dataset_name=dataset_name, G=G, dataset_kwargs=dict(dataset_kwargs), num_gpus=num_gpus,
                                         rank=rank, device=device, progress=progress, **kw)
        if rank == 0:
            metric_main.report_metric(result, run_dir=run_dir, snapshot_pkl=snapshot)
        if rank == 0 and verbose:
            print()
        out[metric] = result
    return out


def _worker(rank, overrides, opts, temp_dir):
    """one process per GPU (reference subprocess_fn :27-81): rendezvous over a file store, build G, run the metrics"""
    from . import arguments
    dev_type = resolve_device(opts['device'])
    num_gpus = opts['gpus']
    if num_gpus > 1:
        init_method = 'file://' + os.path.abspath(os.path.join(temp_dir, '.torch_distributed_init'))
        torch.distributed.init_process_group(backend='nccl' if dev_type == 'cuda' else 'gloo', init_method=init_method, rank=rank, world_size=num_gpus)
    try:
        device = torch.device('cuda', rank) if dev_type == 'cuda' else torch.device('cpu')
        if dev_type == 'cuda':
            torch.cuda.set_device(device)
        config = arguments.load_config(overrides)
        if rank == 0 and opts['verbose']:
            print(f'Loading network from "{opts["snapshot"]}"...')
        G = load_generator(config, opts['snapshot'], device, announce=False)
        kw = dataset_kwargs_for(config, G, data=opts['data'], mirror=opts['mirror'])
        if rank == 0 and opts['verbose']:
            print('Dataset options:', kw)
        run_dir = os.path.dirname(os.path.abspath(opts['snapshot']))
        if not os.path.isfile(os.path.join(run_dir, 'training_options.json')):      # the reference's run-dir rule
            run_dir = None
        results = calc_metrics(G, opts['metrics'], kw, opts['detector'], num_gpus=num_gpus, rank=rank, device=device, run_dir=run_dir,
                               snapshot=os.path.abspath(opts['snapshot']), dataset_name=config.data.dataset, verbose=bool(opts['verbose']))
        if rank == 0 and opts['verbose']:
            print('Exiting...')
        return results
    finally:
        if num_gpus > 1:
            torch.distributed.destroy_process_group()


# ---------------------------------------------------------------------------------------------------------------- CLI

def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the tool's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.calc_metrics', description=__doc__.split('\n')[0])
    add_snapshot_option(ap)
    ap.add_argument('--metrics', type=comma_list, default=['fid50k_full'], help='comma-separated list or "none" (default: fid50k_full)')
    ap.add_argument('--data', help='data set to evaluate against, folder or zip (default: the run\'s data.dataset_path)')
    ap.add_argument('--mirror', type=int, choices=(0, 1), help='whether the data set was augmented with x-flips during training (default: the run\'s data.mirror)')
    ap.add_argument('--gpus', type=int, default=1, help='number of GPUs to use (default: 1)')
    ap.add_argument('--detector', help='local TorchScript detector, or a directory holding inception-2015-12-05.pt / vgg16.pt; required unless no '
                    'metric of --metrics needs one (swd16k)')
    ap.add_argument('--verbose', type=int, choices=(0, 1), default=1, help='print optional information (default: 1)')
    add_device_option(ap)
    args, rest = ap.parse_known_args(argv)
    try:
        check_metrics(args.metrics)
    except ValueError as e:
        ap.error(str(e))
    if args.gpus < 1:
        ap.error('--gpus must be at least 1')
    if args.gpus > MAX_GPUS:
        ap.error(f'--gpus must be at most {MAX_GPUS}')
    require_file(ap, '--snapshot', args.snapshot)
    if args.detector is None:
        if needs_detector(args.metrics):
            ap.error('the following arguments are required: --detector')
    elif not os.path.exists(args.detector):
        ap.error(f'--detector={args.detector}: no such TorchScript file or directory (detectors are not downloaded in this build)')
    args.mirror = None if args.mirror is None else bool(args.mirror)
    return config_overrides(ap, rest), args


def run_calc_metrics(argv=None):
    """the parent never touches the GPU: one worker runs in this process for --gpus=1, N fresh ones are spawned otherwise"""
    overrides, args = parse_args(argv)
    opts = dict(vars(args))
    with tempfile.TemporaryDirectory() as temp_dir:
        if args.gpus == 1:
            return _worker(0, overrides, opts, temp_dir)
        torch.multiprocessing.spawn(fn=_worker, args=(overrides, opts, temp_dir), nprocs=args.gpus)
    return None


if __name__ == '__main__':
    run_calc_metrics()
