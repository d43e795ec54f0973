"""DiffAugment: the fused kernels against the torch composition on the same device, forward plus adjoint.

    python scratch/diffaug_bench.py [--reps 200] [--rounds 5] [--out FILE.json]

Shapes [64, 3, 32, 32] and [32, 3, 256, 256].  Per shape and round the two implementations alternate in one process: each is warmed up,
then `reps` calls of forward + adjoint (y = f(x); dx = grad(sum(y * g), x)) are timed with device events.  The launch log gives the
per-kernel times of the fused path in a window of its own (logging slows the host).  Bytes per launch are computed from the shapes:
the sum reads the sample once (4 B / value), the apply reads and writes it (8 B / value), the single-pass kernel the same 8 B / value.
The share of HBM bandwidth is bytes / time over the 6.3 TB/s copy ceiling.  No GPU, no numbers: the script fails."""
import argparse
import json
import statistics
import sys

import torch

sys.path.insert(0, '.')
import style_big_gan_amd  # noqa: E402,F401
from style_big_gan_amd import _lib  # noqa: E402
from style_big_gan_amd.torch_utils.ops import diffaug as D  # noqa: E402
from style_big_gan_amd.train_parts import augmentations as A  # noqa: E402

HBM_CEILING = 6.3e12


def call(fn, x, g):
    y = fn(x)
    dx, = torch.autograd.grad((y * g).sum(), x)
    return dx


def call_fused(fwd, adj, x, g):
    """forward + adjoint without the autograd bookkeeping and the multiply-sum of `call`: the kernels' own cost"""
    fwd(x)
    return adj(g)


def event_time(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps * 1e3            # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=200)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device('cuda:0')
    results = []
    for shape in [(64, 3, 32, 32), (32, 3, 256, 256)]:
        N, C, H, W = shape
        torch.manual_seed(0)
        pipe = A.DiffAugmentPipe(color=1, translation=1, cutout=1)
        prm = pipe.sample(N, C, H, W, p=1.0)
        table = D.pack(prm).to(dev)
        x = (torch.rand(shape, device=dev) * 2 - 1).requires_grad_(True)
        g = torch.randn(shape, device=dev)
        xd = x.detach()
        runs = {
            'kernels (autograd)': lambda: call(lambda t: D.diffaug(t, table), x, g),
            'torch composition (autograd)': lambda: call(lambda t: D.diffaug_reference(t, table), x, g),
            'kernels (two direct calls)': lambda: call_fused(lambda t: D.diffaug(t, table), lambda t: D.diffaug_adjoint(t, table), xd, g),
        }
        err = float((runs['kernels (autograd)']() - runs['torch composition (autograd)']()).abs().max())
        times = {k: [] for k in runs}
        for _ in range(args.rounds):
            for name, fn in runs.items():           # alternate inside every round
                for _ in range(10):
                    fn()
                torch.cuda.synchronize()
                times[name].append(event_time(fn, args.reps))
        # per-kernel times from the launch log
        fn = runs['kernels (two direct calls)']
        torch.cuda.synchronize(); _lib.prof_enable(True); _lib.prof_fetch()
        for _ in range(50):
            fn()
        torch.cuda.synchronize(); _lib.prof_enable(False)
        kernels = {}
        for r in _lib.prof_fetch():
            if r['kind'] == 'diffaug':
                kernels.setdefault(_lib.DIFFAUG_VARIANTS[r['dims'][0]], []).append((r['ms'] * 1e3, r['bytes']))
        rec = dict(shape=shape, max_abs_diff_dx=err, values=N * C * H * W,
                   us_per_call={k: dict(median=statistics.median(v), min=min(v), max=max(v)) for k, v in times.items()},
                   kernels={k: dict(us_median=statistics.median(t for t, _ in v), bytes=v[0][1],
                                    hbm_share=v[0][1] / (statistics.median(t for t, _ in v) * 1e-6) / HBM_CEILING) for k, v in kernels.items()})
        results.append(rec)
        print(json.dumps(rec), flush=True)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(results, fh, indent=1)


if __name__ == '__main__':
    main()
