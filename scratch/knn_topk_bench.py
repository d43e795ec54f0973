"""Evidence for DESIGN section 19: time knn_manifold.topk at one shape in a fresh process (a warm-up call, `reps` calls between device events,
then one call under the launch log), the radius mode of the same kernel at the same shape (kth_radius with k - 1: the k-th smallest
distance, the same tiles without indices), and the torch alternative -- a chunked fp32 cdist + topk over float copies.

    python scratch/knn_topk_bench.py 64 100000 4096 5 5
    python scratch/knn_topk_bench.py 1024 100000 4096 1 5
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from style_big_gan_amd import _lib
from style_big_gan_amd.torch_utils.ops import knn_manifold

Q, M, F, k, reps = [int(v) for v in sys.argv[1:6]]
PEAK = 2.5e15               # dense fp16 FLOP/s of one MI355X
dev = torch.device("cuda:0")
_lib.load()
g = torch.Generator(device=dev).manual_seed(1)
A = torch.randn([8, F], device=dev, generator=g)               # low-rank Gaussian features, as the tests' realistic_features
manifold = (torch.randn([M, 8], device=dev, generator=g) @ A + 0.5).to(torch.float16)
queries = (0.8 * torch.randn([Q, 8], device=dev, generator=g) @ A + 0.5).to(torch.float16)
queries[0] = manifold[M // 2]
torch.cuda.synchronize()
out = dict(Q=Q, M=M, F=F, k=k, flops=2.0 * Q * M * F)


def timed(fn):
    fn()                    # warm-up
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b))
    return times


def logged(fn):
    _lib.prof_enable(True)
    _lib.prof_fetch()
    fn()
    torch.cuda.synchronize()
    recs = [r for r in _lib.prof_fetch() if r["kind"] == "pr"]
    _lib.prof_enable(False)
    return [dict(variant=_lib.PR_VARIANTS[r["dims"][0]], dims=r["dims"], ms=r["ms"]) for r in recs]


d2, idx = knn_manifold.topk(queries, manifold, k)
assert float(d2[0, 0]) == 0 and int(idx[0, 0]) == M // 2
for name, fn in (("topk", lambda: knn_manifold.topk(queries, manifold, k)), ("radius", lambda: knn_manifold.kth_radius(queries, manifold, k - 1))):
    times = timed(fn)
    launches = logged(fn)
    tile = [r for r in launches if r["variant"] in ("single", "split")][0]
    out[name] = dict(call_ms=times, launches=launches, tflops_call=out["flops"] / (min(times) * 1e-3) / 1e12,
                     tflops_tile_kernel=out["flops"] / (tile["ms"] * 1e-3) / 1e12, share_of_peak_tile_kernel=out["flops"] / (tile["ms"] * 1e-3) / PEAK)

# the torch alternative on the same device: fp32 copies, cdist + topk in chunks of manifold rows (not the same arithmetic)
qf, mf = queries.to(torch.float32), manifold.to(torch.float32)


def alt():
    best_d, best_i = None, None
    for lo in range(0, M, 16384):
        dd, ii = torch.cdist(qf, mf[lo:lo + 16384]).topk(k, dim=1, largest=False)
        ii = ii + lo
        if best_d is None:
            best_d, best_i = dd, ii
        else:
            cat_d, cat_i = torch.cat([best_d, dd], 1), torch.cat([best_i, ii], 1)
            best_d, sel = cat_d.topk(k, dim=1, largest=False)
            best_i = cat_i.gather(1, sel)
    return best_d, best_i


out["cdist_topk_ms"] = timed(alt)
print(json.dumps(out), flush=True)
