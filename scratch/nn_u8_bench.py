"""Evidence for DESIGN section 18: time nn_u8.topk at one shape in a fresh process (a warm-up call, `reps` calls between device events, then
one call under the launch log), and the torch alternative -- a chunked fp32 cdist over float copies of `cdist_rows` stored rows (0: skip).

    python scratch/nn_u8_bench.py 64 50000 196608 5 3 50000
    python scratch/nn_u8_bench.py 1024 50000 196608 1 3 50000
"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from style_big_gan_amd import _lib
from style_big_gan_amd.torch_utils.ops import nn_u8

Q, M, F, k, reps, cdist_rows = [int(v) for v in sys.argv[1:7]]
dev = torch.device("cuda:0")
_lib.load()
g = torch.Generator(device=dev).manual_seed(1)
store = torch.empty([M, F], dtype=torch.uint8, device=dev)
for lo in range(0, M, 4096):
    store[lo:lo + 4096] = torch.randint(0, 256, [min(4096, M - lo), F], dtype=torch.uint8, device=dev, generator=g)
queries = torch.randint(0, 256, [Q, F], dtype=torch.uint8, device=dev, generator=g)
queries[0] = store[M // 2]
torch.cuda.synchronize()
out = dict(Q=Q, M=M, F=F, k=k)

d2, idx = nn_u8.topk(queries, store, k)          # warm-up
torch.cuda.synchronize()
assert int(d2[0, 0]) == 0 and int(idx[0, 0]) == M // 2
times = []
for _ in range(reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    nn_u8.topk(queries, store, k)
    b.record()
    torch.cuda.synchronize()
    times.append(a.elapsed_time(b))
out["topk_ms"] = times
_lib.prof_enable(True)
_lib.prof_fetch()
nn_u8.topk(queries, store, k)
recs = [r for r in _lib.prof_fetch() if r["kind"] == "nn_u8"]
_lib.prof_enable(False)
out["launches"] = [dict(variant=_lib.NN_VARIANTS[r["dims"][0]], dims=r["dims"], ms=r["ms"], flops=r["flops"], bytes=r["bytes"]) for r in recs]
ops = 2.0 * Q * M * F
best = min(times)
out["int_ops"] = ops
out["tops_call"] = ops / (best * 1e-3) / 1e12
tile = [r for r in recs if _lib.NN_VARIANTS[r["dims"][0]] in ("single", "split")][0]
out["tops_tile_kernel"] = ops / (tile["ms"] * 1e-3) / 1e12
print(json.dumps(out), flush=True)

# the torch alternative: chunked fp32 cdist over float copies of `cdist_rows` stored rows (not exact)
if cdist_rows > 0:
    rows = min(cdist_rows, M)
    qf = queries.to(torch.float32)

    def alt():
        best_d, best_i = None, None
        for lo in range(0, rows, 2048):
            d = torch.cdist(qf, store[lo:min(lo + 2048, rows)].to(torch.float32))
            dd, ii = d.topk(k, dim=1, largest=False)
            ii = ii + lo
            if best_d is None:
                best_d, best_i = dd, ii
            else:
                cat_d, cat_i = torch.cat([best_d, dd], 1), torch.cat([best_i, ii], 1)
                best_d, sel = cat_d.topk(k, dim=1, largest=False)
                best_i = cat_i.gather(1, sel)
        return best_d, best_i

    alt()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    alt()
    torch.cuda.synchronize()
    out["cdist_rows"] = rows
    out["cdist_ms"] = (time.perf_counter() - t0) * 1e3
    print(json.dumps(dict(cdist_rows=rows, cdist_ms=out["cdist_ms"])), flush=True)

os.makedirs(os.path.join(ROOT, "out"), exist_ok=True)
with open(os.path.join(ROOT, "out", f"nn_u8_bench_{Q}_{M}_{F}_{k}.json"), "w") as f:
    json.dump(out, f, indent=1)
