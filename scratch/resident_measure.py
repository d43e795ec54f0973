"""The measurements of DESIGN.md section 16 (the resident loader; report only).  Each sub-command is one process and prints RESULT lines:
    mkdata DIR          2048 generated PNGs at 256 x 256 (a smooth random field plus noise) through dataset_tool into DIR/data
    kernel              sbg_u8_gather_images from the launch log: batch 64 of 3 x 256 x 256, both paths, both output types, with and without flips
    build DIR           the resident store's build time with 16, 4, 1, 4, 16 decoding threads
    rate DIR LOADER     batches per second of `basic` (its defaults) or `resident`, batch 64, after 20 warm-up batches
    step DIR LOADER     ms/step of the reference's sg2ada configuration over DIR/data with `basic` / `resident`, or on `synthetic` data"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import style_big_gan_amd  # noqa
from style_big_gan_amd import _lib, starter
from style_big_gan_amd.torch_utils import misc
from style_big_gan_amd.torch_utils.ops import resident_set
from style_big_gan_amd.train_parts import dataloaders as DL
from style_big_gan_amd.train_parts.datasets import datasets

N, RES, BATCH = int(os.environ.get('MEASURE_N', 2048)), 256, 64


def out(**kw):
    print("RESULT " + json.dumps(kw), flush=True)


def mkdata(root):
    import concurrent.futures
    import PIL.Image
    src = os.path.join(root, "src")
    os.makedirs(src, exist_ok=True)

    def one(i):
        rng = np.random.RandomState(i)
        low = rng.randint(0, 256, [16, 16, 3]).astype(np.uint8)
        img = np.asarray(PIL.Image.fromarray(low).resize((RES, RES), PIL.Image.BICUBIC)).astype(np.int16)
        img = np.clip(img + rng.randint(-12, 13, img.shape), 0, 255).astype(np.uint8)        # smooth field + sensor-like noise
        PIL.Image.fromarray(img).save(os.path.join(src, f"img{i:05d}.png"))

    t0 = time.time()
    with concurrent.futures.ThreadPoolExecutor(16) as pool:
        list(pool.map(one, range(N)))
    t1 = time.time()
    from style_big_gan_amd import dataset_tool
    dataset_tool.run_dataset_tool(["--source", src, "--dest", os.path.join(root, "data"), "--workers", "16"])
    size = sum(os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(os.path.join(root, "data")) for f in fs)
    out(what="mkdata", gen_s=t1 - t0, tool_s=time.time() - t1, png_bytes=size)


def _dataset(root):
    return datasets["image_folder"](path=os.path.join(root, "data"))


def build(root):
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    for workers in (16, 4, 1, 4, 16):
        ds = _dataset(root)
        torch.cuda.synchronize()
        t0 = time.time()
        loader = DL.ResidentDataloader(dataset=ds, sampler=misc.InfiniteSampler(ds, seed=0), batch_size=BATCH, device=dev, workers=workers)
        torch.cuda.synchronize()
        out(what="build", workers=workers, seconds=time.time() - t0, store_gib=loader.store_bytes / 2 ** 30, images=loader.store.shape[0])
        del loader


def rate(root, name):
    dev = torch.device("cuda:0")
    ds = _dataset(root)
    sampler = misc.InfiniteSampler(ds, seed=0)
    if name == "basic":
        it = iter(DL.dataloaders["basic"](dataset=ds, sampler=sampler, batch_size=BATCH))

        def nxt():
            img, c = next(it)
            return img.to(dev, non_blocking=True).to(torch.float32) / 127.5 - 1, c.to(dev, non_blocking=True)
    else:
        it = DL.ResidentDataloader(dataset=ds, sampler=sampler, batch_size=BATCH, device=dev).batches(normalized=True)
        nxt = lambda: next(it)
    for _ in range(20):
        nxt()
    torch.cuda.synchronize()
    n = 200 if name == "basic" else 2000
    t0 = time.time()
    for _ in range(n):
        img, _c = nxt()
    torch.cuda.synchronize()
    dt = time.time() - t0
    out(what="rate", loader=name, batches=n, seconds=dt, img_per_s=n * BATCH / dt, ms_per_batch=dt / n * 1e3)


def kernel():
    dev = torch.device("cuda:0")
    S, C, H, W = N, 3, RES, RES
    buf = torch.randint(0, 256, [S * C * H * W + 4], dtype=torch.uint8, device=dev)
    lut = resident_set.normalisation_table(dev)
    gen = torch.Generator().manual_seed(0)
    for path, store in (("dword", buf[:S * C * H * W].view(S, C, H, W)), ("byte", buf[1:1 + S * C * H * W].view(S, C, H, W))):
        for table in (lut, None):
            for flips in ("mixed", "none"):
                slot = torch.randint(0, S, [BATCH], generator=gen).to(torch.int32).to(dev)
                flip = torch.randint(0, 2, [BATCH], generator=gen).to(torch.uint8).to(dev) if flips == "mixed" else None
                for _ in range(5):
                    resident_set.gather(store, slot, flip, table)
                _lib.prof_enable(True)
                _lib.prof_fetch()
                for _ in range(30):
                    slot = torch.randint(0, S, [BATCH], generator=gen).to(torch.int32).to(dev)
                    resident_set.gather(store, slot, flip, table)
                recs = [r for r in _lib.prof_fetch() if r["kind"] == "resident"]
                _lib.prof_enable(False)
                ms = sorted(r["ms"] for r in recs)
                med = ms[len(ms) // 2]
                out(what="kernel", path=path, logged_path=recs[0]["dims"][6], out="f32" if table is not None else "u8", flips=flips, launches=len(recs),
                    median_us=med * 1e3, min_us=ms[0] * 1e3, bytes=recs[0]["bytes"], gb_per_s=recs[0]["bytes"] / (med * 1e-3) / 1e9)


def step(root, name):
    from golden_util import Golden
    import yaml
    cfg = Golden("reference_configs").meta["configs"]["sg2ada"]
    cfg.pop("datasets_args", None)
    with open(os.path.join(root, "sg2ada.yaml"), "w") as fh:
        yaml.safe_dump(cfg, fh)
    argv = [f"exp.config_dir={root}", "exp.config=sg2ada.yaml", "exp.name=m", f"log.output={root}/logs", "log.metrics=[]", "gen.kimg=100000"]
    if name == "synthetic":
        argv += ["data.dataset=synthetic", f"data.resolution={RES}"]
    else:
        argv += ["data.dataset=image_folder", f"data.dataset_path={root}/data", f"data.dataloader={name}"]
    trainer = starter.main(argv, max_iterations=6)
    torch.cuda.synchronize()
    steps = 24
    t0 = time.time()
    trainer.training_loop(max_iterations=steps)
    torch.cuda.synchronize()
    dt = time.time() - t0
    out(what="step", loader=name, steps=steps, batch=trainer.engine.batch, ms_per_step=dt / steps * 1e3, img_per_s=steps * trainer.engine.batch / dt)


if __name__ == "__main__":
    {"mkdata": mkdata, "build": build, "rate": rate, "kernel": kernel, "step": step}[sys.argv[1]](*sys.argv[2:])
