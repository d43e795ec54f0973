"""Shared pieces of the data set tool's tests: the fixture (tests/golden/dataset_tool.npz, written by
tests/golden/make_golden_dataset_tool.py from the reference's tool), the seeded striped images, the builders of the tiny sources both
sides convert (folders, a zip, full-sized synthetic CIFAR-10 and MNIST archives), and readers of a written archive."""
import gzip
import io
import json
import os
import pickle
import tarfile
import zipfile

import numpy as np
import PIL.Image

from golden_util import Golden


def fixture():
    return Golden("dataset_tool")


def striped(seed, shape):
    """seeded uint8 noise with hard 0 / 255 rows and columns, so that the Lanczos overshoot is clipped at both ends"""
    rng = np.random.RandomState(seed)
    a = rng.randint(0, 256, shape).astype(np.uint8)
    a[::7] = 255
    a[3::7] = 0
    a[:, ::5] = 0
    a[:, 2::5] = 255
    return a


# (a) transform cases: shape of the input, transform, width, height, filter
TRANSFORM_CASES = [
    dict(shape=(60, 80, 3), transform=None, width=32, height=32, filter="lanczos"),
    dict(shape=(60, 80, 3), transform=None, width=32, height=32, filter="box"),
    dict(shape=(60, 80, 3), transform=None, width=120, height=100, filter="lanczos"),
    dict(shape=(60, 80, 3), transform=None, width=120, height=100, filter="box"),
    dict(shape=(50, 70), transform=None, width=33, height=21, filter="lanczos"),
    dict(shape=(50, 70), transform=None, width=33, height=21, filter="box"),
    dict(shape=(50, 70), transform=None, width=140, height=75, filter="lanczos"),
    dict(shape=(48, 64, 3), transform=None, width=32, height=None, filter="lanczos"),
    dict(shape=(48, 64, 3), transform=None, width=None, height=16, filter="lanczos"),
    dict(shape=(48, 64), transform=None, width=64, height=100, filter="box"),
    dict(shape=(48, 64, 3), transform=None, width=64, height=48, filter="lanczos"),
    dict(shape=(37, 53, 3), transform=None, width=1, height=1, filter="lanczos"),
    dict(shape=(37, 53), transform=None, width=1, height=1, filter="box"),
    dict(shape=(120, 160, 3), transform=None, width=64, height=64, filter="lanczos"),
    dict(shape=(119, 157, 3), transform=None, width=61, height=47, filter="lanczos"),
    dict(shape=(90, 60, 3), transform="center-crop", width=32, height=32, filter="lanczos"),
    dict(shape=(61, 97, 3), transform="center-crop", width=32, height=32, filter="lanczos"),
    dict(shape=(61, 97, 3), transform="center-crop", width=32, height=32, filter="box"),
    dict(shape=(20, 31, 3), transform="center-crop", width=64, height=64, filter="lanczos"),
    dict(shape=(90, 160, 3), transform="center-crop-wide", width=64, height=32, filter="lanczos"),
    dict(shape=(91, 161, 3), transform="center-crop-wide", width=128, height=64, filter="box"),
    dict(shape=(50, 60, 3), transform="center-crop-wide", width=64, height=32, filter="lanczos"),        # dropped: narrower than --width
    dict(shape=(30, 160, 3), transform="center-crop-wide", width=64, height=32, filter="lanczos"),       # dropped: too flat
]

# (b) end-to-end runs: source kind, image shapes (one per image), labels, the tool's options, destination kind
RUNS = dict(
    folder=dict(kind="folder", shapes=[(24, 36, 3)] * 6, labels=[2, 0, 1, 1, 0, 2], dest="zip",
                args=["--transform=center-crop", "--width=16", "--height=16"]),
    zip=dict(kind="zip", shapes=[(20, 20)] * 5, labels=None, dest="folder", args=["--width=8", "--height=8", "--resize-filter=box"]),
    wide=dict(kind="folder", shapes=[(36, 64, 3), (20, 30, 3), (36, 64, 3), (40, 70, 3)], labels=[1, 0, 2, 1], dest="zip",
              args=["--transform=center-crop-wide", "--width=32", "--height=16"]),
    cifar=dict(kind="cifar", labels=[3, 9, 0, 7], dest="zip", args=["--max-images=4"]),
    mnist=dict(kind="mnist", labels=[5, 0, 9, 4], dest="zip", args=["--max-images=4"]),
)


def run_inputs(name):
    """the images of a run's source, seeded (the fixture stores the same arrays)"""
    run = RUNS[name]
    if run["kind"] == "cifar":
        return [striped(900 + i, (32, 32, 3)) for i in range(4)]
    if run["kind"] == "mnist":
        return [striped(950 + i, (28, 28)) for i in range(4)]
    return [striped(800 + 10 * len(name) + i, shape) for i, shape in enumerate(run["shapes"])]


def source_names(name):
    return [f"{'ab'[i % 2]}/img{i:03d}.png" for i in range(len(RUNS[name]["shapes"]))]


def build_source(name, images, root):
    """write the run's source under `root` from `images` -> its path"""
    run = RUNS[name]
    os.makedirs(root, exist_ok=True)
    if run["kind"] in ("folder", "zip"):
        names = source_names(name)
        meta = json.dumps({"labels": [[n, l] for n, l in zip(names, run["labels"])]}) if run["labels"] is not None else None
        if run["kind"] == "folder":
            src = os.path.join(root, "src")
            for n, img in zip(names, images):
                os.makedirs(os.path.dirname(os.path.join(src, n)), exist_ok=True)
                PIL.Image.fromarray(img).save(os.path.join(src, n))
            if meta is not None:
                with open(os.path.join(src, "dataset.json"), "w") as f:
                    f.write(meta)
            return src
        src = os.path.join(root, "src.zip")
        with zipfile.ZipFile(src, "w") as z:
            for n, img in zip(names, images):
                bits = io.BytesIO()
                PIL.Image.fromarray(img).save(bits, format="png")
                z.writestr(n, bits.getvalue())
            if meta is not None:
                z.writestr("dataset.json", meta)
        return src
    if run["kind"] == "cifar":          # full-sized (the tool asserts 50000 images): zeros behind the first four
        src = os.path.join(root, "cifar-10-python.tar.gz")
        with tarfile.open(src, "w:gz", compresslevel=1) as tar:
            for batch in range(1, 6):
                data = np.zeros([10000, 3072], dtype=np.uint8)
                labels = [0] * 10000
                if batch == 1:
                    for i, img in enumerate(images):
                        data[i] = img.transpose(2, 0, 1).reshape(-1)
                        labels[i] = run["labels"][i]
                blob = pickle.dumps(dict(data=data, labels=labels), protocol=2)
                info = tarfile.TarInfo(f"cifar-10-batches-py/data_batch_{batch}")
                info.size = len(blob)
                tar.addfile(info, io.BytesIO(blob))
        return src
    src = os.path.join(root, "train-images-idx3-ubyte.gz")     # mnist: 60000 images of 28 x 28 behind a 16-byte header
    data = np.zeros([60000, 28, 28], dtype=np.uint8)
    labels = np.zeros([60000], dtype=np.uint8)
    for i, img in enumerate(images):
        data[i], labels[i] = img, run["labels"][i]
    with gzip.open(src, "wb", compresslevel=1) as f:
        f.write(bytes(16) + data.tobytes())
    with gzip.open(os.path.join(root, "train-labels-idx1-ubyte.gz"), "wb", compresslevel=1) as f:
        f.write(bytes(8) + labels.tobytes())
    return src


def dest_path(name, root, tag="out"):
    return os.path.join(root, tag + ".zip" if RUNS[name]["dest"] == "zip" else tag)


def read_archive(path):
    """a written zip or folder -> (sorted member names, {name: decoded pixels}, the text of dataset.json)"""
    if os.path.isdir(path):
        names = sorted(os.path.relpath(os.path.join(r, f), path).replace("\\", "/") for r, _d, files in os.walk(path) for f in files)
        read = lambda n: open(os.path.join(path, n), "rb").read()       # noqa: E731
    else:
        z = zipfile.ZipFile(path)
        names = sorted(z.namelist())
        read = z.read
    pixels = {n: np.array(PIL.Image.open(io.BytesIO(read(n)))) for n in names if n.endswith(".png")}
    return names, pixels, read("dataset.json").decode()
