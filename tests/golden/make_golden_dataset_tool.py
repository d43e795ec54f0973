"""Generate tests/golden/dataset_tool.npz by running the REFERENCE's data set tool on CPU.

Needs the reference checkout (SBG_REFERENCE, default /root/reference) with click, tqdm and PIL, and no GPU:

    python tests/golden/make_golden_dataset_tool.py

* ``t<i>/x``, ``t<i>/y``: the transform cases of tests/dataset_tool_util.TRANSFORM_CASES through the reference's ``make_transform``
  (stylegan2ada/dataset_tool.py:199-248); a dropped image has no ``y`` and ``dropped`` set in the meta data.
* ``run/<name>/...``: ``convert_dataset`` (:304-439) on the tiny sources of tests/dataset_tool_util.RUNS -- a labelled folder, an
  unlabelled zip, a folder of mixed sizes through ``center-crop-wide`` (one image dropped), and full-sized synthetic CIFAR-10 and MNIST
  archives with ``--max-images 4``.  Stored: the source images, the archive's member names, the decoded pixels of every member and the
  text of ``dataset.json``.  Pixels, not PNG bytes: another PIL may encode differently.
"""
import json
import os
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.environ.get("SBG_REFERENCE", "/root/reference")
sys.path.insert(0, os.path.dirname(HERE))       # tests/
sys.path.insert(0, REF)

from stylegan2ada import dataset_tool as R      # noqa: E402
import dataset_tool_util as du                  # noqa: E402


def main():
    arrays, meta = {}, dict(transforms=[], runs={})
    for i, case in enumerate(du.TRANSFORM_CASES):
        x = du.striped(700 + i, case["shape"])
        y = R.make_transform(case["transform"], case["width"], case["height"], case["filter"])(x)
        arrays[f"t{i}/x"] = x
        if y is not None:
            arrays[f"t{i}/y"] = np.asarray(y)
        meta["transforms"].append(dict(case, key=f"t{i}", dropped=y is None))

    tmp = tempfile.mkdtemp()
    for name, run in du.RUNS.items():
        images = du.run_inputs(name)
        root = os.path.join(tmp, name)
        src = du.build_source(name, images, root)
        dest = du.dest_path(name, root)
        R.convert_dataset.main(args=[f"--source={src}", f"--dest={dest}"] + run["args"], standalone_mode=False)
        names, pixels, text = du.read_archive(dest)
        for k, img in enumerate(images):
            arrays[f"run/{name}/in{k}"] = img
        for k, n in enumerate(n for n in names if n.endswith(".png")):
            arrays[f"run/{name}/out{k}"] = pixels[n]
        meta["runs"][name] = dict(names=names, json=text, inputs=len(images))

    path = os.path.join(HERE, "dataset_tool.npz")
    np.savez_compressed(path, __meta__=np.frombuffer(json.dumps(meta).encode(), dtype=np.uint8), **arrays)
    print(f"dataset_tool: {len(arrays)} arrays, {os.path.getsize(path) / 1024:.1f} KiB")


if __name__ == "__main__":
    main()
