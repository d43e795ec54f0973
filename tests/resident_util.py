"""What the resident-loader tests share: the data sets over golden_util.make_image_folder, a data set that counts its decodes, the store
restated with numpy, and the two tiny training configs."""
import os

import numpy as np
import torch
import yaml

from golden_util import make_image_folder

# the three data sets of the item-equivalence tests: (constructor keywords, distinct stored images of a 14-image folder)
DATASET_CASES = {
    "plain": (dict(), 14),
    "xflip": (dict(xflip=True), 14),
    "subset_xflip_labels": (dict(max_size=5, xflip=True, random_seed=3, use_labels=True), 5),
}

DCGAN_LIKE = {
    "exp": {"trainer": "base"},
    "gen": {"kimg": 1, "batch": 8, "batch_gpu": 8, "loss_arch": "base", "loss": "bcew", "generator": "cnn32_dcgan", "discriminator": "cnn32_dcgan",
            "g_reg_interval": 0, "d_reg_interval": 0},
    "gens_args": {"cnn32_dcgan": {"z_dim": 100}},
    "optim_gen_args": {"adam": {"lr": 0.0002, "betas": [0.5, 0.9]}},
    "optim_disc_args": {"adam": {"lr": 0.0002, "betas": [0.5, 0.9]}},
    "ema": {"use_ema": False},
    "aug": {"aug": "noaug"},
    "log": {"metrics": []},
}

SG2_TINY = {
    "exp": {"trainer": "sg2"},
    "gen": {"kimg": 1, "batch": 8, "batch_gpu": 8, "generator": "sg2_classic", "discriminator": "sg2_classic", "disc_regs": ["r1"]},
    "disc_regs_all": {"r1": {"r1_gamma": 0.01}},
    "losses_arch_args": {"sg2": {"style_mixing_prob": 0}},
    "aug": {"aug": "noaug"},
    "log": {"metrics": []},
    "gens_args": {"sg2_classic": {"z_dim": 16, "w_dim": 16, "mapping_kwargs": {"num_layers": 2},
                                  "synthesis_kwargs": {"channel_base": 512, "channel_max": 16, "num_fp16_res": 0, "block_kwargs": {"conv_clamp": 256}}}},
    "discs_args": {"sg2_classic": {"channel_base": 512, "channel_max": 16, "num_fp16_res": 0, "architecture": "orig",
                                   "epilogue_kwargs": {"mbstd_group_size": 4}}},
}


def write_config(tmp, cfg, path, *more):
    """-> argv of a run of `cfg` over the image folder `path`"""
    with open(os.path.join(str(tmp), "cfg.yaml"), "w") as fh:
        yaml.safe_dump(cfg, fh)
    return [f"exp.config_dir={tmp}", "exp.config=cfg.yaml", "exp.name=run", f"log.output={os.path.join(str(tmp), 'logs')}", "data.dataset=image_folder",
            f"data.dataset_path={path}"] + list(more)


def image_folder_class():
    from style_big_gan_amd.train_parts.datasets import datasets
    return datasets["image_folder"]


def counting_dataset(**kw):
    """an image folder data set whose `decoded` lists the stored images read since it was last cleared"""
    base = image_folder_class()

    class Counting(base):
        decoded = None

        def _load_raw_image(self, raw_idx):
            if self.decoded is not None:
                self.decoded.append(int(raw_idx))
            return super()._load_raw_image(raw_idx)

    ds = Counting(**kw)
    ds.decoded = []         # the constructor's probe of image 0 is not the loader's
    return ds


def numpy_store(dataset, raw):
    """the store a loader must build: the stored images `raw`, in that order"""
    return torch.from_numpy(np.ascontiguousarray(np.stack([dataset._load_raw_image(r) for r in raw])))
