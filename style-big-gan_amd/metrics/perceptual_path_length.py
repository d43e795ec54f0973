"""Perceptual Path Length (PPL) from "A Style-Based Generator Architecture for Generative Adversarial Networks".

Counterpart of the reference's ``stylegan2ada/metrics/perceptual_path_length.py``: ``slerp`` (:23-32), ``PPLSampler`` (:36-94) and
``compute_ppl`` (:98-134), same signatures and semantics.  Differences:
* the arithmetic around G and the detector -- both interpolation endpoints, crop + area mean + scale + grey -> RGB, and the distance --
  runs as three HIP kernels (torch_utils/ops/ppl.py) instead of chains of tensor ops; CPU tensors take the reference's formulas;
* the random draws (t, z0, z1, the noise buffers) can be handed in (``PPLSampler.forward(c, draws=...)``) so a run can be replayed;
* the detector is a local ``vgg16.pt`` or a callable stand-in (MetricOptions.detector / detector_dir); nothing is fetched;
* the per-rank distances are exchanged by ONE ``all_gather`` after the loop instead of ``world`` broadcasts per iteration; the result
  is interleaved back into the reference's order (iteration-major, then rank);
* ``jit`` is accepted for signature parity and ignored (there is no tracing compiler on this path).
"""
import copy

import numpy as np
import torch

from ..torch_utils.ops import ppl as ppl_ops
from . import metric_utils
from .scores import VGG16      # reference: the nvlabs-fi-cdn URL of vgg16.pt (:101)

LPIPS_KWARGS = dict(resize_images=False, return_lpips=True)

slerp = ppl_ops.slerp


class PPLSampler(torch.nn.Module):
    """`vgg16_kwargs`: keyword arguments of the detector call -- the reference's TorchScript file takes `resize_images=False,
    return_lpips=True` (the default); a callable stand-in takes the images alone (pass {})."""

    def __init__(self, G, G_kwargs, epsilon, space, sampling, crop, vgg16, vgg16_kwargs=None):
        assert space in ['z', 'w']
        assert sampling in ['full', 'end']
        super().__init__()
        self.G = copy.deepcopy(G)
        self.G_kwargs = G_kwargs
        self.epsilon = epsilon
        self.space = space
        self.sampling = sampling
        self.crop = crop
        self.vgg16 = copy.deepcopy(vgg16)
        self.vgg16_kwargs = dict(LPIPS_KWARGS if vgg16_kwargs is None else vgg16_kwargs)

    def noise_buffers(self):
        return [buf for name, buf in self.G.named_buffers() if name.endswith('.noise_const')]

    def forward(self, c, draws=None):
        """`draws`: None (drawn here, in the reference's order: t, then z, then one randn_like per noise buffer) or a dict with
        't' [B], 'z0' / 'z1' [B, z_dim] and 'noise' (one tensor per `.noise_const` buffer, in `named_buffers` order)."""
        B = c.shape[0]
        if draws is None:
            t = torch.rand([B], device=c.device) * (1 if self.sampling == 'full' else 0)
            z0, z1 = torch.randn([B * 2, self.G.z_dim], device=c.device).chunk(2)
        else:
            t = draws['t'].to(c.device, torch.float32)
            if self.sampling == 'end':
                t = t * 0
            z0, z1 = draws['z0'].to(c.device, torch.float32), draws['z1'].to(c.device, torch.float32)

        # both endpoints of every pair in one batch: rows 0..B-1 at t, rows B..2B-1 at t + epsilon
        if self.space == 'w':
            w = self.G.mapping(z=torch.cat([z0, z1]), c=torch.cat([c, c]))
            ws = ppl_ops.lerp_endpoints(w[:B], w[B:], t, self.epsilon)
        else:
            zt = ppl_ops.slerp_endpoints(z0, z1, t, self.epsilon)
            ws = self.G.mapping(z=zt, c=torch.cat([c, c]))

        # new noise for this batch; every synthesis layer reads noise_const afresh (noise_const * noise_strength per call)
        bufs = self.noise_buffers()
        if draws is None:
            for buf in bufs:
                buf.copy_(torch.randn_like(buf))
        else:
            assert len(draws['noise']) == len(bufs), 'draws: one noise tensor per .noise_const buffer'
            for buf, val in zip(bufs, draws['noise']):
                buf.copy_(val)

        img = self.G.synthesis(ws=ws, noise_mode='const', force_fp32=True, **self.G_kwargs)
        img = ppl_ops.prep_images(img, crop=self.crop, factor=self.G.img_resolution // 256)
        lpips = self.vgg16(img, **self.vgg16_kwargs)
        return ppl_ops.lpips_distance(lpips, self.epsilon)


def ppl_from_distances(dist):
    """rank 0's tail (:128-133): the mean of the distances between the 1st ('lower') and the 99th ('higher') percentile, inclusive"""
    dist = np.asarray(dist)
    lo = np.percentile(dist, 1, method='lower')
    hi = np.percentile(dist, 99, method='higher')
    return float(np.extract(np.logical_and(dist >= lo, dist <= hi), dist).mean())


def gather_distances(parts, num_samples, num_gpus):
    """this rank's per-iteration distances -> every rank's, in the reference's order (iteration by iteration, ranks in order), truncated to
    num_samples.  One all_gather: every rank issues it once, whatever its share."""
    x = torch.stack(parts)                          # [iterations, batch]
    if num_gpus > 1:
        everyone = [torch.empty_like(x) for _ in range(num_gpus)]
        torch.distributed.all_gather(everyone, x.contiguous())
        x = torch.stack(everyone, dim=1)            # [iterations, rank, batch]
    return x.flatten()[:num_samples]


def compute_ppl(opts, num_samples, epsilon, space, sampling, crop, batch_size, jit=False, dataset_name='image_folder', sampler=None):
    """`sampler` (extension): a callable c -> [batch] distances standing in for PPLSampler (the detector is then not resolved)."""
    from ..train_parts.datasets import datasets
    dataset = datasets[dataset_name](**opts.dataset_kwargs)

    if sampler is None:
        vgg16 = metric_utils._detector(opts, VGG16)
        kw = metric_utils.detector_call_kwargs(opts, VGG16, LPIPS_KWARGS)
        sampler = PPLSampler(G=opts.G, G_kwargs=opts.G_kwargs, epsilon=epsilon, space=space, sampling=sampling, crop=crop, vgg16=vgg16,
                             vgg16_kwargs=kw)
        sampler.eval().requires_grad_(False).to(opts.device)

    device = torch.device(opts.device)
    parts = []
    progress = opts.progress.sub(tag='ppl sampling', num_items=num_samples)
    with torch.no_grad():
        for batch_start in range(0, num_samples, batch_size * opts.num_gpus):
            progress.update(batch_start)
            c = [dataset.get_label(np.random.randint(len(dataset))) for _i in range(batch_size)]
            c = torch.from_numpy(np.stack(c))
            c = (c.pin_memory() if device.type == 'cuda' else c).to(device)
            parts.append(sampler(c).to(torch.float32))
    progress.update(num_samples)
    dist = gather_distances(parts, num_samples, opts.num_gpus)

    if opts.rank != 0:
        return float('nan')
    return ppl_from_distances(dist.cpu().numpy())
