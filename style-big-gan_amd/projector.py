"""Project an image into the latent space of a trained generator.

Counterpart of the reference's ``stylegan2ada/projector.py`` (``project()`` :25-131, the CLI :135-210), same signature, same order of
work and same result ([num_steps, num_ws, w_dim]).  Differences:
* the noise regulariser, the noise renormalisation and the LPIPS distance run as HIP kernels over the whole set of noise buffers
  (torch_utils/ops/projector.py) instead of ~1 600 small tensor ops per step; CPU tensors take the reference's formulas;
* the detector is a local ``vgg16.pt`` (TorchScript) or a callable stand-in; nothing is fetched;
* the random draws (the initial noise buffers and every step's w noise) can be handed in (``draws``) so a run can be replayed;
* without ``verbose`` the loop never synchronises with the host.  The reference formats ``dist`` and ``float(loss)`` on every step,
  even when nothing is printed; here they are read only when they are printed;
* the CLI builds G from the run's config (the ``key=value`` list ``starter`` takes) and loads a ``network-snapshot-*.pt`` of this build.

    python -m style_big_gan_amd.projector exp.config_dir=<dir> exp.config=<file.yaml> --snapshot=<network-snapshot-*.pt> \\
        --target=<image> --outdir=<dir> --detector=<vgg16.pt> [--num-steps=1000] [--seed=303] [--save-video]
"""
import argparse
import copy
import os
from time import perf_counter

import numpy as np
import torch
import torch.nn.functional as F

from .tool_support import add_snapshot_option, config_overrides, generator_common_kwargs, load_generator, save_png     # noqa: F401
from .torch_utils.ops import projector as proj_ops

LPIPS_KWARGS = dict(resize_images=False, return_lpips=True)


def learning_rate(step, num_steps, initial_learning_rate=0.1, lr_rampdown_length=0.25, lr_rampup_length=0.05):
    """the reference's learning-rate schedule (:85-88): cosine ramp-down over the last `lr_rampdown_length`, linear ramp-up"""
    t = step / num_steps
    lr_ramp = min(1.0, (1.0 - t) / lr_rampdown_length)
    lr_ramp = 0.5 - 0.5 * np.cos(lr_ramp * np.pi)
    lr_ramp = lr_ramp * min(1.0, t / lr_rampup_length)
    return initial_learning_rate * lr_ramp


def w_noise_scale(step, num_steps, w_std, initial_noise_factor=0.05, noise_ramp_length=0.75):
    """the reference's w-noise schedule (:84): quadratic ramp to 0 over the first `noise_ramp_length`"""
    t = step / num_steps
    return w_std * initial_noise_factor * max(0.0, 1.0 - t / noise_ramp_length) ** 2


def resolve_detector(vgg16, device, vgg16_kwargs=None):
    """`vgg16`: a local TorchScript file (called with the reference's LPIPS keyword arguments) or a callable stand-in (called with the
    images alone) -> (detector, call kwargs).  `vgg16_kwargs` overrides the call kwargs."""
    if callable(vgg16):
        det, kw = vgg16, {}
    else:
        path = str(vgg16)
        if path.startswith(('http://', 'https://')) or not os.path.isfile(path):
            raise RuntimeError(f'projector: the detector must be a local vgg16.pt or a callable (got {path}); nothing is fetched')
        det, kw = torch.jit.load(path, map_location=device).eval(), dict(LPIPS_KWARGS)
    return det, dict(kw if vgg16_kwargs is None else vgg16_kwargs)


def noise_buffers(G):
    """G.synthesis' `noise_const` buffers in `named_buffers` order (the reference's `noise_bufs`, :60)"""
    return {name: buf for (name, buf) in G.synthesis.named_buffers() if 'noise_const' in name}


def project(
    G,
    target,                         # [C, H, W], dynamic range [0, 255]; H and W match G's output resolution
    *,
    num_steps=1000,
    w_avg_samples=10000,
    initial_learning_rate=0.1,
    initial_noise_factor=0.05,
    lr_rampdown_length=0.25,
    lr_rampup_length=0.05,
    noise_ramp_length=0.75,
    regularize_noise_weight=1e5,
    verbose=False,
    device,
    vgg16,
    vgg16_kwargs=None,
    draws=None,
):
    """-> w for every step, [num_steps, num_ws, w_dim] on `device`.  `draws`: None (drawn from torch's global RNG in the reference's call
    order: one randn_like per noise buffer, then one per step) or a dict with 'noise' (one tensor per `.noise_const` buffer, in
    `named_buffers` order) and 'w_noise' ([num_steps, 1, w_dim] unit normals)."""
    assert target.shape == (G.img_channels, G.img_resolution, G.img_resolution)

    def logprint(*args):
        if verbose:
            print(*args)

    G = copy.deepcopy(G).eval().requires_grad_(False).to(device)
    num_ws = G.mapping.num_ws

    # Compute w stats.
    logprint(f'Computing W midpoint and stddev using {w_avg_samples} samples...')
    z_samples = np.random.RandomState(123).randn(w_avg_samples, G.z_dim)
    w_samples = G.mapping(torch.from_numpy(z_samples).to(device), None)     # [N, L, C]
    w_samples = w_samples[:, :1, :].cpu().numpy().astype(np.float32)         # [N, 1, C]
    w_avg = np.mean(w_samples, axis=0, keepdims=True)                         # [1, 1, C]
    w_std = (np.sum((w_samples - w_avg) ** 2) / w_avg_samples) ** 0.5

    noise_bufs = noise_buffers(G)
    vgg16, vgg16_kwargs = resolve_detector(vgg16, device, vgg16_kwargs)

    # Features for the target image.
    target_images = target.unsqueeze(0).to(device).to(torch.float32)
    if target_images.shape[2] > 256:
        target_images = F.interpolate(target_images, size=(256, 256), mode='area')
    target_features = vgg16(target_images, **vgg16_kwargs)

    w_opt = torch.tensor(w_avg, dtype=torch.float32, device=device, requires_grad=True)
    w_out = torch.zeros([num_steps] + list(w_opt.shape[1:]), dtype=torch.float32, device=device)
    optimizer = torch.optim.Adam([w_opt] + list(noise_bufs.values()), betas=(0.9, 0.999), lr=initial_learning_rate)

    # Init noise.
    if draws is not None:
        assert len(draws['noise']) == len(noise_bufs), 'draws: one noise tensor per .noise_const buffer'
        assert draws['w_noise'].shape[0] >= num_steps, 'draws: one w noise per step'
    for i, buf in enumerate(noise_bufs.values()):
        buf[:] = torch.randn_like(buf) if draws is None else draws['noise'][i].to(device, torch.float32)
        buf.requires_grad = True
    bufs = list(noise_bufs.values())

    for step in range(num_steps):
        # Learning rate schedule.
        noise_scale = w_noise_scale(step, num_steps, w_std, initial_noise_factor, noise_ramp_length)
        lr = learning_rate(step, num_steps, initial_learning_rate, lr_rampdown_length, lr_rampup_length)
        for param_group in optimizer.param_groups:
            param_group['lr'] = lr

        # Synth images from opt_w.
        unit = torch.randn_like(w_opt) if draws is None else draws['w_noise'][step].to(device, torch.float32).reshape(w_opt.shape)
        w_noise = unit * noise_scale
        ws = (w_opt + w_noise).repeat([1, num_ws, 1])
        synth_images = G.synthesis(ws, noise_mode='const')

        # Downsample image to 256x256 if it's larger than that.  VGG was built for 224x224 images.
        synth_images = (synth_images + 1) * (255 / 2)
        if synth_images.shape[2] > 256:
            synth_images = F.interpolate(synth_images, size=(256, 256), mode='area')

        # Features for synth images; the distance and the noise regulariser.
        synth_features = vgg16(synth_images, **vgg16_kwargs)
        dist = proj_ops.sqdist(target_features, synth_features)
        reg_loss = proj_ops.noise_reg(bufs)
        loss = dist + reg_loss * regularize_noise_weight

        # Step
        optimizer.zero_grad(set_to_none=True)
        loss.backward()
        optimizer.step()
        if verbose:         # the only host read of the loop
            logprint(f'step {step + 1:>4d}/{num_steps}: dist {float(dist):<4.2f} loss {float(loss):<5.2f}')

        # Save projected W for each optimization step.
        w_out[step] = w_opt.detach()[0]

        # Normalize noise.
        proj_ops.noise_normalize_(bufs)

    return w_out.repeat([1, num_ws, 1])


# ---------------------------------------------------------------------------------------------------------------- CLI

def load_target(path, resolution):
    """the reference's target preparation (:172-178): RGB, centre crop to a square, LANCZOS resize -> (PIL image, uint8 [H, W, 3])"""
    import PIL.Image
    target_pil = PIL.Image.open(path).convert('RGB')
    w, h = target_pil.size
    s = min(w, h)
    target_pil = target_pil.crop(((w - s) // 2, (h - s) // 2, (w + s) // 2, (h + s) // 2))
    target_pil = target_pil.resize((resolution, resolution), PIL.Image.LANCZOS)
    return target_pil, np.array(target_pil, dtype=np.uint8)


def parse_args(argv=None):
    """-> (config overrides as `key=value` strings, the projector's options)"""
    ap = argparse.ArgumentParser(prog='python -m style_big_gan_amd.projector', description=__doc__.split('\n')[0])
    add_snapshot_option(ap)
    ap.add_argument('--target', required=True, help='target image file to project')
    ap.add_argument('--outdir', required=True, help='where to save the output images')
    ap.add_argument('--num-steps', type=int, default=1000, help='number of optimization steps (default: 1000)')
    ap.add_argument('--seed', type=int, default=303, help='random seed (default: 303)')
    ap.add_argument('--detector', required=True, help='local vgg16.pt (TorchScript LPIPS detector)')
    ap.add_argument('--save-video', action='store_true', help='save an mp4 of the optimisation (needs imageio)')
    args, rest = ap.parse_known_args(argv)
    return config_overrides(ap, rest), args


def run_projection(argv=None):
    overrides, args = parse_args(argv)
    from . import arguments
    config = arguments.load_config(overrides)
    if args.save_video:
        try:
            import imageio
        except ImportError as e:
            raise RuntimeError('--save-video needs the imageio package, which is not installed') from e
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)

    device = torch.device('cuda')
    G = load_generator(config, args.snapshot, device)

    target_pil, target_uint8 = load_target(args.target, G.img_resolution)

    start_time = perf_counter()
    projected_w_steps = project(G, target=torch.tensor(target_uint8.transpose([2, 0, 1]), device=device), num_steps=args.num_steps,
                                device=device, verbose=True, vgg16=args.detector)
    print(f'Elapsed: {(perf_counter() - start_time):.1f} s')

    def render(w):
        img = G.synthesis(w.unsqueeze(0), noise_mode='const')
        img = (img + 1) * (255 / 2)
        return img.permute(0, 2, 3, 1).clamp(0, 255).to(torch.uint8)[0].cpu().numpy()

    os.makedirs(args.outdir, exist_ok=True)
    with torch.no_grad():
        if args.save_video:
            video = imageio.get_writer(f'{args.outdir}/proj.mp4', mode='I', fps=10, codec='libx264', bitrate='16M')
            print(f'Saving optimization progress video "{args.outdir}/proj.mp4"')
            for projected_w in projected_w_steps:
                video.append_data(np.concatenate([target_uint8, render(projected_w)], axis=1))
            video.close()

        target_pil.save(f'{args.outdir}/target.png')
        projected_w = projected_w_steps[-1]
        save_png(render(projected_w), f'{args.outdir}/proj.png')
        np.savez(f'{args.outdir}/projected_w.npz', w=projected_w.unsqueeze(0).cpu().numpy())


if __name__ == '__main__':
    run_projection()
