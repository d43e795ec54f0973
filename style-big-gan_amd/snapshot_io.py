"""What the command-line tools (projector, generate, style_mixing) share: a generator built from the run's config and a
``network-snapshot-*.pt`` of this build (written by ``BaseTrainer.save_snapshot``), and the ``key=value`` config overrides ``starter`` takes."""
import re

import torch


def config_overrides(parser, rest):
    """the arguments an argparse parser did not recognise must all be `key=value` config overrides -> the list, or the parser's error"""
    bad = [r for r in rest if '=' not in r or r.startswith('-')]
    if bad:
        parser.error(f'unrecognised arguments: {" ".join(bad)}')
    return rest


def generator_common_kwargs(state):
    """c_dim, img_resolution and img_channels of a generator, read from its state dict (the CLI has no data set to ask)"""
    res = [int(m.group(1)) for k in state for m in [re.match(r'synthesis\.b(\d+)\.', k)] if m]
    if not res:
        raise RuntimeError('the snapshot holds no mapping/synthesis generator')
    img_resolution = max(res)
    torgb = state.get(f'synthesis.b{img_resolution}.torgb.weight')
    embed = state.get('mapping.embed.weight')
    return dict(c_dim=int(embed.shape[1]) if embed is not None else 0, img_resolution=img_resolution,
                img_channels=int(torgb.shape[0]) if torgb is not None else 3)


def build_generator(config, state, device):
    """G through the `generators` registry with the config's gens_args, weights from `state` (strict)"""
    from .train_parts.generators import generators
    from .train_parts.trainers import BaseTrainer
    name = config.gen.generator
    kw = BaseTrainer._model_kwargs(config.gens_args[name], generator_common_kwargs(state))
    G = generators[name](**kw)
    G.load_state_dict(state, strict=True)
    return G.eval().requires_grad_(False).to(device)


def snapshot_generator_state(path):
    """G_ema of a network-snapshot-*.pt, or G when the run kept no average"""
    snap = torch.load(path, map_location='cpu', weights_only=True)
    key = 'G_ema' if snap.get('G_ema') is not None else 'G'
    if key not in snap:
        raise RuntimeError(f'{path} holds neither G_ema nor G')
    return snap[key]
