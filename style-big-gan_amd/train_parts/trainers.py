"""Training step engine (host code) -- the G+D step the headline metric counts.

Counterpart of the hot loop of the reference's ``train_parts/trainers.py``: phase construction with lazy
regularisation (``setup_training_phases`` :601-633: Gmain / Greg / Dmain / Dreg, lr and betas rescaled by
``mb_ratio = interval / (interval + 1)``), the per-iteration body of ``training_loop`` (:711-765: per-phase
``zero_grad`` -> accumulation rounds of ``loss.accumulate_gradients`` -> ``nan_to_num`` of the gradients ->
``opt.step()``), the generator EMA (:752-761) and the data-parallel wiring of ``distrib_acrros_gpu`` (:587-597) /
``SG2Trainer`` (:883-893: mapping, synthesis and D are separate data-parallel modules so they can be synchronised
independently).  The engine itself logs nothing; two switches (`time_phases`, `report_grad_health`) let the trainer's run log read
per-phase device times and the gradient health of every phase without a host synchronisation.

MI355X specifics: gradients live in flat fp32 buckets (``parallel.GradReducer``) that are all-reduced over RCCL as soon
as their last gradient of the phase's final accumulation round has been written, overlapping xGMI traffic with the rest
of backward; ``nan_to_num`` and Adam run over the flat buckets / foreach lists instead of per-parameter launches.
"""
import copy
import json
import os
import time

import numpy as np
import torch

from .. import utils
from ..parallel import GradReducer
from ..torch_utils import misc, training_stats
from ..torch_utils.ops import layer_health
from ..utils import EasyDict
from .discriminators import discriminators
from .generators import generators
from .losses_base import losses_arch
from .optimizers import Adam, optimizers

trainers = utils.ClassRegistry()

merge_rounds = os.environ.get('SBG_MERGE_ROUNDS', '1') != '0'      # accumulation rounds of a phase in one pass (StepEngine._rounds_in_one_pass)


def setup_snapshot_image_grid(training_set, random_seed=0):
    """-> ((gw, gh), uint8 images [gw * gh, C, H, W], labels [gw * gh, label_dim]): the samples of the snapshot grid (reference :63-98).
    The grid covers about 7680 x 4320 pixels, at least 7 x 4 and at most 32 x 32 cells.  Without labels: a random subset of the
    data set in shuffled order.  With labels: one class per grid row, classes in sorted order, each class's samples shuffled and
    handed out gw at a time."""
    rnd = np.random.RandomState(random_seed)
    gw = int(np.clip(7680 // training_set.image_shape[2], 7, 32))
    gh = int(np.clip(4320 // training_set.image_shape[1], 4, 32))
    if not training_set.has_labels:
        all_indices = list(range(len(training_set)))
        rnd.shuffle(all_indices)
        grid_indices = [all_indices[i % len(all_indices)] for i in range(gw * gh)]
    else:
        label_groups = dict()       # label => [idx, ...]
        for idx in range(len(training_set)):
            label = tuple(training_set.get_details(idx).raw_label.flat[::-1])
            label_groups.setdefault(label, []).append(idx)
        label_order = sorted(label_groups.keys())
        for label in label_order:
            rnd.shuffle(label_groups[label])
        grid_indices = []
        for y in range(gh):
            label = label_order[y % len(label_order)]
            indices = label_groups[label]
            grid_indices += [indices[x % len(indices)] for x in range(gw)]
            label_groups[label] = [indices[(i + gw) % len(indices)] for i in range(len(indices))]
    images, labels = zip(*[training_set[i] for i in grid_indices])
    return (gw, gh), np.stack(images), np.stack(labels)


def write_grid_png(canvas, fname):
    """uint8 HWC canvas -> PNG: mode 'L' for one channel, 'RGB' for three (reference :114-118); the tools' writer"""
    from ..tool_support import save_png
    save_png(canvas, fname)


def save_image_grid(img, fname, drange, grid_size):
    """images [gw * gh, C, H, W] (array or tensor, any real dtype) -> PNG of the gw x gh grid (reference :102-118): cast to float32,
    (x - lo) * (255 / (hi - lo)), round half to even, clip.  A device tensor is quantised and tiled by the HIP kernel, so one byte per
    value crosses to the host; anything on the host takes the reference's numpy expression."""
    from ..torch_utils.ops import image_export
    img = img if isinstance(img, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(img))
    gw, gh = grid_size
    assert img.shape[0] == gw * gh
    write_grid_png(image_export.tile(img.to(torch.float32), (gw, gh), 'grid', drange).cpu().numpy(), fname)


def lazy_reg_opt_kwargs(opt_kwargs, interval):
    """lr and betas of a phase that also carries a regulariser applied every `interval` iterations (reference :619-623)"""
    mb_ratio = interval / (interval + 1)
    out = dict(opt_kwargs)
    out['lr'] = opt_kwargs['lr'] * mb_ratio
    out['betas'] = [beta ** mb_ratio for beta in opt_kwargs['betas']]
    return out


def format_time(seconds):
    """seconds -> '42s' | '3m 07s' | '5h 00m 12s' | '2d 03h 15m' (reference stylegan2ada/dnnlib/util.py:139-150)"""
    s = int(np.rint(seconds))
    if s < 60:
        return f"{s}s"
    if s < 60 * 60:
        return f"{s // 60}m {s % 60:02}s"
    if s < 24 * 60 * 60:
        return f"{s // (60 * 60)}h {(s // 60) % 60:02}m {s % 60:02}s"
    return f"{s // (24 * 60 * 60)}d {(s // (60 * 60)) % 24:02}h {(s // 60) % 60:02}m"


def cpu_mem_gb():
    """resident set of this process in GiB, from /proc/self/statm (0 where there is no procfs)"""
    try:
        with open("/proc/self/statm") as fh:
            return int(fh.read().split()[1]) * os.sysconf("SC_PAGE_SIZE") / 2 ** 30
    except (OSError, ValueError, IndexError):
        return 0.0


def _option_lines(obj, tabs=0):
    """nested options, one 'key : value' line each, groups indented by four (the layout of the reference's banner, :121-128)"""
    out = []
    for key, value in obj.items():
        if isinstance(value, dict):
            out.append(" " * tabs + f"{key}:")
            out += _option_lines(value, tabs + 4)
        else:
            out.append(" " * tabs + f"{key} : {value}")
    return out


@trainers.add_to_registry("step_engine")
class StepEngine:
    """Owns G, D, G_ema, the optimizers and the phase schedule; `train_iteration` is one G+D step on this rank.

    batch       -- images per iteration on THIS rank (the reference's ``batch // num_gpus``)
    batch_gpu   -- micro-batch per accumulation round
    """

    def __init__(self, device, generator='sg2_classic', discriminator='sg2_classic', gen_kwargs=None, disc_kwargs=None,
                 loss_arch='sg2', loss='softplus', loss_arch_kwargs=None, gen_regs=(), dis_regs=(('r1', dict(r1_gamma=10.)),),
                 optim_gen=('adam', dict(lr=0.0025, betas=[0, 0.99], eps=1e-8)), optim_disc=('adam', dict(lr=0.0025, betas=[0, 0.99], eps=1e-8)),
                 g_reg_interval=16, d_reg_interval=4, n_dis=1, batch=64, batch_gpu=32, ema_kimg=10., ema_rampup=None, use_ema=True,
                 world_size=1, rank=0, process_group=None, seed=0,
                 augment_kwargs=None, augment_type='sg2_ada', augment_p=0.0, ada_target=None, ada_interval=4, ada_kimg=500):
        self.device = torch.device(device)
        self.rank, self.world_size = rank, world_size
        self.batch, self.batch_gpu = batch, batch_gpu
        assert batch % batch_gpu == 0
        self.ema_kimg, self.ema_rampup, self.use_ema = ema_kimg, ema_rampup, use_ema
        self.cur_nimg = 0
        self.batch_idx = 0
        self._round_plan = {}
        self._round_proven = set()  # merged-round plans that have run once without exhausting device memory
        self._count_nonfinite = False
        self.comm_stats = None      # bench.py: {phase: dict(pairs=[event pairs around waits for exchanges], nonfinite=device counter)}
        self.time_phases = False            # a device-event pair around every executed phase (reference :730, :749); nothing on a CPU device
        self.report_grad_health = False     # Grad/<phase>/{norm, absmax, nonfinite} after every phase's finish(): device scalars, no sync (set_grad_health)
        self._phase_events = {}             # phase name -> (start, end): the pair of the phase's latest execution
        self.layer_health = False           # per-parameter gradient and update health into running device tables (set_layer_health)
        self._layer_health, self._layer_health_t = {}, {}      # phase name -> its tables; id(optimizer) -> steps taken, counted on the host

        torch.manual_seed(seed * max(world_size, 1) + rank)     # reference :507-508
        self.G = generators[generator](**(gen_kwargs or {})).train().requires_grad_(False).to(self.device)
        self.D = discriminators[discriminator](**(disc_kwargs or {})).train().requires_grad_(False).to(self.device)
        self.G_ema = copy.deepcopy(self.G).eval() if use_ema else None
        self.z_dim = self.G.z_dim
        self.c_dim = self.G.c_dim or 0

        # data-parallel wrappers (broadcast rank 0's weights, own the gradient buckets)
        self.sg2 = (loss_arch == 'sg2')
        dp = dict(world_size=world_size, process_group=process_group)
        if self.sg2:
            self.dp_modules = dict(G_mapping=GradReducer(self.G.mapping, **dp), G_synthesis=GradReducer(self.G.synthesis, **dp),
                                   D=GradReducer(self.D, **dp))
            la = dict(G_mapping=self.dp_modules['G_mapping'], G_synthesis=self.dp_modules['G_synthesis'])
        else:
            self.dp_modules = dict(G=GradReducer(self.G, **dp), D=GradReducer(self.D, **dp))
            la = dict(G=self.dp_modules['G'])
        la.update(loss_arch_kwargs or {})
        if self.G_ema is not None:      # G now holds rank 0's weights (the wrappers broadcast them): the average starts from those on every rank
            misc.copy_params_and_buffers(self.G, self.G_ema, require_all=True)

        # discriminator augmentation + the ADA heuristic's statistics (reference trainers.py:575-584)
        self.augment_pipe, self.ada_stats = None, None
        self.ada_target, self.ada_interval, self.ada_kimg = ada_target, ada_interval, ada_kimg
        if augment_kwargs is not None and (augment_p > 0 or ada_target is not None):
            from .augmentations import augmentations
            self.augment_pipe = augmentations[augment_type](**augment_kwargs).train().requires_grad_(False).to(self.device)
            self.augment_pipe.p.copy_(torch.as_tensor(float(augment_p)))
            if ada_target is not None:
                self.ada_stats = training_stats.Collector(regex='Loss/signs/real')        # kept for reporting parity (reference :584)
                # The reference reads E[sign(D(real))] through that collector: a host synchronisation every `ada_interval` iterations
                # that drains the launch queue.  Here the running [count, sum] of the reported signs stays on the device and the
                # adjustment of `p` is computed there; SBG_ADA_SYNC=1 restores the synchronous path.
                self._ada_sync = os.environ.get('SBG_ADA_SYNC', '0') == '1' or self.device.type != 'cuda'
                if not self._ada_sync:
                    self._ada_acc = torch.zeros([2], dtype=torch.float64, device=self.device)
                    def tap(v, acc=self._ada_acc):
                        if v.device == acc.device:
                            acc.add_(torch.stack([torch.full([], float(v.numel()), dtype=torch.float64, device=v.device), v.sum(dtype=torch.float64)]))
                    self._ada_tap = training_stats.add_tap('Loss/signs/real', tap)
                    self._ada_adopt_at = None                   # iteration at whose start the pipe adopts the announced strength
            la['augment_pipe'] = self.augment_pipe
        # the fused training-time synthesis layers are first order only: the loss orchestration switches them off for the passes of a generator
        # regulariser (path length differentiates G twice) and on for every other pass (losses_base.accumulate_gradients)
        from ..torch_utils.ops import modconv
        modconv.enabled = True
        self.loss = losses_arch[loss_arch](device=self.device, gen_regs=list(gen_regs), dis_regs=list(dis_regs),
                                           D=self.dp_modules['D'], loss=loss, **la)

        # phases (reference :601-633).  The branch is on the interval alone: with an interval > 0 a 'reg' phase slot exists (and the
        # optimizer's lr / betas are rescaled for it) whether or not a regulariser is configured -- the headline sg2ada.yaml has
        # g_reg_interval = 16 and no generator regulariser, and trains G with lr * 16/17.  A slot whose program is empty draws its
        # latents like any other phase and does nothing else (the reference's optimizer step sees no gradients there and skips).
        # `n_dis` stretches only the un-split 'Gboth' phase (:609-610, :618).
        self.phases = []
        g_reducers = [self.dp_modules[k] for k in self.dp_modules if k.startswith('G')]
        for name, module, reducers, (opt_name, opt_kwargs), interval, both_interval in [
                ('G', self.G, g_reducers, optim_gen, g_reg_interval, int(n_dis)),
                ('D', self.D, [self.dp_modules['D']], optim_disc, d_reg_interval, 1)]:
            if interval is None or interval <= 0:
                opt = optimizers[opt_name](params=module.parameters(), **dict(opt_kwargs))
                slots = [(name + 'both', both_interval)]
            else:
                opt = optimizers[opt_name](params=module.parameters(), **lazy_reg_opt_kwargs(dict(opt_kwargs), interval))
                slots = [(name + 'main', 1), (name + 'reg', int(interval))]
            for phase_name, phase_interval in slots:
                self.phases.append(EasyDict(name=phase_name, module=module, reducers=reducers, opt=opt, interval=phase_interval,
                                            idle=len(self.loss.program(phase_name)) == 0))

    def close(self):
        """detach from process-wide hooks (the statistics tap of the ADA heuristic) so that a later engine starts clean"""
        tap = getattr(self, '_ada_tap', None)
        if tap is not None:
            training_stats.remove_tap('Loss/signs/real', tap)
            self._ada_tap = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------------------------------------------------
    def train_iteration(self, real_img, real_c, all_gen_z=None, all_gen_c=None):
        """real_img: [batch, C, H, W] float in [-1, 1] on the device; real_c: [batch, c_dim].  One pass over the phases."""
        assert real_img.shape[0] == self.batch
        if getattr(self, '_ada_adopt_at', None) is not None and self.batch_idx >= self._ada_adopt_at:
            self.augment_pipe.adopt_strength()
            self._ada_adopt_at = None
        n_phase = len(self.phases)
        if all_gen_z is None:
            all_gen_z = torch.randn([n_phase * self.batch, self.z_dim], device=self.device)
        if all_gen_c is None:
            all_gen_c = real_c.repeat(n_phase, 1) if real_c is not None and real_c.numel() else torch.zeros([n_phase * self.batch, self.c_dim], device=self.device)
        reals = real_img.split(self.batch_gpu)
        real_cs = (real_c if real_c is not None else torch.zeros([self.batch, self.c_dim], device=self.device)).split(self.batch_gpu)
        zs = [z.split(self.batch_gpu) for z in all_gen_z.split(self.batch)]
        cs = [c.split(self.batch_gpu) for c in all_gen_c.split(self.batch)]
        rounds = self.batch // self.batch_gpu

        for phase, phase_z, phase_c in zip(self.phases, zs, cs):
            if phase.idle or self.batch_idx % phase.interval != 0:
                continue
            events = None
            if self.time_phases and self.device.type == 'cuda':
                events = self._phase_events.get(phase.name) or (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                self._phase_events[phase.name] = None       # not readable until the end event is recorded
                events[0].record(torch.cuda.current_stream(self.device))
            with torch.autograd.profiler.record_function(phase.name):
                for r in phase.reducers:
                    r.zero_grad()
                phase.module.requires_grad_(True)
                merged = self._rounds_in_one_pass(phase.name, rounds)
                if merged:
                    # every loss term is a mean over the pass: the mean over `rounds` rounds times `rounds` is the sum of the rounds' means
                    mapping = getattr(self.G, 'mapping', None)
                    first_try = (phase.name, rounds) not in self._round_proven
                    w_avg0 = mapping.w_avg.clone() if first_try and mapping is not None and hasattr(mapping, 'w_avg') else None
                    if mapping is not None:
                        mapping.w_avg_rounds = rounds
                    try:
                        self.loss.accumulate_gradients(phase=phase.name, real_img=real_img, real_c=torch.cat(real_cs), gen_z=torch.cat(phase_z),
                                                       gen_c=torch.cat(phase_c), sync=True, gain=phase.interval * rounds, segments=rounds)
                        self._round_proven.add((phase.name, rounds))
                    except torch.OutOfMemoryError:
                        # `batch_gpu` is the config's memory knob: a run whose rounds fit one at a time must not die because they were merged.
                        # Only the first attempt of a plan may fall back (afterwards the plan is known to fit and an OOM is a real one).
                        if not first_try:
                            raise
                        merged = False
                        self._round_plan[(phase.name, rounds)] = False
                        for r in phase.reducers:
                            r.finish(nan_to_num=False, reduce=False); r.zero_grad()
                        if w_avg0 is not None:
                            mapping.w_avg.copy_(w_avg0)
                        torch.cuda.empty_cache()
                    finally:
                        if mapping is not None:
                            mapping.w_avg_rounds = 1
                if not merged:
                    for round_idx, (img, c, z, gc) in enumerate(zip(reals, real_cs, phase_z, phase_c)):
                        sync = (round_idx == rounds - 1)
                        self.loss.accumulate_gradients(phase=phase.name, real_img=img, real_c=c, gen_z=z, gen_c=gc, sync=sync, gain=phase.interval)
                phase.module.requires_grad_(False)
            with torch.autograd.profiler.record_function(phase.name + '_opt'):
                st = self.comm_stats.setdefault(phase.name, dict(pairs=[], nonfinite=torch.zeros([], dtype=torch.int64, device=self.device), runs=0)) \
                    if self.comm_stats is not None else None
                lh = self._layer_health[phase.name] if self.layer_health else None
                for i, r in enumerate(phase.reducers):
                    if st is not None and self._count_nonfinite:
                        r.nonfinite = st['nonfinite']
                    if lh is not None:      # the reducer folds into this phase's rows of the running table
                        r.health_running = lh.running[lh.row0[i]:lh.row0[i + 1]]
                    r.finish()              # wait for the all-reduce, average, nan_to_num (reference :745-747)
                    if st is not None:
                        st['pairs'].extend(r.timing or []); r.timing = []
                        r.nonfinite = None
                if st is not None:
                    st['runs'] += 1
                if self.report_grad_health:
                    self._report_grad_health(phase)
                phase.opt.step()
                if self.layer_health:
                    self._layer_health_update(phase)
            if events is not None:
                events[1].record(torch.cuda.current_stream(self.device))
                self._phase_events[phase.name] = events

        if self.G_ema is not None:
            with torch.autograd.profiler.record_function('Gema'):
                self.update_ema()
        self.cur_nimg += self.batch * self.world_size
        self.batch_idx += 1

        # ADA heuristic (reference :768-771): nudge the strength so that E[sign(D(real))] tracks `ada_target`
        if self.ada_stats is not None and self.batch_idx % self.ada_interval == 0:
            step = (self.batch * self.world_size * self.ada_interval) / (self.ada_kimg * 1000)
            if self._ada_sync:
                self.ada_stats.update()
                adjust = np.sign(self.ada_stats['Loss/signs/real'] - self.ada_target) * step
                self.augment_pipe.p.copy_((self.augment_pipe.p + adjust).clamp_(min=0))
            else:
                acc = self._ada_acc
                if self.world_size > 1:
                    torch.distributed.all_reduce(acc)
                mean = acc[1] / acc[0].clamp(min=1)
                adjust = torch.where(acc[0] > 0, torch.sign(mean - self.ada_target) * step, torch.zeros_like(mean))
                self.augment_pipe.p.copy_((self.augment_pipe.p + adjust.to(self.augment_pipe.p.dtype)).clamp_(min=0))
                acc.zero_()
                # the sampler keeps the old strength for exactly one more iteration, then switches (deterministic, identical on all ranks)
                self.augment_pipe.announce_strength_update()
                self._ada_adopt_at = self.batch_idx + 1

    def set_grad_health(self, on=True):
        """switch `report_grad_health` and, with it, the reducers' fused finish that measures the gradients (GradReducer.health)"""
        self.report_grad_health = bool(on)
        for r in self.dp_modules.values():
            r.health = bool(on)

    def set_layer_health(self, on=True):
        """log.layer_health: per parameter and phase, the gradient's size and non-finite count (GradReducer.layer_health, measured before
        nan_to_num erases them) and the size of the optimizer's update against the weight's (torch_utils/ops/layer_health.py), kept in one
        running float64 table [parameters of the phase, 8] per phase on the device until `layer_health_report` reads it.  The update pass
        restates Adam's step from the moments and needs this project's `adam` with amsgrad off, no weight decay, one parameter group and a
        host learning rate; for any other optimizer the update fields stay None (`layer_health_unsupported` names the phases).  The step
        count t of the bias corrections is kept here, per optimizer, read ONCE from the optimizer's own state['step'] -- now, never in
        steady state."""
        self.layer_health = bool(on)
        self._layer_health = {}
        self._layer_health_t = {}
        for r in self.dp_modules.values():
            r.layer_health = bool(on)
            r.health_running = None
        if not on:
            return
        for phase in self.phases:
            if phase.idle:
                continue
            names = {id(p): name for name, p in phase.module.named_parameters()}
            segs = [s for r in phase.reducers for s in r.layer_health_segments()]
            row0 = [0]
            for r in phase.reducers:
                row0.append(row0[-1] + len(r.layer_health_segments()))
            opt, g = phase.opt, phase.opt.param_groups[0]
            why = None
            if type(opt) is not Adam:
                why = f"optimizer {type(opt).__name__}"
            elif len(opt.param_groups) != 1 or g.get('amsgrad') or g.get('weight_decay') or g.get('maximize') or isinstance(g['lr'], torch.Tensor):
                why = "adam with amsgrad, weight decay, maximize, a tensor learning rate or several parameter groups"
            if id(opt) not in self._layer_health_t:
                steps = [opt.state[s.param]['step'] for s in segs if 'step' in opt.state.get(s.param, {})]
                self._layer_health_t[id(opt)] = int(float(steps[0])) if steps else 0
            self._layer_health[phase.name] = EasyDict(names=[names[id(s.param)] for s in segs], numels=[s.n for s in segs], params=[s.param for s in segs],
                                                      row0=row0, running=layer_health.new_running(len(segs), self.device), unsupported=why, table=None)

    @property
    def layer_health_unsupported(self):
        """{phase name: why its update fields are None}"""
        return {name: lh.unsupported for name, lh in self._layer_health.items() if lh.unsupported}

    def _layer_health_update(self, phase):
        """after opt.step(): count the optimizer's step on the host and measure |w| and the update the step just made (see set_layer_health)"""
        opt, lh = phase.opt, self._layer_health[phase.name]
        t = self._layer_health_t[id(opt)] = self._layer_health_t[id(opt)] + 1
        if lh.unsupported:
            return
        g = opt.param_groups[0]
        bc1, bc2 = layer_health.bias_corrections(g['betas'][0], g['betas'][1], t)
        triples = None
        if lh.table is None or self.device.type != 'cuda':
            triples = [(p.detach(), opt.state[p]['exp_avg'], opt.state[p]['exp_avg_sq']) for p in lh.params]
        if self.device.type != 'cuda':
            layer_health.updates_cpu(triples, g['lr'], g['eps'], bc1, bc2, lh.running)
            return
        if lh.table is None:        # the moments exist from the first step on and stay where they are
            lh.table = layer_health.update_table(triples)
        layer_health.updates(lh.table, g['lr'], g['eps'], bc1, bc2, lh.running)

    def layer_health_fetch(self):
        """start the copy of every phase's running table to pinned host memory and zero the tables, without waiting -> an object for
        `layer_health_report` (the tick calls the two around its one host synchronisation)"""
        host, event = {}, None
        for name, lh in self._layer_health.items():
            if lh.running.is_cuda:
                buf = torch.empty(lh.running.shape, dtype=lh.running.dtype, pin_memory=True)
                buf.copy_(lh.running, non_blocking=True)
                host[name] = buf
            else:
                host[name] = lh.running.clone()
            lh.running.zero_()
        if self.device.type == 'cuda':
            event = torch.cuda.Event()
            event.record(torch.cuda.current_stream(self.device))
        return host, event

    def layer_health_report(self, fetched):
        """-> {phase: {steps, params: {name: numbers (layer_health.derive)}, nonfinite_params: [names]}} from a `layer_health_fetch`"""
        host, event = fetched
        if event is not None:
            event.synchronize()
        out = {}
        for name, lh in self._layer_health.items():
            run = host[name].numpy()
            rows = layer_health.derive(run, lh.numels, with_updates=not lh.unsupported)
            out[name] = dict(steps=int(run[:, 0].max()) if len(run) else 0, params=dict(zip(lh.names, rows)),
                             nonfinite_params=[n for n, d in zip(lh.names, rows) if d['nonfinite'] > 0])
        return out

    def _report_grad_health(self, phase):
        """Grad/<phase>/norm = sqrt of the reducers' sums of squares added up, /absmax, /nonfinite (elements that were not finite BEFORE
        nan_to_num replaced them), from the records finish() left on the device (GradReducer.last_health)"""
        health = [r.last_health for r in phase.reducers if r.last_health is not None]
        if not health:
            return
        h = torch.stack(health)
        training_stats.report(f'Grad/{phase.name}/norm', h[:, 1].sum().sqrt())
        training_stats.report(f'Grad/{phase.name}/absmax', h[:, 2].max())
        training_stats.report(f'Grad/{phase.name}/nonfinite', h[:, 0].sum())

    def phase_times(self):
        """{phase name: milliseconds of its latest execution} from the event pairs of `time_phases`; waits for each end event"""
        out = {}
        for name, events in self._phase_events.items():
            if events is not None:
                events[1].synchronize()
                out[name] = events[0].elapsed_time(events[1])
        return out

    def collect_comm_stats(self, on=True, nonfinite=True):
        """bench.py: per phase, the device-event pairs around every wait for a gradient exchange (what backward did not hide) and, with
        `nonfinite`, the number of non-finite gradient elements BEFORE nan_to_num (one more pass over the flat buckets per phase: warm-up
        only).  No host synchronisation; read after torch.cuda.synchronize()."""
        self.comm_stats = {} if on else None
        self._count_nonfinite = bool(nonfinite)
        for r in self.dp_modules.values():
            r.timing = [] if on else None
            r.nonfinite = None

    def _rounds_in_one_pass(self, phase_name, rounds):
        """The accumulation rounds of a phase exist in the reference because a round is what fits its device (`batch_gpu`); here 288 GB hold
        them all, and every network pass carries ~1 ms of fixed cost ("passes per round").  The rounds of a phase are therefore
        evaluated in ONE pass over [round 0; round 1; ...] when that computes the same thing: per-sample-independent networks (StyleGAN2 blocks
        without attention: no batch statistics, no power iterations), the mapping network's running average advanced once per round in order
        (MappingNetwork.w_avg_rounds), minibatch-std groups kept those of the separate rounds (Discriminator.merged_batch_order), stateless
        regularisers, and no tensor of the pass at the op layer's 2 GiB limit.  Same losses, statistics and parameter gradients up to
        summation order; the per-layer noise and the augmentation pipe draw once for the whole pass instead of once per round (same
        distribution).  SBG_MERGE_ROUNDS=0 keeps the rounds apart."""
        if rounds <= 1 or not merge_rounds or not getattr(self.G, 'rounds_mergeable', False):
            return False
        hit = self._round_plan.get((phase_name, rounds))
        if hit is None:
            syn = getattr(self.G, 'synthesis', None)
            fits = syn.pass_plan(rounds * self.batch_gpu) is not None if hasattr(syn, 'pass_plan') else True
            hit = fits and self.loss.rounds_mergeable(phase_name, self.batch_gpu, rounds)
            self._round_plan[(phase_name, rounds)] = hit
        return hit

    # -- snapshot / resume (reference trainers.py:636-656 pickles whole modules; here plain state dicts + counters) ---------
    def state_dict(self):
        """Everything needed to continue the run: networks, the augmentation pipe's strength, optimizer moments (a superset of the
        reference's snapshot, which drops the optimizers) and the progress counters -- tensors and plain containers only, so the file
        loads with ``torch.load(..., weights_only=True)``."""
        opts = {}
        for ph in self.phases:
            opts.setdefault(ph.name[0], ph.opt.state_dict())       # 'G' / 'D': main and lazy-reg phases share one optimizer
        out = dict(G=self.G.state_dict(), D=self.D.state_dict(), optimizers=opts,
                   progress=dict(cur_nimg=int(self.cur_nimg), batch_idx=int(self.batch_idx)))
        if self.G_ema is not None:
            out['G_ema'] = self.G_ema.state_dict()
        if self.augment_pipe is not None:
            out['augment_pipe'] = self.augment_pipe.state_dict()
        return out

    def load_state_dict(self, state, strict=True, networks_only=False):
        """`networks_only`: transfer learning (reference :350-366 -- weights are copied, the schedule restarts)."""
        self.G.load_state_dict(state['G'], strict=strict)
        self.D.load_state_dict(state['D'], strict=strict)
        if self.G_ema is not None:
            self.G_ema.load_state_dict(state.get('G_ema', state['G']), strict=strict)
        if self.augment_pipe is not None and 'augment_pipe' in state and not networks_only:
            self.augment_pipe.load_state_dict(state['augment_pipe'], strict=strict)
            self.augment_pipe._strength()       # un-announced write: read synchronously, the resumed strength applies from the first call
            self._ada_adopt_at = None
        if networks_only:
            return
        for ph in self.phases:
            if ph.name[0] in state.get('optimizers', {}):
                ph.opt.load_state_dict(state['optimizers'][ph.name[0]])
        self.cur_nimg = int(state['progress']['cur_nimg'])
        self.batch_idx = int(state['progress']['batch_idx'])
        if self.layer_health:       # the optimizers' moments are new tensors and their step counts have moved: set up again
            self.set_layer_health(True)

    @torch.no_grad()
    def update_ema(self):
        """G_ema <- lerp(G, G_ema, beta), buffers copied (reference :752-761)"""
        global_batch = self.batch * self.world_size
        ema_nimg = self.ema_kimg * 1000
        if self.ema_rampup is not None:
            ema_nimg = min(ema_nimg, self.cur_nimg * self.ema_rampup)
        beta = 0.5 ** (global_batch / max(ema_nimg, 1e-8))
        p_ema, p = list(self.G_ema.parameters()), list(self.G.parameters())
        torch._foreach_lerp_(p_ema, p, 1.0 - beta)      # p_ema + (p - p_ema) * (1 - beta) == p.lerp(p_ema, beta)
        b_ema, b = list(self.G_ema.buffers()), list(self.G.buffers())
        if b_ema:
            torch._foreach_copy_(b_ema, b)              # one multi-tensor launch instead of one copy per buffer (noise constants, filters, w_avg)


# ----------------------------------------------------------------------------------------------------------------
# Config-driven trainers: the lifecycle `starter.multiprocesses_main` drives (reference starter.py:32-45), over StepEngine.

class SyntheticDataset:
    """Stands in for the reference's ImageFolderDataset (out of scope: the metric uses synthetic reals): uint8 U[0, 255]
    images and uniformly drawn one-hot labels, exposing the properties the trainer reads (train_parts/datasets.py:129-157)."""

    def __init__(self, resolution=32, num_channels=3, num_classes=0, seed=0):
        self.resolution, self.num_channels, self.label_dim = resolution, num_channels, num_classes
        self.image_shape = [num_channels, resolution, resolution]
        self.has_labels = num_classes > 0
        self.seed = int(seed)
        self._gen = torch.Generator().manual_seed(seed)

    # What the snapshot image grid reads (setup_snapshot_image_grid): a nominal size and per-index samples.  Sample `idx` is drawn from
    # a generator of its own, so indexing never moves the stream `batch` draws from.
    nominal_size = 4096

    def __len__(self):
        return self.nominal_size

    def _raw_label(self, idx):
        g = torch.Generator().manual_seed((self.seed * 1000003 + int(idx)) * 2 + 1)
        return int(torch.randint(0, self.label_dim, [1], generator=g)) if self.has_labels else 0

    def get_details(self, idx):
        return EasyDict(raw_idx=int(idx), xflip=False, raw_label=np.asarray(self._raw_label(idx), dtype=np.int64))

    def __getitem__(self, idx):
        """-> (uint8 image [C, H, W], float32 one-hot label [label_dim]) as numpy arrays, like the real data sets"""
        g = torch.Generator().manual_seed((self.seed * 1000003 + int(idx)) * 2)
        img = torch.randint(0, 256, self.image_shape, generator=g, dtype=torch.uint8).numpy()
        label = np.zeros([self.label_dim], dtype=np.float32)
        if self.has_labels:
            label[self._raw_label(idx)] = 1
        return img, label

    def batch(self, n, device):
        img = torch.randint(0, 256, [n] + self.image_shape, generator=self._gen, dtype=torch.uint8).to(device)
        if self.has_labels:
            idx = torch.randint(0, self.label_dim, [n], generator=self._gen)
            c = torch.nn.functional.one_hot(idx, self.label_dim).float().to(device)
        else:
            c = torch.zeros([n, 0], device=device)
        return img, c


def training_set_kwargs_from_config(config, seed, path=None, mirror=None, use_labels=None):
    """the data set constructor's kwargs a run on `config` trains with (reference train.py:230-261: probe the data once, then be explicit
    about resolution / labels / size).  The trainer passes nothing but the seed; calc_metrics, whose snapshots hold no such record,
    overrides the path (--data), the flips (--mirror) and lets the labels follow the network."""
    from .datasets import datasets
    kw = {k: v for k, v in dict(config.get("datasets_args", {}).get(config.data.dataset, {})).items() if k not in ("args", "kwargs") and v != utils.MISSING}
    kw["path"] = config.data.dataset_path if path is None else path
    if use_labels:
        kw["use_labels"] = True         # a conditional network: probe the data set with its labels
    probe = datasets[config.data.dataset](**kw)
    kw.update(resolution=probe.resolution, use_labels=probe.has_labels, max_size=len(probe))
    cond = config.data.cond if use_labels is None else use_labels
    if cond and not kw["use_labels"]:
        raise ValueError("data.cond=true requires labels specified in dataset.json" if use_labels is None else
                         "the network is conditional: the data set needs labels specified in dataset.json")
    if not cond:
        kw["use_labels"] = False
    if config.data.subset:
        if not 1 <= config.data.subset <= kw["max_size"]:
            raise ValueError(f"data.subset must be between 1 and {kw['max_size']}")
        if config.data.subset < kw["max_size"]:
            kw.update(max_size=int(config.data.subset), random_seed=seed)
    if config.data.mirror if mirror is None else mirror:
        kw["xflip"] = True
    probe.close()
    return kw


@trainers.add_to_registry("base")
class BaseTrainer:
    """One data-parallel G / D pair (reference BaseTrainer :155-876, hot path only)."""

    split_generator = False      # SG2Trainer synchronises mapping and synthesis separately

    def __init__(self):
        self.rank = 0
        self.config = None
        self.grid_size = self.grid_z = self.grid_c = None       # the snapshot image grid, set by the first save_image_snapshot
        self.run_capped = True      # starter.multiprocesses_main says whether training_loop gets an iteration cap (log.run_log=auto reads it)
        self.run_log = False        # decided by setup_logs
        self.cur_tick = 0           # the tick in progress
        self.start_time = None
        self._log_txt = self._stats_jsonl = self._layers_jsonl = None
        self.layer_health = False   # log.layer_health: layers.jsonl, one line per tick with every parameter's gradient and update health

    # -- argument assembly / validation (reference :155-395) -----------------------------------------------------------
    def setup_arguments(self, config):
        gen, perf = config.gen, config.perf
        gpus = int(perf.gpus)
        if gpus < 1 or gpus & (gpus - 1):
            raise ValueError("perf.gpus must be a power of two")
        if gen.batch < 1 or gen.batch_gpu < 1:
            raise ValueError("gen.batch and gen.batch_gpu must be set")
        batch_gpu = min(gen.batch_gpu, gen.batch // gpus)
        if gen.batch % gpus != 0 or gen.batch % (gpus * batch_gpu) != 0:
            raise ValueError("gen.batch must be a multiple of perf.gpus * gen.batch_gpu")
        self.aug = self._augment_arguments(config)
        self.real_data = config.data.dataset != "synthetic"
        if self.real_data:
            from .datasets import datasets
            if config.data.dataset not in datasets:
                raise ValueError(f"data.dataset={config.data.dataset}: use 'synthetic' (data.resolution=<R> data.num_classes=<K>) or one of {sorted(datasets.classes)}")
        self.resume_path = None if config.trans.resume == "noresume" else str(config.trans.resume)     # a network-snapshot-*.pt of this build
        if self.resume_path is not None and not os.path.isfile(self.resume_path):
            raise ValueError(f"trans.resume={self.resume_path}: no such snapshot file (named transfer-learning sources are URL fetches and "
                             "reference .pkl snapshots are pickled modules; neither is loaded here -- pass a .pt written by save_snapshot)")
        self.run_dir = os.path.join(str(config.log.output), str(config.exp.name)) if config.exp.get("name", utils.MISSING) != utils.MISSING else None
        mode = config.log.get("run_log", "auto")
        mode = {True: "on", False: "off"}.get(mode, mode) if isinstance(mode, bool) else mode      # yaml reads a bare on / off as a boolean
        if mode not in ("auto", "on", "off"):
            raise ValueError(f"log.run_log={mode}: use auto, on or off")
        self.run_log_mode = mode
        lh = config.log.get("layer_health", "off")
        lh = {True: "on", False: "off"}.get(lh, lh) if isinstance(lh, bool) else lh
        if lh not in ("on", "off"):
            raise ValueError(f"log.layer_health={lh}: use on or off")
        if lh == "on" and mode == "off":
            raise ValueError("log.layer_health=on writes layers.jsonl at the ticks of the run log: it needs log.run_log=on (or auto in a run without an iteration cap)")
        self.layer_health = lh == "on"
        self.kimg_per_tick = float(config.log.kimg_per_tick)
        self.snap_ticks = int(config.log.snap) if config.log.snap else None        # ticks between image / network snapshots of the run log
        self.snapshot_iterations = None     # iterations between snapshots; None = only on request
        self.image_snapshot_iterations = None       # iterations between image snapshots (fakes<kimg>.png); None = only on request
        from ..metrics import metric_main
        self.metrics = [str(m) for m in config.log.get("metrics", [])]      # reference :215-217
        bad = [m for m in self.metrics if not metric_main.is_valid_metric(m)]
        if bad:
            raise ValueError(f"log.metrics contains {bad}; valid: {metric_main.list_valid_metrics()}")
        self.metric_detector = config.log.get("metric_detector", None)      # local TorchScript file (or directory holding the reference's file names)
        self.stats_metrics, self.metrics_time = dict(), 0.0
        self.config = config
        self.num_gpus, self.batch_size, self.batch_gpu = gpus, gen.batch, batch_gpu
        if self.real_data:      # reference :230-261: probe the data once, then be explicit about resolution / labels / size
            from .datasets import datasets
            kw = training_set_kwargs_from_config(config, seed=gen.seed)
            self.training_set_kwargs = kw
            self.data_loader_kwargs = {k: v for k, v in dict(config.get("dataloaders_args", {}).get(config.data.dataloader, {})).items()
                                       if k not in ("args", "kwargs") and v != utils.MISSING}
            if self.data_loader_kwargs.pop("device", None) is not None:     # a loader's `device` is the rank's training device (setup_dataset)
                raise ValueError(f"dataloaders_args.{config.data.dataloader}.device is not a setting: the trainer passes each rank's training device")
            self.dataset = datasets[config.data.dataset](**kw)
        else:
            self.dataset = SyntheticDataset(int(config.data.get("resolution", 32)), 3,
                                            int(config.data.get("num_classes", 0)) if config.data.cond else 0, seed=gen.seed)
        common = dict(c_dim=self.dataset.label_dim, img_resolution=self.dataset.resolution, img_channels=self.dataset.num_channels)
        self.G_kwargs = self._model_kwargs(config.gens_args[gen.generator], common)
        self.D_kwargs = self._model_kwargs(config.discs_args[gen.discriminator], common)
        strip = lambda d: {k: v for k, v in d.items() if k != "params"}
        self.G_opt = (gen.optim_gen, strip(config.optim_gen_args[gen.optim_gen]))
        self.D_opt = (gen.optim_disc, strip(config.optim_disc_args[gen.optim_disc]))
        self.gen_regs = [(name, dict(config.gen_regs_all[name])) for name in gen.gen_regs]
        self.dis_regs = [(name, dict(config.disc_regs_all[name])) for name in gen.disc_regs]
        la = dict(config.losses_arch_args[gen.loss_arch])
        self.loss_arch_kwargs = {k: v for k, v in la.items() if k not in ("args", "G_mapping", "G_synthesis") and v != utils.MISSING}
        self.ema_kimg = config.ema.kimg
        self.ema_rampup = config.ema.ramp if config.ema.ramp >= 0 else None
        self.total_kimg = gen.kimg
        if self.metrics and not (isinstance(self.metric_detector, str) and os.path.exists(self.metric_detector)):
            # the reference fetches its detectors from a URL at the first snapshot; this build never downloads.  A run on a real data set that
            # is configured with metrics (the reference's DEFAULT is [fid50k_full, is50k]) and has nothing to compute them with would train
            # for hours and report nothing: refuse at setup.  Synthetic data has no data set to score against: the metrics are dropped, loudly.
            # Metrics that compute on the data set alone (metric_main.needs_detector: swd16k) run without a detector.
            if self.real_data:
                if any(metric_main.needs_detector(m) for m in self.metrics):
                    raise ValueError(f"log.metrics={self.metrics} needs log.metric_detector=<local TorchScript file or directory holding "
                                     "inception-2015-12-05.pt / vgg16.pt> (detectors are not downloaded in this build); log.metrics=[] turns them off")
            else:
                import warnings
                warnings.warn(f"log.metrics={self.metrics} ignored: data.dataset=synthetic has no data set to score against")
                self.metrics = []
        self._check_ppl_metrics(gen.generator)
        return self

    def _check_ppl_metrics(self, generator):
        """the perceptual-path-length metrics need the VGG16 LPIPS detector and a generator with `mapping` / `synthesis` (reference
        perceptual_path_length.py:57-70): refuse at setup what would fail at the first snapshot"""
        ppl = [m for m in self.metrics if m.startswith(("ppl_", "ppl2_"))]
        if not ppl:
            return
        from ..metrics import metric_utils, perceptual_path_length
        det = self.metric_detector
        if os.path.isdir(det):
            if not os.path.isfile(os.path.join(det, perceptual_path_length.VGG16)):
                raise ValueError(f"log.metrics={ppl} needs the LPIPS detector {perceptual_path_length.VGG16}: log.metric_detector={det} does not hold it")
        elif metric_utils.get_feature_detector_name(det) != metric_utils.get_feature_detector_name(perceptual_path_length.VGG16):
            raise ValueError(f"log.metrics={ppl} needs the LPIPS detector {perceptual_path_length.VGG16}; log.metric_detector={det} is another "
                             "detector (pass a directory holding vgg16.pt)")
        from .generators import Generator
        if not issubclass(generators[generator], Generator):
            raise ValueError(f"log.metrics={ppl} needs a generator with mapping and synthesis networks; gen.generator={generator} has neither")

    @staticmethod
    def _augment_arguments(config):
        """aug.{aug, p, target, augpipe} -> StepEngine keywords (reference :295-335).  The reference looks `aug.augpipe` ('bgc', ...) up
        in a registry that only holds the class name 'sg2_ada' (:335) and fails; the names mean the subsets of
        stylegan2ada/train.py:271-283, which is what is resolved here.  Every registered pipe (`aug.aug_type`) has its own table of
        policy names: 'sg2_ada' those subsets, 'diffaug' the combinations of color / translation / cutout."""
        from .augmentations import augmentations, policy_tables
        aug = config.aug
        out = dict(augment_kwargs=None, augment_type=aug.get("aug_type", "sg2_ada"), augment_p=0.0, ada_target=None, ada_interval=4, ada_kimg=500)
        if aug.aug == "ada":
            out["ada_target"] = 0.6
        elif aug.aug == "fixed":
            if aug.p < 0:
                raise ValueError(f"--aug={aug.aug} requires specifying --p")
        elif aug.aug != "noaug":
            raise ValueError(f"--aug={aug.aug} not supported")
        if aug.p >= 0:
            if aug.aug != "fixed":
                raise ValueError("--p can only be specified with --aug=fixed")
            if not 0 <= aug.p <= 1:
                raise ValueError("--p must be between 0 and 1")
            out["augment_p"] = float(aug.p)
        if aug.target >= 0:
            if aug.aug != "ada":
                raise ValueError("--target can only be specified with --aug=ada")
            if not 0 <= aug.target <= 1:
                raise ValueError("--target must be between 0 and 1")
            out["ada_target"] = float(aug.target)
        if aug.aug != "noaug":
            if out["augment_type"] not in policy_tables:
                raise ValueError(f"aug.aug_type={out['augment_type']} not in {sorted(augmentations.classes)}")
            augpipe_specs = policy_tables[out["augment_type"]]
            if aug.augpipe not in augpipe_specs:
                raise ValueError(f"aug.augpipe={aug.augpipe} not in {sorted(augpipe_specs)} (the policies of aug.aug_type={out['augment_type']})")
            base = config.get("augpipe_specs", {}).get(out["augment_type"], {})        # constructor arguments (std-devs, ranges) from the config
            out["augment_kwargs"] = {**{k: v for k, v in dict(base).items() if k not in ("args", "kwargs")}, **augpipe_specs[aug.augpipe]}
        return out

    @staticmethod
    def _model_kwargs(group, common):
        import inspect
        kw = {k: (dict(v) if isinstance(v, dict) else v) for k, v in group.items() if not (isinstance(v, str) and v == utils.MISSING)}
        kw = {k: v for k, v in kw.items() if k not in ("args", "kwargs")}
        kw.update({k: v for k, v in common.items() if k in group or k in ("c_dim", "img_resolution", "img_channels")})
        return kw

    # -- lifecycle ------------------------------------------------------------------------------------------------------
    def setup_logs(self):
        """log.run_log: `on`, `off`, or `auto` = on exactly when the training loop runs without an iteration cap.  With the run log on,
        rank 0 creates the run directory, prints the banner (reference :418-430) and opens log.txt and stats.jsonl for appending (a
        resumed run continues both files)."""
        self.stats = training_stats.Collector(regex=".*")
        self.start_time = time.time()
        self.run_log = self.run_log_mode == "on" or (self.run_log_mode == "auto" and not self.run_capped)
        if not self.run_log:
            if self.layer_health:
                raise ValueError("log.layer_health=on writes layers.jsonl at the ticks of the run log, and log.run_log=auto keeps no run log in a run with "
                                 "an iteration cap: set log.run_log=on")
            return
        if self.kimg_per_tick <= 0:
            raise ValueError("log.kimg_per_tick must be positive")
        if self.run_dir is None:
            raise ValueError("the run log needs exp.name (the run directory is log.output/exp.name); log.run_log=off turns it off")
        if self.rank != 0:
            return
        os.makedirs(self.run_dir, exist_ok=True)
        self._log_txt = open(os.path.join(self.run_dir, "log.txt"), "at")
        self._stats_jsonl = open(os.path.join(self.run_dir, "stats.jsonl"), "at")
        if self.layer_health:
            self._layers_jsonl = open(os.path.join(self.run_dir, "layers.jsonl"), "at")
        data = self.config.data
        self.log("", "Training options:", *_option_lines(self.config), "",
                 f"Output directory:   {self.run_dir}",
                 f"Training data:      {data.dataset_path if self.real_data else 'synthetic'}",
                 f"Data loader:        {self._loader_line()}",
                 f"Training duration:  {self.total_kimg} kimg",
                 f"Number of GPUs:     {self.num_gpus}",
                 f"Number of images:   {len(self.dataset)}",
                 f"Image resolution:   {self.dataset.resolution}",
                 f"Conditional model:  {bool(self.dataset.has_labels)}",
                 f"Dataset x-flips:    {bool(data.mirror)}", "")

    def _loader_line(self):
        """the banner's loader entry: the registry name, and for the resident loader the size of the store it is about to build"""
        if not self.real_data:
            return "none (synthetic batches)"
        name = str(self.config.data.dataloader)
        if name != "resident":
            return name
        from .dataloaders import resident_footprint
        return f"{name} (store {resident_footprint(self.dataset)[0] / 2 ** 30:.3f} GiB)"

    def log(self, *lines):
        """everything the trainer says: rank 0 prints each line and, with the run log on, appends it to log.txt"""
        if self.rank != 0:
            return
        for line in lines:
            print(line, flush=True)
            if self._log_txt is not None:
                self._log_txt.write(str(line) + "\n")
        if self._log_txt is not None:
            self._log_txt.flush()

    def close_logs(self):
        for fh in (self._log_txt, self._stats_jsonl, self._layers_jsonl):
            if fh is not None:
                fh.close()
        self._log_txt = self._stats_jsonl = self._layers_jsonl = None

    def __getstate__(self):
        state = dict(self.__dict__)     # the trainer crosses to the rank processes before any file is open; never carry a handle
        state["_log_txt"] = state["_stats_jsonl"] = state["_layers_jsonl"] = None
        return state

    def distribute_torch(self, temp_dir):
        if self.num_gpus > 1:
            init_file = os.path.abspath(os.path.join(temp_dir, ".torch_distributed_init"))
            backend = "nccl" if torch.cuda.is_available() else "gloo"
            torch.distributed.init_process_group(backend=backend, init_method=f"file://{init_file}", rank=self.rank, world_size=self.num_gpus)
        sync_device = self.device() if self.num_gpus > 1 else None
        training_stats.init_multiprocessing(rank=self.rank, sync_device=sync_device)

    def device(self):
        return torch.device("cuda", self.rank) if torch.cuda.is_available() else torch.device("cpu")

    def init_params(self):
        seed = self.config.gen.seed
        np.random.seed(seed * self.num_gpus + self.rank)
        torch.manual_seed(seed * self.num_gpus + self.rank)

    def setup_dataset(self):
        """real data: endless rank-sharded stream of uint8 batches (reference :517-524); synthetic batches are drawn on demand"""
        self.training_set_iterator = self.training_image_iterator = None
        if self.real_data:
            from .dataloaders import accepts_device, dataloaders
            sampler = misc.InfiniteSampler(dataset=self.dataset, rank=self.rank, num_replicas=self.num_gpus, seed=self.config.gen.seed)
            loader_class = dataloaders[self.config.data.dataloader]
            if accepts_device(loader_class):        # a loader that delivers device tensors is told the training device
                self.data_loader_kwargs = dict(self.data_loader_kwargs, device=self.device())
            loader = loader_class(dataset=self.dataset, sampler=sampler, batch_size=self.batch_size // self.num_gpus, **self.data_loader_kwargs)
            self.training_set_iterator = iter(loader)
            if hasattr(loader, "batches"):          # normalised fp32 batches straight from the loader (next_images)
                self.training_image_iterator = loader.batches(normalized=True)

    def next_batch(self, n, device):
        """-> (uint8 images [n, C, H, W], float32 labels [n, label_dim]) on `device` (normalisation happens there)"""
        if self.training_set_iterator is None:
            return self.dataset.batch(n, device)
        img, c = next(self.training_set_iterator)
        return img.to(device, non_blocking=True), c.to(device, non_blocking=True)

    def next_images(self, n, device):
        """-> (float32 images [n, C, H, W] in [-1, 1], float32 labels [n, label_dim]) on `device`: what a training iteration is fed.  A
        loader that offers `batches` (the resident one) delivers them normalised; every other source goes through `next_batch` and
        the reference's expression (:716)"""
        if getattr(self, "training_image_iterator", None) is not None:
            img, c = next(self.training_image_iterator)
            return img.to(device, non_blocking=True), c.to(device, non_blocking=True)
        img, c = self.next_batch(n, device)
        return img.to(torch.float32) / 127.5 - 1, c

    def setup_networks(self):
        gen = self.config.gen
        self.engine = StepEngine(self.device(), generator=gen.generator, discriminator=gen.discriminator, gen_kwargs=self.G_kwargs,
                                 disc_kwargs=self.D_kwargs, loss_arch=gen.loss_arch, loss=gen.loss, loss_arch_kwargs=self.loss_arch_kwargs,
                                 gen_regs=self.gen_regs, dis_regs=self.dis_regs, optim_gen=self.G_opt, optim_disc=self.D_opt,
                                 g_reg_interval=gen.g_reg_interval, d_reg_interval=gen.d_reg_interval, n_dis=int(gen.n_dis),
                                 batch=self.batch_size // self.num_gpus, batch_gpu=self.batch_gpu, ema_kimg=self.config.ema.kimg,
                                 ema_rampup=self.ema_rampup, use_ema=self.config.ema.use_ema, world_size=self.num_gpus, rank=self.rank,
                                 seed=gen.seed, **self.aug)
        self.engine.time_phases = self.run_log
        self.engine.set_grad_health(self.run_log)
        if self.layer_health:
            self.engine.set_layer_health(True)
            self.log("Layer health:       layers.jsonl, one line per tick", *[f"Layer health:       {name}: no update fields ({why})"
                                                                               for name, why in self.engine.layer_health_unsupported.items()], "")

    def setup_augmentations(self):
        self.augment_pipe = self.engine.augment_pipe        # built by StepEngine (it owns the loss object the pipe plugs into)
        if self.resume_path is not None:    # networks, pipe and optimizers exist now: continue from the snapshot
            self.resume(self.resume_path)

    def save_snapshot(self, cur_nimg=None, run_dir=None, cur_tick=None):
        """network-snapshot-<kimg>.pt + training_options.json with `start_options` (reference :636-656, :821-832).  Rank 0 writes."""
        run_dir = run_dir or self.run_dir
        assert run_dir is not None, "save_snapshot needs exp.name / log.output or an explicit run_dir"
        cur_nimg = self.engine.cur_nimg if cur_nimg is None else cur_nimg
        path = os.path.join(run_dir, f"network-snapshot-{cur_nimg // 1000:06d}.pt")
        if self.rank == 0:
            os.makedirs(run_dir, exist_ok=True)
            state = self.engine.state_dict()
            start_options = dict(cur_nimg=int(self.engine.cur_nimg), batch_idx=int(self.engine.batch_idx))
            if self.run_log:        # the tick a run resumed from this file starts with (reference :827)
                state["progress"]["cur_tick"] = start_options["cur_tick"] = int(self.cur_tick if cur_tick is None else cur_tick)
            torch.save(state, path)
            options = dict(start_options=start_options,
                           snapshot=os.path.basename(path), num_gpus=self.num_gpus, batch_size=self.batch_size, batch_gpu=self.batch_gpu)
            with open(os.path.join(run_dir, "training_options.json"), "wt") as f:
                json.dump(options, f, indent=2)
        return path

    def evaluate_metrics(self, snapshot_path=None, detector=None, metrics=None):
        """every configured metric on G_ema (G when the average is off) against the training set (reference :659-674).  Unless none of the
        metrics needs one (metric_main.needs_detector), the feature detector must be local (`log.metric_detector=<TorchScript file | directory>` or the `detector` argument: a path or a callable);
        the reference's URL fetch does not exist here, so without one this raises instead of silently skipping."""
        from ..metrics import metric_main
        detector = detector if detector is not None else self.metric_detector
        names = list(self.metrics if metrics is None else metrics)
        if not names:
            return {}
        if not self.real_data:
            raise ValueError("metrics need a real data set (data.dataset=image_folder ...)")
        kw = dict(detector=None, detector_dir=None)
        if callable(detector) or (isinstance(detector, str) and os.path.isfile(detector)):
            kw["detector"] = detector
        elif isinstance(detector, str) and os.path.isdir(detector):
            kw["detector_dir"] = detector
        elif any(metric_main.needs_detector(m) for m in names):
            raise ValueError("no local feature detector: set log.metric_detector=<TorchScript file or directory> (detectors are not downloaded)")
        G = self.engine.G_ema if self.engine.G_ema is not None else self.engine.G
        self.metrics_time = 0.0
        for metric in names:
            result = metric_main.calc_metric(metric=metric, dataset_name=self.config.data.dataset, G=G, dataset_kwargs=self.training_set_kwargs,
                                             num_gpus=self.num_gpus, rank=self.rank, device=self.engine.device, **kw)
            self.metrics_time += result["total_time"]
            if self.rank == 0:
                metric_main.report_metric(result, run_dir=self.run_dir, snapshot_pkl=snapshot_path)
            self.stats_metrics.update(result.results)
        return dict(self.stats_metrics)

    def resume(self, path, networks_only=False):
        state = torch.load(path, map_location=self.engine.device, weights_only=True)
        self.engine.load_state_dict(state, networks_only=networks_only)
        if not networks_only:
            self.cur_tick = int(state["progress"].get("cur_tick", 0))
        if self.num_gpus > 1:       # every rank read the same file; keep the data-parallel invariant explicit
            for module in (self.engine.G, self.engine.D):
                for t in list(module.parameters()) + list(module.buffers()):
                    torch.distributed.broadcast(t.detach(), src=0)
        return state["progress"]

    def distrib_acrros_gpu(self):
        pass        # StepEngine wraps its modules in GradReducer at construction (broadcast of rank 0's weights included)

    def setup_training_phases(self):
        return self.engine.phases

    def export_sample_images(self):
        """reals.png and fakes_init.png at the start of a run (reference :677-696), when image snapshots are switched on"""
        if self.image_snapshot_iterations or self.run_log:
            self.save_image_snapshot()

    def save_image_snapshot(self, run_dir=None):
        """The run's sample images (reference :677-696, :807-815).  The first call picks the grid's real samples, writes reals.png, draws
        the grid's latents `grid_z` (labels `grid_c` from the picked samples) and writes fakes_init.png; every later call writes
        fakes<kimg:06d>.png from the same latents.  Images come from G_ema (G in eval mode when the run keeps no average) with
        noise_mode='const', in `batch_gpu` chunks; on the device each chunk is quantised and tiled straight into the uint8 canvas.  Rank 0
        writes; -> the file written (None on other ranks)."""
        run_dir = run_dir or self.run_dir
        assert run_dir is not None, "save_image_snapshot needs exp.name / log.output or an explicit run_dir"
        if self.rank != 0:
            return None
        from ..torch_utils.ops import image_export
        eng = self.engine
        os.makedirs(run_dir, exist_ok=True)
        first = self.grid_size is None
        if first:
            self.log('Exporting sample images...')
            self.grid_size, images, labels = setup_snapshot_image_grid(training_set=self.dataset)
            save_image_grid(images, os.path.join(run_dir, 'reals.png'), drange=[0, 255], grid_size=self.grid_size)
            self.grid_z = torch.randn([labels.shape[0], eng.z_dim], device=eng.device).split(self.batch_gpu)
            self.grid_c = torch.from_numpy(labels).to(eng.device).split(self.batch_gpu)
        path = os.path.join(run_dir, 'fakes_init.png' if first else f'fakes{eng.cur_nimg // 1000:06d}.png')
        G = eng.G_ema if eng.G_ema is not None else eng.G
        was_training = G.training
        G.eval()
        canvas, cell = None, 0
        with torch.no_grad():
            for z, c in zip(self.grid_z, self.grid_c):
                img = G(z, c, noise_mode='const').to(torch.float32)
                canvas = image_export.tile(img, self.grid_size, 'grid', [-1, 1], canvas=canvas, cell0=cell)
                cell += z.shape[0]
        G.train(was_training)
        write_grid_png(canvas.cpu().numpy(), path)
        return path

    def training_loop(self, max_iterations=None):
        """Iterate until gen.kimg (or the cap).  With the run log on, a tick after the first iteration of a fresh run, then whenever
        log.kimg_per_tick thousand images have passed since the last one, and one at the end (reference :773-776)."""
        eng = self.engine
        total = self.total_kimg * 1000
        if self.run_log:
            self.log(f"Training for {self.total_kimg} kimg...", "")
            self._tick_start_nimg, self._tick_start_time = eng.cur_nimg, time.time()
            self._maintenance_time = self._tick_start_time - self.start_time
        it = 0
        while (max_iterations is None or it < max_iterations) and (total < 0 or eng.cur_nimg < total or it == 0):
            eng.train_iteration(*self.next_images(eng.batch, eng.device))
            it += 1
            if self.snapshot_iterations and it % self.snapshot_iterations == 0:
                path = self.save_snapshot()
                if self.metrics:            # every configured metric after each snapshot, on all ranks (reference :834-836)
                    self.evaluate_metrics(snapshot_path=path)
            if self.image_snapshot_iterations and it % self.image_snapshot_iterations == 0:
                self.save_image_snapshot()
            if self.run_log:
                done = (total >= 0 and eng.cur_nimg >= total) or (max_iterations is not None and it >= max_iterations)
                if done or self.cur_tick == 0 or eng.cur_nimg >= self._tick_start_nimg + self.kimg_per_tick * 1000:
                    self.tick(done)
            if max_iterations is None and total >= 0 and eng.cur_nimg >= total:
                break
        if not self.run_log:        # with the run log the closing tick has made the update: one collective and one host synchronisation per tick
            self.stats.update()
        return it

    def tick(self, done):
        """One tick of the run log, in the reference's order (:778-876): status line, image snapshot, network snapshot, metrics, phase
        times, ONE Collector.update() on all ranks (the tick's host synchronisation), one stats.jsonl line on rank 0, counters."""
        eng = self.engine
        report0 = training_stats.report0
        cur_nimg, cur_tick = eng.cur_nimg, self.cur_tick
        tick_end_time = time.time()
        sec_per_tick = tick_end_time - self._tick_start_time
        sec_per_kimg = sec_per_tick / max(cur_nimg - self._tick_start_nimg, 1) * 1e3
        total_sec = tick_end_time - self.start_time
        kimg_left = max(self.total_kimg - cur_nimg / 1000, 0) if self.total_kimg >= 0 else 0
        snapshots_left = int(kimg_left / self.kimg_per_tick) // (self.snap_ticks or 1) + 1
        on_gpu = eng.device.type == "cuda"
        gpu_mem = torch.cuda.max_memory_allocated(eng.device) / 2 ** 30 if on_gpu else 0.0
        if on_gpu:
            torch.cuda.reset_peak_memory_stats(eng.device)
        augment = float(self.augment_pipe._strength()) if self.augment_pipe is not None else 0.0       # the pipe's host copy: no device read
        fields = [f"tick {report0('Progress/tick', cur_tick):<5d}",
                  f"kimg {report0('Progress/kimg', cur_nimg / 1e3):<8.1f}",
                  f"time {format_time(report0('Timing/total_sec', total_sec)):<12s}",
                  f"time left {format_time(int(kimg_left * sec_per_kimg) + snapshots_left * self.metrics_time):<12s}",
                  f"sec/tick {report0('Timing/sec_per_tick', sec_per_tick):<7.1f}",
                  f"sec/kimg {report0('Timing/sec_per_kimg', sec_per_kimg):<7.2f}",
                  f"maintenance {report0('Timing/maintenance_sec', self._maintenance_time):<6.1f}",
                  f"cpumem {report0('Resources/cpu_mem_gb', cpu_mem_gb()):<6.2f}",
                  f"gpumem {report0('Resources/peak_gpu_mem_gb', gpu_mem):<6.2f}",
                  f"augment {report0('Progress/augment', augment):.3f}"]
        report0('Timing/total_hours', total_sec / (60 * 60))
        report0('Timing/total_days', total_sec / (24 * 60 * 60))
        self.log(' '.join(fields))

        if self.snap_ticks is not None and (done or cur_tick % self.snap_ticks == 0):
            self.save_image_snapshot()
            path = self.save_snapshot(cur_tick=cur_tick + 1)
            if self.metrics:
                self.evaluate_metrics(snapshot_path=path)

        for name, ms in eng.phase_times().items():
            report0('Timing/' + name, ms)
        layers = eng.layer_health_fetch() if self.layer_health else None       # copies in flight; the update below is the wait
        self.stats.update()
        if self._stats_jsonl is not None:
            self._stats_jsonl.write(json.dumps(dict(self.stats.as_dict(), timestamp=time.time())) + "\n")
            self._stats_jsonl.flush()
        if self._layers_jsonl is not None:
            line = dict(tick=cur_tick, kimg=cur_nimg / 1e3, timestamp=time.time(), phases=eng.layer_health_report(layers))
            self._layers_jsonl.write(json.dumps(line, allow_nan=False) + "\n")
            self._layers_jsonl.flush()

        self.cur_tick = cur_tick + 1
        self._tick_start_nimg, self._tick_start_time = cur_nimg, time.time()
        self._maintenance_time = self._tick_start_time - tick_end_time


@trainers.add_to_registry("sg2")
class SG2Trainer(BaseTrainer):
    """StyleGAN2 trainer: the generator's mapping and synthesis networks are separate data-parallel modules (reference :881-893)."""
    split_generator = True
