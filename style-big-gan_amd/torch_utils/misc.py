"""Host-side helpers shared by the models and the trainer.

Counterparts of the functions the hot path uses from ``stylegan2ada/torch_utils/misc.py``: ``assert_shape`` (:80),
``profiled_function`` (:98), ``InfiniteSampler`` (:109), ``params_and_buffers`` / ``copy_params_and_buffers``
(:145-163), ``ddp_sync`` (:167), ``check_ddp_consistency`` (:179) and ``print_module_summary`` (:193).  ``ddp_sync`` understands both
torch's DistributedDataParallel and this package's ``parallel.GradReducer`` wrapper.  ``module_summary`` returns the entries the summary
table is printed from (network_summary.py adds its numerics columns to them).
"""
import contextlib
import re

import numpy as np
import torch


def assert_shape(tensor, ref_shape):
    if tensor.ndim != len(ref_shape):
        raise AssertionError(f"Wrong number of dimensions: got {tensor.ndim}, expected {len(ref_shape)}")
    for idx, (size, ref) in enumerate(zip(tensor.shape, ref_shape)):
        if ref is not None and int(size) != int(ref):
            raise AssertionError(f"Wrong size for dimension {idx}: got {size}, expected {ref}")


def profiled_function(fn):
    """run `fn` inside a record_function scope named after it (shows up as a roctx range under rocprofv3)"""
    def wrapper(*args, **kwargs):
        with torch.autograd.profiler.record_function(fn.__name__):
            return fn(*args, **kwargs)
    wrapper.__name__ = fn.__name__
    return wrapper


class InfiniteSampler(torch.utils.data.Sampler):
    """Endless shuffled index stream, sharded by rank, with windowed re-shuffling (reference misc.py:109-140)."""

    def __init__(self, dataset, rank=0, num_replicas=1, shuffle=True, seed=0, window_size=0.5):
        assert len(dataset) > 0 and num_replicas > 0 and 0 <= rank < num_replicas and 0 <= window_size <= 1
        super().__init__()
        self.dataset, self.rank, self.num_replicas = dataset, rank, num_replicas
        self.shuffle, self.seed, self.window_size = shuffle, seed, window_size

    def __iter__(self):
        order = np.arange(len(self.dataset))
        rnd, window = None, 0
        if self.shuffle:
            rnd = np.random.RandomState(self.seed)
            rnd.shuffle(order)
            window = int(np.rint(order.size * self.window_size))
        idx = 0
        while True:
            i = idx % order.size
            if idx % self.num_replicas == self.rank:
                yield order[i]
            if window >= 2:
                j = (i - rnd.randint(window)) % order.size
                order[i], order[j] = order[j], order[i]
            idx += 1


def params_and_buffers(module):
    assert isinstance(module, torch.nn.Module)
    return list(module.parameters()) + list(module.buffers())


def named_params_and_buffers(module):
    assert isinstance(module, torch.nn.Module)
    return list(module.named_parameters()) + list(module.named_buffers())


def copy_params_and_buffers(src_module, dst_module, require_all=False):
    src = dict(named_params_and_buffers(src_module))
    for name, tensor in named_params_and_buffers(dst_module):
        assert (name in src) or (not require_all)
        if name in src:
            tensor.copy_(src[name].detach()).requires_grad_(tensor.requires_grad)


@contextlib.contextmanager
def ddp_sync(module, sync):
    """Suppress the gradient all-reduce of a data-parallel wrapper unless `sync` (reference misc.py:167-174)."""
    assert isinstance(module, torch.nn.Module)
    if sync or not hasattr(module, "no_sync"):
        yield
    else:
        with module.no_sync():
            yield


def check_ddp_consistency(module, ignore_regex=None):
    """Assert that every parameter / buffer equals rank 0's copy (reference misc.py:179-188)."""
    assert isinstance(module, torch.nn.Module)
    for name, tensor in named_params_and_buffers(module):
        fullname = type(module).__name__ + "." + name
        if ignore_regex is not None and re.fullmatch(ignore_regex, fullname):
            continue
        tensor = tensor.detach()
        other = tensor.clone()
        torch.distributed.broadcast(tensor=other, src=0)
        assert (torch.nan_to_num(tensor) == torch.nan_to_num(other)).all(), fullname


class _Cat0(torch.autograd.Function):
    """torch.cat(tensors) along the batch axis as plain slice copies into one allocation.  aten's batched cat kernel moves a [128, 3, 256, 256]
    16-bit batch at ~125 GB/s on MI355X (815 us of a 111 ms step, profiles/r03b_kernel_stats.csv); a slice copy runs at the copy ceiling.
    Differentiable to any order (backward = views of the incoming gradient, themselves differentiable)."""

    @staticmethod
    def forward(ctx, *tensors):
        ctx.sizes = [t.shape[0] for t in tensors]
        first = tensors[0]
        fmt = torch.channels_last if (first.ndim == 4 and first.is_contiguous(memory_format=torch.channels_last) and not first.is_contiguous()) else torch.contiguous_format
        out = torch.empty([sum(ctx.sizes), *first.shape[1:]], dtype=first.dtype, device=first.device, memory_format=fmt)
        i = 0
        for t in tensors:
            out.narrow(0, i, t.shape[0]).copy_(t)
            i += t.shape[0]
        return out

    @staticmethod
    def backward(ctx, dout):
        return tuple(dout.split(ctx.sizes))


def cat0(tensors):
    """torch.cat(tensors, dim=0) for same-dtype tensors of equal trailing shape (see _Cat0); one tensor is returned as it is"""
    tensors = list(tensors)
    if len(tensors) == 1:
        return tensors[0]
    if any(t.dtype != tensors[0].dtype or t.shape[1:] != tensors[0].shape[1:] for t in tensors) or tensors[0].device.type != 'cuda':
        return torch.cat(tensors)
    return _Cat0.apply(*tensors)



class SummaryEntry:
    """one row group of the module summary: a module that ran, its name in the summarised module ('<top-level>' for the module itself), the
    element counts of the parameters and buffers no earlier entry owned, and the tensors it returned (`outputs`; `new_outputs` are those no
    earlier entry returned)"""

    def __init__(self, module, name, outputs):
        self.module, self.name, self.outputs = module, name, outputs
        self.params = self.buffers = 0
        self.new_outputs = []

    @property
    def redundant(self):
        return not (self.params or self.buffers or self.new_outputs)

    def labels(self):
        """the row names: the entry's name, with ':0', ':1', ... when it returned several tensors"""
        return [self.name] if len(self.outputs) < 2 else [f'{self.name}:{i}' for i in range(len(self.outputs))]


def module_summary(module, inputs, max_nesting=3, skip_redundant=True, visit=None):
    """Run `module(*inputs)` once with hooks on every submodule -> (entries, outputs): a SummaryEntry for every module call nested at most
    `max_nesting` deep, in the order the calls RETURNED (children before their parent, the module itself last).  A parameter, buffer or
    output tensor is counted by the first entry that holds it, so a shared parameter is counted once and the totals are those of the module.
    With `skip_redundant`, entries that own nothing new (no parameter, no buffer, no output that was not seen before) are dropped.  The
    forward draws from the random generators if the module does: callers that train afterwards must not call this first.
    `visit(index, entry)` is called from the module's forward hook the moment a call returns -- before a later in-place layer can change the
    tensor -- with the entry's index among ALL entries (those `skip_redundant` drops included; two forwards of one control flow number
    their calls alike)."""
    if not isinstance(module, torch.nn.Module) or isinstance(module, torch.jit.ScriptModule):
        raise TypeError('module_summary: expects an eager torch.nn.Module')
    if not isinstance(inputs, (tuple, list)):
        raise TypeError('module_summary: inputs must be a tuple or list of the positional arguments')
    names = {m: name for name, m in module.named_modules()}
    depth = 0
    entries = []

    def entering(_module, _args):
        nonlocal depth
        depth += 1

    def leaving(mod, _args, result):
        nonlocal depth
        depth -= 1
        if depth <= max_nesting:
            results = result if isinstance(result, (tuple, list)) else [result]
            entries.append(SummaryEntry(mod, '<top-level>' if mod is module else names[mod], [t for t in results if isinstance(t, torch.Tensor)]))
            if visit is not None:
                visit(len(entries) - 1, entries[-1])

    handles = []
    for m in module.modules():
        handles += [m.register_forward_pre_hook(entering), m.register_forward_hook(leaving)]
    try:
        outputs = module(*inputs)
    finally:
        for h in handles:
            h.remove()

    seen = set()
    for e in entries:
        for attr, tensors in (('params', e.module.parameters()), ('buffers', e.module.buffers())):
            fresh = [t for t in tensors if id(t) not in seen]
            seen.update(id(t) for t in fresh)
            setattr(e, attr, sum(t.numel() for t in fresh))
        e.new_outputs = [t for t in e.outputs if id(t) not in seen]
        seen.update(id(t) for t in e.new_outputs)
    if skip_redundant:
        entries = [e for e in entries if not e.redundant]
    return entries, outputs


def summary_rows(module, entries):
    """-> the table's cells: header, rule, one row per output of every entry (an entry without a tensor output gets one row of dashes), rule,
    totals.  Every row of an entry shows the SHAPE OF THE ENTRY'S FIRST OUTPUT, as the reference's table does (its :239 reads outputs[0]
    for every row); the dtype is each output's own.  network_summary.py writes the true shapes to summary.json."""
    header = [type(module).__name__, 'Parameters', 'Buffers', 'Output shape', 'Datatype']
    rows = [header, ['---'] * len(header)]
    for e in entries:
        first = [str(e.params) if e.params else '-', str(e.buffers) if e.buffers else '-']
        if not e.outputs:
            rows.append([e.name] + first + ['-', '-'])
        for i, (label, t) in enumerate(zip(e.labels(), e.outputs)):
            rows.append([label] + (first if i == 0 else ['-', '-']) + [str(list(e.outputs[0].shape)), str(t.dtype).split('.')[-1]])
    rows.append(['---'] * len(header))
    rows.append(['Total', str(sum(e.params for e in entries)), str(sum(e.buffers for e in entries)), '-', '-'])
    return rows


def format_table(rows):
    """cells -> lines: two-space gaps, every cell padded to its column's width (trailing spaces included)"""
    widths = [max(len(row[i]) for row in rows) for i in range(len(rows[0]))]
    return ['  '.join(cell.ljust(width) for cell, width in zip(row, widths)) for row in rows]


def print_module_summary(module, inputs, max_nesting=3, skip_redundant=True):
    """Print the per-layer table of the reference (torch_utils/misc.py :193: class name, Parameters, Buffers, Output shape, Datatype; a blank
    line before and after) for one forward of `module(*inputs)` and return the module's outputs."""
    entries, outputs = module_summary(module, inputs, max_nesting=max_nesting, skip_redundant=skip_redundant)
    print()
    for line in format_table(summary_rows(module, entries)):
        print(line)
    print()
    return outputs
