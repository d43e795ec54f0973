"""Per-parameter gradient and update health (csrc/layer_health.hip): what the run log's ``layers.jsonl`` is made of.

One definition for both devices.  A parameter is a segment of n fp32 elements, read in memory order.

Gradient pass, per element x of a segment and a scale s -- the definition of ``grad_finish``, nothing written back:

    y = x * s            one fp32 multiply, skipped when s == 1
    z = nan -> +0, +inf -> 1e5, -inf -> -1e5, anything else y
    record = [number of non-finite y, sum of z^2 in float64, max |z|]

Update pass, per element, in float64 from the fp32 weight w and Adam moments m, v after ``opt.step()``:

    d = lr * (m / bc1) / (sqrt(v / bc2) + eps)          bc1 = 1 - beta1^t, bc2 = 1 - beta2^t, every operation rounded once
    record = [sum of w^2, max |w|, sum of d^2]

Order of additions: a segment is cut into chunks of 4096 elements counted from its own first element.  Inside a chunk, vector v holds the
elements 4v .. 4v + 3; lane t of 256 adds the elements of its vectors t, t + 256, t + 512, t + 768 in ascending order, ``block_sum`` adds the
lanes.  The fold adds a parameter's chunk records (lane t the records t, t + 256, ..., then ``block_sum``: ``strided_sum_np``) into its row of
the running float64 table ``[P, 8]``, fields ``FIELDS``: the gradient records add to steps, steps_with_nonfinite, nonfinite, grad_sumsq and
maximise grad_absmax; the update records overwrite weight_sumsq and weight_absmax and add to update_sumsq.

``grads`` / ``updates`` run the kernels over a ``Table`` (device tables built once on the host).  ``grads_cpu`` / ``updates_cpu`` are the same
value graph with the same lane order in numpy (``_exact_common``), for CPU buckets and for the tests.  Device inputs that are not dense fp32 are
an error, never a quiet torch path.  ``derive`` turns a running table into the numbers of the log on the host.
"""
import collections
import ctypes
import math

import numpy as np
import torch

from ... import _lib
from . import _exact_common as ec

CHUNK = _lib.LAYER_HEALTH_CHUNK
FIELDS = ("steps", "steps_with_nonfinite", "nonfinite", "grad_sumsq", "grad_absmax", "weight_sumsq", "weight_absmax", "update_sumsq")
NF = len(FIELDS)
assert NF == _lib.LAYER_HEALTH_FIELDS
GRADS, UPDATES = 0, 1       # the fold's modes

Segment = collections.namedtuple("Segment", "name ptr n bucket offset param")


def new_running(num_params, device):
    """an empty running table: float64 [P, 8] of zeros"""
    return torch.zeros([int(num_params), NF], dtype=torch.float64, device=device)


def is_dense(t):
    """does t cover numel() consecutive elements of memory exactly once (dense in some memory format)?"""
    if t.numel() == 0:
        return True
    expect = 1
    for size, stride in sorted(((s, st) for s, st in zip(t.shape, t.stride()) if s != 1), key=lambda p: p[1]):
        if stride != expect:
            return False
        expect *= size
    return True


def memory_order(t):
    """1-d view of a dense tensor's elements in memory order (a channels_last weight is read as it lies, not in index order)"""
    if not is_dense(t):
        raise RuntimeError(f"layer_health: a tensor of shape {tuple(t.shape)} and strides {t.stride()} is not dense in any memory format")
    return torch.as_strided(t, (t.numel(),), (1,), t.storage_offset())


def segments(reducer):
    """the parameters of a GradReducer as segments of its flat gradient buckets, in bucket order -> [Segment(name, ptr, n, bucket, offset,
    param)]: `name` as in reducer.module.named_parameters(), `ptr` the address of the gradient's first element (offsets are the running sums
    of numel(): 4-byte aligned only), `bucket` / `offset` where it starts in reducer._buckets[bucket].flat"""
    names = {id(p): name for name, p in reducer.module.named_parameters()}
    out = []
    for bi, b in enumerate(reducer._buckets):
        off = 0
        for p in b.params:
            out.append(Segment(names[id(p)], b.flat.data_ptr() + off * b.flat.element_size(), p.numel(), bi, off, p))
            off += p.numel()
    return out


class Table:
    """The device tables of one launch over P segments: `segs` int64 [P, K + 1] = {K addresses, n}, `wg` int32 [records, 2] = (segment, chunk),
    `rec_start` int64 [P + 1], and the float64 records the pass writes.  Built once on the host and uploaded; `keep` holds the tensors the
    addresses point into."""

    def __init__(self, ptr_rows, sizes, device, keep=None):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"layer_health.Table: device tables are for a ROCm device (device type 'cuda'), got '{device}'; CPU data goes through grads_cpu / updates_cpu")
        sizes = [int(n) for n in sizes]
        ptr_rows = [tuple(int(a) for a in row) for row in ptr_rows]
        if len(ptr_rows) != len(sizes) or any(n < 0 for n in sizes) or len({len(r) for r in ptr_rows}) > 1:
            raise RuntimeError("layer_health.Table: one row of addresses and one non-negative size per segment")
        if any(a % 4 or (a == 0 and n) for row, n in zip(ptr_rows, sizes) for a in row):
            raise RuntimeError("layer_health.Table: segment addresses must be non-null and 4-byte aligned")
        self.P, self.K, self.device, self.keep = len(sizes), len(ptr_rows[0]) if ptr_rows else 0, device, keep
        self.sizes, self.total_n = sizes, sum(sizes)
        chunks = np.array([-(-n // CHUNK) for n in sizes], dtype=np.int64)
        rec_start = np.concatenate([np.zeros(1, np.int64), np.cumsum(chunks)])
        self.records = int(rec_start[-1])
        wg = np.zeros([self.records, 2], dtype=np.int32)
        wg[:, 0] = np.repeat(np.arange(self.P, dtype=np.int64), chunks)
        wg[:, 1] = np.arange(self.records, dtype=np.int64) - np.repeat(rec_start[:-1], chunks)
        segs = np.array([row + (n,) for row, n in zip(ptr_rows, sizes)], dtype=np.int64).reshape(self.P, self.K + 1)
        self.segs = torch.from_numpy(segs).to(device)
        self.wg = torch.from_numpy(wg).to(device)
        self.rec_start = torch.from_numpy(rec_start).to(device)
        self.out = torch.zeros([max(self.records, 1), 3], dtype=torch.float64, device=device)


def _dense_f32_device(t, what):
    _lib.require_cuda(t, what)
    _lib.require_dtype(t, torch.float32, what)
    if not is_dense(t):
        raise RuntimeError(f"{what}: a tensor of shape {tuple(t.shape)} and strides {t.stride()} is not dense in any memory format")
    return t


def grad_table(segs, device, keep=None):
    """Table of the gradient pass over [Segment] (or any objects with .ptr and .n)"""
    return Table([(s.ptr,) for s in segs], [s.n for s in segs], device, keep=keep)


def buffer_table(flat, sizes):
    """Table of the gradient pass over consecutive segments of `sizes` elements of one dense 1-d fp32 device buffer"""
    _dense_f32_device(flat, "layer_health.buffer_table")
    if flat.ndim != 1 or sum(sizes) > flat.numel():
        raise RuntimeError("layer_health.buffer_table: the segments must lie inside a 1-d buffer")
    offs = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    return Table([(flat.data_ptr() + 4 * int(o),) for o in offs], sizes, flat.device, keep=flat)


def update_table(triples):
    """Table of the update pass over [(w, exp_avg, exp_avg_sq)]: dense fp32 device tensors, the three of a parameter with the same shape and
    strides (the moments are made by zeros_like(w, preserve_format)), read in memory order"""
    rows, sizes = [], []
    for w, m, v in triples:
        for t in (w, m, v):
            _dense_f32_device(t, "layer_health.update_table")
        if not (w.shape == m.shape == v.shape and w.stride() == m.stride() == v.stride() and w.device == m.device == v.device):
            raise RuntimeError(f"layer_health.update_table: a weight of shape {tuple(w.shape)} / strides {w.stride()} and its moments do not share a layout")
        rows.append((w.data_ptr(), m.data_ptr(), v.data_ptr()))
        sizes.append(w.numel())
    if not triples:
        raise RuntimeError("layer_health.update_table: no parameters")
    return Table(rows, sizes, triples[0][0].device, keep=[tuple(t) for t in triples])


def _check_running(table, running, what):
    _lib.require_cuda(running, what)
    _lib.require_dtype(running, torch.float64, what + " (running)")
    if running.shape != (table.P, NF) or not running.is_contiguous() or running.device != table.device:
        raise RuntimeError(f"{what}: running must be a dense float64 [{table.P}, {NF}] on the table's device, got {tuple(running.shape)} on {running.device}")


def _fold(table, mode, running):
    lib = _lib.load()
    _lib.check(lib.sbg_layer_health_fold(table.out.data_ptr(), table.rec_start.data_ptr(), table.P, table.records, mode, running.data_ptr(),
                                         _lib.stream_ptr(table.device)), "sbg_layer_health_fold")


def grads(table, scale, running):
    """the gradient pass over `table` (K = 1) and the fold of its records into `running` [P, 8]: two launches, nothing read back"""
    if table.K != 1:
        raise RuntimeError("layer_health.grads: expects a table of the gradient pass (one address per segment)")
    _check_running(table, running, "layer_health.grads")
    lib = _lib.load()
    _lib.check(lib.sbg_layer_health_grads(table.segs.data_ptr(), table.wg.data_ptr(), table.records, table.total_n, ctypes.c_float(float(scale)),
                                          table.out.data_ptr(), _lib.stream_ptr(table.device)), "sbg_layer_health_grads")
    _fold(table, GRADS, running)
    return running


def updates(table, lr, eps, bc1, bc2, running):
    """the update pass over `table` (K = 3) and the fold of its records into `running` [P, 8]: two launches, nothing read back"""
    if table.K != 3:
        raise RuntimeError("layer_health.updates: expects a table of the update pass (w, exp_avg, exp_avg_sq per segment)")
    _check_running(table, running, "layer_health.updates")
    lib = _lib.load()
    _lib.check(lib.sbg_layer_health_updates(table.segs.data_ptr(), table.wg.data_ptr(), table.records, table.total_n, float(lr), float(eps),
                                            float(bc1), float(bc2), table.out.data_ptr(), _lib.stream_ptr(table.device)), "sbg_layer_health_updates")
    _fold(table, UPDATES, running)
    return running


# -- the same value graph on the host -----------------------------------------------------------------------------------------------------
def _chunk_sums(v):
    """float64 [n] (n >= 1) of non-negative terms -> float64 [chunks]: the kernels' order inside every chunk"""
    chunks = -(-v.size // CHUNK)
    x = np.zeros(chunks * CHUNK, dtype=np.float64)
    x[:v.size] = v                                                  # + 0.0 changes nothing
    x = x.reshape(chunks, CHUNK // (ec.NT * 4), ec.NT, 4)           # [chunk, u, lane, element]
    acc = np.zeros([chunks, ec.NT], dtype=np.float64)
    for u in range(x.shape[1]):
        for e in range(4):
            acc = acc + x[:, u, :, e]
    return ec.block_sum_np(acc)


def _segment_sum(v):
    """the sum a segment's running row receives: chunk records in the kernels' order, then the fold's order"""
    return float(ec.strided_sum_np(_chunk_sums(v))) if v.size else 0.0


def _f32_memory(t, what):
    if t.device.type != "cpu":
        raise RuntimeError(f"{what}: tensor is on '{t.device}'; device tensors go through the kernels (grads / updates)")
    _lib.require_dtype(t, torch.float32, what)
    return memory_order(t.detach()).numpy()


def _running_np(running, P, what):
    if running.device.type != "cpu" or running.dtype != torch.float64 or running.shape != (P, NF) or not running.is_contiguous():
        raise RuntimeError(f"{what}: running must be a dense float64 [{P}, {NF}] CPU tensor")
    return running.numpy()


def grads_cpu(views, scale, running):
    """views: one fp32 CPU tensor per parameter (dense, read in memory order; never written).  The gradient pass and its fold, in numpy."""
    run = _running_np(running, len(views), "layer_health.grads_cpu")
    s = np.float32(scale)
    for row, t in zip(run, views):
        x = _f32_memory(t, "layer_health.grads_cpu")
        with np.errstate(all="ignore"):
            y = x * s if s != np.float32(1.0) else x
            bad = ~np.isfinite(y)
            z = np.where(np.isnan(y), np.float32(0.0), np.where(y == np.inf, np.float32(1e5), np.where(y == -np.inf, np.float32(-1e5), y))).astype(np.float32)
        count = float(np.count_nonzero(bad))
        zd = z.astype(np.float64)
        row[0] += 1.0
        row[1] += 1.0 if count > 0 else 0.0
        row[2] += count
        row[3] += _segment_sum(zd * zd)
        row[4] = max(row[4], float(np.abs(z).max()) if z.size else 0.0)
    return running


def updates_cpu(triples, lr, eps, bc1, bc2, running):
    """triples: (w, exp_avg, exp_avg_sq) fp32 CPU tensors per parameter, one layout each.  The update pass and its fold, in numpy."""
    run = _running_np(running, len(triples), "layer_health.updates_cpu")
    lr, eps, bc1, bc2 = (np.float64(a) for a in (lr, eps, bc1, bc2))
    for row, (w, m, v) in zip(run, triples):
        if not (w.shape == m.shape == v.shape and w.stride() == m.stride() == v.stride()):
            raise RuntimeError(f"layer_health.updates_cpu: a weight of shape {tuple(w.shape)} / strides {w.stride()} and its moments do not share a layout")
        wn, mn, vn = (_f32_memory(t, "layer_health.updates_cpu") for t in (w, m, v))
        wd = wn.astype(np.float64)
        d = lr * (mn.astype(np.float64) / bc1) / (np.sqrt(vn.astype(np.float64) / bc2) + eps)
        row[5] = _segment_sum(wd * wd)
        row[6] = float(np.abs(wn).max()) if wn.size else 0.0
        row[7] += _segment_sum(d * d)
    return running


def bias_corrections(beta1, beta2, t):
    """(1 - beta1^t, 1 - beta2^t) on the host, as torch.optim.Adam computes them (Python floats)"""
    return 1.0 - float(beta1) ** int(t), 1.0 - float(beta2) ** int(t)


def _num(x):
    return float(x) if x is not None and math.isfinite(x) else None


def derive(running, numels, with_updates=True):
    """running [P, 8] (any device; this reads it) and the parameters' sizes -> one dict per parameter, float64 on the host:
    numel, grad_rms (per element, over the steps), grad_absmax, nonfinite, steps_with_nonfinite, weight_rms, weight_absmax, update_ratio =
    sqrt(update_sumsq / steps) / sqrt(weight_sumsq).  A number that does not exist is None: everything but the counts without a step, the
    weight and update fields without an update pass (`with_updates=False`), update_ratio with a weight norm of 0."""
    run = running.detach().cpu().numpy() if isinstance(running, torch.Tensor) else np.asarray(running, dtype=np.float64)
    out = []
    for row, n in zip(run, numels):
        steps, n = float(row[0]), int(n)
        some = steps > 0 and n > 0
        d = dict(numel=n,
                 grad_rms=_num(math.sqrt(row[3] / (steps * n))) if some else None,
                 grad_absmax=_num(float(row[4])) if some else None,
                 nonfinite=int(row[2]), steps_with_nonfinite=int(row[1]),
                 weight_rms=None, weight_absmax=None, update_ratio=None)
        if with_updates and some:
            d["weight_rms"] = _num(math.sqrt(row[5] / n))
            d["weight_absmax"] = _num(float(row[6]))
            if row[5] > 0:
                d["update_ratio"] = _num(math.sqrt(row[7] / steps) / math.sqrt(row[5]))
        out.append(d)
    return out
