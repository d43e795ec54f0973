"""What the layer-health tests share: a plain float64 restatement of the two passes' definitions (numpy sums in numpy's own order, so only the
VALUES are the package's, never its order of additions), inputs with non-finite values sprinkled in, and the checks on a layers.jsonl line."""
import json

import numpy as np

U = 2.0 ** -53              # a float64 sum of n non-negative terms, in any order, is within a relative n * 2^-53 of the exact one
PARAM_KEYS = {"numel", "grad_rms", "grad_absmax", "nonfinite", "steps_with_nonfinite", "weight_rms", "weight_absmax", "update_ratio"}
LENGTHS = [1, 2, 3, 4, 5, 4095, 4096, 4097, 3 * 4096 + 1]     # back to back: offsets 0, 1, 3, 6, 10, 15, 4110, 8206, 12303 -- every residue mod 4


def grads_plain(x, scale):
    """x float32 [n] -> (count, sumsq, absmax) of the gradient pass, by the definition"""
    with np.errstate(all="ignore"):
        y = x * np.float32(scale) if scale != 1.0 else x.copy()
    assert y.dtype == np.float32
    count = int((~np.isfinite(y)).sum())
    z = y.copy()
    z[np.isnan(y)] = 0.0
    z[y == np.inf] = 1e5
    z[y == -np.inf] = -1e5
    zd = z.astype(np.float64)
    return count, float((zd * zd).sum()), float(np.abs(z).max()) if z.size else 0.0


def updates_plain(w, m, v, lr, eps, bc1, bc2):
    """float32 [n] each -> (weight_sumsq, weight_absmax, update_sumsq) of the update pass, by the definition"""
    wd, md, vd = (a.astype(np.float64) for a in (w, m, v))
    d = lr * (md / bc1) / (np.sqrt(vd / bc2) + eps)
    return float((wd * wd).sum()), float(np.abs(w).max()) if w.size else 0.0, float((d * d).sum())


def sprinkled(lengths, seed):
    """float32 [sum(lengths)]: normal values over many binades with NaN, +inf and -inf sprinkled in -- the first and the last element of
    segments included -- and the segments' offsets"""
    rng = np.random.RandomState(seed)
    n = int(sum(lengths))
    x = (rng.randn(n) * np.exp2(rng.randint(-20, 20, size=n))).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum(lengths)])[:-1].astype(np.int64)
    bad = [np.nan, np.inf, -np.inf]
    for i, (o, ln) in enumerate(zip(offs, lengths)):
        if i % 2 == 0:
            x[o] = bad[i % 3]                       # a segment's first element
        if i % 3 != 1:
            x[o + ln - 1] = bad[(i + 1) % 3]        # ... and its last
        if ln > 100:
            x[o + rng.randint(1, ln - 1, size=5)] = np.array(bad + bad[:2], dtype=np.float32)
    return x, offs


def _raise(token):
    raise AssertionError(f"not strict JSON: {token}")


def parse_strict(text):
    return json.loads(text, parse_constant=_raise)


def read_layers(path):
    with open(path) as fh:
        return [parse_strict(ln) for ln in fh]


def check_line(line, tick, phases):
    """the shape of one layers.jsonl line: {phase: [parameter names]} must all be there, every parameter with exactly the documented keys"""
    assert set(line) == {"tick", "kimg", "timestamp", "phases"} and line["tick"] == tick and line["timestamp"] > 0
    assert set(line["phases"]) == set(phases)
    for ph, names in phases.items():
        entry = line["phases"][ph]
        assert set(entry) == {"steps", "params", "nonfinite_params"}
        assert sorted(entry["params"]) == sorted(names), ph
        for name, d in entry["params"].items():
            assert set(d) == PARAM_KEYS, (ph, name)
