"""`knn_manifold.topk` without a device: the torch path against the numpy oracle of knn_topk_util on the small exact shapes, `exclude`, the
refusals that need no device, and the new names in the header, the ctypes table and the library's exports."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

import knn_topk_util as U
from style_big_gan_amd import _lib
from style_big_gan_amd.torch_utils.ops import knn_manifold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("F", [8, 64, 4096])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_cpu_path_equals_the_oracle(F, k):
    for Q, M in itertools.product((1, 37, 300), (k, 130, 260)):
        queries, manifold, planted, want = U.exact_case(Q, M, F, k)
        got = knn_manifold.topk(torch.from_numpy(queries), torch.from_numpy(manifold), k)
        assert U.same(got, want), (Q, M, F, k)


def test_cpu_path_in_row_blocks_and_on_any_width(monkeypatch):
    monkeypatch.setattr(knn_manifold, "_CPU_ROWS", 16)
    for Q, M, F, k in [(37, 130, 7, 2), (70, 260, 44, 8)]:      # the CPU path has no 16-byte pieces: any F
        queries, manifold = U.exact_features(Q, F, seed=1), U.exact_features(M, F, seed=2)
        queries[::4] = manifold[:len(queries[::4])]
        exclude = np.random.RandomState(k).randint(-1, M + 1, size=Q).astype(np.int32)
        exclude[0] = 0
        q, m = torch.from_numpy(queries), torch.from_numpy(manifold)
        assert U.same(knn_manifold.topk(q, m, k), U.oracle_topk(queries, manifold, k))
        got = knn_manifold.topk(q, m, k, torch.from_numpy(exclude))
        assert U.same(got, U.oracle_topk(queries, manifold, k, exclude))
        assert int(got[1][0, 0]) != 0 and not np.any(got[1].numpy() == exclude[:, None])


def test_exclude_skips_one_row_only():
    M, F, k = 260, 64, 3
    manifold = U.exact_features(M, F, seed=5).copy()
    manifold[200], manifold[31] = manifold[17], manifold[140]
    rows = np.array([17, 200, 140, 31], dtype=np.int32)
    q, m = torch.from_numpy(manifold[rows]), torch.from_numpy(manifold)
    d2, idx = knn_manifold.topk(q, m, k)
    assert idx[:, 0].tolist() == [17, 17, 31, 31] and d2[:, 0].tolist() == [0, 0, 0, 0]
    d2, idx = knn_manifold.topk(q, m, k, torch.from_numpy(rows))
    assert idx[:, 0].tolist() == [200, 17, 31, 140] and d2[:, 0].tolist() == [0, 0, 0, 0]
    assert U.same((d2, idx), U.oracle_topk(manifold[rows], manifold, k, rows))
    got = knn_manifold.topk(q, m[:5], 5, torch.tensor([5, -1, 9, 7], dtype=torch.int32))       # M == k, no entry in range
    assert U.same(got, U.oracle_topk(manifold[rows], manifold[:5], 5))


def test_refusals_without_a_device():
    q, m = torch.zeros([4, 48], dtype=torch.float16), torch.zeros([12, 48], dtype=torch.float16)
    for args, message in [((q, m, 0), "k = 0 neighbours"), ((q, m, 9), "k = 9 neighbours"), ((q, m, 2.0), "k = 2.0 neighbours"),
                          ((q, m[:2], 3), "the manifold has 2 rows"), ((q.float(), m.float(), 3), "expects float16"),
                          ((q, m[:, :40], 3), r"expects \[Q, F\] and \[M, F\]"), ((q[0], m, 3), r"expects \[Q, F\] and \[M, F\]"),
                          ((q[:0], m, 3), "empty queries"), ((q.numpy(), m, 3), "torch tensor"),
                          ((q, m, 3, torch.zeros([4], dtype=torch.int64)), "exclude must be an int32"),
                          ((q, m, 3, torch.zeros([5], dtype=torch.int32)), "exclude must be an int32"),
                          ((q, m[:3], 3, torch.tensor([0, 5, 5, 5], dtype=torch.int32)), "one is excluded")]:
        with pytest.raises(RuntimeError, match=message):
            knn_manifold.topk(*args)


def test_new_names_in_header_binding_and_library():
    header = open(os.path.join(ROOT, "include", "sbg_hip.h")).read()
    bound = {name: (restype, argtypes) for name, restype, argtypes in _lib.SYMBOLS}
    assert re.search(r"int64_t\s+sbg_knn_topk_workspace\s*\(\s*int Q, int M, int k\s*\)", header)
    assert re.search(r"\bint\s+sbg_knn_topk\s*\(\s*const void\* queries, const void\* manifold, int Q, int M, int64_t F, int k, const int32_t\* exclude, "
                     r"float\* d2, int32_t\* index,\s*void\* workspace, sbg_stream_t stream\s*\)", header)
    assert bound["sbg_knn_topk_workspace"] == (ctypes.c_int64, [ctypes.c_int] * 3)
    restype, argtypes = bound["sbg_knn_topk"]
    assert restype == ctypes.c_int and len(argtypes) == 11 and argtypes[4] == ctypes.c_int64
    assert callable(knn_manifold.topk) and knn_manifold.MAX_TOPK == 8
    assert "3 top-k" in open(os.path.join(ROOT, "style-big-gan_amd", "_lib.py")).read()
    lib = _lib.load()
    assert lib.sbg_knn_topk is not None
    # the size query needs no device: the norms, and per (row, run) a list of 1 | 4 | 8 64-bit keys when the manifold is split
    assert lib.sbg_knn_topk_workspace(4, 12, 0) == -1 and lib.sbg_knn_topk_workspace(4, 12, 9) == -1
    assert lib.sbg_knn_topk_workspace(300, 100, 5) == 1200 + 400
    ctiles, runs, _ = U.plan(37, 200000)
    for k, KL in ((1, 1), (4, 4), (5, 8), (8, 8)):
        assert lib.sbg_knn_topk_workspace(37, 200000, k) == 160 + 800000 + 8 * 37 * runs * KL
