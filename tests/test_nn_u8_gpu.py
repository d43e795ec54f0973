"""The exact uint8 nearest-row kernels (csrc/nn_u8.hip) against the numpy oracle of nn_u8_util, bit for bit: small and ragged shapes with
planted ties, the i32 accumulator's range, the largest row length, several tiles per workgroup and several runs, `exclude`,
determinism and the refusals.  The data is asymmetric (Q != M, random full-range bytes), which settles rows against columns."""
import itertools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import style_big_gan_amd  # noqa: E401,F401
from style_big_gan_amd import _lib
from style_big_gan_amd.torch_utils.ops import nn_u8
import knn_manifold_util
import nn_u8_util as U

pytestmark = pytest.mark.gpu


def _logged(fn):
    """run fn with the launch log on -> (its result, [(variant, dims)] of every nn_u8 launch it made)"""
    _lib.prof_enable(True)
    try:
        _lib.prof_fetch()
        out = fn()
        return out, [(_lib.NN_VARIANTS[r["dims"][0]], r["dims"]) for r in _lib.prof_fetch() if r["kind"] == "nn_u8"]
    finally:
        _lib.prof_enable(False)


def _dev(a, dev):
    return torch.from_numpy(a).to(dev)


@pytest.mark.parametrize("F", [16, 48, 80, 3072])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_small_and_ragged_shapes(dev, F, k):
    """Q in {1, 37, 300} x M in {k, 130, 260}: fewer rows than a tile, a ragged second tile, a ragged third one; k = 1, 5, 8 take the three
    list lengths.  Copies of earlier rows make ties that must go to the lower index"""
    for Q, M in itertools.product((1, 37, 300), (k, 130, 260)):
        queries, store, planted = U.make_case(Q, M, F, seed=1000 * k + F + Q + M)
        assert M < 100 or planted
        got = nn_u8.topk(_dev(queries, dev), _dev(store, dev), k)
        want = U.oracle_topk(queries, store, k)
        assert U.same(got, want), (Q, M, F, k)
        for a, b in planted:                                    # a query that is a changed copy of row a finds a, then its copy b
            hit = np.nonzero(want[1][:, 0] == a)[0]
            if k > 1 and len(hit):
                assert want[1][hit[0], 1] == b and want[0][hit[0], 0] == want[0][hit[0], 1]


def test_accumulator_range(dev):
    """F = 196608: an all-0 row against an all-0 query is s = +3.2e9 after re-centring, an all-255 row against it s = -3.2e9; either wraps
    an i32 accumulator that is never flushed"""
    Q, M, F, k = 2, 130, 196608, 8
    rng = np.random.RandomState(3)
    store = rng.randint(0, 256, [M, F], dtype=np.uint8)
    queries = rng.randint(0, 256, [Q, F], dtype=np.uint8)
    store[5], store[77], queries[0] = 0, 255, 0
    got = nn_u8.topk(_dev(queries, dev), _dev(store, dev), k)
    assert U.same(got, U.oracle_topk(queries, store, k))
    assert int(got[0][0, 0]) == 0 and int(got[1][0, 0]) == 5
    sub = store[70:78]                                          # all 8 rows are returned: the all-255 row is the last of query 0
    got = nn_u8.topk(_dev(queries, dev), _dev(sub, dev), 8)
    assert U.same(got, U.oracle_topk(queries, sub, 8))
    assert int(got[0][0, 7]) == 196608 * 65025 and int(got[1][0, 7]) == 7


def test_largest_row_length(dev):
    Q, M, F, k = 2, 9, 3 * 1024 * 1024, 8
    rng = np.random.RandomState(4)
    store = rng.randint(0, 256, [M, F], dtype=np.uint8)
    queries = rng.randint(0, 256, [Q, F], dtype=np.uint8)
    store[1], store[6], queries[0] = 255, 0, 0
    q, s = _dev(queries, dev), _dev(store, dev)
    got = nn_u8.topk(q, s, k)
    assert U.same(got, U.oracle_topk(queries, store, k))
    assert int(got[0][0, 0]) == 0 and int(got[1][0, 0]) == 6
    exclude = np.array([2, 3], dtype=np.int32)                  # 8 rows are left: the all-255 row is the last of query 0
    got = nn_u8.topk(q, s, k, _dev(exclude, dev))
    assert U.same(got, U.oracle_topk(queries, store, k, exclude))
    assert int(got[0][0, 7]) == F * 65025 and int(got[1][0, 7]) == 1


@pytest.mark.parametrize("Q,M,F,k,plan", [(37, 200000, 48, 5, "split"), (2100, 13000, 48, 8, "split"), (33000, 300, 48, 3, "single")])
def test_several_tiles_and_runs(dev, Q, M, F, k, plan):
    """one query tile x 391 runs of 4 tiles; 17 query tiles x 26 runs of 4 tiles; 258 query tiles, so one run of 3 tiles.  The same rows
    are planted in different runs (j and j + 4100; j and j + 150 where the store is one run of three tiles)"""
    far = 4100 if M > 8200 else 150
    queries, store, planted = U.make_case(Q, M, F, seed=Q + M, far=far)
    assert any(b - a == far for a, b in planted)
    _, plan_runs, plan_tiles_per_run = knn_manifold_util.plan(Q, M)
    assert plan_runs == {37: 391, 2100: 26, 33000: 1}[Q] and plan_tiles_per_run == (4 if plan == "split" else 3)
    got, log = _logged(lambda: nn_u8.topk(_dev(queries, dev), _dev(store, dev), k))
    want = U.oracle_topk(queries, store, k)
    assert U.same(got, want)
    for a, b in planted:
        hit = np.nonzero(want[1][:, 0] == a)[0]
        assert len(hit) == 0 or want[1][hit[0], 1] == b
    assert [v for v, _ in log] == ["norms", "norms"] + (["split", "merge"] if plan == "split" else ["single"]), log
    dims = log[2][1]
    assert dims[1:5] == (Q, M, F, k)
    runs, tiles = dims[5], (M + 127) // 128
    assert runs == plan_runs and all(d[5] == plan_runs for _, d in log[2:]), log
    assert (runs > 1) == (plan == "split") and (tiles + runs - 1) // runs >= 3, (runs, tiles)
    if plan == "split":
        tiles_per_run = (tiles + runs - 1) // runs
        assert tiles_per_run == plan_tiles_per_run
        assert any(a // (128 * tiles_per_run) != b // (128 * tiles_per_run) for a, b in planted), "no planted pair straddles two runs"


def test_exclude(dev):
    Q, M, F, k = 150, 260, 48, 3
    rng = np.random.RandomState(5)
    store = rng.randint(0, 256, [M, F], dtype=np.uint8)
    store[200], store[31] = store[17], store[140]               # a copy behind and a copy in front of the row itself
    rows = np.concatenate([[17, 200, 140, 31], rng.permutation(M)[:Q - 4]]).astype(np.int32)
    queries = store[rows]
    q, s = _dev(queries, dev), _dev(store, dev)
    d2, idx = nn_u8.topk(q, s, k)
    assert U.same((d2, idx), U.oracle_topk(queries, store, k))
    assert bool((d2[:, 0] == 0).all())
    first = idx[:, 0].cpu().numpy()
    assert first[0] == 17 and first[1] == 17 and first[2] == 31 and first[3] == 31     # ties to the lower row
    assert all(first[i] == rows[i] for i in range(4, Q) if rows[i] not in (17, 200, 140, 31))
    d2, idx = nn_u8.topk(q, s, k, _dev(rows, dev))
    assert U.same((d2, idx), U.oracle_topk(queries, store, k, rows))
    assert [int(v) for v in d2[:4, 0]] == [0, 0, 0, 0] and [int(v) for v in idx[:4, 0]] == [200, 17, 31, 140]
    others = [i for i in range(4, Q) if rows[i] not in (17, 200, 140, 31)]
    assert bool((d2[others, 0] > 0).all()) and not np.any(idx.cpu().numpy() == rows[:, None])
    outside = np.full([Q], -1, dtype=np.int32)                  # rows outside [0, M) exclude nothing
    outside[1::2] = M
    assert U.same(nn_u8.topk(q, s, k, _dev(outside, dev)), U.oracle_topk(queries, store, k))


def test_two_calls_give_the_same_bits(dev):
    queries, store, _ = U.make_case(300, 20000, 80, seed=6, far=4100)
    q, s = _dev(queries, dev), _dev(store, dev)
    (a, log_a), (b, log_b) = _logged(lambda: nn_u8.topk(q, s, 8)), _logged(lambda: nn_u8.topk(q, s, 8))
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert [d for _, d in log_a] == [d for _, d in log_b] and "split" in [v for v, _ in log_a]
    assert U.same(a, U.oracle_topk(queries, store, 8))


def test_images_are_flattened(dev):
    rng = np.random.RandomState(7)
    store = rng.randint(0, 256, [40, 3, 8, 8], dtype=np.uint8)
    queries = rng.randint(0, 256, [5, 3, 8, 8], dtype=np.uint8)
    got = nn_u8.topk(_dev(queries, dev), _dev(store, dev), 4)
    assert U.same(got, U.oracle_topk(queries.reshape(5, -1), store.reshape(40, -1), 4))


def test_refusals(dev):
    q = torch.zeros([4, 48], dtype=torch.uint8, device=dev)
    s = torch.zeros([12, 48], dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="k = 0 neighbours"):
        nn_u8.topk(q, s, 0)
    with pytest.raises(RuntimeError, match="k = 9 neighbours"):
        nn_u8.topk(q, s, 9)
    with pytest.raises(RuntimeError, match="the store has 5 rows"):
        nn_u8.topk(q, s[:5], 6)
    with pytest.raises(RuntimeError, match="one is excluded"):
        nn_u8.topk(q, s[:5], 5, torch.tensor([0, -1, 9, 7], dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="multiple of 16"):
        nn_u8.topk(torch.zeros([4, 40], dtype=torch.uint8, device=dev), torch.zeros([12, 40], dtype=torch.uint8, device=dev), 3)
    with pytest.raises(RuntimeError, match="must be dense"):
        nn_u8.topk(q, torch.zeros([12, 96], dtype=torch.uint8, device=dev)[:, ::2], 3)
    with pytest.raises(RuntimeError, match="queries are on cpu"):
        nn_u8.topk(q.cpu(), s, 3)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        nn_u8.topk(q, torch.zeros([13 * 48 + 8], dtype=torch.uint8, device=dev)[8:8 + 12 * 48].view(12, 48), 3)
    with pytest.raises(RuntimeError, match="must be uint8"):
        nn_u8.topk(q.float(), s, 3)
    lib = _lib.load()                                           # the C entry point refuses on its own, with a message
    out = torch.zeros([64], dtype=torch.int64, device=dev)
    assert lib.sbg_u8_nn_workspace(4, 12, 9) == -1 and lib.sbg_u8_nn_workspace(4, 12, 0) == -1
    for args, message in [((4, 12, 40, 3), "multiple of 16"), ((4, 12, 48, 9), "k = 9"), ((4, 2, 48, 3), "the store has 2 rows")]:
        status = lib.sbg_u8_nn_topk(q.data_ptr(), s.data_ptr(), *args, None, out.data_ptr(), out.data_ptr(), out.data_ptr(), None)
        assert status != 0 and message in lib.sbg_last_error().decode()
    # a store of exactly k rows is searched when `exclude` names no row of it
    got = nn_u8.topk(q, s[:5], 5, torch.tensor([5, -1, 9, 7], dtype=torch.int32, device=dev))
    assert got[1].cpu().tolist() == [[0, 1, 2, 3, 4]] * 4
