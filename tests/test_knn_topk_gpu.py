"""The feature-space top-k mode of the k-NN kernels (csrc/knn_manifold.hip, `knn_manifold.topk`) on the device: bit for bit against the numpy
oracle of knn_topk_util on integer features (small and ragged shapes, several tiles per workgroup, several runs, ties across runs),
`exclude`, determinism, real-valued features within the derived summation bound, and the refusals."""
import itertools

import numpy as np
import pytest
import torch

import knn_topk_util as U
from style_big_gan_amd import _lib
from style_big_gan_amd.torch_utils.ops import knn_manifold

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("F", [8, 64, 4096])
@pytest.mark.parametrize("k", [1, 5, 8])
def test_small_and_ragged_shapes(dev, F, k):
    """Q in {1, 37, 300} x M in {k, 130, 260}: fewer rows than a tile, a ragged second tile, a ragged third one; k = 1, 5, 8 take the three
    list lengths.  Values in [-2, 2] at a narrow F give many ties, F = 4096 is the cancellation case; copies of earlier rows and queries
    equal to a stored row make ties at d2 = 0 that must go to the lower row"""
    for Q, M in itertools.product((1, 37, 300), (k, 130, 260)):
        queries, manifold, planted, want = U.exact_case(Q, M, F, k)
        assert M < 100 or planted
        got = knn_manifold.topk(U.to_dev(queries, dev), U.to_dev(manifold, dev), k)
        assert U.same(got, want), (Q, M, F, k)
        assert want[0][0, 0] == 0                               # query 0 equals a stored row
        if M >= 130 and k > 1:
            assert want[1][0, 0] == planted[0][0] and want[0][0, 1] == 0        # and that row has a copy: both at d2 = 0, the lower row first
            if F <= 64:
                assert (want[0][:, :-1] == want[0][:, 1:]).any()


@pytest.mark.parametrize("Q,M,F,k,variant,runs", [(37, 200000, 48, 5, "split", 391), (2100, 13000, 64, 8, "split", 26), (33000, 300, 48, 3, "single", 1)])
def test_several_tiles_and_runs(dev, Q, M, F, k, variant, runs):
    """one query tile x 391 runs of 4 tiles; 17 query tiles x 26 runs of 4 tiles; 258 query tiles, so one run of 3 tiles.  Rows j and
    j + 4100 are identical (j and j + 150 where the manifold is one run), so a tie crosses runs and must go to the lower row"""
    far = 4100 if M > 8200 else 150
    queries, manifold, planted, want = U.exact_case(Q, M, F, k, far)
    ctiles, plan_runs, tiles_per_run = U.plan(Q, M)
    assert plan_runs == runs and tiles_per_run == (4 if variant == "split" else 3)
    assert any(b - a == far for a, b in planted)
    if variant == "split":
        assert any(b - a == far and a // (128 * tiles_per_run) != b // (128 * tiles_per_run) for a, b in planted), "no planted pair straddles two runs"
    with U.topk_launches() as log:
        got = knn_manifold.topk(U.to_dev(queries, dev), U.to_dev(manifold, dev), k)
        got = (got[0].cpu(), got[1].cpu())
    assert U.same(got, want)
    hit = [q for q in range(0, Q, 3) if any(want[1][q, 0] == a and b - a == far for a, b in planted)]
    assert hit and all(want[0][q, 1] == 0 and want[1][q, 1] > want[1][q, 0] for q in hit)   # the far copy follows at the same d2
    assert [v for v, _ in log] == ["norms", "norms"] + (["split", "merge"] if variant == "split" else ["single"]), log
    for _, dims in log[2:]:
        assert dims[1:7] == (Q, M, F, k, runs, U.TOPK_MODE), dims


def test_exclude(dev):
    Q, M, F, k = 150, 260, 64, 3
    manifold = U.exact_features(M, F, seed=5).copy()
    manifold[200], manifold[31] = manifold[17], manifold[140]   # a copy behind and a copy in front of the row itself
    rng = np.random.RandomState(5)
    rows = np.concatenate([[17, 200, 140, 31], rng.permutation(M)[:Q - 4]]).astype(np.int32)
    queries = manifold[rows]
    q, m = U.to_dev(queries, dev), U.to_dev(manifold, dev)
    d2, idx = knn_manifold.topk(q, m, k)
    assert U.same((d2, idx), U.oracle_topk(queries, manifold, k))
    assert bool((d2[:, 0] == 0).all())
    first = idx[:, 0].cpu().numpy()
    assert first[:4].tolist() == [17, 17, 31, 31]               # ties to the lower row
    d2, idx = knn_manifold.topk(q, m, k, U.to_dev(rows, dev))
    assert U.same((d2, idx), U.oracle_topk(queries, manifold, k, rows))
    assert d2[:4, 0].cpu().tolist() == [0, 0, 0, 0] and idx[:4, 0].cpu().tolist() == [200, 17, 31, 140]    # the duplicate is still found
    assert not np.any(idx.cpu().numpy() == rows[:, None])
    outside = np.full([Q], -1, dtype=np.int32)                  # entries outside [0, M) exclude nothing
    outside[1::2] = M
    assert U.same(knn_manifold.topk(q, m, k, U.to_dev(outside, dev)), U.oracle_topk(queries, manifold, k))
    # a manifold of exactly k rows is searched when `exclude` names no row of it
    got = knn_manifold.topk(q[:4], m[:5], 5, torch.tensor([5, -1, 9, 7], dtype=torch.int32, device=dev))
    assert U.same(got, U.oracle_topk(queries[:4], manifold[:5], 5))
    assert sorted(got[1][0].cpu().tolist()) == [0, 1, 2, 3, 4]


def test_two_calls_give_the_same_bits(dev):
    queries, manifold, _, want = U.exact_case(300, 20000, 64, 8, 4100)
    q, m = U.to_dev(queries, dev), U.to_dev(manifold, dev)
    with U.topk_launches() as log_a:
        a = knn_manifold.topk(q, m, 8)
    with U.topk_launches() as log_b:
        b = knn_manifold.topk(q, m, 8)
    assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32)) and torch.equal(a[1], b[1])
    assert [d for _, d in log_a] == [d for _, d in log_b] and "split" in [v for v, _ in log_a]
    assert U.same(a, want)


def test_real_valued_features_within_the_summation_bound(dev):
    """300 x 2000 x 4096, k = 5.  The sums are not exact and near ties may swap, so the comparison is by a derived bound: the three fp32
    sums n(x), n(y), s of F terms each are off by at most F 2^-24 times the sum of their terms' magnitudes (first order; the factor 4
    below covers the rounding of the final operations and the second-order terms), and sum |x_f y_f| <= (n(x) + n(y)) / 2, so
    |d2 - d2_64| <= B = 4 F 2^-24 (n(x) + n(y))"""
    Q, M, F, k = 300, 2000, 4096, 5
    manifold, queries = U.realistic_features(M, Q, F, seed=3)
    d2, idx = knn_manifold.topk(U.to_dev(queries, dev), U.to_dev(manifold, dev), k)
    d2, idx = d2.cpu().numpy().astype(np.float64), idx.cpu().numpy().astype(np.int64)
    ref = U.d2_f64(queries, manifold)
    x, y = queries.astype(np.float64), manifold.astype(np.float64)
    B = 4 * F * 2.0 ** -24 * ((x * x).sum(1)[:, None] + (y * y).sum(1)[None, :])
    assert ((idx >= 0) & (idx < M)).all()
    assert all(len(set(row)) == k for row in idx.tolist())                          # indices within a query are distinct
    rows = np.arange(Q)[:, None]
    err = np.abs(d2 - ref[rows, idx])
    kth = np.sort(ref, axis=1)[:, k - 1]
    print(f"max |d2 - d2_64| / B = {(err / B[rows, idx]).max():.4f}; max (d2_64(index) - kth) / 2B = {((ref[rows, idx] - kth[:, None]) / (2 * B[rows, idx])).max():.4f}")
    assert (err <= B[rows, idx]).all()
    assert (ref[rows, idx] <= kth[:, None] + 2 * B[rows, idx]).all()
    assert (d2[:, :-1] <= d2[:, 1:]).all()


def test_refusals(dev):
    q = torch.zeros([4, 48], dtype=torch.float16, device=dev)
    m = torch.zeros([12, 48], dtype=torch.float16, device=dev)
    with pytest.raises(RuntimeError, match="k = 0 neighbours"):
        knn_manifold.topk(q, m, 0)
    with pytest.raises(RuntimeError, match="k = 9 neighbours"):
        knn_manifold.topk(q, m, 9)
    with pytest.raises(RuntimeError, match="the manifold has 5 rows"):
        knn_manifold.topk(q, m[:5], 6)
    with pytest.raises(RuntimeError, match="one is excluded"):
        knn_manifold.topk(q, m[:5], 5, torch.tensor([0, -1, 9, 7], dtype=torch.int32, device=dev))
    with pytest.raises(RuntimeError, match="multiple of 8"):
        knn_manifold.topk(torch.zeros([4, 44], dtype=torch.float16, device=dev), torch.zeros([12, 44], dtype=torch.float16, device=dev), 3)
    with pytest.raises(RuntimeError, match="must be dense"):
        knn_manifold.topk(q, torch.zeros([12, 96], dtype=torch.float16, device=dev)[:, ::2], 3)
    with pytest.raises(RuntimeError, match="16-byte aligned"):
        knn_manifold.topk(q, torch.zeros([13 * 48 + 4], dtype=torch.float16, device=dev)[4:4 + 12 * 48].view(12, 48), 3)
    with pytest.raises(RuntimeError, match="expects float16"):
        knn_manifold.topk(q.float(), m.float(), 3)
    with pytest.raises(RuntimeError, match="different devices"):
        knn_manifold.topk(q.cpu(), m, 3)
    with pytest.raises(RuntimeError, match="exclude must be an int32"):
        knn_manifold.topk(q, m, 3, torch.zeros([4], dtype=torch.int64, device=dev))
    lib = _lib.load()                                           # the C entry points refuse on their own, with a message
    d2 = torch.zeros([64], dtype=torch.float32, device=dev)
    index = torch.zeros([64], dtype=torch.int32, device=dev)
    ws = torch.zeros([1024], dtype=torch.float32, device=dev)
    excl = torch.zeros([4], dtype=torch.int32, device=dev)
    assert lib.sbg_knn_topk_workspace(4, 12, 9) == -1 and lib.sbg_knn_topk_workspace(4, 12, 0) == -1 and lib.sbg_knn_topk_workspace(0, 12, 3) == -1
    assert lib.sbg_knn_topk_workspace(4, (1 << 24) + 1, 3) == -1 and lib.sbg_knn_topk_workspace(4, 12, 3) > 0
    for args, exclude, message in [((4, 12, 44, 3), None, "multiple of 8"), ((4, 12, 48, 9), None, "k = 9"), ((4, 12, 48, 0), None, "k = 0"),
                                   ((4, 2, 48, 3), None, "the manifold has 2 rows"), ((4, 3, 48, 3), excl, "one may be excluded"),
                                   ((0, 12, 48, 3), None, "bad sizes")]:
        status = lib.sbg_knn_topk(q.data_ptr(), m.data_ptr(), *args, _lib.ptr(exclude), d2.data_ptr(), index.data_ptr(), ws.data_ptr(), None)
        assert status != 0 and message in lib.sbg_last_error().decode(), (args, lib.sbg_last_error())
    assert lib.sbg_knn_topk(q.data_ptr() + 2, m.data_ptr(), 4, 12, 48, 3, None, d2.data_ptr(), index.data_ptr(), ws.data_ptr(), None) != 0
    assert "16-byte aligned" in lib.sbg_last_error().decode()
    assert lib.sbg_knn_topk(None, m.data_ptr(), 4, 12, 48, 3, None, d2.data_ptr(), index.data_ptr(), ws.data_ptr(), None) != 0
    assert "null pointer" in lib.sbg_last_error().decode()
