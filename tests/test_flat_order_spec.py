"""CPU check of the fixtures tests/test_zz_gpu_flat_real.py runs on the GPU (tests/flat_order_spec.py).

The flat kernels claim the reference's l2_scalar / dot_scalar value bit for bit: 16 lane accumulators folded in lane order, the
d % 16 tail summed first.  A test can only hold a kernel to that claim if a kernel that sums in ANOTHER order would return other
bits on the test's data.  Three things are asserted here:
  1. the numpy model of the claimed order equals the oracle's flat_knn, ids and distance bits, on every real-valued f32 fixture;
  2. on those fixtures each wrong order (sequential, lanes folded pairwise, tail added last) changes at least 10 % of the returned
     distances wherever that order is distinguishable at all (measured: see test_real_valued_fixtures_discriminate's docstring);
  3. on the integer-valued fixtures of the older flat tests every wrong order changes exactly ZERO returned distances -- every
     partial sum near the answer is an integer below 2^24 (or a multiple of 2^-16 below 2^8), so any order of additions gives the
     same bits.  That is why the real-valued GPU file exists: the older tests cannot see a wrong summation order."""
import numpy as np
import pytest

import flat_order_spec as S

f32 = np.float32
NQ, K = 4, 50                       # 200 returned distances per fixture
F32_DIMS = (3, 16, 17, 20, 32, 40, 96, 100, 128, 136, 144, 200, 1536, 2047, 2048, 2049)      # every f32 dimension of the GPU file
F16_DIMS = (8, 16, 20, 128, 136)


def distinguishable(order, d):
    if order == "pairwise":
        return d >= 17
    if order == "sequential":
        return d >= 32
    return d > 16 and d % 16 >= 1


def changed_share(x, q, ids, dist, metric, order):
    """share of the returned distances (ids / dist [nq][k] from the oracle) that the wrong order computes differently"""
    diff = total = 0
    for qi in range(q.shape[0]):
        w = S.distances(x[ids[qi].astype(np.int64)], q[qi], metric, order)
        diff += int((w.view(np.uint32) != dist[qi].view(np.uint32)).sum())
        total += w.size
    return diff / total


@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("d", F32_DIMS)
def test_model_matches_the_oracle(oracle, metric, d):
    x, q = S.real_f32(1500, d, NQ, 100 + d)
    oi, od = oracle.flat_knn(x, q, K, metric)
    for qi in range(NQ):
        mi, md = S.topk(S.distances(x, q[qi], metric), K)
        assert (mi == oi[qi]).all(), (metric, d, qi)
        assert (md.view(np.uint32) == od[qi].view(np.uint32)).all(), (metric, d, qi)


def test_model_matches_the_oracle_on_f16_rows(oracle):
    for d in F16_DIMS:
        x, q = S.real_f16(1500, d, NQ, 200 + d)
        oi, od = oracle.flat_knn(x, q, K, "l2")
        for qi in range(NQ):
            mi, md = S.topk(S.distances(x, q[qi], "l2"), K)
            assert (mi == oi[qi]).all() and (md.view(np.uint32) == od[qi].view(np.uint32)).all(), (d, qi)


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_real_valued_fixtures_discriminate(oracle, metric):
    """>= 10 % is a condition on the INPUTS, not a tolerance.  Measured shares of 200 returned distances (4 queries x k = 50):
    f32 pairwise 41-64 %, sequential 67-97 % (92 % and more from d = 1536 up), tail-last 31-63 %; f16 L2 pairwise 39-59 %,
    sequential 84-86 %, tail-last 53 %.  (`pytest -s` prints every figure.)"""
    lines = []
    for kind, dims in (("f32", F32_DIMS), ("f16", F16_DIMS if metric == "l2" else ())):      # f16 dot: 32 lanes, not this model
        for d in dims:
            x, q = (S.real_f32 if kind == "f32" else S.real_f16)(1500, d, NQ, 100 + d)
            oi, od = oracle.flat_knn(x, q, K, metric)
            for order in S.ORDERS:
                if not distinguishable(order, d):
                    continue
                share = changed_share(x, q, oi, od, metric, order)
                lines.append(f"{kind} {metric} d={d} {order}: {share:.3f}")
                assert share >= 0.10, lines[-1]
    print("\n" + "\n".join(lines))


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_integer_fixtures_cannot_see_the_order(oracle, metric):
    """today's fixtures (tests/test_zz_gpu_flat_small.py and the f16 columns of the IVF / flat tests): every wrong order returns
    the same bits, so those tests pass whatever order a kernel sums in"""
    for d, n in ((128, 20_000), (100, 20_000), (20, 9_000), (1536, 6_000), (16, 5_000), (7, 5_000), (17, 5_000), (136, 5_000), (200, 5_000)):
        x, q = S.sift_like_flat_small(n, d, NQ, 17 + d)
        oi, od = oracle.flat_knn(x, q, K, metric)
        for order in S.ORDERS:
            assert changed_share(x, q, oi, od, metric, order) == 0.0, ("sift_like", metric, d, order)
    if metric == "l2":
        for d in (40, 128):
            x, q = S.f16_over_256(10_000, d, NQ, 18 + d)
            oi, od = oracle.flat_knn(x, q, K, "l2")
            for order in S.ORDERS:
                assert changed_share(x, q, oi, od, "l2", order) == 0.0, ("f16 / 256", d, order)
