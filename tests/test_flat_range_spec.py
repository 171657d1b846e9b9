"""CPU checks of tests/flat_range_spec.py: every fixture tests/test_zz_gpu_flat_range.py uses tells the specification of the flat scan's
distance range from the wrong models that apply to it, and the numpy models of the two-sided surrogate test reject no
in-range pair while rejecting the bulk of the below-range pairs.  Also the host side of the feature: the Python entry points take the
range and an un-ranged call makes the library call it made before."""
import inspect

import numpy as np
import pytest

import flat_order_spec as S
import flat_range_spec as R
import magnitude_spec as M
import multivec_spec as MV

f32 = np.float32
K = 10


@pytest.fixture(scope="module")
def main32(oracle):
    x, q = R.main_fixture(32)
    ai, ad = R.every_row(oracle, x, q, "l2")
    return x, q, ai, ad, float(np.median(ad))


def test_total_order_keys():
    """-NaN < -inf < -1 < -0 < +0 < 1 < +inf < +NaN, and the absent bound is no test"""
    v = np.array([0, 0, -np.inf, -1, -0.0, 0.0, 1, np.inf, np.nan], f32)
    v.view(np.uint32)[0] = R.NEG_NAN_BITS
    v.view(np.uint32)[1] = 0xFFFFFFFF        # the negative NaN with every mantissa bit set: key 0
    k = S.keys(v)
    assert k[1] == 0 and (np.sort(np.concatenate([k[1:2], k[0:1], k[2:]])) == np.concatenate([k[1:2], k[0:1], k[2:]])).all()
    assert R.in_range(v, None, None).all()
    assert R.in_range(v, -np.inf, None).tolist() == [False, False, True, True, True, True, True, True, True]       # below every lower bound
    assert R.in_range(v, None, np.inf).tolist() == [True, True, True, True, True, True, True, False, False]        # +inf excluded, +NaN above it
    assert R.in_range(v, 0.0, None).tolist() == [False] * 5 + [True] * 4                                            # -0 lies below +0
    assert R.in_range(v, -0.0, 0.0).tolist() == [False] * 4 + [True] + [False] * 4
    assert R.in_range_ieee(v, 0.0, None).tolist() == [False, False, False, False, True, True, True, True, False]   # the wrong model: -0 kept, NaN dropped
    assert R.key(0.0) > R.key(-0.0)          # (+0, -0): lower above upper, refused


def test_main_fixture_post_filter_differs_for_every_query(main32):
    x, q, ai, ad, lower = main32
    spec = R.select(ai, ad, K, lower, None)
    assert (spec[0] != R.UNSET).all()
    assert R.differs_per_query(spec, R.post_filtered(ai, ad, K, lower, None)).all()
    # both bounds on returned distances: the row on `lower` is kept, the row on `upper` is dropped
    lo, hi = float(spec[1][0, 2]), float(spec[1][0, 7])
    both = R.select(ai, ad, K, lo, hi)
    assert both[1][0, 0].view(np.uint32) == f32(lo).view(np.uint32) and (S.keys(both[1][0, :5]) < R.key(hi)).all() and both[0][0, 5] == R.UNSET
    assert not R.same(both, R.WRONG["closed_upper"](ai, ad, K, lo, hi)) and not R.same(both, R.WRONG["open_lower"](ai, ad, K, lo, hi))


@pytest.mark.parametrize("d", [32, 128])
def test_two_sided_model_on_the_main_fixture(oracle, d):
    """no in-range pair rejected; the bulk of the below-range pairs rejected; the queue (2048 per query and epoch) holds what is left --
    and does NOT hold what the one-sided filter queues: without the lower-side reject nine queries in ten overflow it, the median query fourfold and more"""
    x, q = R.main_fixture(d)
    ai, ad = R.every_row(oracle, x, q, "l2")
    lower = float(np.median(ad))
    dist = np.empty_like(ad)
    np.put_along_axis(dist, ai.astype(np.int64), ad, axis=1)          # [nq][row]
    first = M.FLAT_FIRST_EPOCH
    T = np.array([np.sort(dist[i, :first][R.in_range(dist[i, :first], lower, None)])[K - 1] for i in range(len(q))], f32)
    queued, rej = R.short_row_model(x[first:], q, T, lower)
    inr = R.in_range(dist[:, first:], lower, None)
    assert not (rej & inr).any()
    answer = inr & (dist[:, first:] <= T[:, None])
    assert not (answer & ~queued).any()
    below = ~inr
    assert rej[below].mean() > 0.95
    assert queued.sum(axis=1).max() < 2048 // 4
    one_sided = R.short_row_model(x[first:], q, T, -np.inf)[0].sum(axis=1)      # (the bound is the median of ALL pairs: a few queries lie mostly above it)
    assert np.median(one_sided) > 2048 * 4 and (one_sided > 2048).mean() > 0.9


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_long_row_model_on_the_main_fixture(oracle, metric):
    x, q = R.long_fixture()
    ai, ad = R.every_row(oracle, x, q, metric)
    lower = float(np.median(ad))
    dist = np.empty_like(ad)
    np.put_along_axis(dist, ai.astype(np.int64), ad, axis=1)
    first = M.FLAT_FIRST_EPOCH
    T = np.array([np.sort(dist[i, :first][R.in_range(dist[i, :first], lower, None)])[K - 1] for i in range(len(q))], f32)
    queued, rej = R.long_row_model(x[first:], q, T, lower, metric)
    inr = R.in_range(dist[:, first:], lower, None)
    assert not (rej & inr).any()
    assert not (inr & (dist[:, first:] <= T[:, None]) & ~queued).any()
    assert rej[~inr].mean() > 0.8
    assert queued.sum(axis=1).max() < 2048
    one_sided = R.long_row_model(x[first:], q, T, -np.inf, metric)[0].sum(axis=1)
    assert np.median(one_sided) > 2048 * 4 and (one_sided > 2048).mean() > 0.9
    assert R.differs_per_query(R.select(ai, ad, K, lower, None), R.post_filtered(ai, ad, K, lower, None)).all()


# ---- the epoch schedule under a lower bound: what the GPU tests' counter assertions stand on ------------------------------------------
def _schedules(oracle, x, q, metric, model):
    ai, ad, dist, lower = R.all_distances(oracle, x, q, metric)
    return [R.sized_schedule(len(x), K, R.model_fill(x, q, dist, lower, K, model, reject=rej, metric=metric)) for rej in (True, False)]


@pytest.mark.parametrize("metric,d", [("l2", 32), ("l2", 128), ("dot", 32)])
def test_short_row_schedule(oracle, metric, d):
    """with the two-sided test: one exact epoch, then the matrix cores to the end, queues a twentieth full, no fallback.  With the
    one-sided test the first sized epoch queues half its rows or more and the rest goes to the exact filter: the GPU test's
    `count:flat_lower_fallback did not advance` fails on a build without the lower-side reject"""
    (epochs, fell), (epochs1, fell1) = _schedules(oracle, *R.main_fixture(d), metric, R.short_row_model)
    assert [e[2] for e in epochs] == ["exact", "mc", "mc"] and not fell and epochs[-1][1] == 20000
    assert max(e[3] for e in epochs[1:]) < R.QUEUE_CAP // 8 and epochs[1][3] * 4 < R.LO_FIRST_ROWS * (R.QUEUE_CAP // 2) // R.LO_MIN_ROWS
    assert fell1 and [e[2] for e in epochs1] == ["exact", "mc", "exact"] and epochs1[1][3] > R.LO_FIRST_ROWS // 2


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_long_row_schedule(oracle, metric):
    (epochs, fell), (epochs1, fell1) = _schedules(oracle, *R.long_fixture(), metric, R.long_row_model)
    assert [e[2] for e in epochs] == ["exact", "mc", "mc"] and not fell
    assert max(e[3] for e in epochs[1:]) < R.QUEUE_CAP // 4 and epochs[1][3] * 2 < R.LO_FIRST_ROWS * (R.QUEUE_CAP // 2) // R.LO_MIN_ROWS
    assert fell1 and epochs1[1][3] > R.LO_FIRST_ROWS // 2


def test_schedule_rule():
    """the rule alone: the un-ranged epochs when the queues stay empty; half-full queues keep the length; a dense band falls back"""
    assert [e[:3] for e in R.sized_schedule(10 ** 6, 10, lambda a, b: 0)[0]][:3] == [(0, 2048, "exact"), (2048, 4096, "mc"), (4096, 102400, "mc")]
    ep, fell = R.sized_schedule(10 ** 6, 10, lambda a, b: (b - a) // 64)
    assert not fell and ep[2][1] - ep[2][0] == 65536 and max(e[3] for e in ep[1:]) <= R.QUEUE_CAP // 2
    ep, fell = R.sized_schedule(10 ** 6, 10, lambda a, b: (b - a) // 8)
    assert fell and [e[2] for e in ep[:3]] == ["exact", "mc", "exact"] and ep[-1][1] == 10 ** 6


@pytest.mark.parametrize("d", [32, 128])
@pytest.mark.parametrize("how", ["e-10", "e0", "e13", "r4", "r7", "r10"])
def test_two_sided_model_rejects_no_in_range_pair_across_magnitudes(oracle, d, how):
    """magnitude_spec's flat fixture at 2^-10 .. 2^13 (1e-3 .. 1e4) and with 2^4 .. 2^10 added to every element (the distances then
    are small differences of large norms: the case a relative margin is made for)"""
    fx = M.flat_fixture(d)
    fx = M.scaled(fx, int(how[1:])) if how[0] == "e" else M.offset(fx, int(how[1:]))
    x, q = fx.x[:3000], fx.q[:32]
    ai, ad = R.every_row(oracle, x, q, "l2")
    dist = np.empty_like(ad)
    np.put_along_axis(dist, ai.astype(np.int64), ad, axis=1)
    for quant in (0.02, 0.5, 0.98):
        lower = float(np.quantile(ad, quant))
        T = np.full(len(q), np.inf, f32)
        for model in (R.short_row_model, R.long_row_model):
            _, rej = model(x, q, T, lower)
            assert not (rej & R.in_range(dist, lower, None)).any(), (model.__name__, quant)
    if how[0] == "e":      # (a scale keeps the shape of the distribution: the model still rejects; an offset of 2^10 leaves it nothing to prove)
        assert R.short_row_model(x, q, np.full(len(q), np.inf, f32), float(np.median(ad)))[1].any()


def test_tie_fixture_rows_on_both_bounds_and_ties_across_k(oracle):
    x, q = R.tie_fixture()
    for metric in ("l2", "dot"):
        ai, ad = R.every_row(oracle, x, q, metric)
        lo, hi = float(np.quantile(ad, 0.3, method="lower")), float(np.quantile(ad, 0.6, method="lower"))
        assert lo < hi
        spec = R.select(ai, ad, K, lo, hi)
        for i in range(len(q)):
            assert (ad[i] == f32(lo)).sum() > K and (ad[i] == f32(hi)).sum() > 0         # rows exactly on either bound, and more ties than k
            assert (spec[1][i] == f32(lo)).all()                                           # ... so the answer is the tie's smallest row ids
            assert (np.diff(spec[0][i].astype(np.int64)) > 0).all()
        for name in ("post_filter", "open_lower"):      # (closed_upper: the narrow range below; ieee: no NaN or -0 here)
            assert not R.same(spec, R.WRONG[name](ai, ad, K, lo, hi)), name
        narrow = R.select(ai, ad, 1024, lo, lo + 2)       # a range k = 1024 exhausts: the rows ON the upper bound are what the closed model adds
        assert (narrow[0] == R.UNSET).any(axis=1).all() and not R.same(narrow, R.WRONG["closed_upper"](ai, ad, 1024, lo, lo + 2))
        # short and empty answers, lower == upper
        top = float(ad[:, -1].max())
        short = R.select(ai, ad, K, float(ad[0, -3]), None)
        assert (short[0] == R.UNSET).any() and (short[0] != R.UNSET).any()
        assert (R.select(ai, ad, K, np.nextafter(f32(top), f32(np.inf)), None)[0] == R.UNSET).all()
        assert (R.select(ai, ad, K, lo, lo)[0] == R.UNSET).all()


def test_special_values_fixture(oracle):
    """+inf distances, positive and negative NaN: the open ends keep them, the largest finite bounds do not"""
    x0, q = S.real_f32(6000, 24, 5, 77)
    x, rows = R.specials(x0)
    ai, ad = R.every_row(oracle, x, q, "l2")
    kk = S.keys(ad)
    nn, inf_, pn = len(rows["neg_nan"]), len(rows["inf"]), len(rows["pos_nan"])
    assert (kk[:, :nn] < R.key(-np.inf)).all() and (np.sort(ai[:, :nn], axis=1) == np.sort(rows["neg_nan"])).all()        # the negative NaN sorts first
    assert np.isposinf(ad[:, -pn - inf_:-pn]).all() and (kk[:, -pn:] > R.key(np.inf)).all()
    lo = float(ad[0, 3000])
    open_end = R.select(ai, ad, 6000, lo, None)
    capped = R.select(ai, ad, 6000, lo, R.FLT_MAX)
    assert not R.same(open_end, capped)                                                  # (lo, None) against (lo, FLT_MAX)
    assert np.isposinf(open_end[1][0][open_end[0][0] != R.UNSET]).sum() == inf_ and np.isnan(open_end[1]).sum() == pn * len(q)
    assert not np.isnan(capped[1]).any()
    none_hi = R.select(ai, ad, K, None, lo)
    assert (S.keys(none_hi[1][:, :nn]) < R.key(-np.inf)).all()                           # (None, hi) keeps the negative-NaN rows
    assert not R.same(none_hi, R.select(ai, ad, K, -R.FLT_MAX, lo)) and not R.same(none_hi, R.select(ai, ad, K, -np.inf, lo))
    to_inf = R.select(ai, ad, 6000, None, np.inf)                                        # (None, +inf): every finite row and the negative NaN
    assert ((to_inf[0] != R.UNSET).sum(axis=1) == 6000 - inf_ - pn).all()
    for lo_, hi_ in ((lo, None), (None, lo), (None, np.inf)):
        assert not R.same(R.select(ai, ad, 6000, lo_, hi_), R.WRONG["ieee"](ai, ad, 6000, lo_, hi_)), (lo_, hi_)


def test_zero_sign_fixture(oracle):
    x, q = R.zero_sign_fixture()
    ai, ad = R.every_row(oracle, x, q, "l2")
    assert (ad[:, 0].view(np.uint32) == 0).all()                                         # +0.0: the row equal to the query
    assert (R.select(ai, ad, K, 0.0, None)[1][:, 0].view(np.uint32) == 0).all()
    assert (R.select(ai, ad, K, None, 0.0)[0] == R.UNSET).all()
    assert (R.select(ai, ad, K, -0.0, 0.0)[0] == R.UNSET).all() and R.key(-0.0) < R.key(0.0)
    assert (R.select(ai, ad, K, -0.0, None)[1][:, 0].view(np.uint32) == 0).all()


def test_duplicates_fixture(oracle):
    x, q = R.duplicates_fixture()
    ai, ad = R.every_row(oracle, x, q, "l2")
    assert ((ad == 1.0).sum(axis=1) >= 4200).all() and ((ad < 1.0).sum(axis=1) >= 12).all()
    spec = R.select(ai, ad, K, 1.0, None)
    assert (spec[1] == 1.0).all()
    assert not R.same(spec, R.post_filtered(ai, ad, K, 1.0, None)) and not R.same(spec, R.WRONG["open_lower"](ai, ad, K, 1.0, None))


def test_multivector_ranges(oracle):
    lens = MV.lengths(300, 1, 9, 5)
    values, off, q = MV.column(lens, 24, 5, 31)
    dist = MV.distances(oracle, values, off, q, "l2")
    rid = MV.row_ids(300, 9)
    ids, d = MV.topk(dist, 40, rid)
    lo, hi = float(d[5]), float(d[30])
    got = R.multivec_topk(dist, 10, lo, hi, rid)
    assert (got[0] == ids[5:15]).all() and got[1][0] == f32(lo)
    assert (R.multivec_topk(dist, 40, lo, hi, rid)[0][25:] == R.UNSET).all()             # the row on `upper` is dropped, the rest padding
    assert (R.multivec_topk(dist, 10, lo, lo, rid)[0] == R.UNSET).all()


# ---- the host side ---------------------------------------------------------------------------------------------------------------------
def test_python_entry_points_take_the_range():
    import lance_amd
    from lance_amd import _lib, vector
    from lance_amd.engine import Engine
    for fn, names in ((Engine.flat_topk, ("lower", "upper")), (Engine.multivec_topk, ("lower", "upper")),
                      (vector.flat_knn, ("distance_range",)), (vector.multivector_flat_knn, ("distance_range",))):
        p = inspect.signature(fn).parameters
        assert all(n in p and p[n].default is None for n in names), fn
    assert "lance_hip_flat_topk_range" in _lib.SYMBOLS and "lance_hip_flat_multivec_topk_range" in _lib.SYMBOLS
    assert "not tested" in vector.flat_knn.__doc__.lower() and "IvfFlatIndex.nearest" in vector.flat_knn.__doc__


def test_unranged_flat_knn_makes_the_call_it_made_before():
    """distance_range = None (and (None, None)): flat_topk is called without range arguments; a range is handed on as lower / upper"""
    from lance_amd import vector

    class Rec:
        def __init__(self):
            self.calls = []

        def flat_topk(self, *a, **kw):
            self.calls.append(("flat", len(a), kw))
            return None, None

        def multivec_topk(self, *a, **kw):
            self.calls.append(("mv", len(a), kw))
            return None, None

    x = np.zeros((4, 8), f32)
    e = Rec()
    vector.flat_knn(x, x[:1], 2, engine=e)
    vector.flat_knn(x, x[:1], 2, engine=e, distance_range=(None, None))
    vector.flat_knn(x, x[:1], 2, engine=e, distance_range=(1.0, None))
    assert e.calls[0] == ("flat", 4, {}) and e.calls[1] == ("flat", 4, {}) and e.calls[2] == ("flat", 4, {"lower": 1.0, "upper": None})
    off = np.array([0, 2, 4], np.int64)
    vector.multivector_flat_knn(x, off, x[:2], 1, "l2", engine=e)
    vector.multivector_flat_knn(x, off, x[:2], 1, "l2", engine=e, distance_range=(None, 2.0))
    assert e.calls[3] == ("mv", 5, {"row_ids": None}) and e.calls[4] == ("mv", 5, {"row_ids": None, "lower": None, "upper": 2.0})


def test_engine_range_arguments():
    from lance_amd.engine import _flat_range_args
    assert _flat_range_args(None, None) is None
    assert _flat_range_args(1.5, None) == (1, 1.5, 0, 0.0) and _flat_range_args(None, 0.1) == (0, 0.0, 1, float(f32(0.1)))
