"""Distance ranges on the exhaustive scan (lance_hip_flat_topk_range / lance_hip_flat_multivec_topk_range): every kernel
route of flat_topk answers `lower <= d < upper` with the ids and the distance BITS of tests/flat_range_spec.py -- the un-ranged scan's
rows (the oracle's, k = n), kept by the total-order key comparison, the k nearest of them, padded.  Bounds are taken from distances an
un-ranged call returned, so rows lie exactly on them.  The shapes are the smallest that reach each route (flat.hip's dispatch in
flat_topk_impl and the *_supported gates); tests/test_flat_range_spec.py shows on the CPU that these fixtures tell the specification
from the post-filter, `d <= upper`, `d > lower` and the IEEE comparison.

The two matrix-core tests also assert WHICH kernels answered.  Under a lower bound flat_topk_v2 sizes the matrix-core epochs by the
fullest queue of the epoch before and hands the column to the exact filter (count:flat_lower_fallback) when more than one pair in
sixteen cannot be decided.  With the bound at the median of all distances a filter WITHOUT the lower-side reject queues half of its first
2048-row epoch, falls back, and the exact filter answers -- right ids and bits.  So the tests assert that count:flat_mfma /
count:flat_mfma_wide advanced by the number of matrix-core epochs tests/flat_range_spec.py's schedule model gives for the two-sided filter
(two: rows 2048..4095, then the rest), that count:flat_lower_fallback did not advance and that count:flat_repair did not;
tests/test_flat_range_spec.py shows on the CPU that the one-sided filter fails the first two."""
import ctypes as C

import numpy as np
import pytest
import torch

import flat_order_spec as S
import flat_range_spec as R
import multivec_spec as MV

pytestmark = pytest.mark.gpu
f32 = np.float32
K = 10


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _dev(a):
    import lance_amd.engine as E
    return E.to_device(a)


def _count(eng, stage):
    return eng.timing_query("count:" + stage)[1]


def _eq(got, want, tag):
    gi, gd = got[0].cpu().numpy().view(np.uint64), got[1].cpu().numpy()
    assert (gi == want[0]).all(), tag
    assert (gd.view(np.uint32) == want[1].view(np.uint32)).all(), tag


def _bounds(eng, xd, qd, metric, kk, a, b, rid=None):
    """two distances the UN-RANGED scan returned for query 0 (positions a < b of its top kk): rows lie exactly on both"""
    d = eng.flat_topk(xd, qd, kk, metric, row_ids=rid)[1][0].cpu().numpy()
    return float(d[a]), float(d[b])


def _ranges(lo, hi):
    return ((lo, hi), (lo, None), (None, hi))


def _run(eng, oracle, x, q, metric, ks, a=5, b=60, rid=None, tag=None, ranges=None):
    """every range of `ranges` (default: both bounds, lower alone, upper alone, on returned distances) at every k, against the spec"""
    xd, qd = _dev(x), _dev(q)
    rd = None if rid is None else _dev(rid.view(np.int64))
    ai, ad = R.every_row(oracle, x if x.dtype == np.float16 else x.astype(f32), q if q.dtype == np.float16 else q.astype(f32), metric, rid)
    if ranges is None:
        ranges = _ranges(*_bounds(eng, xd, qd, metric, max(b + 1, 64), a, b, rd))
    for lo, hi in ranges:
        for k in ks:
            _eq(eng.flat_topk(xd, qd, k, metric, row_ids=rd, lower=lo, upper=hi), R.select(ai, ad, k, lo, hi), (tag, metric, k, lo, hi))
    return ai, ad


def _data(kind, n, d, nq, seed):
    return {"f32": S.real_f32, "f16": S.real_f16, "i8": S.int8_rows}[kind](n, d, nq, seed)


# ---- the single-pass kernel (flat_small.hip): one and two queries, n >= 4096, k <= 128 ---------------------------------------------------
@pytest.mark.parametrize("kind,metric", [("f32", "l2"), ("f32", "dot"), ("f16", "l2"), ("i8", "l2"), ("i8", "dot")])
@pytest.mark.parametrize("d", [24, 128])
def test_single_pass(eng, oracle, kind, metric, d):
    x, q = _data(kind, 5000, d, 2, 400 + d)
    for nq in (1, 2):
        _run(eng, oracle, x, q[:nq], metric, (10, 128), a=5, b=100, tag=("small", kind, d, nq))


# ---- the fixed-dimension exact filter (flat_filter_kernel): two epochs (2048 rows, then the rest) ---------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("d", [8, 32, 128])
@pytest.mark.parametrize("nq", [5, 100])
def test_fixed_dimension_filter(eng, oracle, metric, d, nq):
    x, q = S.real_f32(6000, d, nq, 500 + d)
    _run(eng, oracle, x, q, metric, (K, 128), tag=("fixed", d, nq))


@pytest.mark.parametrize("kind,metric", [("f16", "l2"), ("i8", "l2"), ("i8", "dot")])
def test_fixed_dimension_filter_native_columns(eng, oracle, kind, metric):
    x, q = _data(kind, 6000, 32, 5, 541)
    _run(eng, oracle, x, q, metric, (K,), tag=("native", kind))


def test_ties_on_both_bounds_and_across_k(eng, oracle):
    """small integers: hundreds of rows tied at every distance, rows exactly on either bound; k = 1024 (the v1 route) exhausts the
    narrow range, so a scan that kept the rows ON the upper bound would show them"""
    x, q = R.tie_fixture()
    for metric in ("l2", "dot"):
        ai, ad = R.every_row(oracle, x, q, metric)
        lo, hi = float(np.quantile(ad, 0.3, method="lower")), float(np.quantile(ad, 0.6, method="lower"))
        _run(eng, oracle, x, q, metric, (K, 128), ranges=((lo, hi), (lo, lo), (float(ad[0, -3]), None), (float(ad.max()) + 1.0, None)), tag="ties")
        _run(eng, oracle, x, q, metric, (1024,), ranges=((lo, lo + 2),), tag="ties-narrow")


# ---- the any-dimension filter (wide.hip) -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,d", [("l2", 200), ("dot", 200), ("l2", 20), ("dot", 20), ("cosine", 64)])
def test_any_dimension_filter(eng, oracle, metric, d):
    x, q = S.real_f32(6000, d, 5, 600 + d)
    _run(eng, oracle, x, q, metric, (K, 128), tag=("wide", d))


# ---- the matrix-core filters -------------------------------------------------------------------------------------------------------------
def _matrix_core(eng, oracle, x, q, metric, stage, model):
    xd, qd = _dev(x), _dev(q)
    ai, ad, dist, lower = R.all_distances(oracle, x, q, metric)
    epochs, fell = R.sized_schedule(len(x), K, R.model_fill(x, q, dist, lower, K, model, metric=metric))
    want = sum(e[2] == "mc" for e in epochs)
    assert want == 2 and not fell and epochs[-1][2] == "mc"          # the model: the matrix cores answer every row after the first epoch
    m0, r0, f0 = _count(eng, stage), _count(eng, "flat_repair"), _count(eng, "flat_lower_fallback")
    got = eng.flat_topk(xd, qd, K, metric, lower=lower)
    eng.synchronize()
    m1, r1, f1 = _count(eng, stage), _count(eng, "flat_repair"), _count(eng, "flat_lower_fallback")
    _eq(got, R.select(ai, ad, K, lower, None), (stage, metric, "lower"))
    assert f1 == f0, "count:flat_lower_fallback advanced: the filter left too many pairs undecided and the exact filter took the column"
    assert m1 - m0 == want, f"count:{stage} advanced by {m1 - m0}, not by the {want} matrix-core epochs of the schedule"
    assert r1 == r0, "count:flat_repair advanced: the queues overflowed and the exact kernel rescanned the column"
    # both bounds, on distances the ranged call returned (a row exactly on each), and the upper bound alone
    d0 = got[1][0].cpu().numpy()
    for lo, hi in ((float(d0[2]), float(d0[7])), (lower, float(d0[7])), (None, float(np.quantile(ad, 0.01)))):
        _eq(eng.flat_topk(xd, qd, K, metric, lower=lo, upper=hi), R.select(ai, ad, K, lo, hi), (stage, metric, lo, hi))
    assert _count(eng, "flat_repair") == r0 and _count(eng, "flat_lower_fallback") == f0


@pytest.mark.parametrize("metric,d", [("l2", 32), ("l2", 128), ("dot", 32)])
def test_short_row_matrix_core_filter(eng, oracle, metric, d):
    x, q = R.main_fixture(d)
    _matrix_core(eng, oracle, x, q, metric, "flat_mfma", R.short_row_model)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_long_row_matrix_core_filter(eng, oracle, metric):
    x, q = R.long_fixture()
    _matrix_core(eng, oracle, x, q, metric, "flat_mfma_wide", R.long_row_model)


# ---- the v1 route: k > 128, cosine at d = 8, f16 dot ----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric,d,ks", [("f32", "l2", 32, (200, 1024)), ("f32", "dot", 20, (200,)), ("f32", "cosine", 8, (K, 200)),
                                              ("f16", "dot", 40, (K, 200))])
def test_v1_route(eng, oracle, kind, metric, d, ks):
    x, q = _data(kind, 6000, d, 5, 700 + d)
    _run(eng, oracle, x, q, metric, ks, a=5, b=150, tag=("v1", kind, d))


# ---- query chunks, the repair loop -------------------------------------------------------------------------------------------------------
def test_second_query_chunk_starts_from_the_bound(eng, oracle):
    x, q = S.real_f32(300, 8, 2100, 801)           # FLAT_QCHUNK = 2048: queries 2048.. are a second pass over the rows
    xd, qd = _dev(x), _dev(q)
    ai, ad = R.every_row(oracle, x, q, "l2")
    hi = float(np.quantile(ad, 0.02))
    want = R.select(ai, ad, K, None, hi)
    assert (want[0][2048:] == R.UNSET).any() and (want[0][2048:] != R.UNSET).any()
    _eq(eng.flat_topk(xd, qd, K, "l2", upper=hi), want, "chunks")
    lo = float(np.quantile(ad, 0.01))
    _eq(eng.flat_topk(xd, qd, K, "l2", lower=lo, upper=hi), R.select(ai, ad, K, lo, hi), "chunks-both")


def test_repair_loop_keeps_the_range(eng, oracle):
    """4200 rows tied at distance == lower behind a first epoch of far rows: every one of them is under the first threshold, the pool of
    4096 overflows, the repair rounds rescan -- and must still drop the rows under the bound (the copies of the queries, distance 0)"""
    x, q = R.duplicates_fixture()
    xd, qd = _dev(x), _dev(q)
    ai, ad = R.every_row(oracle, x, q, "l2")
    r0 = _count(eng, "flat_repair")
    got = eng.flat_topk(xd, qd, K, "l2", lower=1.0)
    assert _count(eng, "flat_repair") > r0, "the fixture did not reach the repair loop"
    _eq(got, R.select(ai, ad, K, 1.0, None), "repair")
    _eq(eng.flat_topk(xd, qd, K, "l2", lower=1.0, upper=2.0), R.select(ai, ad, K, 1.0, 2.0), "repair-both")


# ---- empty and degenerate inputs ---------------------------------------------------------------------------------------------------------
def test_empty_and_degenerate(eng, oracle, engine):
    x, q = S.real_f32(6000, 32, 5, 901)
    xd, qd = _dev(x), _dev(q)
    ai, ad = R.every_row(oracle, x, q, "l2")
    gi, gd = eng.flat_topk(xd[:0], qd, K, "l2", lower=0.0, upper=10.0)                     # n = 0
    assert (gi.cpu().numpy() == -1).all() and np.isposinf(gd.cpu().numpy()).all()
    lo = float(ad[0, -4])                                                                   # k > in-range rows
    want = R.select(ai, ad, K, lo, None)
    assert (want[0] == R.UNSET).any() and (want[0][0, :4] != R.UNSET).all()
    _eq(eng.flat_topk(xd, qd, K, "l2", lower=lo), want, "short")
    for lo_, hi_ in ((float(ad.max()) * 2, None), (None, 0.0), (5.0, 5.0), (-0.0, 0.0), (None, -np.inf)):      # ranges holding nothing
        want = R.select(ai, ad, K, lo_, hi_)
        assert (want[0] == R.UNSET).all()
        _eq(eng.flat_topk(xd, qd, K, "l2", lower=lo_, upper=hi_), want, (lo_, hi_))
    for lo_, hi_ in ((2.0, 1.0), (0.0, -0.0), (np.inf, 1.0)):                                # lower above upper, in the total order
        with pytest.raises(engine.LanceHipError, match="lower bound .* is above the upper bound"):
            eng.flat_topk(xd, qd, K, "l2", lower=lo_, upper=hi_)


def test_zero_sign(eng, oracle):
    x, q = R.zero_sign_fixture()
    ai, ad = _run(eng, oracle, x, q, "l2", (K,), ranges=((0.0, None), (-0.0, None), (None, 0.0), (0.0, 1.0)), tag="zero")
    assert (ad[:, 0].view(np.uint32) == 0).all()


# ---- NaN rows and open ends ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,nq", [(24, 5), (32, 5), (24, 1), (32, 130)])
def test_nan_rows_and_open_ends(eng, oracle, d, nq):
    """rows at +inf, at the positive NaN and at the negative NaN (flat_range_spec.specials) through the any-dimension filter, the fixed
    filter, the single-pass kernel and the matrix-core filter.  The un-ranged answer is checked first: the ranged one is defined on it"""
    x0, q = S.real_f32(6000, d, nq, 950 + d)
    x, rows = R.specials(x0)
    xd, qd = _dev(x), _dev(q)
    ai, ad = R.every_row(oracle, x, q, "l2")
    _eq(eng.flat_topk(xd, qd, 64, "l2"), (ai[:, :64], ad[:, :64]), "un-ranged: the negative-NaN rows first")
    lo = float(ad[0, 3000])
    big = 128
    for lo_, hi_ in ((lo, None), (lo, R.FLT_MAX), (None, lo), (-R.FLT_MAX, lo), (-np.inf, lo), (None, np.inf), (float(ad[0, 5900]), None),
                     (float(ad[0, 5900]), np.inf)):
        for k in (K, big):
            _eq(eng.flat_topk(xd, qd, k, "l2", lower=lo_, upper=hi_), R.select(ai, ad, k, lo_, hi_), (d, nq, k, lo_, hi_))
    tail = float(ad[0, 5900])           # fewer than 128 rows from here on: the answer reaches the +inf and the NaN rows
    a, b = R.select(ai, ad, big, tail, None), R.select(ai, ad, big, tail, R.FLT_MAX)
    assert np.isnan(a[1]).any() and np.isposinf(a[1][a[0] != R.UNSET]).any() and not R.same(a, b)      # (lo, None) against (lo, FLT_MAX)


# ---- row ids, the prefilter ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq", [1, 5, 130])
def test_row_ids(eng, oracle, nq):
    n = 6000
    x, q = S.real_f32(n, 32, nq, 1001)
    rid = np.random.default_rng(3).permutation(n).astype(np.uint64) * 7 + (np.uint64(1) << np.uint64(33))      # permuted, above 2^32
    _run(eng, oracle, x, q, "l2", (K, 128), rid=rid, tag=("rid", nq))


def test_flat_knn_prefilter_and_range(eng, oracle, engine):
    n = 6000
    x, q = S.real_f32(n, 32, 5, 1101)
    mask = np.random.default_rng(5).random(n) < 0.4
    keep = np.flatnonzero(mask).astype(np.uint64)
    ai, ad = R.every_row(oracle, x[mask], q, "l2", keep)
    lo, hi = float(ad[0, 5]), float(ad[0, 60])
    for rng in ((lo, hi), (lo, None), (None, hi)):
        _eq(engine.flat_knn(_dev(x), _dev(q), K, "l2", engine=eng, prefilter=mask, distance_range=rng), R.select(ai, ad, K, *rng), ("prefilter", rng))
    ai, ad = R.every_row(oracle, x, q, "l2")
    _eq(engine.flat_knn(_dev(x), _dev(q), K, "l2", engine=eng, distance_range=(lo, hi)), R.select(ai, ad, K, lo, hi), "flat_knn")
    _eq(engine.flat_knn(_dev(x), _dev(q), K, "l2", engine=eng, distance_range=(None, None)), (ai[:, :K], ad[:, :K]), "(None, None)")


# ---- multivector columns -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("d", [32, 24])           # a fixed-dimension kernel and the generic one
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_multivector(eng, oracle, engine, kind, d, metric):
    n = 3000                                       # two selection blocks of 2048
    lens = MV.lengths(n, 1, 6, 21)
    values, off, q = MV.column(lens, d, 5, 1200 + d, kind)
    rid = MV.row_ids(n, 4)
    dist = MV.distances(oracle, values, off, q, metric)
    vd, qd, rd = _dev(values), _dev(q), _dev(rid.view(np.int64))
    got = eng.multivec_topk(vd, off, qd, 64, metric, row_ids=rd)
    d0 = got[1].cpu().numpy()
    lo, hi = float(d0[5]), float(d0[40])           # returned distances: a row exactly on each bound
    for lo_, hi_ in ((lo, hi), (lo, None), (None, hi), (lo, lo), (float(dist.max()) + 1.0, None)):
        for k in (K, 1024):
            g = eng.multivec_topk(vd, off, qd, k, metric, row_ids=rd, lower=lo_, upper=hi_)
            w = R.multivec_topk(dist, k, lo_, hi_, rid)
            _eq((g[0][None], g[1][None]), (w[0][None], w[1][None]), ("mv", kind, d, metric, k, lo_, hi_))
    g = engine.multivector_flat_knn(vd, off, qd, K, metric, engine=eng, row_ids=rd, distance_range=(lo, hi))
    w = R.multivec_topk(dist, K, lo, hi, rid)
    _eq((g[0][None], g[1][None]), (w[0][None], w[1][None]), "multivector_flat_knn")
    with pytest.raises(engine.LanceHipError, match="flat_multivec_topk_range: lower bound .* is above the upper bound"):
        eng.multivec_topk(vd, off, qd, K, metric, lower=2.0, upper=1.0)


# ---- the C boundary ------------------------------------------------------------------------------------------------------------------------
def test_c_boundary(eng, engine):
    from lance_amd import _lib
    lib = eng.lib
    x, q = S.real_f32(6000, 32, 5, 1301)
    xd, qd = _dev(x), _dev(q)
    ids = torch.empty((5, K), dtype=torch.int64, device=xd.device)
    dists = torch.empty((5, K), dtype=torch.float32, device=xd.device)
    p = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()

    def call(x_=p(xd), q_=p(qd), ids_=p(ids), dists_=p(dists), dtype=_lib.F32, metric=_lib.L2, k=K, rng=(1, 1.0, 1, 2.0)):
        return lib.lance_hip_flat_topk_range(eng.h, dtype, metric, x_, None, 6000, 32, q_, 5, k, *rng, ids_, dists_)

    for kw, msg in (({"x_": None}, "flat_topk_range: NULL argument"), ({"q_": None}, "flat_topk_range: NULL argument"),
                    ({"ids_": None}, "flat_topk_range: NULL argument"), ({"dists_": None}, "flat_topk_range: NULL argument"),
                    ({"metric": 7}, "flat_topk_range: bad metric 7"), ({"k": 0}, "flat_topk_range: k=0 not supported"),
                    ({"k": 1025}, "flat_topk_range: k=1025 not supported"), ({"dtype": 9}, "flat_topk_range"),
                    ({"rng": (1, 2.0, 1, 1.0)}, "flat_topk_range: lower bound 2 is above the upper bound 1")):
        assert call(**kw) == _lib.EINVAL, kw
        assert msg in lib.lance_hip_last_error().decode(), (kw, lib.lance_hip_last_error().decode())
    # an absent bound's value is ignored: (has_lower = 0, lower = 9e9) is no lower bound
    assert call(rng=(0, 9e9, 1, 60.0)) == _lib.OK
    a = (ids.clone(), dists.clone())
    b = eng.flat_topk(xd, qd, K, "l2", upper=60.0)
    assert (a[0] == b[0]).all() and (a[1].view(torch.int32) == b[1].view(torch.int32)).all()
    # multivector entry
    off = _dev(np.array([0, 3000, 6000], np.int64))
    one = lambda **kw: lib.lance_hip_flat_multivec_topk_range(eng.h, kw.get("dtype", _lib.F32), _lib.L2, p(xd), kw.get("off", p(off)), None, 2, 32, p(qd), 5,
                                                              kw.get("k", 1), 1, 0.0, 0, 0.0, kw.get("ids", p(ids)), p(dists))
    for kw, msg in (({"off": None}, "flat_multivec_topk_range: NULL argument"), ({"ids": None}, "flat_multivec_topk_range: NULL argument"),
                    ({"k": 1025}, "flat_multivec_topk_range: k=1025 not supported"), ({"dtype": _lib.I8}, "flat_multivec_topk_range: unsupported element type")):
        assert one(**kw) == _lib.EINVAL, kw
        assert msg in lib.lance_hip_last_error().decode(), (kw, lib.lance_hip_last_error().decode())
    assert one() == _lib.OK


@pytest.mark.parametrize("shape", [(5000, 24, 1, 10), (6000, 32, 5, 10), (6000, 200, 5, 10), (6000, 32, 130, 10), (6000, 32, 5, 200)])
def test_unranged_parity_through_the_new_entry(eng, shape):
    """has_lower = has_upper = 0 through lance_hip_flat_topk_range equals lance_hip_flat_topk bit for bit, on every route"""
    n, d, nq, k = shape
    x, q = S.real_f32(n, d, nq, 1400 + d)
    xd, qd = _dev(x), _dev(q)
    want = eng.flat_topk(xd, qd, k, "l2")
    ids, dists = torch.empty_like(want[0]), torch.empty_like(want[1])
    torch.cuda.synchronize()
    from lance_amd import _lib
    _lib.check(eng.lib.lance_hip_flat_topk_range(eng.h, _lib.F32, _lib.L2, C.c_void_p(xd.data_ptr()), None, n, d, C.c_void_p(qd.data_ptr()), nq, k,
                                                 0, 123.0, 0, -5.0, C.c_void_p(ids.data_ptr()), C.c_void_p(dists.data_ptr())))
    assert (ids == want[0]).all() and (dists.view(torch.int32) == want[1].view(torch.int32)).all()
