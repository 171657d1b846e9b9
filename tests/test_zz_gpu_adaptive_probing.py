"""Adaptive probing (minimum_nprobes / maximum_nprobes) of IvfFlatIndex, IvfSqIndex and IvfRqIndex.nearest on the GPU against
ivfflat_range_spec.adaptive over the index type's own specification (ivfflat_range_spec.search, sq_spec.search, rq_spec.search,
refine_spec.*_search_refine), bit for bit: ids and distance bits.  3000-row, 8-list fixtures; a prefilter selecting 30 rows starves
queries at 1, 2 and 4 partitions, one selecting 7 rows (fewer than k) takes late_search's shortcut -- unless a refine factor or a
range rules it out.  What the fixtures exercise is checked on the CPU by tests/test_ivfflat_range_spec.py.  Sorted last: newest
device code last."""
import functools

import numpy as np
import pytest

import ivfflat_range_spec as V
import refine_spec as RF
import rq_spec as R
import sq_spec as S

pytestmark = pytest.mark.gpu
f32 = np.float32
K, NLIST, N = V.K, V.NLIST, 3000
KINDS = ("flat", "sq", "rq")


def eng():
    import lance_amd
    return lance_amd.default_engine()


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


@functools.lru_cache(maxsize=None)
def spec_side(kind):
    """-> (q, row ids, raw column | None, spec(q, k, nprobes, prefilter, refine_factor, distance_range) -> (ids, dists), what the
    device index is built from)"""
    import oracle
    if kind == "flat":
        x, q, cent = V.base_fixture()
        rid = S.permuted_ids(N, 3)

        def spec(qq, k, npb, prefilter, rf, rng):
            lo, hi = rng or (None, None)
            return V.search(oracle, x, cent, qq, k, npb, "l2", lo, hi, row_ids=rid, prefilter=prefilter)
        return q[:33], rid, None, spec, (x, cent)
    if kind == "sq":
        x, q = S.gaussian(N, 32, 33, seed=71)
        cent = S.centroids_with_gaps(x, NLIST, seed=1)
        xs, part = S.prepare_rows(oracle, x, cent, "l2")
        b = S.bounds(xs[:64])
        codes = S.encode(xs, *b)
        rid = S.permuted_ids(N, 2)
        raw = RF.raw_by_row_id(x, rid)

        def spec(qq, k, npb, prefilter, rf, rng):
            if rf:
                return RF.sq_search_refine(oracle, codes, part, cent, qq, k, rf, npb, "l2", *b, raw, row_ids=rid, prefilter=prefilter)
            return S.search(oracle, codes, part, cent, qq, k, npb, "l2", *b, row_ids=rid, prefilter=prefilter)
        return q, rid, raw, spec, (xs, cent, part, b)
    x, q = R.clustered(N, 64, 33, seed=72)
    cent = S.centroids_with_gaps(x, NLIST, seed=1)
    P = R.rotation(64, 5)
    part, codes, add, scale = R.build(oracle, x, cent, P, "l2")
    rid = R.permuted_ids(N, 3)
    raw = RF.raw_by_row_id(x, rid)

    def spec(qq, k, npb, prefilter, rf, rng):
        if rf:
            return RF.rq_search_refine(oracle, codes, add, scale, part, cent, P, qq, k, rf, npb, "l2", raw, row_ids=rid, prefilter=prefilter)
        return R.search(oracle, codes, add, scale, part, cent, P, qq, k, npb, "l2", row_ids=rid, prefilter=prefilter)
    return q, rid, raw, spec, (x, cent, P, part)


@functools.lru_cache(maxsize=None)
def device_side(kind):
    """the index wrapper, built with params=None: nearest takes the number of partitions from the index itself"""
    import oracle
    import lance_amd
    from lance_amd.engine import DeviceFlatIndex, DeviceRqIndex, DeviceSqIndex
    q, rid, raw, _, parts = spec_side(kind)
    e = eng()
    if kind == "flat":
        x, cent = parts
        part, _ = oracle.assign(x, cent, "l2")
        return lance_amd.vector.IvfFlatIndex(DeviceFlatIndex.create(e, "l2", cent, x, part.view(np.int32), rid), None, None, None)
    if kind == "sq":
        xs, cent, part, b = parts
        ix = DeviceSqIndex.create(e, "l2", cent, e.sq_encode(xs, b), part, b, row_ids=rid)
        ix.set_raw(raw)
        return lance_amd.vector.IvfSqIndex(ix, None, None, None)
    x, cent, P, part = parts
    gc, ga, gs = e.rq_encode(x, part.view(np.int32), oracle.assign(x, cent, "l2")[1], cent, P, "l2")
    ix = DeviceRqIndex.create(e, "l2", cent, P, gc, ga, gs, part.view(np.int32), row_ids=rid)
    ix.set_raw(raw)
    return lance_amd.vector.IvfRqIndex(ix, None, None, None)


def mask_selecting(rid, count, seed):
    """a prefilter over row ids selecting `count` of the rows"""
    rows = np.random.default_rng(seed).choice(len(rid), count, replace=False)
    mask = np.zeros(int(rid.max()) + 1, bool)
    mask[rid[rows].astype(np.int64)] = True
    return mask


def run(kind, k, min_np, max_np, prefilter=None, rf=None, rng=None, nprobes=1):
    """nearest(minimum_nprobes=, maximum_nprobes=) against adaptive() over the specification -> (ids, partitions searched per query)"""
    q, rid, _, spec, _ = spec_side(kind)
    kw = {}
    if rf is not None:
        kw["refine_factor"] = rf
    if rng is not None:
        kw["distance_range"] = rng
    gi, gd = device_side(kind).nearest(q, k, nprobes, prefilter=prefilter, minimum_nprobes=min_np, maximum_nprobes=max_np, **kw)
    shortcut = prefilter is not None and rf is None and rng is None
    oi, od, used = V.adaptive(lambda sel, npb: spec(q[sel], k, npb, prefilter, rf, rng), len(q), k, nprobes if min_np is None else min_np,
                              (nprobes if min_np is None else None) if max_np is None else max_np, NLIST,
                              selected_ids=np.flatnonzero(prefilter) if shortcut else None)
    assert gi.dtype == np.uint64 and (gi == oi).all(), (kind, k, min_np, max_np, rf, rng, np.argwhere(gi != oi)[:4])
    assert same_bits(gd, od), (kind, k, min_np, max_np, rf, rng)
    return oi, od, used


@pytest.mark.parametrize("kind", KINDS)
def test_selective_prefilter_extends_the_search(kind):
    _, rid, _, _, _ = spec_side(kind)
    m30 = mask_selecting(rid, 30, 6)
    oi, _, used = run(kind, K, 1, 8, prefilter=m30)
    assert (used > 2).any() and (used < 8).any() and (V.found(oi) == K).all()       # starved at 1 and at 2, satisfied later
    _, _, used_all = run(kind, K, 1, None, prefilter=m30)                           # maximum_nprobes=None: all lists
    assert (used_all == used).all()
    oi2, _, used2 = run(kind, K, 1, 2, prefilter=m30)                               # the maximum stops queries that are still short
    assert (used2 <= 2).all() and (V.found(oi2) < K).any()
    run(kind, K, 2, 5, prefilter=m30)                                               # 2 -> 4 -> 5: the last step is cut at the maximum


@pytest.mark.parametrize("kind", KINDS)
def test_shortcut_when_the_prefilter_selects_at_most_k_rows(kind):
    _, rid, _, _, _ = spec_side(kind)
    m7 = mask_selecting(rid, 7, 3)
    oi, od, used = run(kind, K, 1, 8, prefilter=m7)
    assert (used == 1).all()
    short = np.isinf(od[:, :7]).any(axis=1)
    assert short.any() and (od[:, 7:] == np.inf).all() and (oi[:, 7:] == V.UNSET).all()
    assert all(sorted(r[:7].tolist()) == np.flatnonzero(m7).tolist() for r in oi)    # found rows first, the rest at +inf by row id
    oi1, _, _ = run(kind, K, None, None, prefilter=m7, nprobes=1)                    # nprobes alone: no extension, no shortcut
    assert (V.found(oi1) < 7).any()


@pytest.mark.parametrize("kind", ("sq", "rq"))
def test_refine_factor_rules_the_shortcut_out(kind):
    _, rid, _, _, _ = spec_side(kind)
    m7 = mask_selecting(rid, 7, 3)
    oi, od, used = run(kind, K, 1, 8, prefilter=m7, rf=3)
    assert (used == 8).all() and (V.found(oi) == 7).all() and np.isfinite(od[:, :7]).all()      # every selected row, re-ranked
    m30 = mask_selecting(rid, 30, 6)
    oi, _, used = run(kind, K, 1, 8, prefilter=m30, rf=3)                            # judged after re-ranking
    assert (used > 1).any() and (V.found(oi) == K).all()


def test_ivfflat_range_starves_queries():
    oi, _, used = run("flat", K, 1, 8, rng=V.STARVING_RANGE)
    assert ((V.found(oi) < K) & (used == 8)).any() and ((V.found(oi) == K) & (used < 8)).any()
    _, rid, _, _, _ = spec_side("flat")
    m7 = mask_selecting(rid, 7, 3)
    oi, od, used = run("flat", K, 1, None, prefilter=m7, rng=(None, 150.0))          # a range rules the shortcut out too
    assert (used == 8).all() and np.isfinite(od[oi != V.UNSET]).all()


@pytest.mark.parametrize("kind", KINDS)
def test_nprobes_alone_means_minimum_and_maximum(kind):
    q, rid, _, spec, _ = spec_side(kind)
    m30 = mask_selecting(rid, 30, 6)
    for n in (1, 3):
        oi, _, used = run(kind, K, None, None, prefilter=m30, nprobes=n)
        assert (used == n).all()
        want, _ = spec(q, K, n, m30, None, None)
        assert (oi == want).all()
    assert (V.found(run(kind, K, None, None, prefilter=m30, nprobes=1)[0]) < K).any()
    run(kind, K, None, 4, prefilter=m30, nprobes=2)                                  # maximum alone: minimum = nprobes
    run(kind, K, 3, 2, prefilter=m30)                                                # maximum below minimum: the minimum holds
    run(kind, K, 20, None, prefilter=m30)                                            # more than there are: all lists
