"""The operand-magnitude fixtures (tests/magnitude_spec.py) checked on the oracle alone: what tests/test_zz_gpu_magnitude.py compares the
kernels with is what this file says it is.

  * invariance: at every exponent the spec labels `invariant` (every square the reference forms is normal, every sum finite) the
    oracle's ids, codes and probes equal the unscaled ones and its distances equal base x 4^e bit for bit;
  * at every exponent labelled `subnormal` the oracle's distances really hold f32 subnormals;
  * the dot fixtures are NaN-free (above 2^58 the reference generates inf - inf, whose sign belongs to the host CPU);
  * the derived exponents straddle 2^-100 for every route shape, and the top of the range;
  * the fixtures can see the bug class: a numpy model of flat_mfma.hip's filter WITHOUT a lower guard rejects true neighbours at the
    subnormal exponents, the guarded model rejects none anywhere.  Measured on the committed seeds (d = 64, n = 6000, nq = 130):
    k = 10: 124 of 1300 neighbours rejected at 2^-75, 13 at 2^-72, 0 from 2^-70 to 2^58; all 1300 at 2^60, where |q|^2 overflows and
    T - |q|^2 is a NaN -- the unguarded model has no upper guard on the query side either.  d = 128: 98 / 10 at 2^-75 / 2^-72, 1279 at 2^59.

Wall time on the CPU: 35 tests in 15 s."""
import numpy as np
import pytest

import magnitude_spec as M

f32 = np.float32


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def answer(oracle, fx):
    """the oracle's answer for a fixture -> ({name: integer array}, {name: f32 array})"""
    with np.errstate(all="ignore"):
        if fx.kind == "flat":
            i, d = oracle.flat_knn(fx.x, fx.q, 100)
            return {"ids": i}, {"dists": d}
        if fx.kind == "assign":
            i, d = oracle.assign(fx.x, fx.cent)
            return {"part": i}, {"dists": d}
        if fx.kind == "coarse":
            i, d = oracle.find_partitions(fx.q, fx.cent, 10)
            return {"probes": i}, {"dists": d}
        if fx.kind == "xform":
            part, d = oracle.assign(fx.x, fx.cent)
            codes = oracle.pq_encode(oracle.residual(fx.x, fx.cent, part), fx.cb)
            return {"part": part, "codes": codes}, {"dists": d}
        if fx.kind == "ivfflat":
            i, d = oracle.ivfflat_search(fx.x, fx.cent, fx.q, 10, 4)
            return {"ids": i}, {"dists": d}
        if fx.kind == "ivfpq":
            idx = oracle.build_index(fx.x, fx.cent, fx.cb)
            i0, d0 = idx.search(fx.q, 10, 8)
            i4, d4 = idx.search(fx.q, 10, 8, refine=4, raw=fx.x)
            return {"part": idx.part_ids, "codes": idx.codes_rowmajor, "ids": i0, "ids_refined": i4}, {"dists": d0, "dists_refined": d4}
    raise KeyError(fx.kind)


CASES = {
    "flat-64": (lambda: M.flat_fixture(64), "flat", [("x", "q")]),
    "assign-64": (lambda: M.assign_fixture(64), "assign", [("x", "cent")]),
    "coarse-64x100": (lambda: M.coarse_fixture(64, 100), "coarse", [("q", "cent")]),
    "xform-32x4": (lambda: M.xform_fixture(32, 4), "xform", [("x", "cent")]),
    "ivfflat": (lambda: M.ivfflat_fixture(), "assign", [("x", "cent"), ("q", "cent"), ("x", "q")]),
    "ivfpq": (lambda: M.ivfpq_fixture("f32", n=6000, nq=200), "assign", [("x", "cent"), ("q", "cent")]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_labels_hold_on_the_oracle(oracle, name):
    make, route, pairs = CASES[name]
    fx = make()
    ints0, flts0 = answer(oracle, fx)
    d0 = flts0["dists"]
    dist_lo = float(d0[np.isfinite(d0) & (d0 > 0)].min())
    smallest, largest2 = M.smallest_term(fx, pairs), M.largest_norm2(fx)
    labels = {e: M.classify(e, smallest, largest2, dist_lo) for e in M.exponents_for(route, fx)}
    print(name, labels)
    assert labels[0] == labels[-30] == labels[30] == "invariant" and labels[-75] == "subnormal"
    assert "overflow" in labels.values()
    for e, label in labels.items():
        if label == "invariant":
            ints, flts = answer(oracle, M.scaled(fx, e))
            for k in ints0:
                assert (ints[k] == ints0[k]).all(), (name, e, k)
            for k in flts0:
                assert (_bits(flts[k]) == _bits(flts0[k] * M.pow2(e) * M.pow2(e))).all(), (name, e, k)
        elif label == "subnormal":
            _, flts = answer(oracle, M.scaled(fx, e))
            assert M.has_subnormals(flts["dists"]), (name, e)


ROUTE_SHAPES = [("flat", lambda: M.flat_fixture(64)), ("flat", lambda: M.flat_fixture(128)), ("flat_wide", lambda: M.flat_fixture(256)),
                ("assign", lambda: M.assign_fixture(64)), ("assign", lambda: M.assign_fixture(128)), ("assign", lambda: M.assign_fixture(256, n=3000, k=64)),
                ("coarse", lambda: M.coarse_fixture(64, 100)), ("coarse", lambda: M.coarse_fixture(128, 960)), ("coarse", lambda: M.coarse_fixture(64, 1024)),
                ("xform", lambda: M.xform_fixture(32, 4)), ("xform", lambda: M.xform_fixture(128, 16)),
                ("pq", lambda: M.xform_fixture(32, 4)), ("pq", lambda: M.xform_fixture(128, 16))]


@pytest.mark.parametrize("route,make", ROUTE_SHAPES, ids=[f"{r}-{i}" for i, (r, _) in enumerate(ROUTE_SHAPES)])
def test_guard_exponents_straddle_the_guard(route, make):
    """the derived exponents: at the two lowest near-guard exponents EVERY row's E2 is <= 2^-100, at the two highest every row's is
    above; the overflow exponents straddle the point where the largest |x|^2 leaves f32"""
    fx = make()
    near = M.guard_exponents(route, fx)
    guard = 2.0 ** M.GUARD_LOG2
    lo, hi = M.e2_range(route, fx)
    assert len(near) >= 4 and near == tuple(range(near[0], near[-1] + 1))
    assert all(hi * 4.0 ** e <= guard for e in near[:2]) and all(lo * 4.0 ** e > guard for e in near[-2:])
    assert hi * 4.0 ** near[0] > guard / 2 ** 6 and lo * 4.0 ** near[-1] < guard * 2 ** 6          # ... and close to it
    top = M.overflow_exponents(fx)
    big = M.largest_norm2(fx)
    assert len(top) >= 3 and big * 4.0 ** top[0] < 2.0 ** 128 and big * 4.0 ** top[1] < 2.0 ** 128 <= big * 4.0 ** top[2]
    # the same in f32, as a kernel sums it
    with np.errstate(over="ignore"):
        for e, finite in ((top[1], True), (top[2], False)):
            s = M.scaled(fx, e)
            n2 = max(float((a.astype(f32) ** 2).sum(axis=-1, dtype=f32).max()) for a in (s[k] for k in M.FLOAT_KEYS if k in s))
            assert np.isfinite(n2) == finite, (e, n2)
    sweep = M.exponents_for(route, fx)
    assert set(M.FIXED) <= set(sweep) and sweep[0] == -75 and 56 <= sweep[-1] <= 60 and -53 <= near[0] and near[-1] <= -45


def test_mscan_predicate_flips_inside_the_sweep(oracle):
    """search_ms.hip's pair predicate for a typical pair of the scan fixture: true at e = 0, false at both ends, and the exponents
    where it flips are in the route's sweep"""
    fx = M.ivfpq_fixture("f32", n=6000, nq=200)
    idx = oracle.build_index(fx.x, fx.cent, fx.cb)
    T0 = float(np.median(idx.search(fx.q, 10, 8)[1][:, -1]))
    flips, ok = M.mscan_exponents(fx, T0)
    print("mscan flips", flips)
    assert ok(0) and ok(-30) and ok(30) and not ok(-75) and not ok(64)
    assert len(flips) >= 4 and set(flips) <= set(M.exponents_for("mscan", fx, T0))
    for a, b in zip(flips[::2], flips[1::2]):
        assert b == a + 1 and ok(a) != ok(b)


def _ivfpq_dot(oracle, f):
    idx = oracle.build_index(f.x, f.cent, f.cb, "dot")
    return np.concatenate([idx.search(f.q, 10, 8)[1], idx.search(f.q, 10, 8, refine=4, raw=f.x)[1]])


def _xform_dot(oracle, f):
    """the transform has no distances of its own to return: the assign distances its loss sums"""
    return oracle.assign(f.x, f.cent, "dot")[1]


def _sq_dot(oracle, f):
    import refine_spec as F
    import sq_spec as S
    xs, part = S.prepare_rows(oracle, f.x, f.cent, "dot")
    b = S.bounds(xs[:64])
    codes = S.encode(xs, *b)
    rid = np.arange(f.x.shape[0], dtype=np.uint64)
    d0 = S.search(oracle, codes, part, f.cent, f.q, 10, 4, "dot", *b, row_ids=rid)[1]
    cand = S.search(oracle, codes, part, f.cent, f.q, 40, 4, "dot", *b, row_ids=rid)[0]
    return np.concatenate([d0, F.refine(oracle, cand, f.x, f.q, 10, "dot")[1]])


def _rq_dot(oracle, f):
    import refine_spec as F
    import rq_spec as R
    P = R.rotation(64, 7)
    part, codes, add, scale = R.build(oracle, f.x, f.cent, P, "dot")
    rid = np.arange(f.x.shape[0], dtype=np.uint64)
    d0 = R.search(oracle, codes, add, scale, part, f.cent, P, f.q, 10, 4, "dot", row_ids=rid)[1]
    cand = R.search(oracle, codes, add, scale, part, f.cent, P, f.q, 40, 4, "dot", row_ids=rid)[0]
    return np.concatenate([d0.ravel(), F.refine(oracle, cand, f.x, f.q, 10, "dot")[1].ravel(), add.ravel(), scale.ravel()])


DOT_CASES = {
    "flat-64": (lambda: M.flat_fixture(64), lambda o, f: o.flat_knn(f.x, f.q, 100, "dot")[1]),
    "flat-128": (lambda: M.flat_fixture(128), lambda o, f: o.flat_knn(f.x, f.q, 100, "dot")[1]),
    "flat-256": (lambda: M.flat_fixture(256), lambda o, f: o.flat_knn(f.x, f.q, 100, "dot")[1]),
    "assign-64": (lambda: M.assign_fixture(64), lambda o, f: o.assign(f.x, f.cent, "dot")[1]),
    "assign-128": (lambda: M.assign_fixture(128), lambda o, f: o.assign(f.x, f.cent, "dot")[1]),
    "coarse-64x100": (lambda: M.coarse_fixture(64, 100), lambda o, f: o.find_partitions(f.q, f.cent, 10, "dot")[1]),
    "ivfflat": (lambda: M.ivfflat_fixture(), lambda o, f: o.ivfflat_search(f.x, f.cent, f.q, 10, 4, "dot")[1]),
    "ivfpq": (lambda: M.ivfpq_fixture("f32", metric="dot"), _ivfpq_dot),
    "xform-32x4": (lambda: M.xform_fixture(32, 4, metric="dot"), _xform_dot),
    "xform-128x16": (lambda: M.xform_fixture(128, 16, metric="dot"), _xform_dot),
    "ivf_sq": (lambda: M.sqrq_fixture(metric="dot"), _sq_dot),
    "ivf_rq": (lambda: M.sqrq_fixture(metric="dot"), _rq_dot),
}


@pytest.mark.parametrize("name", list(DOT_CASES))
def test_dot_fixtures_hold_no_nan(oracle, name):
    """every dot fixture the GPU test compares with, at every exponent of DOT_EXPONENTS (the GPU test checks each answer again)"""
    make, call = DOT_CASES[name]
    fx = make()
    for e in M.DOT_EXPONENTS:
        with np.errstate(all="ignore"):
            d = call(oracle, M.scaled(fx, e))
        assert not np.isnan(d).any(), (name, e)


def test_f16_columns():
    """at 2^-13 at least a third of the elements are binary16 subnormals; at 2^3 nothing is near 65504"""
    share = {s: M.f16_subnormal_share(M.f16_fixture(s).x) for s in M.F16_SCALES}
    print(share)
    assert share[-13] >= 1 / 3 and share[-13] > share[-11] > share[-8] > share[3]
    big = M.f16_fixture(3)
    assert np.isfinite(big.x.astype(f32)).all() and np.abs(big.x.astype(f32)).max() <= 60000


def test_mixed_scale_and_offset_fixtures(oracle):
    fx = M.assign_fixture(64)
    mixed = M.mixed_cases(fx)
    assert set(mixed) == {"row block 2^58", "centroid 2^40"}
    # the flat fixtures: the scaled block lies past the first epoch (the exact kernel's), and some block is past the filters' 2^126 guard
    # on |x|^2 while its queries are not -- at d = 64 only the 2^59 block is
    for d in (64, 128, 256):
        ff = M.flat_fixture(d)
        fm = M.mixed_cases(ff)
        assert set(fm) == {"rows 2^-52", "queries 2^-52", "row block 2^58", "row block 2^59"}
        b0 = M.row_block_start(ff)
        assert b0 >= M.FLAT_FIRST_EPOCH and b0 % 128 and b0 + 128 <= ff.x.shape[0]
        assert M.n2(ff.q).max() < 2.0 ** 20
        for e, past in ((58, d >= 128), (59, True)):
            x = fm[f"row block 2^{e}"].x
            changed = np.nonzero((x != ff.x).any(axis=1))[0]
            assert changed[0] == b0 and changed[-1] == b0 + 127 and len(changed) == 128
            n2 = M.n2(x[b0:b0 + 128])      # (d = 128 at 2^58: 2^126.2 on average, a few rows of the block stay below the guard)
            assert (np.median(n2) >= 2.0 ** 126) == past and (n2.max() < 2.0 ** 126) == (not past), (d, e)
    c = mixed["centroid 2^40"].cent
    assert M.n2(c).max() > 2.0 ** 80 and np.isfinite((c.astype(f32) ** 2).sum(axis=1, dtype=f32)).all()
    # offset: the margin 2^-12 (|x|^2 + max|c|^2) against the gap between the nearest and the second centroid
    for r in M.OFFSETS:
        o = M.offset(fx, r)
        assert o.cent.shape == fx.cent.shape and not (o.cent == fx.cent).all()
        assert abs(float(o.x.mean()) - 2.0 ** r) < 1.0
    # the reference answers the flat offset fixtures without a tie at the k-th place
    for r in M.OFFSETS:
        o = M.offset(M.flat_fixture(64), r)
        d = oracle.flat_knn(o.x, o.q, 11)[1]
        assert (d[:, 9] < d[:, 10]).all(), r


def test_the_flat_fixture_can_see_an_unguarded_filter(oracle):
    """the numbers in this file's docstring"""
    fx = M.flat_fixture(64)
    seen = {}
    for e in M.exponents_for("flat", fx):
        s = M.scaled(fx, e)
        with np.errstate(all="ignore"):
            ids, dists = oracle.flat_knn(s.x, s.q, 10)
        seen[e] = (M.rejected_neighbours(s.x, s.q, ids, dists, guard=False), M.rejected_neighbours(s.x, s.q, ids, dists, guard=True))
    print(seen)
    assert all(g == 0 for _, g in seen.values()), seen
    assert seen[-72][0] >= 1 and seen[-75][0] >= 1, seen
    assert seen[0][0] == 0 and seen[-30][0] == 0 and seen[30][0] == 0
