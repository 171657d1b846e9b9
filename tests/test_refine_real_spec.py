"""CPU checks of tests/refine_real_spec.py: the fixtures of tests/test_zz_gpu_refine_real.py can tell a kernel that sums in the reference's
order from one that does not, and an integer-valued column cannot.  For every (kind, metric, d) of the GPU grid:
  * the numpy model of the reference's sum equals oracle.flat_knn bit for bit on the fixture's candidate lists;
  * every wrong order (half the lane accumulators; multiply-then-add for the fused multiply-add of f32 cosine; the pair kernel's fold
    with its halves swapped; the four-lane cosine path's shuffles in the other order) changes the distance
    bits of at least a quarter of all candidates, and at least one returned (id, distance bits) row at k = 10, refine_factor = 10;
    where the sums are exact whatever the order (int8 rows up to d = 128) it changes nothing, and the test says so instead;
  * the layout: the spoiled rows are candidates, their NaN distances sort last, the equal rows lie across rank k and rank keff."""
import functools

import numpy as np
import pytest

import refine_real_spec as S

f32 = np.float32


@functools.lru_cache(maxsize=None)
def _candidates(kind, metric, d):
    fx = S.fixture(kind, metric, d)
    cand, _ = fx.oidx.search(S.oracle_rows(fx.q), S.KEFF, S.NLIST)
    return fx, cand


def _flat_knn_refine(oracle, fx, cand, raw, q, k):
    """the specification of the refine: flat_knn over the taken rows (tests/refine_spec.py), in the column's element type"""
    import refine_spec as F
    return F.refine(oracle, cand, S.oracle_rows(raw), np.asarray(q).astype(f32), k, fx.metric)


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


GRID = [(arm, d) for arm, _, _, d in S.GRID]
IDS = [f"{a}-{d}" for a, d in GRID]


@pytest.mark.parametrize("arm,d", GRID, ids=IDS)
def test_reference_model_equals_the_oracle(oracle, arm, d):
    kind, metric, _ = S.ARMS[arm]
    fx, cand = _candidates(kind, metric, d)
    oi, od = _flat_knn_refine(oracle, fx, cand, fx.x, fx.q, S.KEFF)
    mi, md, every = S.refine_with(lambda q, rows: S.model(metric, kind, q, rows), cand, fx.x, fx.q, S.KEFF)
    assert (mi == oi).all() and (_bits(md) == _bits(od)).all()
    # and per candidate, against the function flat_knn uses
    for qi in (S.Q_SHORT, S.Q_DUP, S.NQ - 1):
        ok = cand[qi] != S.NONE_ID
        assert (_bits(every[qi, ok]) == _bits(S.oracle_distances(metric, fx.q[qi], fx.x[cand[qi][ok].astype(np.int64)]))).all()


@pytest.mark.parametrize("arm,d", GRID, ids=IDS)
def test_wrong_orders_show(oracle, arm, d):
    kind, metric, _ = S.ARMS[arm]
    fx, cand = _candidates(kind, metric, d)
    valid = cand != S.NONE_ID
    _, _, ref = S.refine_with(lambda q, rows: S.oracle_distances(metric, q, rows), cand, fx.x, fx.q, S.K)
    oi, od = fx.oidx.search(S.oracle_rows(fx.q), S.K, S.NLIST, refine=S.RF, raw=S.oracle_rows(fx.x).astype(f32))
    names = list(S.wrong_order(metric, kind, fx.q[0], fx.x[:1]))
    assert "half_lanes" in names and (("no_fma" in names) == (metric == "cosine" and kind != "f16" and d not in (8, 16)))
    assert ("fold_halves_swapped" in names) == arm.endswith("-pair") and ("quad_pairs_swapped" in names) == arm.endswith("-wide")
    for name in names:
        wi, wd, every = S.refine_with(lambda q, rows: S.wrong_order(metric, kind, q, rows)[name], cand, fx.x, fx.q, S.K)
        share = float((_bits(every) != _bits(ref))[valid].mean())
        rows_changed = int(((wi != oi) | (_bits(wd) != _bits(od))).any(axis=1).sum())
        print(f"{arm} d={d} {name}: {share:.3f} of the candidates' distance bits differ, {rows_changed} of {S.NQ} returned rows change")
        if S.order_shows(kind, metric, d):
            assert share >= 0.25, (arm, d, name, share)
            assert rows_changed >= 1, (arm, d, name)
        else:
            assert share == 0.0 and rows_changed == 0, (arm, d, name, "the sums were to be exact whatever the order")


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
@pytest.mark.parametrize("d", [100, 128])
def test_integer_columns_cannot_see_the_order(oracle, metric, d):
    """the reason for refine_real_spec.py: on a SIFT-like column (integers 0 .. 218) no wrong order changes one bit"""
    x, q = S.sift_like(2000, d, 5), S.sift_like(16, d, 6)
    cand, _ = oracle.flat_knn(x, q, S.KEFF, metric)
    _, _, ref = S.refine_with(lambda qq, rows: S.oracle_distances(metric, qq, rows), cand, x, q, S.K)
    for order in ("reference", "half_lanes") + (("no_fma",) if metric == "cosine" else ()):
        _, _, every = S.refine_with(lambda qq, rows: S.model(metric, "f32", qq, rows, order), cand, x, q, S.K)
        assert (_bits(every) == _bits(ref)).all(), (metric, d, order)


def _spoiled():
    import test_zz_gpu_refine_real as R
    return R.SPOILED


@pytest.mark.parametrize("kind,metric,d", _spoiled())
def test_spoiled_rows_and_the_equal_rows(oracle, kind, metric, d):
    fx, raw, rows, what, qs = S.spoiled_fixture(kind, metric, d)
    assert set(what) == set(S.spoils_for(kind, metric)) and len(rows) == 40
    assert (raw[rows].view(np.uint8) != fx.x[rows].view(np.uint8)).any(axis=1).all()
    assert not (metric == "cosine" and (raw.astype(f32) == 0).all(axis=1).any()), "an all-zero row under cosine"
    qo, rawo = S.oracle_rows(qs), S.oracle_rows(raw).astype(f32)
    cand, _ = fx.oidx.search(qo, S.KEFF, S.NLIST)
    assert np.isin(rows, cand).all(), ("changed rows that are no candidate", rows[~np.isin(rows, cand)])
    _, part = S._sizes(kind, metric, fx.x, fx.cent)
    assert len(set(part[rows].tolist())) >= 5, "the changed rows are to be spread over the lists"
    # every candidate returned: the rows with a NaN element come last, as the positive NaN
    oi, od = fx.oidx.search(qo, S.KEFF, S.NLIST, refine=1, raw=rawo)
    nan_rows = rows[np.array(what) == "nan"]
    met = 0
    for r in range(len(qs)):
        isn = np.isnan(od[r])
        c = int((~isn).sum())
        assert not isn[:c].any() and isn[c:].all()
        assert (_bits(od[r, c:]) == 0x7FC00000).all() and np.isin(oi[r, c:], nan_rows).all()
        met += S.KEFF - c
    assert met >= len(nan_rows)
    # the equal rows, for the last query: across keff in the candidate list (which of them are in is the partition heap's business:
    # not the lowest ids), across k in the answer (the lowest ids of those)
    inside = cand[-1][np.isin(cand[-1], fx.block)]
    assert 0 < inside.size < S.NDUP
    ri, rd = fx.oidx.search(qo[-1:], S.K, S.NLIST, refine=S.RF, raw=rawo)
    tied = np.sort(np.concatenate([inside, [np.uint64(fx.tie)]]))
    ahead = int((_bits(rd[0]) != _bits(rd[0, -1:])).sum())      # (a row of 1e-30 among the candidates: -inf under cosine, first)
    assert ahead <= 2 and tied.size > S.K and (ri[0, ahead:] == tied[:S.K - ahead]).all(), "the tie does not lie across the k-th place"
