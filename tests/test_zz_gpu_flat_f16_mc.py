"""Batched flat KNN over a FLOAT16 column on the f16 matrix cores (lance_amd/csrc/flat_mfma_f16.hip): v_mfma_f32_32x32x16_f16 filters the
(query, row) pairs from the column and the queries as they are stored, and the pairs that can beat a query's threshold are recomputed in
the reference's arithmetic for half::f16 (l2.rs:57-91 16-lane order, dot.rs:91-102 32-lane order, cosine.rs:171-179 cosine_scalar) -- so
row ids and distance bits must equal the oracle's flat_knn (pinned on the reference by tests/test_oracle_golden.py), for L2, dot and
cosine at any d % 8 == 0.  Every case asserts whether the filter ran (`flat_mfma_f16` stage counter): on the code before that file the
counter never moves.  n is about 6000: rows 0..2047 go to the exact first epoch, the rest to one (k <= 10) or two (k = 128) matrix epochs."""
import numpy as np
import pytest

import flat_range_spec as R

pytestmark = pytest.mark.gpu
f16 = np.float16
ULP = 2.0 ** -10      # of an f16 in [1, 2)


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _ran(eng):
    return eng.timing_query("count:flat_mfma_f16")[1]


def _check(eng, oracle, x, q, k, metric, row_ids=None, tag=None, expect=True, lower=None, upper=None, drop_nan=False):
    before = _ran(eng)
    gi, gd = eng.flat_topk(x, q, k, metric, row_ids=row_ids, lower=lower, upper=upper)
    assert (_ran(eng) > before) == expect, (tag, "f16 matrix-core filter " + ("not taken" if expect else "taken unexpectedly"))
    gi = gi.cpu().numpy().view(np.uint64); gd = gd.cpu().numpy()
    if lower is not None or upper is not None:
        oi, od = R.select(*R.every_row(oracle, x, q, metric, row_ids), k, lower, upper)
    elif drop_nan:      # a NaN the division makes (inf / inf) has the dividing machine's sign: compared without (test_zz_gpu_flat_wide.py)
        ai, ad = oracle.flat_knn(x, q, k + 4, metric, row_ids=row_ids)
        oi = np.stack([r[~np.isnan(v)][:k] for r, v in zip(ai, ad)]); od = np.stack([v[~np.isnan(v)][:k] for v in ad])
    else:
        oi, od = oracle.flat_knn(x, q, k, metric, row_ids=row_ids)
    bad = np.nonzero((gi != oi).any(axis=1))[0]
    assert bad.size == 0, (tag, f"ids differ for {bad.size} of {q.shape[0]} queries, first {bad[:5]}")
    assert (gd.view(np.uint32) == od.view(np.uint32)).all(), (tag, "distance bits differ")
    return gd


def _data(rng, n, nq, d, integer=False):
    centers = rng.normal(0, 1.0, (24, d))
    x = centers[rng.integers(0, 24, n)] + rng.normal(0, 0.35, (n, d))
    q = centers[rng.integers(0, 24, nq)] + rng.normal(0, 0.35, (nq, d))
    if integer:
        x, q = np.rint(x * 20), np.rint(q * 20)
    return x.astype(f16), q.astype(f16)


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
@pytest.mark.parametrize("d", [40, 72, 64, 200, 768, 1536])      # 40, 72: a stage tail that is % 8 only; 64 under L2: the fixed-dimension route
def test_matches_the_oracle(eng, oracle, d, metric):
    rng = np.random.default_rng(2000 + d)
    x, q = _data(rng, 6001, 150, d)
    x[3000] = x[7]; x[5000] = x[7]; x[5500] = x[2100]; q[0] = x[7]; q[1] = x[2100]      # exact ties: the smaller row id first
    for k in (10, 1, 128):
        _check(eng, oracle, x, q, k, metric, tag=(d, metric, k), expect=not (metric == "l2" and d == 64))


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_integer_rows_mass_ties_and_row_ids(eng, oracle, metric):
    """Integer-valued rows: many exactly equal distances around every threshold; 3000 copies of one row (more than a queue holds: the
    repair decides); row ids unrelated to the storage order."""
    rng = np.random.default_rng(7)
    n, d = 6100, 72
    x, q = _data(rng, n, 140, d, integer=True)
    x[2500:5500] = x[9]
    q[:20] = x[9] + rng.integers(0, 2, (20, d)).astype(f16)
    rid = rng.permutation(n).astype(np.uint64) * 3 + 5
    _check(eng, oracle, x, q, 10, metric, row_ids=rid, tag=("ties", metric))


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_degenerate_elements(eng, oracle, metric):
    """Past row 2048, where the matrix filter sees them: a row of f16 subnormals, a row of 65504, a row with one inf, a row with one NaN,
    a query of subnormals; under L2 and dot a zero row and a zero query too (cosine: 0 / 0, left to test_zz_gpu_flat_wide.py's treatment)."""
    rng = np.random.default_rng(9)
    x, q = _data(rng, 6003, 140, 200)
    x[3000] = (x[3000].astype(np.float32) * 2.0 ** -20).astype(f16)
    x[3001] = 65504.0
    x[3002, 5] = np.inf
    x[3003, 7] = np.nan
    q[3] = (q[3].astype(np.float32) * 2.0 ** -20).astype(f16)
    assert 0 < np.abs(x[3000]).max() < 2.0 ** -14 and 0 < np.abs(q[3]).max() < 2.0 ** -14
    if metric != "cosine":
        x[3004] = 0.0; q[4] = 0.0
    _check(eng, oracle, x, q, 10, metric, tag=("degenerate", metric), drop_nan=metric == "cosine")


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_accumulation_worst_case(eng, oracle, metric):
    """d = 4096, every element positive in [1, 2): nothing cancels in the f32 accumulation.  Each query has a base vector; 12 rows that
    differ from it in 1 to 5 elements by one f16 ulp arrive after a first epoch whose 12 farther variants (20 to 40 elements lowered by
    an ulp) already set a tight threshold.  The near rows carry the smallest row ids, so they win the ties cosine's f32 cannot resolve."""
    rng = np.random.default_rng(17)
    d, nq = 4096, 128
    base = 1.5 + rng.integers(0, 510, (nq, d)) * ULP

    def variants(lo, hi, sign):
        out = np.repeat(base, 12, axis=0)
        for r in out:
            at = rng.choice(d, int(rng.integers(lo, hi + 1)), replace=False)
            r[at] += ULP * (sign if sign else rng.choice([-1.0, 1.0], at.size))
        return out

    first, near = variants(20, 40, -1.0), variants(1, 5, 0)
    filler = 1.0 + rng.integers(0, 512, (1928, d)) * ULP
    x = np.concatenate([first, filler[:512], filler[512:1512], near, filler[1512:]]).astype(f16)      # near: rows 3048 .. 4583
    q = base.astype(f16)
    rid = np.arange(x.shape[0], dtype=np.uint64) + 5000
    rid[3048:4584] = np.arange(1536, dtype=np.uint64)
    oi, _ = oracle.flat_knn(x, q, 10, metric, row_ids=rid)
    assert (oi < 1536).any(axis=1).all(), "the fixture shows nothing: the oracle ranks the near rows outside the top k"
    _check(eng, oracle, x, q, 10, metric, row_ids=rid, tag=("accumulation", metric))


def test_many_query_chunks(eng, oracle):
    """More queries than one pass takes (2048): the row constants are made once; the last 100 queries take the route from before."""
    rng = np.random.default_rng(13)
    x, q = _data(rng, 5000, 2048 + 100, 72)
    _check(eng, oracle, x, q, 10, "cosine", tag="chunks")


def test_gate(eng, oracle):
    rng = np.random.default_rng(11)
    x, q = _data(rng, 6001, 140, 72)
    _check(eng, oracle, x, q[:100], 10, "dot", tag="nq < 128", expect=False)
    dist = _check(eng, oracle, x, q, 64, "dot", tag="un-ranged")[0]
    lo, hi = float(dist[5]), float(dist[60])      # rows lie exactly on both bounds
    _check(eng, oracle, x, q, 10, "dot", tag="lower", expect=False, lower=lo)
    _check(eng, oracle, x, q, 10, "dot", tag="upper alone", expect=True, upper=hi)
