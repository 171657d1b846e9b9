"""The combined search on the GPU: lance_hip_take_flat_knn alone and lance_amd.VectorColumn.nearest over every index type,
ids and distance BITS against tests/knn_combined_spec.py (the reference plan in numpy on the oracle's pieces;
tests/test_knn_combined_spec.py shows on the CPU that its fixtures tell it from three wrong variants).

take_flat_knn: every row reader -- 16-byte words (d * element size a multiple of 16, column on the 16-byte grid), element by element (any
other d, a column off the grid), rows read in place (a row longer than a wave's 8 KiB slice: d = 2100) --, every element type and metric,
the limits of k and of the candidate count, empty slots, ties across the lists, duplicated ids, rows with NaN / inf elements, bounds that
lie exactly on returned distances, and a row id beyond the column.
VectorColumn: each layout of deltas and unindexed fragment runs the issue names; the indices are built on the GPU (create_delta), the
specification is given their model and the rows they store."""
import numpy as np
import pytest
import torch

import flat_range_spec as FR
import knn_combined_spec as KC

pytestmark = pytest.mark.gpu
f32 = np.float32
METRICS = ["l2", "dot", "cosine"]


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _dev(a):
    import lance_amd.engine as E
    return E.to_device(a)


def _i64(ids):
    return np.ascontiguousarray(np.asarray(ids, np.uint64)).view(np.int64)


def _eq(got, want, tag=None):
    gi = (got[0].cpu().numpy() if isinstance(got[0], torch.Tensor) else np.asarray(got[0])).view(np.uint64)
    gd = got[1].cpu().numpy() if isinstance(got[1], torch.Tensor) else np.asarray(got[1])
    assert (gi == want[0]).all(), (tag, np.argwhere(gi != want[0])[:5])
    assert (gd.view(np.uint32) == want[1].view(np.uint32)).all(), (tag, np.argwhere(gd.view(np.uint32) != want[1].view(np.uint32))[:5])


def _take(eng, oracle, x, q, a, k, metric, b=None, db=None, lower=None, upper=None, tag=None, xd=None, qd=None):
    got = eng.take_flat_knn(_dev(x) if xd is None else xd, _dev(q) if qd is None else qd, _i64(a), k, metric, ids_b=None if b is None else _i64(b),
                            dists_b=db, lower=lower, upper=upper)
    want = KC.take_flat_knn(oracle, x, q, a, k, metric, ids_b=b, dists_b=db, lower=lower, upper=upper)
    _eq(got, want, tag)
    return want


def _lists(n, nq, ca, cb, seed, holes=True):
    """random candidate lists with empty slots and ids present in both"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, (nq, ca)).astype(np.uint64)
    b = rng.integers(0, n, (nq, cb)).astype(np.uint64) if cb else None
    if holes:
        a[rng.random(a.shape) < 0.1] = KC.UNSET
        if cb:
            b[rng.random(b.shape) < 0.1] = KC.UNSET
            b[:, 0] = a[:, min(1, ca - 1)]
    return a, b


def _rows(n, d, nq, seed, dtype="float32"):
    rng = np.random.default_rng(seed)
    if dtype == "int8":
        return rng.integers(-100, 101, (n, d)).astype(np.int8), rng.integers(-100, 101, (nq, d)).astype(np.int8)
    x = (rng.standard_normal((n, d)) * 1.5 + 0.25).astype(dtype)
    q = (rng.standard_normal((nq, d)) * 1.5 - 0.25).astype(dtype)
    return x, q


# ---- take_flat_knn alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [1, 3, 32, 128, 1536, 2100])
def test_take_row_lengths(eng, oracle, d):
    """f32 rows: 16-byte words at d = 32, 128, 1536 (1536: one 6 KiB row per wave and step), element by element at d = 1, 3, in place at 2100"""
    x, q = _rows(400, d, 5, d)
    a, b = _lists(400, 5, 40, 25, d + 1)
    for metric in METRICS:
        _take(eng, oracle, x, q, a, 10, metric, b=b, tag=(d, metric))


@pytest.mark.parametrize("dtype", ["float16", "int8"])
@pytest.mark.parametrize("metric", METRICS)
def test_take_element_types(eng, oracle, dtype, metric):
    """f16: half::f16's 32-lane dot / cosine and the widened 16-lane L2; int8: widened rows, cosine refused.  d = 40 / 48 are whole 16-byte
    words (f16 / int8), d = 33 is not; d = 5000 (f16) / 9000 (int8) rows are read in place"""
    from lance_amd import _lib
    for d in (48 if dtype == "int8" else 40, 33, 9000 if dtype == "int8" else 5000):
        n = 300 if d < 100 else 40
        x, q = _rows(n, d, 4, d, dtype)
        a, b = _lists(n, 4, 30, 35, d + 2)
        if dtype == "int8" and metric == "cosine":
            with pytest.raises(_lib.LanceHipError) as e:
                eng.take_flat_knn(_dev(x), _dev(q), _i64(a), 10, metric, ids_b=_i64(b))
            assert e.value.code == _lib.EINVAL and "int8 cosine" in str(e.value)
        else:
            _take(eng, oracle, x, q, a, 10, metric, b=b, tag=(dtype, d))


def test_take_k_and_candidate_limits(eng, oracle):
    """k in {1, 10, 1024} x ca + cb in {1, 65, 4096}; fewer candidates than k; beyond either limit: LANCE_HIP_EINVAL"""
    from lance_amd import _lib
    x, q = _rows(6000, 32, 3, 7)
    for ca, cb in ((1, 0), (40, 25), (3072, 1024)):
        a, b = _lists(6000, 3, ca, cb, ca, holes=ca > 1)
        for k in (1, 10, 1024):
            _take(eng, oracle, x, q, a, k, "l2", b=b, tag=(ca, cb, k))
    a, b = _lists(6000, 3, 4000, 97, 3)
    for kw in (dict(k=10, ids_b=_i64(b)), dict(k=1025), dict(k=0)):
        with pytest.raises(_lib.LanceHipError) as e:
            eng.take_flat_knn(_dev(x), _dev(q), _i64(a), kw.pop("k"), "l2", **kw)
        assert e.value.code == _lib.EINVAL


def test_take_empty_slots(eng, oracle):
    x, q = _rows(200, 8, 3, 11)
    a = np.full((3, 12), KC.UNSET, np.uint64)
    b = np.full((3, 5), KC.UNSET, np.uint64)
    want = _take(eng, oracle, x, q, a, 10, "l2", b=b, tag="only empty slots")
    assert (want[0] == KC.UNSET).all() and np.isinf(want[1]).all()
    a[0, 7], a[1, 0], b[1, 4] = 5, 6, 7
    want = _take(eng, oracle, x, q, a, 10, "dot", b=b, tag="fewer than k")
    assert (want[0] != KC.UNSET).sum(axis=1).tolist() == [1, 2, 0]


def test_take_ties_and_duplicates(eng, oracle):
    """integer rows in four copies: equal distances across the two lists come back in row id order, a row id in both lists twice"""
    rng = np.random.default_rng(5)
    base = rng.integers(-2, 3, (50, 6)).astype(f32)
    x = np.concatenate([base, base, base, base])
    q = rng.integers(-2, 3, (4, 6)).astype(f32)
    a = np.stack([rng.permutation(200)[:60] for _ in range(4)]).astype(np.uint64)
    b = np.stack([rng.permutation(200)[:60] for _ in range(4)]).astype(np.uint64)
    b[:, :5] = a[:, :5]
    for metric in ("l2", "dot"):
        want = _take(eng, oracle, x, q, a, 40, metric, b=b, tag=metric)
        for i in range(4):
            assert len(set(want[0][i].tolist())) < 40 and len(set(want[1][i].tolist())) < 20      # duplicated ids, and ties
    want = _take(eng, oracle, x, q, np.array([[7, 7, 7]] * 4, np.uint64), 3, "l2")
    assert (want[0] == 7).all()


def test_take_special_rows(eng, oracle, metric="l2"):
    """rows with an element whose square overflows, a positive and a negative NaN element (flat_range_spec.specials, L2 as in
    tests/test_zz_gpu_flat_range.py: the fixture holds no NaN that arithmetic generates, whose sign belongs to the machine)"""
    x, q = _rows(300, 16, 3, 13)
    x, rows = FR.specials(x)
    special = np.concatenate(list(rows.values())).astype(np.uint64)
    a = np.tile(np.concatenate([special, np.arange(30, dtype=np.uint64)]), (3, 1))
    want = _take(eng, oracle, x, q, a, 54, metric, tag="all")
    assert not np.isfinite(want[1]).all()
    _take(eng, oracle, x, q, a, 54, metric, lower=0.0, tag="lower keeps +inf and +NaN")
    _take(eng, oracle, x, q, a, 54, metric, upper=float(np.finfo(f32).max), tag="upper keeps -NaN")


@pytest.mark.parametrize("metric", METRICS)
def test_take_bounds_on_returned_distances(eng, oracle, metric):
    from lance_amd import _lib
    x, q = _rows(500, 24, 4, 17)
    a, b = _lists(500, 4, 50, 30, 19)
    free = _take(eng, oracle, x, q, a, 80, metric, b=b)
    lo, hi = float(free[1][0][4]), float(free[1][0][30])
    for lower, upper in ((lo, hi), (lo, None), (None, hi), (lo, lo), (hi, float(np.nextafter(f32(hi), f32(np.inf))))):
        want = _take(eng, oracle, x, q, a, 10, metric, b=b, lower=lower, upper=upper, tag=(lower, upper))
        if lower == upper:
            assert (want[0] == KC.UNSET).all()
    assert _take(eng, oracle, x, q, a, 10, metric, b=b, lower=lo, upper=hi)[1][0][0] == f32(lo)       # the row ON the lower bound is kept
    with pytest.raises(_lib.LanceHipError) as e:
        eng.take_flat_knn(_dev(x), _dev(q), _i64(a), 10, metric, lower=hi, upper=lo)
    assert e.value.code == _lib.EINVAL


@pytest.mark.parametrize("dtype, d", [("float32", 32), ("float32", 7), ("float16", 40), ("int8", 48)])
def test_take_off_the_16_byte_grid(eng, oracle, dtype, d):
    """the column and the queries one element off the 16-byte grid: the same bits as on it"""
    x, q = _rows(300, d, 3, 23, dtype)
    a, b = _lists(300, 3, 40, 25, 29)
    want = _take(eng, oracle, x, q, a, 10, "l2", b=b)
    xb, qb = torch.zeros(x.size + 16, dtype=_dev(x).dtype, device="cuda"), torch.zeros(q.size + 16, dtype=_dev(q).dtype, device="cuda")
    for shift in (1, 3):
        xs, qs = xb[shift:shift + x.size].view(x.shape), qb[shift:shift + q.size].view(q.shape)
        xs.copy_(_dev(x)); qs.copy_(_dev(q))
        assert xs.data_ptr() % 16 != 0 and qs.data_ptr() % 16 != 0
        for metric in ("l2", "dot"):
            _take(eng, oracle, x, q, a, 10, metric, b=b, xd=xs, qd=qs, tag=shift)
    _eq(eng.take_flat_knn(xs, qs, _i64(a), 10, "l2", ids_b=_i64(b)), want)


def test_take_row_id_beyond_the_column(eng, oracle):
    from lance_amd import _lib
    x, q = _rows(100, 8, 3, 31)
    a, _ = _lists(100, 3, 20, 0, 37)
    for bad in (100, 2 ** 40, 2 ** 64 - 2):
        a2 = a.copy()
        a2[1, 3] = bad
        with pytest.raises(_lib.LanceHipError) as e:
            eng.take_flat_knn(_dev(x), _dev(q), _i64(a2), 5, "l2")
        assert e.value.code == _lib.EINVAL and "n_rows" in str(e.value)
        with pytest.raises(_lib.LanceHipError):
            eng.take_flat_knn(_dev(x), _dev(q), _i64(a), 5, "l2", ids_b=_i64(a2), dists_b=np.zeros(a2.shape, f32))
    _take(eng, oracle, x, q, a, 5, "l2")                   # the context answers the next call


@pytest.mark.parametrize("dtype", ["float32", "float16", "int8"])
def test_take_given_and_recomputed_list_b_are_the_same_bits(eng, oracle, dtype):
    """list B as the flat scan returns it for the unindexed rows: its distances handed over or recomputed"""
    x, q = _rows(3000, 32, 6, 41, dtype)
    a, _ = _lists(2000, 6, 50, 0, 43)
    for metric in METRICS:
        if dtype == "int8" and metric == "cosine":
            continue
        rid = torch.arange(2000, 3000, dtype=torch.int64, device="cuda")
        bi, bd = eng.flat_topk(_dev(x)[2000:], _dev(q), 20, metric, row_ids=rid)
        given = eng.take_flat_knn(_dev(x), _dev(q), _i64(a), 20, metric, ids_b=bi, dists_b=bd)
        again = eng.take_flat_knn(_dev(x), _dev(q), _i64(a), 20, metric, ids_b=bi)
        assert torch.equal(given[0], again[0]) and torch.equal(given[1].view(torch.int32), again[1].view(torch.int32))
        _eq(given, KC.take_flat_knn(oracle, x, q, a, 20, metric, ids_b=bi.cpu().numpy().view(np.uint64)), (dtype, metric))


# ---- VectorColumn ----------------------------------------------------------------------------------------------------------------------
SIZES = [1500, 300, 1200, 1, 999]
N, D, NQ, K, NLIST = sum(SIZES), 32, 6, 10, 8
LAYOUTS = {                                   # the fragments of each delta; the rest is unindexed
    "tail_1_row": [[0, 1, 2, 4]],
    "tail_300_rows": [[0, 2, 3, 4]],
    "two_tail_runs": [[0, 2, 4]],
    "two_deltas_tail": [[0], [2]],
    "three_deltas_no_tail": [[0, 1], [2, 3], [4]],
    "one_delta_no_tail": [[0, 1, 2, 3, 4]],
}
KINDS = {
    "pq8_l2": dict(index_type="IVF_PQ", metric="l2", num_sub_vectors=8, num_bits=8),
    "pq8_cosine": dict(index_type="IVF_PQ", metric="cosine", num_sub_vectors=8, num_bits=8),
    "pq4_l2": dict(index_type="IVF_PQ", metric="l2", num_sub_vectors=8, num_bits=4),
    "flat_l2": dict(index_type="IVF_FLAT", metric="l2"),
    "flat_dot": dict(index_type="IVF_FLAT", metric="dot"),
    "sq_l2": dict(index_type="IVF_SQ", metric="l2"),
    "sq_cosine": dict(index_type="IVF_SQ", metric="cosine"),
    "rq_l2": dict(index_type="IVF_RQ", metric="l2"),
}


@pytest.fixture(scope="module")
def data():
    x = KC.clustered(N, D, 3)
    rng = np.random.default_rng(4)
    q = (x[rng.choice(N, NQ, replace=False)] + rng.standard_normal((NQ, D)).astype(f32) * f32(0.1)).astype(f32)
    allow = rng.random(N) < 0.6
    return x, q, allow


def _build(engine, eng, x, kind, layout):
    col = engine.VectorColumn(x, SIZES, engine=eng)
    for frags in LAYOUTS[layout]:
        col = col.create_delta(frags, num_partitions=NLIST, max_iters=4, engine=eng, **KINDS[kind])
    return col


def _spec_column(oracle, x, kind, col, stored=None):
    """the specification's column from the GPU column's own models; stored: the rows each delta stores when they are not its fragments'"""
    args = KINDS[kind]
    sc = KC.Column(x, args["metric"], SIZES)
    for j, (ix, frags) in enumerate(col._deltas):
        rows = None if stored is None else stored[j]
        cent = ix.centroids
        if args["index_type"] == "IVF_PQ":
            sc.deltas.append(KC.pq_delta(oracle, sc, frags, cent, ix.codebook, nbits=args["num_bits"], rows=rows))
        elif args["index_type"] == "IVF_FLAT":
            sc.deltas.append(KC.flat_delta(oracle, sc, frags, cent, rows=rows))
        elif args["index_type"] == "IVF_SQ":
            sc.deltas.append(KC.sq_delta(oracle, sc, frags, cent, ix.bounds, rows=rows))
        else:
            sc.deltas.append(KC.rq_delta(oracle, sc, frags, cent, ix.rotation, rows=rows))
    return sc


def _range(oracle, x, q, metric):
    """bounds on exact distances query 0 has: rows lie on both"""
    d = oracle.flat_knn(x, q[:1], 40, metric)[1][0]
    return float(d[3]), float(d[30])


def _searches(kind, allow, rng):
    out = [dict(), dict(refine_factor=3), dict(prefilter=allow), dict(refine_factor=2, prefilter=allow)]
    if KINDS[kind]["index_type"] in ("IVF_PQ", "IVF_FLAT"):
        out += [dict(distance_range=rng), dict(distance_range=rng, refine_factor=3, prefilter=allow), dict(distance_range=(rng[0], None))]
    return out


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("kind", list(KINDS))
def test_column_nearest(engine, eng, oracle, data, kind, layout):
    x, q, allow = data
    col = _build(engine, eng, x, kind, layout)
    assert len(col.deltas) == len(LAYOUTS[layout])
    for a, b in zip(col.deltas, col.deltas[1:]):       # create_delta took the first delta's model
        assert (a.centroids.view(np.uint32) == b.centroids.view(np.uint32)).all()
    sc = _spec_column(oracle, x, kind, col)
    metric = KINDS[kind]["metric"]
    for kw in _searches(kind, allow, _range(oracle, x, q, metric)):
        got = col.nearest(q, k=K, nprobes=3, **kw)
        assert got[0].dtype == np.int64 and got[1].dtype == f32
        _eq(got, KC.nearest(oracle, sc, q, k=K, nprobes=3, **kw), (kind, layout, sorted(kw)))
    if layout == "two_tail_runs":
        for kw in (dict(fast_search=True), dict(fast_search=True, refine_factor=2)):
            got = col.nearest(q, k=K, nprobes=3, **kw)
            _eq(got, KC.nearest(oracle, sc, q, k=K, nprobes=3, **kw), (kind, "fast_search"))
            assert not np.isin(got[0], np.arange(1500, 1800)).any()          # no unindexed row
        for kw in (dict(), dict(prefilter=allow, distance_range=_range(oracle, x, q, metric))):
            got = col.nearest(q, k=K, use_index=False, **kw)
            _eq(got, KC.nearest(oracle, sc, q, k=K, use_index=False, **kw), (kind, "use_index=False"))
            _eq(engine.flat_knn(x, q, K, metric, engine=eng, **kw), (got[0].view(np.uint64), got[1]))


@pytest.mark.parametrize("kind", list(KINDS))
def test_one_delta_without_tail_is_the_index_itself(engine, eng, data, kind):
    """bit for bit index.nearest, with and without a refine factor (IVF_FLAT's nearest has none) and under a prefilter"""
    x, q, allow = data
    col = _build(engine, eng, x, kind, "one_delta_no_tail")
    index = col.deltas[0]
    cases = [dict(), dict(prefilter=allow)]
    if KINDS[kind]["index_type"] != "IVF_FLAT":
        cases += [dict(refine_factor=3), dict(refine_factor=2, prefilter=allow)]
    for kw in cases:
        want = index.nearest(q, k=K, nprobes=3, **kw)
        want = (np.asarray(want[0]).view(np.uint64), want[1])
        _eq(col.nearest(q, k=K, nprobes=3, **kw), want, (kind, sorted(kw)))
        if "refine_factor" in kw:
            # the two forms of steps 2 + 3 are the same bits: the delta's own refined search (what the column takes when the delta has
            # this column attached) and its search for keff rows followed by take_flat_knn (what it takes otherwise)
            assert col._refines_on_this_column(index, KINDS[kind]["index_type"])
            ids, _ = col._ann(index, KINDS[kind]["index_type"], q, K * kw["refine_factor"], 3, kw.get("prefilter"), {})
            _eq(eng.take_flat_knn(col._x, q, ids, K, KINDS[kind]["metric"]), want, (kind, "search + take_flat_knn", sorted(kw)))


def _recall(ids, truth):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / len(b) for a, b in zip(ids.view(np.uint64), truth)]))


@pytest.mark.parametrize("kind", ["pq8_l2", "flat_l2", "sq_l2", "rq_l2"])
def test_create_delta_and_optimize(engine, eng, oracle, data, kind):
    """a column that grows: index fragment 0, search (rows of the tail are found exactly); a delta over fragments 1 and 2; the rest folded
    into the last delta by optimize (IVF_RQ: refused, create_delta instead).  Every state against the specification bit for bit, and
    against the flat_knn ground truth: a true neighbour that lies in an unindexed fragment is ALWAYS returned (its scan and the final
    re-ranking are exact), and the recall is the specification's."""
    x, q, _ = data
    metric = KINDS[kind]["metric"]
    truth = oracle.flat_knn(x, q, K, metric)[0]
    col = _build(engine, eng, x, kind, "two_deltas_tail")
    col = engine.VectorColumn(x, SIZES, engine=eng).with_index(col.deltas[0], [0])
    states = [(col, None)]
    col2 = col.create_delta([1, 2])
    states.append((col2, None))
    rows = lambda frags: np.concatenate([np.arange(sum(SIZES[:f]), sum(SIZES[:f + 1]), dtype=np.uint64) for f in frags])
    if kind == "rq_l2":
        with pytest.raises(NotImplementedError) as e:
            col2.optimize()
        assert "IVF_RQ: append is not supported" in str(e.value)
        col3 = col2.create_delta()
        states.append((col3, None))
    else:
        col3 = col2.optimize()
        states.append((col3, [rows([0]), rows([1, 2, 3, 4])]))
    assert col3.unindexed_fragments() == [] and col2.unindexed_fragments() == [3, 4] and col.unindexed_fragments() == [1, 2, 3, 4]
    for c, stored in states:
        sc = _spec_column(oracle, x, kind, c, stored)
        tail_rows = rows(c.unindexed_fragments()) if c.unindexed_fragments() else np.empty(0, np.uint64)
        for kw in (dict(nprobes=NLIST), dict(nprobes=NLIST, refine_factor=4)):
            got = c.nearest(q, k=K, **kw)
            want = KC.nearest(oracle, sc, q, k=K, **kw)
            _eq(got, want, (kind, len(c.deltas), sorted(kw)))
            assert _recall(got[0], truth) == _recall(want[0].view(np.int64), truth)
            for i in range(NQ):
                assert set(truth[i][np.isin(truth[i], tail_rows)].tolist()) <= set(got[0][i].view(np.uint64).tolist())
