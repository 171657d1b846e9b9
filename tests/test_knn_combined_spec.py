"""CPU: the specification of the combined search (tests/knn_combined_spec.py) against its three wrong variants, and the host logic of
lance_amd.VectorColumn over stub indices and a stub engine: overlapping fragments, mismatched deltas, the refusals, and which library
calls a plan makes (recorded calls, as tests/test_nearest_calls_cpu.py records them)."""
import numpy as np
import pytest
import torch

import flat_order_spec as FO
import flat_range_spec as FR
import knn_combined_spec as KC
from lance_amd import vector as V

f32 = np.float32
METRICS = ["l2", "dot", "cosine"]


# ---- the fixtures tell every mutant from the specification -------------------------------------------------------------------------
@pytest.fixture(scope="module", params=METRICS)
def fixture(request, oracle):
    return request.param, KC.mutant_fixture(oracle, request.param)


def _answers(oracle, f, distance_range=None):
    kw = dict(k=f["k"], nprobes=f["nprobes"], distance_range=distance_range)
    return KC.nearest(oracle, f["col"], f["q"], **kw), {m: KC.nearest(oracle, f["col"], f["q"], mutant=m, **kw) for m in KC.MUTANTS}


def test_fixture_holds_what_the_reference_alone_decides(fixture, oracle):
    metric, f = fixture
    col, q, k = f["col"], f["q"], f["k"]
    ai, ad = f["ann"]
    spec = KC.nearest(oracle, col, q, k=k, nprobes=f["nprobes"])
    # a tail row that displaces an ANN row: a row of fragment 2 (unindexed, not in the index) is returned and a found ANN row is not
    pure_tail = spec[0] >= np.uint64(1200)
    assert ((spec[0] != KC.UNSET) & pure_tail).any()
    assert any(set(ai[i][ai[i] != KC.UNSET].tolist()) - set(spec[0][i].tolist()) for i in np.nonzero(pure_tail.any(axis=1))[0])
    # a row id present in both lists comes back twice
    both = [i for i in range(len(q)) if len(set(spec[0][i].tolist())) < k]
    assert both, "no query returns a row of fragment 1 twice"
    for i in both:
        ids, counts = np.unique(spec[0][i], return_counts=True)
        assert ((ids[counts > 1] >= 900) & (ids[counts > 1] < 1200)).all() and (counts <= 2).all()
    # an ANN row whose approximate distance is in range and whose exact one is not
    assert f["range"] is not None
    i, r = f["range_query"], f["range_row"]
    assert r in ai[i].tolist() and ad[i][ai[i].tolist().index(r)] == f32(f["range_pq"])
    exact = KC.take_flat_knn(oracle, col.x, q[i:i + 1], np.array([[r]], np.uint64), 1, metric)[1][0, 0]
    assert exact.view(np.uint32) == f32(f["range_exact"]).view(np.uint32)
    assert FR.in_range(np.asarray([f["range_pq"]], f32), *f["range"])[0] and not FR.in_range(np.asarray([exact], f32), *f["range"])[0]


def test_every_mutant_differs_from_the_specification(fixture, oracle):
    metric, f = fixture
    spec, wrong = _answers(oracle, f)
    assert not KC.same(spec, wrong["approx"]), "the ANN list's approximate distances must not survive the union"
    assert not KC.same(spec, wrong["dedup"]), "the union is not de-duplicated"
    assert KC.same(spec, wrong["bounds_before"])                 # (no range: nothing to tell)
    spec, wrong = _answers(oracle, f, distance_range=f["range"])
    assert not KC.same(spec, wrong["bounds_before"]), "the bounds are tested on the exact distances after the union"
    found = spec[0] != KC.UNSET
    assert FR.in_range(spec[1][found], *f["range"]).all()
    i, r = f["range_query"], np.uint64(f["range_row"])
    assert r not in spec[0][i] and r in wrong["bounds_before"][0][i]      # the row out of range by its exact distance, kept by the wrong variant


def test_take_flat_knn_model(oracle):
    x = KC.clustered(300, 7, 3)
    q = x[[5, 50]] + f32(0.25)
    a = np.array([[5, 7, KC.UNSET, 9, 5], [50, 51, 52, KC.UNSET, KC.UNSET]], np.uint64)
    b = np.array([[200, 5], [KC.UNSET, 250]], np.uint64)
    for metric in METRICS:
        want_i, want_d = oracle.flat_knn(x, q, 300, metric)
        dist = {(i, int(r)): want_d[i, j] for i in range(2) for j, r in enumerate(want_i[i])}
        ids, d = KC.take_flat_knn(oracle, x, q, a, 8, metric, ids_b=b)
        assert sorted(ids[0][:6].tolist()) == [5, 5, 5, 7, 9, 200] and (ids[0][6:] == KC.UNSET).all() and np.isinf(d[0][6:]).all()
        assert sorted(ids[1][:4].tolist()) == [50, 51, 52, 250]
        for i in range(2):
            got = [(int(r), v) for r, v in zip(ids[i], d[i]) if r != KC.UNSET]
            assert all(np.float32(v).view(np.uint32) == np.float32(dist[(i, r)]).view(np.uint32) for r, v in got)
            keys = [(int(FO.keys(np.asarray([v], f32))[0]), r) for r, v in got]
            assert keys == sorted(keys)
        # list B's distances given: taken as they are
        db = np.array([[dist[(0, 200)], dist[(0, 5)]], [np.inf, dist[(1, 250)]]], f32)
        assert KC.same((ids, d), KC.take_flat_knn(oracle, x, q, a, 8, metric, ids_b=b, dists_b=db))
    with pytest.raises(ValueError):
        KC.take_flat_knn(oracle, x, q, np.array([[300], [1]], np.uint64), 1, "l2")


# ---- host logic of VectorColumn ------------------------------------------------------------------------------------------------------
NLIST, D, I = 8, 4, float("inf")


class _Ix:
    """what VectorColumn touches of a device index: centroids, data_dtype and the searches of its kind; every search answers the ids
    `found` at the distances 0, 1, ..."""

    def __init__(self, kind, found, log, name, dtype=torch.float32, d=D):
        self.centroids, self.data_dtype, self.kind = torch.zeros(NLIST, d), dtype, kind

        def answer(method, q, k, nprobes, rf, allow, rng):
            log.append((name, method, int(np.asarray(q).reshape(-1, d).shape[0]), k, nprobes, rf, allow is not None, rng))
            nq = int(np.asarray(q).reshape(-1, d).shape[0])
            ids = torch.full((nq, k), -1, dtype=torch.int64)
            dists = torch.full((nq, k), I, dtype=torch.float32)
            m = min(k, len(found))
            ids[:, :m] = torch.tensor(found[:m], dtype=torch.int64)
            dists[:, :m] = torch.arange(m, dtype=torch.float32)
            return ids, dists
        if kind == "pq":
            self.search = lambda q, k, nprobes, rf=0: answer("search", q, k, nprobes, rf, None, None)
            self.search_filtered = lambda q, k, nprobes, allow, rf=0: answer("search_filtered", q, k, nprobes, rf, allow, None)
            self.search_range = lambda q, k, nprobes, lo, hi, refine_factor=0, allow=None: answer("search_range", q, k, nprobes, refine_factor, allow, (lo, hi))
        elif kind == "flat":
            self.search = lambda q, k, nprobes, allow=None, lower=None, upper=None: answer(
                "search", q, k, nprobes, 0, allow, None if lower is None and upper is None else (lower, upper))
        else:
            self.search = lambda q, k, nprobes, allow=None, refine_factor=0: answer("search", q, k, nprobes, refine_factor, allow, None)


class _Engine:
    """records flat_topk / take_flat_knn / merge_topk; answers the first ids it is given"""

    def __init__(self, log):
        self.log = log

    def flat_topk(self, x, q, k, metric="l2", row_ids=None, lower=None, upper=None):
        rid = np.arange(x.shape[0]) if row_ids is None else np.asarray(row_ids)
        self.log.append(("engine", "flat_topk", int(x.shape[0]), int(rid[0]), int(rid[-1]), k, metric, lower, upper))
        nq = np.asarray(q).reshape(-1, D).shape[0]
        ids = torch.full((nq, k), -1, dtype=torch.int64)
        m = min(k, rid.size)
        ids[:, :m] = torch.as_tensor(rid[:m].copy(), dtype=torch.int64)
        return ids, torch.zeros((nq, k), dtype=torch.float32)

    def take_flat_knn(self, x, q, ids_a, k, metric="l2", ids_b=None, dists_b=None, lower=None, upper=None):
        self.log.append(("engine", "take_flat_knn", int(ids_a.shape[1]), 0 if ids_b is None else int(ids_b.shape[1]), dists_b is not None, k, metric,
                         lower, upper))
        return ids_a[:, :k].clone(), torch.zeros((ids_a.shape[0], k), dtype=torch.float32)

    def merge_topk(self, ids, dists, k, exact=None, keff=None):
        self.log.append(("engine", "merge_topk", int(ids.shape[1]), k))
        return ids[:, :k].clone(), dists[:, :k].clone()


def _wrap(kind, found, log, name, metric="l2", **kw):
    ix = _Ix(kind, list(found), log, name, **kw)
    params = V.IvfPqParams(num_partitions=NLIST, metric=metric)
    if kind == "pq":
        return V.IvfPqIndex(ix, params)
    return {"flat": V.IvfFlatIndex, "sq": V.IvfSqIndex, "rq": V.IvfRqIndex}[kind](ix, params, None, None)


def _column(sizes=(10, 5, 5, 20, 10), log=None):
    log = [] if log is None else log
    return V.VectorColumn(torch.zeros(sum(sizes), D), list(sizes), engine=_Engine(log)), log


Q = np.zeros((3, D), f32)


def test_fragments_and_overlap():
    col, log = _column()
    assert col.num_fragments == 5 and col.unindexed_fragments() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        V.VectorColumn(torch.zeros(10, D), [3, 3])
    a = _wrap("pq", [1, 2], log, "a")
    c1 = col.with_index(a, [0, 1])
    assert col.unindexed_fragments() == [0, 1, 2, 3, 4], "with_index returns a new column"
    assert c1.unindexed_fragments() == [2, 3, 4] and c1.deltas == [a]
    with pytest.raises(ValueError) as e:
        c1.with_index(_wrap("pq", [3], log, "b"), [1, 2])
    assert "[1]" in str(e.value) and "overlap" in str(e.value)
    with pytest.raises(ValueError):
        c1.with_index(_wrap("pq", [3], log, "b"), [7])
    assert c1._runs([2, 4]) == [(15, 20), (40, 50)] and c1._runs([2, 3, 4]) == [(15, 50)]
    assert log == []


@pytest.mark.parametrize("kw, word", [(dict(kind="flat"), "index type"), (dict(metric="dot"), "metric"), (dict(dtype=torch.float16), "element type")])
def test_mismatched_deltas_are_refused(kw, word):
    col, log = _column()
    c1 = col.with_index(_wrap("pq", [1], log, "a"), [0])
    args = dict(kind="pq", metric="l2")
    args.update(kw)
    with pytest.raises(ValueError) as e:
        c1.with_index(_wrap(args.pop("kind"), [2], log, "b", **args), [1])
    assert word in str(e.value)


def test_dimension_and_multivector_refusals():
    col, log = _column()
    with pytest.raises(ValueError) as e:
        col.with_index(_wrap("pq", [1], log, "a", d=8), [0])
    assert "dimension" in str(e.value)
    with pytest.raises(NotImplementedError):
        V.VectorColumn([torch.zeros(3, D), torch.zeros(2, D)])
    with pytest.raises(NotImplementedError):
        V.VectorColumn(torch.zeros(4, 3, D))
    with pytest.raises(NotImplementedError):
        col.with_index(V.IvfPqMultivectorIndex(_Ix("pq", [1], log, "m"), V.IvfPqParams(), None, None, torch.zeros(3, dtype=torch.int64)), [0])


def test_refusals_of_create_delta():
    """arguments the column sets itself, and -- with a delta there -- a model or sizes that are not that delta's: refused before any device work"""
    col, log = _column()
    for name in ("keep_raw", "_row_ids", "_sq_bounds"):
        with pytest.raises(ValueError) as e:
            col.create_delta([0], **{name: None})
        assert name in str(e.value)
    c1 = col.with_index(_wrap("pq", [1], log, "a"), [0])
    for kw, word in ((dict(index_type="IVF_FLAT"), "index_type"), (dict(metric="dot"), "metric"), (dict(num_partitions=NLIST + 1), "num_partitions"),
                     (dict(num_sub_vectors=2), "num_sub_vectors"), (dict(num_bits=4), "num_bits"), (dict(ivf_centroids=np.zeros((NLIST, D), f32)), "ivf_centroids"),
                     (dict(pq_codebook=np.zeros((16, 256, 1), f32)), "pq_codebook")):
        with pytest.raises(ValueError) as e:
            c1.create_delta([1], **kw)
        assert word in str(e.value)
    with pytest.raises(ValueError):
        c1.create_delta([0])                                 # covered by another delta
    assert log == []


def test_refusals_of_nearest():
    col, log = _column()
    c1 = col.with_index(_wrap("pq", [1], log, "a"), [0])
    for name in ("minimum_nprobes", "maximum_nprobes"):
        with pytest.raises(NotImplementedError) as e:
            c1.nearest(Q, **{name: 2})
        assert name in str(e.value)
    for rf in (0, -2):
        with pytest.raises(ValueError) as e:
            c1.nearest(Q, refine_factor=rf)
        assert str(e.value) == "Refine factor can not be zero"
    for kind, name in (("sq", "IVF_SQ"), ("rq", "IVF_RQ")):
        c2 = col.with_index(_wrap(kind, [1], log, "a"), [0])
        with pytest.raises(NotImplementedError) as e:
            c2.nearest(Q, distance_range=(0.0, 1.0))
        assert str(e.value) == f"{name}: distance_range is not supported by this engine"
        c2.nearest(Q, distance_range=(None, None), fast_search=True)          # no range at all
    with pytest.raises(ValueError):
        c1.nearest(Q, metric="dot")
    assert [l for l in log if l[1] != "search"] == []
    rq = col.with_index(_wrap("rq", [1], log, "r"), [0])
    with pytest.raises(NotImplementedError) as e:
        rq.optimize()
    assert "IVF_RQ: append is not supported" in str(e.value)
    with pytest.raises(ValueError):
        col.optimize()


def test_plan_without_an_index_is_one_flat_scan():
    col, log = _column()
    ids, dists = col.nearest(Q, k=4, metric="dot", distance_range=(0.5, None))
    assert log == [("engine", "flat_topk", 50, 0, 49, 4, "dot", 0.5, None)]
    assert ids.dtype == np.int64 and dists.dtype == np.float32 and ids.shape == (3, 4)
    c1 = col.with_index(_wrap("pq", [1], log, "a"), [0])
    del log[:]
    c1.nearest(Q, k=4, use_index=False)
    assert log == [("engine", "flat_topk", 50, 0, 49, 4, "l2", None, None)]
    c2 = col.with_index(_wrap("sq", [1], log, "a", metric="cosine"), [0])
    del log[:]
    c2.nearest(Q, k=4, use_index=False, distance_range=(None, 0.5))           # the deltas' metric; the flat scan answers ranges for every kind
    assert log == [("engine", "flat_topk", 50, 0, 49, 4, "cosine", None, 0.5)]


def test_plan_one_delta_no_tail():
    col, log = _column()
    c = col.with_index(_wrap("pq", [3, 1, 2, 0], log, "a"), [0, 1, 2, 3, 4])
    ids, _ = c.nearest(Q, k=2, nprobes=5)
    assert log == [("a", "search", 3, 2, 5, 0, False, None)] and ids.tolist() == [[3, 1]] * 3
    del log[:]
    c.nearest(Q, k=2, nprobes=5, refine_factor=2, prefilter=np.ones(50, bool))
    assert log == [("a", "search_filtered", 3, 4, 5, 0, True, None), ("engine", "take_flat_knn", 4, 0, False, 2, "l2", None, None)]
    del log[:]
    c.nearest(Q, k=2, nprobes=5, refine_factor=2, distance_range=(None, 9.0))
    assert log == [("a", "search_range", 3, 4, 5, 0, False, (None, 9.0)), ("engine", "take_flat_knn", 4, 0, False, 2, "l2", None, 9.0)]


@pytest.mark.parametrize("kind", ["pq", "sq", "rq", "flat"])
def test_plan_single_delta_refines_in_its_own_search_when_the_column_is_attached(kind):
    """one un-ranged delta whose attached raw vectors ARE the column: steps 2 and 3 are the delta's own refined search for k rows;
    a copy of the column, a range, a second delta or IVF_FLAT (no refine of its own) keep the search for keff rows + take_flat_knn"""
    col, log = _column()
    a = _wrap(kind, [3, 1, 2, 0], log, "a")
    c = col.with_index(a, [0, 1, 2, 3])
    a._ix._raw = col._x
    filtered = "search_filtered" if kind == "pq" else "search"
    c.nearest(Q, k=2, nprobes=5, refine_factor=2, prefilter=np.ones(50, bool))
    if kind == "flat":
        assert log[:2] == [("a", "search", 3, 4, 5, 0, True, None), ("engine", "take_flat_knn", 4, 0, False, 2, "l2", None, None)]
        return
    assert log == [("a", filtered, 3, 2, 5, 2, True, None), ("engine", "flat_topk", 10, 40, 49, 2, "l2", None, None),
                   ("engine", "take_flat_knn", 2, 2, True, 2, "l2", None, None)]
    del log[:]
    c.nearest(Q, k=2, nprobes=5, refine_factor=2, fast_search=True)
    assert log == [("a", "search", 3, 2, 5, 2, False, None)]
    del log[:]
    a._ix._raw = col._x.clone()                                # not the column's storage
    c.nearest(Q, k=2, nprobes=5, refine_factor=2, fast_search=True)
    assert log == [("a", "search", 3, 4, 5, 0, False, None), ("engine", "take_flat_knn", 4, 0, False, 2, "l2", None, None)]
    a._ix._raw = col._x
    if kind == "pq":
        del log[:]
        c.nearest(Q, k=2, nprobes=5, refine_factor=2, fast_search=True, distance_range=(None, 9.0))
        assert [l[1] for l in log] == ["search_range", "take_flat_knn"]
    b = _wrap(kind, [12], log, "b")
    b._ix._raw = col._x
    del log[:]
    c.with_index(b, [4]).nearest(Q, k=2, nprobes=5, refine_factor=2)
    assert [l[1] for l in log] == ["search", "search", "merge_topk", "take_flat_knn"]


@pytest.mark.parametrize("kind", ["pq", "flat", "sq", "rq"])
def test_plan_two_deltas_and_two_tail_runs(kind):
    col, log = _column()
    c = col.with_index(_wrap(kind, [3, 1], log, "a"), [0]).with_index(_wrap(kind, [12, 11], log, "b"), [2])
    assert c._runs(c.unindexed_fragments()) == [(10, 15), (20, 50)]
    filtered = "search_filtered" if kind == "pq" else "search"
    c.nearest(Q, k=2, nprobes=3)
    assert log == [("a", "search", 3, 2, 3, 0, False, None), ("b", "search", 3, 2, 3, 0, False, None), ("engine", "merge_topk", 4, 2),
                   ("engine", "flat_topk", 5, 10, 14, 2, "l2", None, None), ("engine", "flat_topk", 30, 20, 49, 2, "l2", None, None),
                   ("engine", "take_flat_knn", 2, 4, True, 2, "l2", None, None)]
    del log[:]
    c.nearest(Q, k=2, nprobes=3, fast_search=True)
    assert [l[1] for l in log] == ["search", "search", "merge_topk"]
    del log[:]
    allow = np.zeros(50, bool)
    allow[[1, 12, 13, 30]] = True
    c.nearest(Q, k=2, nprobes=3, refine_factor=3, prefilter=allow)
    assert log == [("a", filtered, 3, 6, 3, 0, True, None), ("b", filtered, 3, 6, 3, 0, True, None), ("engine", "merge_topk", 12, 6),
                   ("engine", "take_flat_knn", 6, 0, False, 2, "l2", None, None),
                   ("engine", "flat_topk", 2, 12, 13, 2, "l2", None, None), ("engine", "flat_topk", 1, 30, 30, 2, "l2", None, None),
                   ("engine", "take_flat_knn", 2, 4, True, 2, "l2", None, None)]
    if kind in ("pq", "flat"):
        del log[:]
        c.nearest(Q, k=2, nprobes=3, distance_range=(1.0, 4.0))
        method = "search_range" if kind == "pq" else "search"
        assert log[:2] == [("a", method, 3, 2, 3, 0, False, (1.0, 4.0)), ("b", method, 3, 2, 3, 0, False, (1.0, 4.0))]
        assert log[3:] == [("engine", "flat_topk", 5, 10, 14, 2, "l2", 1.0, 4.0), ("engine", "flat_topk", 30, 20, 49, 2, "l2", 1.0, 4.0),
                           ("engine", "take_flat_knn", 2, 4, True, 2, "l2", 1.0, 4.0)]


def test_plan_chains_beyond_the_candidate_limit():
    """five tail runs at k = 1000: 1000 + 3 x 1000 fit one call, the rest goes to a second call with the first call's k rows as list A"""
    sizes = [1, 1000] * 5 + [1]
    log = []
    col = V.VectorColumn(torch.zeros(sum(sizes), D), sizes, engine=_Engine(log))
    c = col.with_index(_wrap("pq", [0], log, "a"), range(0, 11, 2))
    c.nearest(Q, k=1000, nprobes=1)
    takes = [l for l in log if l[1] == "take_flat_knn"]
    assert takes == [("engine", "take_flat_knn", 1000, 3000, True, 1000, "l2", None, None),
                     ("engine", "take_flat_knn", 1000, 2000, True, 1000, "l2", None, None)]
    assert len([l for l in log if l[1] == "flat_topk"]) == 5


def test_plan_with_a_prefilter_that_empties_the_tail():
    col, log = _column()
    c = col.with_index(_wrap("pq", [3, 1], log, "a"), [0, 1, 2, 3])
    c.nearest(Q, k=2, prefilter=np.zeros(50, bool))
    assert log == [("a", "search_filtered", 3, 2, 1, 0, True, None), ("engine", "take_flat_knn", 2, 0, False, 2, "l2", None, None)]
