"""Characterisation of `nearest` on the four index wrappers (lance_amd/vector.py: IvfPqIndex, IvfFlatIndex, IvfSqIndex, IvfRqIndex) on the
CPU, over a stub device index: which searches adaptive probing sends, for which queries and with how many partitions, and what comes
back.  The stub answers query (f, ...) searched over n partitions with min(k, f * n) rows -- the ids `found[0], found[1], ...` at the
distances 0, 1, ... -- and (-1, +inf) beyond; it logs (method, queries, nprobes, refine factor, allow given?, f of every query,
range).  The expected logs and arrays are literals, recorded once from the implementation this file was first written against."""
import numpy as np
import pytest
import torch

from lance_amd import vector as V

NLIST, K = 8, 4
I = float("inf")
F32_MIN = -3.4028234663852886e+38


class _Ix:
    """what the wrappers touch of a device index: centroids, _raw and the search methods of the kind"""

    def __init__(self, kind, found=(0, 1, 2, 3), raw=True):
        self.kind, self.found, self.log = kind, list(found), []
        self.centroids = torch.zeros(NLIST, 4)
        self._raw = object() if raw else None
        if kind == "pq":
            self.search = lambda q, k, nprobes, rf=0: self._answer("search", q, k, nprobes, rf, None, None)
            self.search_filtered = lambda q, k, nprobes, allow, rf=0: self._answer("search_filtered", q, k, nprobes, rf, allow, None)
            self.search_range = lambda q, k, nprobes, lo, hi, refine_factor=0, allow=None: self._answer("search_range", q, k, nprobes,
                                                                                                       refine_factor, allow, (lo, hi))
        elif kind == "flat":
            self.search = lambda q, k, nprobes, allow=None, lower=None, upper=None: self._answer(
                "search", q, k, nprobes, 0, allow, None if lower is None and upper is None else (lower, upper))
        else:
            self.search = lambda q, k, nprobes, allow=None, refine_factor=0: self._answer("search", q, k, nprobes, refine_factor, allow, None)

    def _answer(self, method, q, k, nprobes, rf, allow, rng):
        first = [int(v) for v in torch.as_tensor(np.asarray(q)).reshape(-1, 4)[:, 0]]
        self.log.append((method, len(first), nprobes, rf, allow is not None, first, rng))
        ids = torch.full((len(first), k), -1, dtype=torch.int64)
        dists = torch.full((len(first), k), I, dtype=torch.float32)
        for i, f in enumerate(first):
            m = min(k, f * nprobes)
            ids[i, :m] = torch.tensor(self.found[:m], dtype=torch.int64)
            dists[i, :m] = torch.arange(m, dtype=torch.float32)
        return ids, dists


def _index(kind, **kw):
    ix = _Ix(kind, **kw)
    params = V.IvfPqParams(num_partitions=NLIST)
    if kind == "pq":
        return V.IvfPqIndex(ix, params), ix
    cls = {"flat": V.IvfFlatIndex, "sq": V.IvfSqIndex, "rq": V.IvfRqIndex}[kind]
    return cls(ix, params, None, None), ix


def _q(*first):
    q = np.zeros((len(first), 4), np.float32)
    q[:, 0] = first
    return q


def _nearest(kind, first, k=K, found=(0, 1, 2, 3), **kw):
    """-> (the stub's log, ids as int64 lists, distances as lists)"""
    index, ix = _index(kind, found=found)
    ids, dists = index.nearest(_q(*first), k=k, **kw)
    assert dists.dtype == np.float32 and ids.shape == dists.shape == (len(first), k)
    assert ids.dtype == (np.int64 if kind == "pq" else np.uint64)
    return ix.log, ids.view(np.int64).tolist(), dists.tolist()


KINDS = ["pq", "flat", "sq", "rq"]
FULL, NONE4 = [0, 1, 2, 3], [-1, -1, -1, -1]
D_FULL, D_NONE4 = [0.0, 1.0, 2.0, 3.0], [I, I, I, I]


@pytest.mark.parametrize("kind", KINDS)
def test_nprobes_alone_is_one_search(kind):
    log, ids, dists = _nearest(kind, (4, 1, 2, 0), nprobes=2)
    assert log == [("search", 4, 2, 0, False, [4, 1, 2, 0], None)]
    assert ids == [FULL, [0, 1, -1, -1], FULL, NONE4]
    assert dists == [D_FULL, [0.0, 1.0, I, I], D_FULL, D_NONE4]


DOUBLING = [("search", 4, 1, 0, False, [4, 1, 2, 0], None), ("search", 3, 2, 0, False, [1, 2, 0], None),
            ("search", 2, 4, 0, False, [1, 0], None), ("search", 1, 8, 0, False, [0], None)]


@pytest.mark.parametrize("kind", KINDS)
def test_minimum_nprobes_doubles_for_the_starved_queries_only(kind):
    log, ids, dists = _nearest(kind, (4, 1, 2, 0), minimum_nprobes=1)
    assert log == DOUBLING                                   # 1 -> 2 -> 4 -> nlist; the last query is never satisfied
    assert ids == [FULL, FULL, FULL, NONE4] and dists == [D_FULL, D_FULL, D_FULL, D_NONE4]
    log, ids, dists = _nearest(kind, (0,), minimum_nprobes=3)
    assert log == [("search", 1, 3, 0, False, [0], None), ("search", 1, 6, 0, False, [0], None), ("search", 1, 8, 0, False, [0], None)]
    assert ids == [NONE4] and dists == [D_NONE4]
    log, ids, dists = _nearest(kind, (4, 2), minimum_nprobes=2)            # nobody starved: one search
    assert log == [("search", 2, 2, 0, False, [4, 2], None)]
    assert ids == [FULL, FULL]


@pytest.mark.parametrize("kind", KINDS)
def test_maximum_nprobes_below_and_above_nlist(kind):
    log, ids, dists = _nearest(kind, (4, 1, 2, 0), minimum_nprobes=1, maximum_nprobes=3)
    assert log == [("search", 4, 1, 0, False, [4, 1, 2, 0], None), ("search", 3, 2, 0, False, [1, 2, 0], None),
                   ("search", 2, 3, 0, False, [1, 0], None)]
    assert ids == [FULL, [0, 1, 2, -1], FULL, NONE4]
    assert dists == [D_FULL, [0.0, 1.0, 2.0, I], D_FULL, D_NONE4]
    log, ids, dists = _nearest(kind, (4, 1, 2, 0), minimum_nprobes=1, maximum_nprobes=20)
    assert log == DOUBLING
    log, ids, dists = _nearest(kind, (4, 1, 2, 0), nprobes=1, maximum_nprobes=20)          # nprobes is the minimum when only a maximum is given
    assert log == DOUBLING
    assert ids == [FULL, FULL, FULL, NONE4]
    log, ids, dists = _nearest(kind, (4, 1), nprobes=20)                                    # nprobes above nlist: nlist
    assert log == [("search", 2, 8, 0, False, [4, 1], None)]


@pytest.mark.parametrize("kind", KINDS)
def test_minimum_above_maximum(kind):
    log, ids, dists = _nearest(kind, (4, 1, 0), minimum_nprobes=6, maximum_nprobes=2)
    assert log == [("search", 3, 6, 0, False, [4, 1, 0], None)]
    assert ids == [FULL, FULL, NONE4]
    log, ids, dists = _nearest(kind, (4, 1, 0), minimum_nprobes=30, maximum_nprobes=20)
    assert log == [("search", 3, 8, 0, False, [4, 1, 0], None)]


MASK3 = np.zeros(10, bool)
MASK3[[1, 3, 9]] = True
MASK5 = np.zeros(10, bool)
MASK5[[1, 3, 5, 7, 9]] = True


def _filtered(kind):
    return "search_filtered" if kind == "pq" else "search"


@pytest.mark.parametrize("kind", KINDS)
def test_prefilter_of_at_most_k_rows_takes_the_shortcut(kind):
    log, ids, dists = _nearest(kind, (1, 0, 3), found=(3, 9, 1, 7), minimum_nprobes=1, prefilter=MASK3)
    assert log == [(_filtered(kind), 3, 1, 0, True, [1, 0, 3], None)]          # and no further call
    assert ids == [[3, 1, 9, -1], [1, 3, 9, -1], [3, 9, 1, -1]]                 # the unfound selected ids, ascending, at +inf
    assert dists == [[0.0, I, I, I], [I, I, I, I], [0.0, 1.0, 2.0, I]]
    log, ids, dists = _nearest(kind, (1, 0, 3), found=(3, 9, 1, 7), minimum_nprobes=1, prefilter=torch.from_numpy(MASK3))
    assert log == [(_filtered(kind), 3, 1, 0, True, [1, 0, 3], None)]
    assert ids == [[3, 1, 9, -1], [1, 3, 9, -1], [3, 9, 1, -1]]
    # fixed nprobes: nothing to extend, nothing appended
    log, ids, dists = _nearest(kind, (1, 0, 3), found=(3, 9, 1, 7), nprobes=1, prefilter=MASK3)
    assert log == [(_filtered(kind), 3, 1, 0, True, [1, 0, 3], None)]
    assert ids == [[3, -1, -1, -1], NONE4, [3, 9, 1, -1]]
    # a prefilter of more than k rows: the ordinary extension, under the mask
    log, ids, dists = _nearest(kind, (1, 0, 3), found=(3, 9, 1, 7), minimum_nprobes=2, maximum_nprobes=5, prefilter=MASK5)
    assert log == [(_filtered(kind), 3, 2, 0, True, [1, 0, 3], None), (_filtered(kind), 2, 4, 0, True, [1, 0], None),
                   (_filtered(kind), 1, 5, 0, True, [0], None)]
    assert ids == [[3, 9, 1, 7], NONE4, [3, 9, 1, 7]]


@pytest.mark.parametrize("kind", ["pq", "sq", "rq"])
def test_refine_factor_suppresses_the_shortcut(kind):
    log, ids, dists = _nearest(kind, (1, 0, 3), found=(3, 9, 1, 7), minimum_nprobes=2, prefilter=MASK3, refine_factor=2)
    assert log == [(_filtered(kind), 3, 2, 2, True, [1, 0, 3], None), (_filtered(kind), 2, 4, 2, True, [1, 0], None),
                   (_filtered(kind), 1, 8, 2, True, [0], None)]
    assert ids == [[3, 9, 1, 7], NONE4, [3, 9, 1, 7]]
    assert dists == [D_FULL, D_NONE4, D_FULL]
    log, ids, dists = _nearest(kind, (1, 4), minimum_nprobes=2, refine_factor=3)           # without a prefilter
    assert log == [("search", 2, 2, 3, False, [1, 4], None), ("search", 1, 4, 3, False, [1], None)]
    assert ids == [FULL, FULL]


@pytest.mark.parametrize("kind", ["pq", "flat"])
def test_range_suppresses_the_shortcut(kind):
    method = "search_range" if kind == "pq" else "search"
    log, ids, dists = _nearest(kind, (1, 0, 3), found=(3, 9, 1, 7), minimum_nprobes=2, prefilter=MASK3, distance_range=(0.5, None))
    assert log == [(method, 3, 2, 0, True, [1, 0, 3], (0.5, None)), (method, 2, 4, 0, True, [1, 0], (0.5, None)),
                   (method, 1, 8, 0, True, [0], (0.5, None))]
    assert ids == [[3, 9, 1, 7], NONE4, [3, 9, 1, 7]]
    log, ids, dists = _nearest(kind, (1, 4), minimum_nprobes=2, distance_range=(None, 2.5))
    assert log == [(method, 2, 2, 0, False, [1, 4], (None, 2.5)), (method, 1, 4, 0, False, [1], (None, 2.5))]
    assert ids == [FULL, FULL]


def test_pq_range_with_refine_factor_and_prefilter():
    log, ids, dists = _nearest("pq", (1, 4), nprobes=2, prefilter=MASK5, distance_range=(0.5, 2.5), refine_factor=3)
    assert log == [("search_range", 2, 2, 3, True, [1, 4], (0.5, 2.5))]
    log, ids, dists = _nearest("pq", (1, 4), nprobes=2, prefilter=MASK5, refine_factor=3)
    assert log == [("search_filtered", 2, 2, 3, True, [1, 4], None)]


def test_flat_open_range_takes_the_range_entry_point():
    log, ids, dists = _nearest("flat", (4, 1), nprobes=2, distance_range=(None, None))
    assert log == [("search", 2, 2, 0, False, [4, 1], (F32_MIN, None))]
    assert ids == [FULL, [0, 1, -1, -1]]
    log, ids, dists = _nearest("flat", (4, 1), nprobes=2, distance_range=(None, None), prefilter=MASK5)
    assert log == [("search", 2, 2, 0, True, [4, 1], (F32_MIN, None))]


@pytest.mark.parametrize("kind", KINDS)
def test_row_id_at_or_above_2_63_counts_as_found(kind):
    """row ids are u64 bit patterns carried in int64 and only 2^64 - 1 (-1) means missing: 2^64 - 2 (-2) is a row"""
    log, ids, dists = _nearest(kind, (2, 1), k=2, found=(-2, 5), minimum_nprobes=1)
    assert log == [("search", 2, 1, 0, False, [2, 1], None), ("search", 1, 2, 0, False, [1], None)]
    assert ids == [[-2, 5], [-2, 5]] and dists == [[0.0, 1.0], [0.0, 1.0]]


@pytest.mark.parametrize("kind", KINDS)
def test_return_types(kind):
    index, _ = _index(kind)
    ids, dists = index.nearest(_q(1, 0), k=3, nprobes=1)
    assert ids.dtype == (np.int64 if kind == "pq" else np.uint64) and dists.dtype == np.float32
    assert isinstance(ids, np.ndarray) and isinstance(dists, np.ndarray)
    missing = -1 if kind == "pq" else 2 ** 64 - 1
    assert ids.tolist() == [[0, missing, missing], [missing] * 3]


@pytest.mark.parametrize("kind, name", [("sq", "IVF_SQ"), ("rq", "IVF_RQ")])
def test_sq_rq_refusals_and_their_order(kind, name):
    index, ix = _index(kind, raw=False)
    q = _q(1)
    with pytest.raises(NotImplementedError) as e:
        index.nearest(q, distance_range=(0.0, 1.0), refine_factor=0)           # the range is refused first
    assert str(e.value) == f"{name}: distance_range is not supported by this engine"
    with pytest.raises(ValueError) as e:
        index.nearest(q, refine_factor=0)                                       # then the refine factor, before the missing column
    assert str(e.value) == "Refine factor can not be zero"
    with pytest.raises(ValueError) as e:
        index.nearest(q, refine_factor=-3)
    assert str(e.value) == "Refine factor can not be zero"
    with pytest.raises(NotImplementedError) as e:
        index.nearest(q, refine_factor=2)
    assert str(e.value) == (f"{name}: refine_factor needs the raw vectors (re-ranking scores the candidates against the column): attach them "
                            "with set_raw(x), or build with create_index(..., keep_raw=True)")
    assert ix.log == []
    assert index.nearest(q, k=1, nprobes=1)[0].tolist() == [[0]]               # without a refine factor the column is not needed
