"""CPU: the specification of IVF_FLAT distance ranges and of adaptive probing (tests/ivfflat_range_spec.py) and its fixtures.  The GPU
tests compare the device with this specification, so these tests show that the fixtures can tell a right answer from a wrong one:
a range applied after the top k differs, rows sit exactly on both bounds, ties cross position k inside the range, some queries
come back short, and the adaptive fixtures starve queries at every step of the doubling.  The conditions are inequalities, not counts:
another numpy release may draw other rows."""
import functools

import numpy as np
import pytest

import ivfflat_range_spec as V

f32 = np.float32
K, NPROBES, NLIST = V.K, V.NPROBES, V.NLIST


@functools.lru_cache(maxsize=None)
def base():
    return V.base_fixture()


@functools.lru_cache(maxsize=None)
def ranged(lower, upper, k=K, nprobes=NPROBES, metric="l2"):
    import oracle
    x, q, cent = base()
    return V.search(oracle, x, cent, q, k, nprobes, metric, lower, upper)


def test_fixture_partitions_span_several_row_blocks():
    import oracle
    x, _, cent = base()
    sizes = V.partition_sizes(oracle, x, cent, "l2")
    assert sizes.sum() == 3000 and sizes.min() > 0 and sizes.max() > 512          # the largest: three 256-row blocks
    d = np.concatenate(V.probed_distances(oracle, x, cent, base()[1], NPROBES, "l2"))
    assert (d == np.rint(d)).all()                                                  # exact integers


def test_range_inside_the_heap_is_not_a_post_filter():
    import oracle
    x, q, cent = base()
    si, sd = ranged(60.0, 90.0)
    pi, _ = V.post_filtered(oracle, x, cent, q, K, NPROBES, "l2", 60.0, 90.0)
    assert (si != pi).any(axis=1).all()                                             # every query tells them apart
    assert ((sd >= 60.0) & (sd < 90.0)).all()
    assert (np.diff(sd, axis=1) >= 0).all()
    # without a range the search is oracle.ivfflat_search
    ni, nd = ranged(None, None)
    oi, od = oracle.ivfflat_search(x, cent, q, K, NPROBES, "l2")
    assert (ni == oi).all() and (nd.view(np.uint32) == od.view(np.uint32)).all()


def test_rows_sit_on_both_bounds_and_ties_cross_position_k():
    import oracle
    x, q, cent = base()
    pd = V.probed_distances(oracle, x, cent, q, NPROBES, "l2")
    assert sum((d == 60.0).any() for d in pd) > 0 and sum((d == 90.0).any() for d in pd) > 0
    si, sd = ranged(60.0, 90.0)
    assert (sd == 60.0).any()                                                       # the lower bound is inclusive ...
    wide = ranged(60.0, 90.0, k=2000)[1]                                            # (everything in range)
    assert not (wide == 90.0).any() and (wide[wide != np.inf] < 90.0).all()         # ... the upper one is not
    tied = 0
    for d in pd:
        r = np.sort(d[(d >= 60.0) & (d < 90.0)])
        tied += len(r) > K and r[K - 1] == r[K]
    assert tied > 0                                                                 # the device has to replay these through the heap


def test_narrow_ranges_come_back_short_or_empty():
    assert (V.found(ranged(40.0, 64.0)[0]) < K).any()
    assert (V.found(ranged(40.0, 64.0, nprobes=1)[0]) < K).any()                    # the nearest partition alone: no bound for these
    assert (V.found(ranged(60.0, 90.0, k=200)[0]) < 200).any()
    for lo, hi in ((0.0, 1.0), (70.0, 70.0)):
        ids, dists = ranged(lo, hi)
        assert (ids == V.UNSET).all() and np.isinf(dists).all()                     # no query coincides with a row here


def test_zero_signs():
    """A query equal to a stored row has distance exactly +0.0.  OrderedFloat compares the zeros equal, order keys (the device's form
    of the comparison) put -0.0 below +0.0; the four cases agree only because no metric here produces -0.0: a lower bound of either
    zero keeps the row, an upper bound of either zero drops it."""
    import oracle
    x, q, cent = base()
    q0 = x[5:6].copy()
    for lower, upper, kept in ((0.0, 1.0, True), (-0.0, 1.0, True), (-5.0, 0.0, False), (-5.0, -0.0, False)):
        ids, dists = V.search(oracle, x, cent, q0, K, 1, "l2", f32(lower), f32(upper))
        assert (V.found(ids)[0] > 0) == kept, (lower, upper)
        if kept:
            assert dists[0, 0] == 0.0 and not np.signbit(dists[0, 0]) and x[int(ids[0, 0])].tolist() == q0[0].tolist()


def test_nan_is_never_in_range():
    import oracle
    ids, dists = oracle.heap_topk(np.array([np.nan, 3.0, -np.nan], f32), np.arange(3, dtype=np.uint64), 3, lower=-1e30)
    assert ids.tolist() == [1]
    ids, dists = oracle.heap_topk(np.array([np.nan, 3.0], f32), np.arange(2, dtype=np.uint64), 3, upper=np.inf)
    assert ids.tolist() == [1]
    x, q, cent = V.nan_fixture()                    # a finite row whose dot with the query is inf - inf
    d = np.concatenate(V.probed_distances(oracle, x, cent, q, 2, "dot"))
    assert np.isnan(d).sum() == 1
    open_ids, _ = V.search(oracle, x, cent, q, 400, 2, "dot", None, None)
    assert (open_ids == V.NAN_ROW).any()                                            # without a range the heap keeps it
    ids, dists = V.search(oracle, x, cent, q, 400, 2, "dot", -1e30, None)
    assert not (ids == V.NAN_ROW).any() and V.found(ids)[0] == V.found(open_ids)[0] - 1
    assert not np.isnan(dists).any()


def test_adaptive_probing_starves_queries_at_every_step():
    import oracle
    x, q, cent = base()
    allow = V.sparse_prefilter()
    assert allow.sum() == 30

    def fn(sel, npb):
        return V.search(oracle, x, cent, q[sel], K, npb, "l2", None, None, prefilter=allow)
    ids, dists, used = V.adaptive(fn, len(q), K, 1, 8, NLIST)
    assert (used > 2).any() and (used == 8).any() and (used < 8).any()              # starved at 1 and at 2; some go on to all 8
    assert (V.found(ids) == K).all() and allow[ids.astype(np.int64)].all()
    at1 = fn(np.arange(len(q)), 1)[0]
    assert (V.found(at1[used > 1]) < K).all() and (V.found(at1[used == 1]) == K).all()
    # nprobes alone: minimum = maximum
    ids1, _, used1 = V.adaptive(fn, len(q), K, 3, 3, NLIST)
    assert (used1 == 3).all() and (ids1 == fn(np.arange(len(q)), 3)[0]).all()

    # a range no partition can satisfy for some queries: never satisfied, they end at all 8 partitions
    def fnr(sel, npb):
        return V.search(oracle, x, cent, q[sel], K, npb, "l2", *V.STARVING_RANGE)
    rids, _, rused = V.adaptive(fnr, len(q), K, 1, None, NLIST)
    assert ((V.found(rids) < K) & (rused == 8)).any() and ((V.found(rids) == K) & (rused < 8)).any()


def test_shortcut_returns_the_unfound_selected_rows_at_infinity():
    import oracle
    x, q, cent = base()
    allow = V.sparse_prefilter(count=7, seed=3)
    sel = np.flatnonzero(allow)

    def fn(s, npb):
        return V.search(oracle, x, cent, q[s], K, npb, "l2", None, None, prefilter=allow)
    ids, dists, used = V.adaptive(fn, len(q), K, 1, 8, NLIST, selected_ids=sel)
    assert (used == 1).all()                                                        # no further partition is searched
    at1 = fn(np.arange(len(q)), 1)
    short = np.flatnonzero(V.found(at1[0]) < 7)
    assert short.size > 0
    for qi in short:
        n = V.found(at1[0])[qi]
        assert (ids[qi, :n] == at1[0][qi, :n]).all() and np.isinf(dists[qi, n:7]).all() and (ids[qi, 7:] == V.UNSET).all()
        tail = ids[qi, n:7]
        assert (np.diff(tail.astype(np.int64)) > 0).all() and sorted(ids[qi, :7].tolist()) == sel.tolist()
    # without the shortcut (a refine factor, a range) the same queries go on
    _, _, used2 = V.adaptive(fn, len(q), K, 1, 8, NLIST)
    assert (used2 == 8).all()
