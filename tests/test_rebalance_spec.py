"""tests/rebalance_spec.py pinned on hand cases and against independent formulations, and the host functions of lance_amd.vector that
decide WHICH partition is split or joined.  No device."""
import collections

import numpy as np
import pytest

import oracle
import rebalance_spec as R


def both(name):
    """the specification's function and the package's (which imports torch)"""
    pytest.importorskip("torch")
    from lance_amd import vector
    return getattr(R, name), getattr(vector, name)


def test_target_partition_size():
    for fn in both("target_partition_size"):
        assert (fn("IVF_FLAT"), fn("IVF_PQ"), fn("IVF_SQ")) == (4096, 8192, 8192)
    with pytest.raises(ValueError):
        both("target_partition_size")[1]("IVF_RQ")


def test_should_split_on_hand_cases():
    for fn in both("should_split"):
        t = 10
        assert fn([40, 3, 40], t) is None                       # exactly 4 * target does not split
        assert fn([40, 3, 41], t) == 2                          # ... one more does
        assert fn([41, 50, 50, 41], t) == 1                     # the largest; on equal sizes the lowest id
        assert fn([], t) is None and fn([41], t) == 0
        assert fn(np.array([7, 4 * 8192 + 1], np.uint32), 8192) == 1


def test_should_join_on_hand_cases():
    for fn in both("should_join"):
        assert 25 * 10 // 100 == 2 and 25 * 30 // 100 == 7      # integer arithmetic
        assert fn([2, 5, 2], 10) is None                        # exactly 25 * target / 100 does not join
        assert fn([2, 5, 1], 10) == 2                           # ... one less does
        assert fn([7, 9, 8], 30) is None and fn([7, 6, 8], 30) == 1
        assert fn([1, 0, 0, 1], 10) == 1                        # the smallest; on equal sizes the lowest id
        assert fn([0], 10) is None and fn([], 10) is None       # nlist == 1 never joins
    # rows mapped to deleted do not count
    offs, ids = np.array([0, 3, 6], np.uint32), np.array([10, 11, 12, 20, 21, 22], np.uint64)
    assert R.surviving_sizes(offs, ids, {}) == [3, 3]
    sizes = R.surviving_sizes(offs, ids, {20: None, 21: None, 10: 99, 77: None})
    assert sizes == [3, 1] and R.should_join(sizes, 10) == 1 and R.should_join([3, 3], 10) is None


@pytest.mark.parametrize("metric", ["l2", "cosine", "dot"])
@pytest.mark.parametrize("nlist", [1, 2, 5, 65, 66, 70])
def test_candidates(metric, nlist):
    rng = np.random.default_rng(nlist)
    cent = rng.normal(0, 1, (nlist, 12)).astype(np.float32)
    for part in {0, nlist // 2, nlist - 1}:
        cands = R.select_candidates(metric, cent, part)
        assert part not in cands and len(set(cands)) == len(cands) == min(65, nlist) - 1 <= 64
        dist = oracle.distance_batch(metric, cent[part], cent)
        keys = R.order_keys(dist)[cands]
        assert (np.diff(keys.astype(np.int64)) >= 0).all()      # nearest first
        # nothing outside the range is nearer than something inside it; P itself is dropped even where it is not the nearest (dot)
        nearest = sorted(range(nlist), key=lambda p: (int(R.order_keys(dist[p:p + 1])[0]), p))[:min(65, nlist)]
        assert cands == [p for p in nearest if p != part][:min(65, nlist) - 1]
    cent[3 % nlist] = cent[0]                                   # equal distances: ordered by partition id
    if nlist >= 5:
        cands = R.select_candidates(metric, cent, 1)
        assert cands.index(0) + 1 == cands.index(3)


def test_total_order_of_the_minimum():
    nan = np.float32(np.nan)
    f = np.array([0.0, -0.0, 1.0, -nan, nan], np.float32)
    assert R.order_keys(f).argsort(kind="stable").tolist() == [3, 1, 0, 2, 4]
    assert R.first_min(np.array([2.0, 1.0, 1.0], np.float32)) == 1 and R.first_min(np.array([0.0, -0.0], np.float32)) == 1
    assert R.first_min(np.array([nan, 5.0], np.float32)) == 1 and R.first_min(np.array([nan, nan], np.float32)) == 0


@pytest.mark.parametrize("metric", ["l2", "cosine", "dot"])
@pytest.mark.parametrize("nlist,d", [(5, 20), (70, 128)])
def test_every_outcome_of_a_split_occurs_and_follows_the_rules(metric, nlist, d):
    c = R.make_case(1, nlist, d, metric)
    got = R.split_dest(metric, c["centroids"], c["offs"], c["ids"], c["part"], c["raw"], c["c12"])
    seen = collections.Counter(got["what"])
    assert all(seen[o] > 0 for o in R.OUTCOMES) and set(seen) == set(R.OUTCOMES), seen
    ids, part, cands = c["ids"][got["pos"]], c["part"], got["cands"]
    # the visit: P first, then the candidates in order, ascending row id inside each; every row of those partitions exactly once
    seg = got["seg_offs"].astype(np.int64)
    assert seg[0] == 0 and seg[-1] == len(ids) == len(set(got["pos"].tolist()))
    for s, p in enumerate([part] + cands):
        mine = ids[seg[s]:seg[s + 1]]
        assert (np.diff(mine.astype(np.int64)) > 0).all()
        assert sorted(mine.tolist()) == sorted(c["ids"][c["offs"][p]:c["offs"][p + 1]].tolist())
    assert not np.array_equal(got["pos"], np.sort(got["pos"]))  # ascending id is not stored order
    # the rules again, row by row, from scalar distances
    dist = {"l2": oracle.l2, "cosine": oracle.cosine, "dot": lambda a, b: np.float32(1.0) - np.float32(oracle.dot(a, b))}[metric]
    f = np.float32
    for i in np.random.default_rng(0).choice(len(ids), 300, replace=False):
        row = c["raw"][int(ids[i])]
        s = int(np.searchsorted(seg, i, side="right")) - 1
        d0, d1, d2 = f(dist(got["seg_cent"][s], row)), f(dist(c["c12"][0], row)), f(dist(c["c12"][1], row))
        new = part if d1 <= d2 else nlist
        if s > 0:
            want = R.NONE if (d0 <= d1 and d0 <= d2) else new
        elif d0 <= d1 and d0 <= d2:
            dc = np.array([dist(row, c["centroids"][p]) for p in cands], f)
            j = int(np.argmin(dc))
            want = cands[j] if (dc[j] <= d1 and dc[j] <= d2) else new
        else:
            want = new
        assert got["dest"][i] == want, (i, got["what"][i])


def test_without_candidates_a_row_goes_by_d1_le_d2():
    c = R.make_case(1, 1, 8, "l2", n=300)
    got = R.split_dest("l2", c["centroids"], c["offs"], c["ids"], 0, c["raw"], c["c12"])
    assert got["cands"] == [] and set(got["what"]) == {"p_direct"} and set(got["dest"].tolist()) == {0, 1}


@pytest.mark.parametrize("metric", ["l2", "cosine", "dot"])
def test_join_sends_every_row_to_its_nearest_candidate_in_the_new_numbering(metric):
    c = R.make_case(2, 6, 20, metric, n=900, part=2, shaped=False)
    got = R.join_dest(metric, c["centroids"], c["offs"], c["ids"], 2, c["raw"])
    assert sorted(got["cand_ids"].tolist()) == [0, 1, 2, 3, 4] and sorted(got["cands"]) == [0, 1, 3, 4, 5]
    ids = c["ids"][got["pos"]]
    assert (np.diff(ids.astype(np.int64)) > 0).all() and len(ids) == c["offs"][3] - c["offs"][2] > 50
    rest = np.delete(c["centroids"], 2, axis=0)                 # the centroid array without row P: the new numbering
    for i in range(0, len(ids), 7):
        dist = oracle.distance_batch(metric, c["raw"][int(ids[i])], rest)
        assert dist[got["dest"][i]] == dist.min()


def test_regroup_keeps_survivors_in_stored_order_and_arrivals_in_visit_order():
    c = R.make_case(1, 5, 20, "l2", n=800)
    got = R.split_dest("l2", c["centroids"], c["offs"], c["ids"], 0, c["raw"], c["c12"])
    n = len(c["ids"])
    old_part = np.repeat(np.arange(5), np.diff(c["offs"].astype(np.int64)))
    moved = got["dest"] != R.NONE
    keep = np.ones(n, bool)
    keep[got["pos"][moved]] = False
    assert not keep[old_part == 0].any()                        # no old row of P survives in place
    arrive_pos = got["pos"][moved]
    stamp = np.arange(n)                                        # a column that records where every row came from
    offs, (ids, src) = R.regroup(6, old_part, keep, arrive_pos, got["dest"][moved], [c["ids"], stamp], [c["ids"][arrive_pos], stamp[arrive_pos]])
    assert sorted(ids.tolist()) == sorted(c["ids"].tolist()) and offs[-1] == n      # every row exactly once
    order_in_visit = {int(p): k for k, p in enumerate(got["pos"])}
    for p in range(6):
        mine = src[offs[p]:offs[p + 1]]
        stay = [r for r in mine if keep[r]]
        come = [r for r in mine if not keep[r]]
        assert mine.tolist() == stay + come and stay == sorted(stay)
        assert [order_in_visit[r] for r in come] == sorted(order_in_visit[r] for r in come)
    assert offs[6] - offs[5] == (got["dest"] == 5).sum() > 0
