"""Partition split / join on the GPU (lance_amd/csrc/rebalance.hip) against tests/rebalance_spec.py, bit for bit: every decision is a
chain of `<=` between f32 distances, so one differing bit of one distance moves a row.  The kernel's indices are checked on the CPU
first (tests/test_rebalance_kernels_cpu.py).  Sorted last: newest device code last.
1. lance_hip_reassign_rows' dest; 2. lance_hip_index_split / _join for IVF_PQ (8- and 4-bit), IVF_FLAT and IVF_SQ: every stored byte,
the centroids, the untouched source, and `nearest` against an index made by the existing create route from the specification's
part ids and codes; 3. append / delete with rebalance=True at and past the thresholds, the defaults, the trained route; 4. refusals.

Shapes: d = 8 and 16 take cosine_once, d = 20 leaves a tail of 4 after one chunk of 16 (a reader that runs past a row shows there),
d = 128 is the flagship's; with 64 candidates d = 141 is the largest dimension whose centroid table and row tile are staged in LDS and
d = 142 the first that reads them in place.  nlist = 1, 2, 5, 70 give 0, 1, 4 and 64 candidates; at 70 five partitions lie outside the
range.  Row ids are a permutation with gaps, so the gather by id and the ascending-id visit order both differ from stored order.  Among
the neighbours of the split partition one is empty, one holds 1 row and one 257 rows (one more than a workgroup)."""
import collections
import ctypes as C
import functools

import numpy as np
import pytest

import rebalance_spec as R

pytestmark = pytest.mark.gpu
METRICS = ["l2", "cosine", "dot"]


def eng():
    import lance_amd
    return lance_amd.default_engine()


@functools.lru_cache(maxsize=None)
def case(seed, nlist, d, metric, n=2400, tie=None):
    """-> (inputs, the specification's split decision): computed once, shared, never modified"""
    c = R.make_case(seed, nlist, d, metric, n=n, tie=tie)
    return c, R.split_dest(metric, c["centroids"], c["offs"], c["ids"], c["part"], c["raw"], c["c12"])


def gpu_split_dest(c, want, ids=None):
    dest = eng().reassign_rows(c["metric"], c["raw"], c["ids"][want["pos"]] if ids is None else ids, want["seg_offs"], want["seg_cent"],
                               np.asarray(want["cands"], np.uint32), c["c12"], c["part"], len(c["centroids"]))
    return dest.cpu().numpy().view(np.uint32)


def twins(c, want):
    """the two candidates with bitwise equal centroids, in candidate order"""
    bits = [c["centroids"][p].tobytes() for p in want["cands"]]
    (a, b), = [(want["cands"][i], want["cands"][j]) for i in range(len(bits)) for j in range(i + 1, len(bits)) if bits[i] == bits[j]]
    return a, b


def staged_counts():
    e = eng()
    return e.timing_query("count:rebalance_reassign")[1], e.timing_query("count:rebalance_reassign_global")[1]


# ---- 1. the decision ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nlist,d", [(1, 8), (2, 16), (5, 20), (5, 128), (70, 8), (70, 20), (70, 128)])
def test_split_dest(metric, nlist, d):
    c, want = case(1, nlist, d, metric)
    sizes = np.diff(c["offs"].astype(np.int64))
    if nlist >= 5:
        assert {0, 1, 257} <= set(sizes[want["cands"][1:4]].tolist())
    assert len(want["cands"]) == min(64, nlist - 1) and 2000 <= len(c["ids"]) <= 5000
    assert not np.array_equal(np.sort(c["ids"]), np.arange(len(c["ids"])))
    before = staged_counts()
    dest = gpu_split_dest(c, want)
    after = staged_counts()
    assert (after[0] - before[0], after[1] - before[1]) == (1, 0)
    wrong = dest != want["dest"]
    assert not wrong.any(), (int(wrong.sum()), collections.Counter(np.asarray(want["what"])[wrong]))
    seen = collections.Counter(want["what"])
    if (nlist, d) in ((5, 20), (70, 128)):                      # no outcome of a split is left untested
        assert all(seen[o] > 0 for o in R.OUTCOMES), seen


@pytest.mark.parametrize("metric,d,in_place", [("l2", 141, 0), ("cosine", 141, 0), ("dot", 141, 0), ("l2", 142, 1), ("cosine", 142, 1), ("dot", 142, 1)])
def test_split_dest_on_either_side_of_the_lds_limit(metric, d, in_place):
    c, want = case(2, 70, d, metric)
    before = staged_counts()
    dest = gpu_split_dest(c, want)
    after = staged_counts()
    assert (after[0] - before[0], after[1] - before[1]) == (1 - in_place, in_place)
    assert len(want["cands"]) == 64 and np.array_equal(dest, want["dest"])


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("tie", ["c1=c0", "c1=c2", "candidates"])
def test_ties(metric, tie):
    c, want = case(29, 5, 20, metric, tie=tie)
    dest = gpu_split_dest(c, want)
    assert np.array_equal(dest, want["dest"])
    p_rows = slice(0, int(want["seg_offs"][1]))
    if tie == "c1=c0":          # d0 == d1 for every row of P: only `<=` lets a row reach the candidates or stay near c0
        assert np.array_equal(c["c12"][0].view(np.uint32), c["centroids"][c["part"]].view(np.uint32))
        assert any(w != "p_direct" for w in want["what"][p_rows])
    if tie == "c1=c2":          # d1 <= d2 sends every moving row to c1
        assert not (dest == len(c["centroids"])).any() and (dest == c["part"]).any()
    if tie == "candidates":     # two bitwise equal candidate centroids: the first position wins
        a, b = twins(c, want)
        assert (dest[p_rows] == a).any() and not (dest[p_rows] == b).any()


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nlist,d", [(2, 8), (5, 20), (70, 128), (70, 150)])
def test_join_dest(metric, nlist, d):
    c, _ = case(1 if d != 150 else 4, nlist, d, metric)
    want = R.join_dest(metric, c["centroids"], c["offs"], c["ids"], c["part"], c["raw"])
    dest = eng().reassign_rows(metric, c["raw"], c["ids"][want["pos"]], want["seg_offs"], want["seg_cent"], want["cand_ids"])
    dest = dest.cpu().numpy().view(np.uint32)
    assert len(dest) > 256 and np.array_equal(dest, want["dest"])
    assert set(dest.tolist()) <= set(want["cand_ids"].tolist()) and dest.max() < nlist - 1


def test_a_row_id_beyond_the_raw_vectors_is_refused():
    import lance_amd
    c, want = case(1, 5, 20, "l2")
    ids = c["ids"][want["pos"]].copy()
    ids[[0, 300, len(ids) - 1]] = [len(c["raw"]), 1 << 40, 2 ** 64 - 1]
    with pytest.raises(lance_amd.LanceHipError, match="n_raw") as ei:
        gpu_split_dest(c, want, ids=ids)
    assert ei.value.code == lance_amd._lib.EINVAL
    assert np.array_equal(gpu_split_dest(c, want), want["dest"])            # ... and the next call is served as usual


def test_reassign_rows_refusals():
    import lance_amd
    c, want = case(1, 5, 20, "l2")
    e = eng()
    args = (c["ids"][want["pos"]], want["seg_offs"], want["seg_cent"], np.asarray(want["cands"], np.uint32))
    with pytest.raises(ValueError, match="float32"):
        e.reassign_rows("l2", c["raw"].astype(np.float16), *args, c["c12"], 0, 5)
    with pytest.raises(ValueError, match="segment offsets"):
        e.reassign_rows("l2", c["raw"], args[0], args[1][:-1], args[2], args[3], c["c12"], 0, 5)
    with pytest.raises(lance_amd.LanceHipError, match="at least one candidate"):
        e.reassign_rows("l2", c["raw"], args[0][:10], np.array([0, 10], np.uint32), args[2][:1], np.zeros(0, np.uint32))
    many = np.arange(65, dtype=np.uint32)
    with pytest.raises(lance_amd.LanceHipError, match="at most 64"):
        e.reassign_rows("l2", c["raw"], args[0][:10], np.full(67, 10, np.uint32), np.zeros((66, 20), np.float32), many, c["c12"], 0, 5)


# ---- 2. the index: lance_hip_index_split / _join ------------------------------------------------------------------------------------
KINDS = [("IVF_PQ", 8), ("IVF_PQ", 4), ("IVF_FLAT", 8), ("IVF_SQ", 8)]
M = 4


class Built:
    """a device index over a case's stored rows (stored partitions as the case gives them, payload by the specification's encoder), and
    the columns it was made from"""

    def __init__(self, kind, nbits, c):
        self.kind, self.nbits, self.c, self.metric = kind, nbits, c, c["metric"]
        d = c["centroids"].shape[1]
        rng = np.random.default_rng(d + nbits)
        self.model = {}
        if kind == "IVF_PQ":
            self.model = dict(codebook=rng.normal(0, 0.8, (M, 1 << nbits, d // M)).astype(np.float32), nbits=nbits)
        if kind == "IVF_SQ":
            self.model = dict(bounds=(-3.0, 3.5))              # rows outside clip
        self.part = R.index_part_ids(c["offs"]).astype(np.uint32)
        self.cols = R.encode_rows(kind, self.metric, c["raw"][c["ids"].astype(np.int64)], self.part, c["centroids"], **self.model)
        self.ix = self.create(c["centroids"], self.part, self.cols, c["ids"])

    def create(self, cent, part, cols, ids):
        from lance_amd.engine import DeviceFlatIndex, DeviceIndex, DeviceSqIndex
        e = eng()
        if self.kind == "IVF_PQ":
            return DeviceIndex.create(e, self.metric, cent, self.model["codebook"], part, cols[0], ids)
        if self.kind == "IVF_FLAT":
            return DeviceFlatIndex.create(e, self.metric, cent, cols[0], part, ids)
        return DeviceSqIndex.create(e, self.metric, cent, cols[0], part, self.model["bounds"], ids)


@functools.lru_cache(maxsize=None)
def built(kind, nbits, seed, nlist, d, metric, n=2400):
    return Built(kind, nbits, R.make_case(seed, nlist, d, metric, n=n))


def stored(ix):
    out = ix.export_rows()
    return out[0], out[-1], list(out[1:-1])


def same_storage(got, offs, ids, cols):
    return np.array_equal(got[0], offs) and np.array_equal(got[1], ids) and len(got[2]) == len(cols) and all(
        a.shape == b.shape and np.array_equal(a.view(np.uint8), np.ascontiguousarray(b).view(np.uint8)) for a, b in zip(got[2], cols))


def same_answers(a, b, q, nlist):
    import torch
    for nprobes in (1, nlist):
        x, y = a.search(q, 10, nprobes), b.search(q, 10, nprobes)
        if not (torch.equal(x[0], y[0]) and torch.equal(x[1].view(torch.int32), y[1].view(torch.int32))):
            return False
    return True


def queries(c):
    rng = np.random.default_rng(9)
    return (c["raw"][c["ids"][rng.choice(len(c["ids"]), 64, replace=False)].astype(np.int64)] + rng.normal(0, 0.05, (64, c["raw"].shape[1]))).astype(np.float32)


@pytest.mark.parametrize("kind,nbits", KINDS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nlist,d", [(1, 8), (5, 20), (70, 128)])
def test_split_partition(kind, nbits, metric, nlist, d):
    b = built(kind, nbits, 1, nlist, d, metric)
    c = b.c
    before = stored(b.ix)
    assert same_storage(before, c["offs"], c["ids"], b.cols)
    got = b.ix.split(c["part"], c["c12"], c["raw"])
    cent, offs, ids, cols, dec = R.split_storage(kind, metric, c["centroids"], c["offs"], c["ids"], b.cols, c["part"], c["raw"], c["c12"], **b.model)
    out = stored(got)
    assert len(offs) == nlist + 2 and sorted(ids.tolist()) == sorted(c["ids"].tolist())      # every row exactly once
    assert same_storage(out, offs, ids, cols)
    assert np.array_equal(got.centroids.cpu().numpy().view(np.uint32), cent.view(np.uint32))
    assert same_storage(stored(b.ix), *before) and got.h.value != b.ix.h.value
    want = b.create(cent, R.index_part_ids(offs).astype(np.uint32), cols, ids)
    assert same_storage(stored(want), offs, ids, cols) and same_answers(got, want, queries(c), nlist + 1)


@pytest.mark.parametrize("kind,nbits", KINDS)
@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("nlist,d,part", [(2, 8, 1), (5, 20, 0), (70, 128, 0), (5, 20, "empty")])
def test_join_partition(kind, nbits, metric, nlist, d, part):
    b = built(kind, nbits, 1, nlist, d, metric)
    c = b.c
    if part == "empty":
        part = int(np.flatnonzero(np.diff(c["offs"].astype(np.int64)) == 0)[0])
    before = stored(b.ix)
    got = b.ix.join(part, c["raw"])
    cent, offs, ids, cols, dec = R.join_storage(kind, metric, c["centroids"], c["offs"], c["ids"], b.cols, part, c["raw"], **b.model)
    assert len(offs) == nlist and sorted(ids.tolist()) == sorted(c["ids"].tolist())
    assert same_storage(stored(got), offs, ids, cols)
    assert np.array_equal(got.centroids.cpu().numpy().view(np.uint32), cent.view(np.uint32))
    assert same_storage(stored(b.ix), *before)
    want = b.create(cent, R.index_part_ids(offs).astype(np.uint32), cols, ids)
    assert same_answers(got, want, queries(c), nlist - 1)


# ---- 3. the wrappers: thresholds, defaults, the trained route ------------------------------------------------------------------------
def wrapped(kind, metric="l2", d=8, n=900, nbits=8):
    """create_index over three clusters with supplied centroids -> (index, rows, centroids)"""
    import lance_amd
    rng = np.random.default_rng(40 + d)
    cent = rng.normal(0, 4, (3, d)).astype(np.float32)
    x = (cent[rng.integers(0, 3, n)] + rng.normal(0, 1, (n, d))).astype(np.float32)
    kw = dict(index_type=kind, metric=metric, num_partitions=3, ivf_centroids=cent, max_iters=2)
    if kind == "IVF_PQ":
        kw.update(num_sub_vectors=M, num_bits=nbits, pq_codebook=rng.normal(0, 0.8, (M, 1 << nbits, d // M)).astype(np.float32))
    return lance_amd.create_index(x, **kw), x, cent


@pytest.mark.parametrize("kind", ["IVF_PQ", "IVF_FLAT", "IVF_SQ"])
def test_append_splits_past_four_times_the_target(kind):
    ix, x, cent = wrapped(kind)
    sizes = np.diff(ix.export_rows()[0].astype(np.int64))
    big = int(np.argmax(sizes))
    k = 4 + (-int(sizes[big])) % 4                              # rows that bring the largest partition to a multiple of 4
    t = (int(sizes[big]) + k) // 4
    more = np.repeat(cent[big:big + 1], k + 1, axis=0) + np.linspace(0, 0.5, k + 1, dtype=np.float32)[:, None]
    raw = np.concatenate([x, more])
    at = ix.append(more[:k], raw=raw, rebalance=True, target_partition_size=t)          # exactly 4 t rows: no split
    plain = ix.append(more[:k])
    assert same_storage(stored(at), *stored(plain)) and len(at.export_rows()[0]) == 4
    assert same_storage(stored(ix.append(more[:k], rebalance=False)), *stored(plain))
    past = ix.append(more, raw=raw, rebalance=True, target_partition_size=t, seed=3)    # 4 t + 1: split
    out = past.export_rows()
    assert len(out[0]) == 5 and past.params.num_partitions == 4 and sorted(out[-1].tolist()) == list(range(len(raw)))
    merged = stored(ix.append(more))
    c12 = R.train_split_centroids("l2", merged[1][merged[0][big]:merged[0][big + 1]], raw, 3)
    assert np.array_equal(past.centroids[[big, 3]].view(np.uint32), c12.view(np.uint32))      # the trained route: the oracle's k-means
    model = {}
    if kind == "IVF_PQ":
        model = dict(codebook=ix.codebook, nbits=8)
    if kind == "IVF_SQ":
        model = dict(bounds=ix.bounds)
    cent_new, offs, ids, cols, _ = R.split_storage(kind, "l2", cent, merged[0], merged[1], merged[2], big, raw, c12, **model)
    assert same_storage(stored(past), offs, ids, cols)
    again = ix.append(more).split_partition(big, raw, seed=3)
    assert same_storage(stored(again), offs, ids, cols)
    with pytest.raises(ValueError, match="raw"):
        ix.append(more, rebalance=True, target_partition_size=t)
    if kind == "IVF_PQ":        # raw stays attached for refine whether or not a partition was split: the same answers as a handle given raw
        q = (raw[::37] + np.float32(0.01)).astype(np.float32)
        for got, n_rows in ((at, len(x) + k), (past, len(raw))):
            a = got.nearest(q, k=5, nprobes=2, refine_factor=4)
            twin = type(got)(type(got._ix).merge([got._ix], raw=raw), got.params)      # an equal copy with raw attached explicitly
            b = twin.nearest(q, k=5, nprobes=2, refine_factor=4)
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
            found = a[0][:, 0] < n_rows                          # refined: the distances are the exact ones of the returned rows
            assert found.all() and all(np.float32(R.oracle.l2(q[i], raw[int(a[0][i, 0])])) == a[1][i, 0] for i in range(0, len(q), 5))


# P holds more than 512 rows (the trainer sees the first 512 in ascending row id), L2 and cosine (normalised rows, trained in L2)
@pytest.mark.parametrize("kind,metric", [("IVF_FLAT", "l2"), ("IVF_FLAT", "cosine"), ("IVF_PQ", "cosine"), ("IVF_SQ", "cosine")])
def test_trained_split_equals_the_oracles_kmeans(kind, metric):
    ix, x, cent = wrapped(kind, metric=metric, n=2100)
    offs, ids, cols = stored(ix)
    big = int(np.argmax(np.diff(offs.astype(np.int64))))
    mine = ids[offs[big]:offs[big + 1]]
    assert len(mine) > 512
    c12 = R.train_split_centroids(metric, mine, x, 7)
    all_rows = R.oracle.kmeans_train(R.oracle.normalize(x[np.sort(mine).astype(np.int64)]) if metric == "cosine" else x[np.sort(mine).astype(np.int64)],
                                     2, max_iters=50, seed=7, metric="l2")[0]
    assert not np.array_equal(c12, all_rows)                    # the truncation to 512 rows matters at this size
    got = ix.split_partition(big, x, seed=7)
    assert np.array_equal(got.centroids[[big, 3]].view(np.uint32), c12.view(np.uint32))
    model = {}
    if kind == "IVF_PQ":
        model = dict(codebook=ix.codebook, nbits=8)
    if kind == "IVF_SQ":
        model = dict(bounds=ix.bounds)
    cent_new, o2, i2, c2, _ = R.split_storage(kind, metric, ix.centroids, offs, ids, cols, big, x, c12, **model)
    assert same_storage(stored(got), o2, i2, c2)


@pytest.mark.parametrize("kind", ["IVF_PQ", "IVF_FLAT", "IVF_SQ"])
def test_delete_joins_below_a_quarter_of_the_target(kind):
    import index_update_spec as U
    ix, x, cent = wrapped(kind)
    offs, ids, cols = stored(ix)
    t = 8
    assert 25 * t // 100 == 2
    mine = ids[offs[1]:offs[2]]
    at = ix.delete(mine[2:], raw=x, rebalance=True, target_partition_size=t)            # 2 rows survive: the threshold itself, no join
    assert same_storage(stored(at), *stored(ix.delete(mine[2:]))) and len(at.export_rows()[0]) == 4
    assert same_storage(stored(ix.delete(mine[2:], rebalance=False)), *stored(ix.delete(mine[2:])))
    below = ix.delete(mine[1:], raw=x, rebalance=True, target_partition_size=t)         # 1 row survives: joined, then the mapping
    model = {}
    if kind == "IVF_PQ":
        model = dict(codebook=ix.codebook, nbits=8)
    if kind == "IVF_SQ":
        model = dict(bounds=ix.bounds)
    cent_new, o2, i2, c2, _ = R.join_storage(kind, "l2", cent, offs, ids, cols, 1, x, **model)
    wo, wi, wc = U.remap_storage(o2, i2, c2, {int(g): None for g in mine[1:]})
    got = stored(below)
    assert len(got[0]) == 3 and below.params.num_partitions == 2 and same_storage(got, wo, wi, wc)
    assert np.array_equal(below.centroids.view(np.uint32), cent[[0, 2]].view(np.uint32))      # ids above the joined partition shift down
    assert int(mine[0]) in got[1] and not set(mine[1:].tolist()) & set(got[1].tolist())
    with pytest.raises(ValueError, match="raw"):
        ix.delete(mine[1:], rebalance=True, target_partition_size=t)


# ---- 4. refusals ------------------------------------------------------------------------------------------------------------------------
def test_split_and_join_refusals():
    import lance_amd
    from lance_amd.engine import DeviceFlatIndex
    ix, x, cent = wrapped("IVF_FLAT")
    c12 = cent[:2]
    before = stored(ix)
    with pytest.raises(ValueError, match="does not exist"):
        ix.split_partition(3, x, centroids=c12)
    with pytest.raises(ValueError, match="does not exist"):
        ix.join_partition(7, x)
    with pytest.raises(ValueError, match="raw"):
        ix.split_partition(0, None, centroids=c12)
    with pytest.raises(ValueError, match="raw"):
        ix.join_partition(0, None)
    with pytest.raises(ValueError, match="n_raw"):                 # a stored row id beyond the raw vectors: nothing ranked or moved
        ix.split_partition(0, x[:100], centroids=c12)
    with pytest.raises(ValueError, match="n_raw"):
        ix.join_partition(0, x[:100])
    offs, ids, _ = before
    one = ix.delete(ids[offs[1] + 1:offs[2]])                     # partition 1 keeps one row
    with pytest.raises(ValueError, match="at least 2"):
        one.split_partition(1, x, centroids=c12)
    with pytest.raises(ValueError, match="at least 2"):
        one.split_partition(1, x)
    single = one.join_partition(1, x).join_partition(1, x)        # down to one partition
    assert len(single.export_rows()[0]) == 2
    with pytest.raises(ValueError, match="nlist == 1"):
        single.join_partition(0, x)
    h = DeviceFlatIndex.create(eng(), "l2", cent.astype(np.float16), x.astype(np.float16), np.zeros(len(x), np.uint32))
    with pytest.raises(lance_amd.LanceHipError, match="f32 columns only") as ei:
        h.split(0, c12, x)
    assert ei.value.code == lance_amd._lib.EINVAL
    with pytest.raises(lance_amd.LanceHipError, match="f32 columns only"):
        h.join(0, x)
    rq = lance_amd.create_index(x, "IVF_RQ", metric="l2", num_partitions=3, num_bits=1, ivf_centroids=cent)
    for call in (lambda: rq.split_partition(0, x), lambda: rq.join_partition(0, x)):
        with pytest.raises(NotImplementedError, match="IVF_RQ"):
            call()
    # ... and the library itself refuses an IVF_RQ handle (EINVAL, nothing handed out)
    c12_d = eng().normalize(c12)                                 # (any [2][d] f32 device array)
    from lance_amd.engine import to_device
    raw_d = to_device(x)
    for name, args in (("lance_hip_index_split", (0, C.c_void_p(c12_d.data_ptr()), C.c_void_p(raw_d.data_ptr()), len(x))),
                       ("lance_hip_index_join", (0, C.c_void_p(raw_d.data_ptr()), len(x)))):
        out = C.c_void_p()
        rc = getattr(eng().lib, name)(eng().h, rq._ix.h, *args, C.byref(out))
        assert rc == lance_amd._lib.EINVAL and out.value is None and b"IVF_RQ" in eng().lib.lance_hip_last_error()
    assert same_storage(stored(ix), *before)
