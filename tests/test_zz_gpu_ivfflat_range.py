"""IVF_FLAT distance ranges on the GPU (lance_amd/csrc/flat.hip, lance_hip_ivfflat_search_range) against tests/ivfflat_range_spec.py,
bit for bit: ids and distance bits.  Every case runs through IvfFlatIndex.nearest.  The fixtures, and what each of them can tell apart,
are checked on the CPU by tests/test_ivfflat_range_spec.py.  d = 16 takes the partition-major kernels (bound pass and main pass),
d = 20, cosine and the f16 column the query-major kernel, k = 200 and the cut ties the heap replay.  Sorted last: newest device code
last."""
import ctypes as C
import functools

import numpy as np
import pytest

import ivfflat_range_spec as V
import rowid_fixtures as F
import sq_spec as S

pytestmark = pytest.mark.gpu
f32 = np.float32
K, NPROBES = V.K, V.NPROBES


def eng():
    import lance_amd
    return lance_amd.default_engine()


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


def build(x, cent, metric, rid=None):
    """an IvfFlatIndex with GIVEN centroids (and row ids), through the index's own transform chain"""
    from lance_amd.engine import DeviceFlatIndex, to_device
    from lance_amd.vector import IvfFlatIndex, _transform_rows
    e = eng()
    ct = to_device(np.ascontiguousarray(cent))
    part, xs = _transform_rows(e, "IVF_FLAT", metric, to_device(np.ascontiguousarray(x)), ct)
    return IvfFlatIndex(DeviceFlatIndex.create(e, metric, ct, xs, part, rid), None, None, None)


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (index, x, q, centroids, metric, row ids | None)"""
    x, q, cent = V.base_fixture()
    metric, rid = "l2", None
    if name in ("dot", "cosine"):
        metric = name
    elif name == "d20":
        x, q, cent = V.padded(x, q, cent)
    elif name in ("f16_dot", "f16_cosine"):
        metric = name[4:]
        x, q, cent = x.astype(np.float16), q.astype(np.float16), cent.astype(np.float16)
    elif name == "permuted":
        rid = S.permuted_ids(len(x), 3)
    elif name == "addresses":
        rid = F.row_addresses(len(x), 3)
    elif name == "small_offsets":
        rid = F.small_offset_addresses(len(x), 3)
    elif name == "nan":
        x, q, cent = V.nan_fixture()
        metric = "dot"
    else:
        assert name == "l2"
    if metric == "cosine":      # centroids of a cosine index live among the normalised rows
        import oracle
        cent = np.ascontiguousarray(np.asarray(oracle.normalize(cent)).astype(x.dtype))
    return build(x, cent, metric, rid), x, q, cent, metric, rid


def check(name, lower, upper, k=K, nprobes=NPROBES, prefilter=None, q=None):
    import oracle
    ix, x, q0, cent, metric, rid = case(name)
    q = q0 if q is None else q
    gi, gd = ix.nearest(q, k, nprobes, prefilter=prefilter, distance_range=(lower, upper))
    oi, od = V.search(oracle, x, cent, q, k, nprobes, metric, lower, upper, row_ids=rid, prefilter=prefilter)
    assert gi.dtype == np.uint64 and (gi == oi).all(), (name, lower, upper, k, nprobes, np.argwhere(gi != oi)[:4])
    assert same_bits(gd, od), (name, lower, upper, k, nprobes)
    return oi, od


DOT_RANGES = [(-20.0, 0.0), (-45.0, -30.0), (-100.0, -99.0), (-10.0, -10.0), (None, -20.0), (10.0, None)]


@pytest.mark.parametrize("i", range(len(V.RANGES)))
def test_partition_major_l2_and_dot(i):
    lower, upper = V.RANGES[i]
    oi, _ = check("l2", lower, upper)
    if (lower, upper) == (60.0, 90.0):
        assert eng().search_stats() >= 1                # ties across position k inside the range: replayed through the heap
    if (lower, upper) in ((0.0, 1.0), (70.0, 70.0)):
        assert (oi == V.UNSET).all()
    dl, du = DOT_RANGES[i]
    di, _ = check("dot", dl, du)
    if i in (2, 3):
        assert (di == V.UNSET).all()
    elif i == 1:
        assert (V.found(di) < K).any() and (V.found(di) > 0).any()


def test_run_time_dimension():
    for lower, upper in V.RANGES:
        oi, od = check("d20", lower, upper)
        ri, rd = check("l2", lower, upper)
        assert (oi == ri).all() and same_bits(od, rd)       # zero padding changes no L2 distance: one answer from both kernels


@pytest.mark.parametrize("name", ["cosine", "f16_dot", "f16_cosine"])
def test_cosine_and_f16_columns_hit_a_bound_exactly(name):
    import oracle
    _, x, q, cent, metric, _ = case(name)
    d0 = np.sort(V.probed_distances(oracle, x, cent, q[:1], NPROBES, metric)[0])
    lower, upper = float(d0[4]), float(d0[59])              # query 0's 5th and 60th smallest probed distance
    oi, od = check(name, lower, upper)
    assert od[0, 0] == f32(lower) and not (od[0] == f32(upper)).any()      # lower inclusive, upper exclusive, on real values
    check(name, None, upper)
    check(name, lower, None)
    check(name, lower, upper, k=200)


def test_every_query_through_the_heap_replay():
    oi, _ = check("l2", 60.0, 90.0, k=200)
    assert (V.found(oi) < 200).any() and eng().search_stats() == oi.shape[0]
    check("dot", -20.0, 0.0, k=200)
    check("d20", 60.0, 90.0, k=129)


def test_nearest_partition_without_a_bound():
    oi, _ = check("l2", 40.0, 64.0, nprobes=1)
    assert (V.found(oi) < K).any() and (V.found(oi) == K).any()
    check("d20", 40.0, 64.0, nprobes=1)


def test_range_with_prefilter_and_explicit_row_ids():
    n = 3000
    _, _, _, _, _, rid = case("permuted")
    third = np.zeros(int(rid.max()) + 1, bool)
    third[::3] = True                                        # every third row id
    for lower, upper in ((60.0, 90.0), (40.0, 64.0), (None, 60.0)):
        oi, _ = check("permuted", lower, upper, prefilter=third)
        assert third[oi[oi != V.UNSET].astype(np.int64)].all()
    check("permuted", 60.0, 90.0, k=200, prefilter=third)
    oi, _ = check("addresses", 60.0, 90.0)                   # Lance row addresses: the ties are broken on all 64 bits
    assert (oi[oi != V.UNSET] >= np.uint64(1 << 31)).all()
    check("addresses", 60.0, 90.0, k=200)
    mask = np.arange(n) % 3 != 0                             # only addresses below n lie inside the mask
    oi, _ = check("small_offsets", 60.0, 90.0, prefilter=mask)
    assert (oi != V.UNSET).any() and (oi[oi != V.UNSET] < n).all()


def test_batch_crossing_the_query_chunk():
    """2100 queries: more than one pass of 2048 (FLAT_QCHUNK, flat.hip)"""
    _, _, q, _, _, _ = case("l2")
    big = np.ascontiguousarray(np.tile(q, (33, 1))[:2100])
    oi, od = check("l2", 60.0, 90.0, q=big)
    assert (oi[:-64] == oi[64:]).all() and same_bits(od[:-64], od[64:])


def test_zero_signs_and_nan():
    """a query equal to a stored row: distance +0.0; see tests/test_ivfflat_range_spec.py::test_zero_signs"""
    _, x, _, _, _, _ = case("l2")
    q0 = x[5:6].copy()
    for lower, upper, kept in ((0.0, 1.0, True), (-0.0, 1.0, True), (-5.0, 0.0, False), (-5.0, -0.0, False)):
        oi, _ = check("l2", lower, upper, nprobes=1, q=q0)
        assert (V.found(oi)[0] > 0) == kept
    _, _, qn, _, _, _ = case("nan")
    for k in (10, 128, 400):                                 # a NaN distance lies above every bound
        oi, od = check("nan", -1e30, None, k=k, nprobes=2)
        assert not (oi == V.NAN_ROW).any() and not np.isnan(od).any()
    ix = case("nan")[0]
    gi, gd = ix.nearest(qn, 400, 2)                          # ... and without a range the row is there, last
    assert (gi == V.NAN_ROW).any() and np.isnan(gd).sum() == 1


def test_refusals_and_empty_batches():
    import torch
    import lance_amd
    ix, _, q, _, _, _ = case("l2")
    with pytest.raises(lance_amd.LanceHipError, match="lower bound .* is above the upper bound"):
        ix.nearest(q, K, NPROBES, distance_range=(2.0, 1.0))
    gi, gd = ix.nearest(q[:0], K, NPROBES, distance_range=(60.0, 90.0))
    assert gi.shape == (0, K) and gd.shape == (0, K) and gi.dtype == np.uint64
    # the entry point refuses an index of another kind
    sq = lance_amd.create_index(S.gaussian(300, 32, 1, seed=1)[0], "IVF_SQ", num_partitions=2, max_iters=2)._ix
    e = eng()
    tq = torch.zeros((2, 32), dtype=torch.float32, device="cuda")
    ids = torch.full((2, 5), -7, dtype=torch.int64, device="cuda")
    dists = torch.zeros((2, 5), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    assert e.lib.lance_hip_ivfflat_search_range(e.h, sq.h, p(tq), 2, 5, 1, None, 0, 0.0, 1.0, p(ids), p(dists)) == lance_amd._lib.EINVAL
    assert (ids.cpu().numpy() == -7).all()


def test_raw_entry_point():
    """lance_hip_ivfflat_search_range called directly: mask pointer NULL (the range alone) and with a mask"""
    import oracle
    import torch
    ix, x, q, cent, metric, _ = case("l2")
    e = eng()
    tq = torch.from_numpy(q).cuda()
    ids = torch.empty((len(q), K), dtype=torch.int64, device="cuda")
    dists = torch.empty((len(q), K), dtype=torch.float32, device="cuda")
    allow = np.arange(len(x)) % 3 == 0
    ta = torch.from_numpy(allow.astype(np.uint8)).cuda()
    p = lambda t: C.c_void_p(t.data_ptr())
    for mask in (None, allow):
        torch.cuda.synchronize()
        rc = e.lib.lance_hip_ivfflat_search_range(e.h, ix._ix.h, p(tq), len(q), K, NPROBES, None if mask is None else p(ta),
                                                  0 if mask is None else ta.numel(), 60.0, 90.0, p(ids), p(dists))
        assert rc == 0
        oi, od = V.search(oracle, x, cent, q, K, NPROBES, metric, 60.0, 90.0, prefilter=mask)
        assert (ids.cpu().numpy().view(np.uint64) == oi).all() and same_bits(dists.cpu().numpy(), od)
    # FLT_MAX ends are the open ends: the un-ranged answer
    fmax = float(np.finfo(f32).max)
    torch.cuda.synchronize()
    assert e.lib.lance_hip_ivfflat_search_range(e.h, ix._ix.h, p(tq), len(q), K, NPROBES, None, 0, -fmax, fmax, p(ids), p(dists)) == 0
    oi, od = oracle.ivfflat_search(x, cent, q, K, NPROBES, metric)
    assert (ids.cpu().numpy().view(np.uint64) == oi).all() and same_bits(dists.cpu().numpy(), od)


def test_unranged_search_is_unchanged(monkeypatch):
    import oracle
    ix, x, q, cent, metric, _ = case("l2")
    e = eng()
    calls = []
    real = e.lib.lance_hip_ivfflat_search_range
    monkeypatch.setattr(e.lib, "lance_hip_ivfflat_search_range", lambda *a: calls.append(1) or real(*a))
    for name in ("l2", "dot", "d20"):
        ix, x, q, cent, metric, _ = case(name)
        for k, nprobes in ((K, NPROBES), (200, 2)):
            gi, gd = ix.nearest(q, k, nprobes)
            oi, od = oracle.ivfflat_search(x, cent, q, k, nprobes, metric)
            assert (gi == oi).all() and same_bits(gd, od), (name, k)
    ix, x, q, cent, metric, _ = case("l2")
    allow = np.arange(len(x)) % 3 == 0
    gi, gd = ix.nearest(q, K, NPROBES, prefilter=allow)
    keep = np.flatnonzero(allow)
    oi, od = oracle.ivfflat_search(x[keep], cent, q, K, NPROBES, metric, row_ids=keep.astype(np.uint64))
    assert (gi == oi).all() and same_bits(gd, od)
    assert not calls
    ix.nearest(q, K, NPROBES, distance_range=(60.0, 90.0))
    assert calls == [1]
