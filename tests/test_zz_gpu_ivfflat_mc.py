"""IVF_FLAT batched search on the matrix cores (lance_amd/csrc/flat_ivf_mc.hip) against the CPU specification of the IVF_FLAT search
(tests/ivfflat_range_spec.py, un-ranged), bit for bit: ids and distance bits, through IvfFlatIndex.nearest.

The fixture.  Centroid p is A e_p; a row of partition p is A e_p plus unit normal noise on every element, so the partition sizes are
the ones asked for (asserted) -- 300, 513 (three row blocks, the last of one row), 129, 128, 127, 0, 77, 1.  A query is
A (w . e) + noise with the weights w a ranking of the partitions: partition 0 is in every query's four probes (two query tiles),
partition 7 (one row: fewer than k, so that query has no bound) in query 0's alone.  Real-valued floats: nothing is exact in bf16.
Near-ties: twelve copies of one row of partition 1 (more than k: the cut falls inside them), two rows one ulp from it in one element,
four copies of a row of partition 2; queries 1 .. 12 sit on top of the twelve.  Sorted last: newest device code last."""
import functools

import numpy as np
import pytest

import ivfflat_range_spec as V
import rowid_fixtures as F
import sq_spec as S

pytestmark = pytest.mark.gpu
f32 = np.float32
SIZES = (300, 513, 129, 128, 127, 0, 77, 1)
NLIST, NPROBES, A = 8, 4, 10.0
QCHUNK, G = 2048, 16                                             # flat.hip FLAT_QCHUNK, IVFFLAT_MC_MIN_PAIRS_PER_LIST


@functools.lru_cache(maxsize=None)
def build(metric, d, nq=200, scale=1.0, ids=None, odd=False, mass=0):
    """-> (IvfFlatIndex, x, q, centroids, row ids | None).  odd: a zero, a NaN and an inf row, and (cosine) a zero query;
    mass: partition 0 is that many identical rows instead"""
    import oracle
    from lance_amd.engine import DeviceFlatIndex, to_device
    from lance_amd.vector import IvfFlatIndex, _transform_rows
    rng = np.random.default_rng(d + nq)
    sizes = (mass,) + SIZES[1:] if mass else SIZES
    cent = np.zeros((NLIST, d), f32)
    cent[np.arange(NLIST), np.arange(NLIST)] = A
    x = (np.repeat(cent, sizes, axis=0) + rng.standard_normal((sum(sizes), d))).astype(f32)
    p1, p2 = sizes[0], sizes[0] + sizes[1]
    if mass:
        x[:mass] = x[0]
    x[p1:p1 + 12] = x[p1]
    x[p1 + 12:p1 + 14] = x[p1]
    x[p1 + 12, 3] = np.nextafter(x[p1, 3], f32(np.inf)); x[p1 + 13, 5] = np.nextafter(x[p1, 5], f32(-np.inf))
    x[p2:p2 + 4] = x[p2]
    w = np.stack([rng.permutation(7) for _ in range(nq)]).astype(f32) / 8          # ranks of partitions 0 .. 6; 7 below them all
    w = np.concatenate([w, np.full((nq, 1), -1, f32)], axis=1)
    w[:, 0] = 0.9                                                                  # partition 0: every query probes it
    w[0, 7] = 1.0                                                                  # partition 7: query 0 alone, and first
    w[1:13, 1] = 1.0
    q = (A * w @ (cent / A) + rng.standard_normal((nq, d))).astype(f32)
    q[1:13] = (x[p1] - cent[1] + A * w[1:13] @ (cent / A) + 0.01 * rng.standard_normal((12, d))).astype(f32)
    x, q, cent = x * f32(scale), q * f32(scale), cent * f32(scale)
    if odd:
        x[20], x[21], x[22, 1] = 0.0, np.nan, np.inf
        if metric == "cosine":
            q[5] = 0.0
    if metric == "cosine":
        cent = np.ascontiguousarray(np.asarray(oracle.normalize(cent)).astype(f32))
    if not odd:
        assert tuple(V.partition_sizes(oracle, x, cent, metric)) == sizes
    rid = {None: None, "permuted": S.permuted_ids(len(x), 3), "small_offsets": F.small_offset_addresses(len(x), 3)}[ids]
    e = eng()
    ct = to_device(cent)
    part, xs = _transform_rows(e, "IVF_FLAT", metric, to_device(np.ascontiguousarray(x)), ct)
    return IvfFlatIndex(DeviceFlatIndex.create(e, metric, ct, xs, part, rid), None, None, None), x, q, cent, rid


def eng():
    import lance_amd
    return lance_amd.default_engine()


def check(metric, d, k=10, prefilter=None, **kw):
    """the batch through nearest() with the stage counters on -> (filter launches, queries the exact kernel replayed)"""
    import oracle
    ix, x, q, cent, rid = build(metric, d, **kw)
    e = eng()
    assert e.ivfflat_plan(len(q), NPROBES, NLIST, d, "float32", metric) == 1
    e.timing(True)
    try:
        before = e.timing_query("count:ivfflat_mc")[1]
        gi, gd = ix.nearest(q, k, NPROBES, prefilter=prefilter)
        ran, replayed = e.timing_query("count:ivfflat_mc")[1] - before, e.search_stats()
    finally:
        e.timing(False)
    oi, od = V.search(oracle, x, cent, q, k, NPROBES, metric, None, None, row_ids=rid, prefilter=prefilter)
    assert ran > 0, "the batch did not take the matrix-core main pass"
    assert gi.dtype == np.uint64 and (gi == oi).all(), (metric, d, k, np.argwhere(gi != oi)[:4])
    assert gd.shape == od.shape and (np.ascontiguousarray(gd).view(np.uint32) == np.ascontiguousarray(od).view(np.uint32)).all(), (metric, d, k)
    return ran, replayed


@pytest.mark.parametrize("d", [36, 200, 1536])                  # less than one stage with a tail; stages plus a tail; whole stages
@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_route_and_bits(metric, d):
    check(metric, d)


@pytest.mark.parametrize("args, want", [
    ((10000, 10, 256, 768, "float32", "l2", False, False), 1),      # the measured shape: 390 pairs per partition
    ((G * 256 // 8, 8, 256, 768, "float32", "l2", False, False), 1), ((G * 256 // 8 - 1, 8, 256, 768, "float32", "l2", False, False), 0),
    ((10000, 10, 256, 128, "float32", "l2", False, False), 0),      # the fixed-dimension kernel's shape stays there
    ((10000, 10, 256, 128, "float32", "cosine", False, False), 1),
    ((10000, 10, 256, 768, "float16", "l2", False, False), 0),
    ((10000, 10, 256, 768, "float32", "l2", True, False), 0),       # a distance range
    ((10000, 10, 256, 768, "float32", "l2", False, True), 0),       # LANCE_HIP_NO_FLAT_MC
    ((10000, 10, 256, 770, "float32", "dot", False, False), 0),     # d % 4
    ((10000, 10, 256, 4096, "float32", "dot", False, False), 1), ((10000, 10, 256, 4100, "float32", "dot", False, False), 0),
    ((2 ** 31, 4, 65536, 768, "float32", "l2", False, False), 1),   # 2^33 pairs: 0 in 32 bits
])
def test_plan(args, want):
    assert eng().ivfflat_plan(*args) == want


@pytest.mark.parametrize("ids", ["permuted", "small_offsets"])  # ids that index the mask; fragment << 32 | offset (only fragment 0's do)
def test_prefilter_and_row_ids(ids):
    n = sum(SIZES)
    mask = np.random.default_rng(8).random(n) < 0.3
    check("l2", 200, ids=ids, prefilter=F.mask_by_id(mask, build("l2", 200, ids=ids)[4]) if ids == "permuted" else mask)


@pytest.mark.parametrize("k", [1, 100])
def test_k_and_queue_overflow(k):
    """3,000 identical rows in the partition every query probes: more rows tie with a bound than a queue holds"""
    _, replayed = check("cosine", 200, k=k, mass=3000)
    assert replayed > 0


@pytest.mark.parametrize("scale", [1e-3, 1e4])
@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_magnitude_and_degenerate_rows(metric, scale):
    check(metric, 36, scale=scale, odd=True)


def test_chunk_crossing():
    ran, _ = check("l2", 36, nq=QCHUNK + 1)
    assert ran >= 2
