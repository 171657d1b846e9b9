"""8-bit scalar quantisation and IVF_SQ on the GPU (lance_amd/csrc/sq.hip) against tests/sq_spec.py, bit for bit: bounds (by value),
codes, distances, and searches -- ids and distance bits.  The fixtures and what they exercise are checked on the CPU by
tests/test_sq_spec.py.  Sorted last: newest device code last."""
import ctypes as C
import functools

import numpy as np
import pytest

import sq_spec as S

pytestmark = pytest.mark.gpu
f32 = np.float32
DIMS = (1, 3, 4, 5, 16, 127, 128, 1024)
KIND = {"f32": np.float32, "f16": np.float16}


def eng():
    import lance_amd
    return lance_amd.default_engine()


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


# ---- bounds and encode ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("d", DIMS)
def test_encode_and_bounds(d, n, kind):
    x, (start, end) = S.encode_fixture(n, d, kind, seed=d * 7 + n)
    e = eng()
    assert (e.sq_encode(x, (start, end)).cpu().numpy() == S.encode(x, start, end)).all()
    assert e.sq_bounds(x) == S.bounds(x)                                   # compared by value: -0.0 == 0.0
    fin = np.where(np.isfinite(x.astype(np.float64)), x, x.dtype.type(0.25))          # finite bounds, as a training sample has
    b = e.sq_bounds(fin)
    assert b == S.bounds(fin)
    assert (e.sq_encode(x, b).cpu().numpy() == S.encode(x, *b)).all()      # bounds that are no round numbers
    half = max(1, n // 2)
    assert e.sq_bounds(fin[half:], e.sq_bounds(fin[:half])) == b           # folded in two calls == folded in one
    assert (e.sq_encode(x, (0.5, 0.5)).cpu().numpy() == 0).all()           # start == end


def test_bounds_of_nothing_but_nan_stay_fresh():
    e = eng()
    assert e.sq_bounds(np.full((3, 5), np.nan, f32)) == S.FRESH_BOUNDS
    assert e.sq_bounds(np.array([[2.0, np.nan]], np.float16), (1.0, 1.5)) == (1.0, 2.0)


def test_encode_saturates_outside_sampled_bounds():
    x, b = S.saturation_fixture()
    codes = eng().sq_encode(x, b).cpu().numpy()
    assert (codes == S.encode(x, *b)).all() and codes[100, 3] == 0 and codes[200, 5] == 255


# ---- distances ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
@pytest.mark.parametrize("d", DIMS)
def test_distances(d, metric, kind):
    rng = np.random.default_rng(d + 1)
    n, nq = 257, 3
    codes = rng.integers(0, 256, (n, d)).astype(np.uint8)
    codes[0] = 255; codes[1] = 0; codes[2, ::2] = 255                      # rows at the extreme codes
    q, b = S.encode_fixture(nq, d, kind, seed=d + 2)
    q[0] = b[0]; q[1] = b[1]                                              # queries encoding to all 0 and all 255
    got = eng().sq_distance(codes, q, b, metric).cpu().numpy()
    assert same_bits(got, S.distances(codes, q, metric, *b))


def test_distances_round_large_sums_to_one_float():
    x, q, b = S.large_sum_fixture()
    e = eng()
    codes = e.sq_encode(x, b)
    for metric in ("l2", "cosine", "dot"):
        got = e.sq_distance(codes, q if metric != "dot" else x[:1], b, metric).cpu().numpy()
        want = S.distances(codes.cpu().numpy(), q if metric != "dot" else x[:1], metric, *b)
        assert same_bits(got, want), metric
    l2 = e.sq_distance(codes, q, b, "l2").cpu().numpy()[0]
    assert l2[0].view(np.uint32) == l2[1].view(np.uint32) and l2[2] > l2[0]


def test_distances_at_the_largest_dimension_and_beyond():
    import lance_amd
    d = lance_amd._lib.SQ_MAX_DIM
    assert d == 16384
    codes = np.zeros((3, d), np.uint8); codes[0] = 255; codes[2, :5] = 1
    b = (0.0, 255.0)
    q = np.zeros((2, d), f32); q[1] = 255.0
    e = eng()
    for metric in ("l2", "dot"):
        assert same_bits(e.sq_distance(codes, q, b, metric).cpu().numpy(), S.distances(codes, q, metric, *b)), metric
    assert e.sq_distance(codes, q, b, "l2").cpu().numpy()[0, 0] == (f32(d * 65025) * f32(65025)) / f32(65025)
    with pytest.raises(lance_amd.LanceHipError) as ei:
        e.sq_distance(np.zeros((2, d + 1), np.uint8), np.zeros((1, d + 1), f32), b)
    assert ei.value.code == lance_amd._lib.EINVAL
    with pytest.raises(lance_amd.LanceHipError):
        e.sq_encode(np.zeros((2, d + 1), f32), b)


# ---- search ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def built(n, d, nlist, metric, kind, seed=0):
    """(device index, what the spec needs) for a Gaussian column; bounds come from a 64-row sample, so rows saturate"""
    import oracle
    from lance_amd.engine import DeviceSqIndex
    x, _ = S.gaussian(n, d, 1, seed=100 + seed + n + d, kind=kind)
    cent = S.centroids_with_gaps(oracle.normalize(x) if metric == "cosine" else x, nlist, seed=seed + 1)
    xs, part = S.prepare_rows(oracle, x, cent, metric)
    b = S.bounds(xs[:64])
    codes = S.encode(xs, *b)
    rid = S.permuted_ids(n, seed + 2)
    ix = DeviceSqIndex.create(eng(), metric, cent, eng().sq_encode(xs, b), part, b, row_ids=rid)
    return ix, (codes, part, cent, b, rid)


def check_search(ix, spec, q, k, nprobes, metric, prefilter=None):
    import oracle
    codes, part, cent, b, rid = spec
    gi, gd = ix.search(q, k, nprobes, allow=prefilter)
    gi = gi.cpu().numpy().view(np.uint64); gd = gd.cpu().numpy()
    oi, od = S.search(oracle, codes, part, cent, q, k, nprobes, metric, *b, row_ids=rid, prefilter=prefilter)
    assert (gi == oi).all(), (k, nprobes, np.argwhere(gi != oi)[:4])
    assert same_bits(gd, od), (k, nprobes)
    return eng().search_stats()


SEARCH_CASES = [
    # n, d, nlist, metric, kind, k, nprobes, nq
    (300, 32, 1, "l2", "f32", 10, 1, 33),
    (300, 32, 1, "dot", "f16", 128, 1, 1),
    (300, 20, 4, "l2", "f32", 1, 3, 257),
    (300, 20, 4, "cosine", "f32", 128, 4, 33),       # partitions with fewer than k rows
    (300, 20, 4, "dot", "f32", 10, 1, 33),
    (300, 32, 16, "l2", "f16", 128, 16, 33),         # every partition below k rows, one empty
    (300, 32, 16, "cosine", "f16", 10, 3, 257),
    (3000, 32, 1, "cosine", "f32", 128, 1, 33),
    (3000, 32, 4, "l2", "f32", 128, 4, 257),
    (3000, 20, 4, "dot", "f16", 10, 3, 33),
    (3000, 32, 16, "l2", "f32", 10, 16, 257),
    (3000, 32, 16, "dot", "f32", 1, 3, 33),
    (3000, 20, 16, "cosine", "f16", 10, 1, 1),
    (3000, 20, 16, "l2", "f16", 128, 3, 33),
]


@pytest.mark.parametrize("n,d,nlist,metric,kind,k,nprobes,nq", SEARCH_CASES)
def test_search(n, d, nlist, metric, kind, k, nprobes, nq):
    ix, spec = built(n, d, nlist, metric, kind)
    _, q = S.gaussian(n, d, nq, seed=100 + n + d, kind=kind)
    check_search(ix, spec, q, k, nprobes, metric)


def test_search_fixture_has_an_empty_and_a_short_partition():
    import oracle
    _, (_, part, cent, _, _) = built(300, 32, 16, "l2", "f16")
    sizes = np.diff(oracle.partition_layout(part, 16)[0].astype(np.int64))
    assert (sizes == 0).any() and ((sizes > 0) & (sizes < 128)).any()


@pytest.mark.parametrize("metric,kind", [("l2", "f32"), ("dot", "f16"), ("cosine", "f32")])
def test_search_prefiltered(metric, kind):
    n, d, nlist, k = 3000, 32, 4, 10
    ix, spec = built(n, d, nlist, metric, kind)
    rid = spec[4]
    _, q = S.gaussian(n, d, 33, seed=100 + n + d, kind=kind)
    rng = np.random.default_rng(8)
    size = int(rid.max()) + 1
    none = np.zeros(size, bool)
    few = none.copy(); few[rid[rng.choice(n, k - 3, replace=False)]] = True           # fewer than k rows selected
    half = none.copy(); half[rid[rng.random(n) < 0.5]] = True
    short = half[: size // 2]                                                          # a mask shorter than the largest row id
    for allow in (none, few, half, short):
        check_search(ix, spec, q, k, nlist, metric, prefilter=allow)
    check_search(ix, spec, q, k, 2, metric, prefilter=half)


# ---- ties -----------------------------------------------------------------------------------------------------------------------
def test_ties_on_a_grid_are_replayed_through_the_heap():
    import oracle
    from lance_amd.engine import DeviceSqIndex
    x, q, rid = S.tie_fixture()
    cent = S.centroids_with_gaps(x, 4, seed=3)
    xs, part = S.prepare_rows(oracle, x, cent, "l2")
    b = S.bounds(xs)
    ix = DeviceSqIndex.create(eng(), "l2", cent, eng().sq_encode(xs, b), part, b, row_ids=rid)
    spec = (S.encode(xs, *b), part, cent, b, rid)
    for k, nprobes in ((10, 3), (1, 1), (128, 4)):
        replays = check_search(ix, spec, q, k, nprobes, "l2")
        assert replays > 0, (k, nprobes)
    assert check_search(ix, spec, q, 10, 3, "l2", prefilter=np.arange(int(rid.max()) + 1) % 3 != 0) > 0


def test_gaussian_column_is_answered_by_the_fast_path():
    n, d, nq = 3000, 32, 257
    ix, spec = built(n, d, 16, "l2", "f32")
    _, q = S.gaussian(n, d, nq, seed=100 + n + d)
    assert check_search(ix, spec, q, 10, 3, "l2") < nq


def test_constant_column_everything_ties():
    import oracle
    from lance_amd.engine import DeviceSqIndex
    n, d = 700, 8
    x = np.full((n, d), 1.25, f32)
    cent = np.ascontiguousarray(np.stack([x[0], x[0] + 1, x[0] - 1]))
    xs, part = S.prepare_rows(oracle, x, cent, "l2")
    rid = S.permuted_ids(n, 4)
    for b in (S.bounds(xs), (0.0, 2.0)):            # start == end (all codes 0), and a proper range
        ix = DeviceSqIndex.create(eng(), "l2", cent, eng().sq_encode(xs, b), part, b, row_ids=rid)
        spec = (S.encode(xs, *b), part, cent, b, rid)
        gi, gd = ix.search(x[:5], 10, 3)
        assert (gd.cpu().numpy() == 0).all()
        assert check_search(ix, spec, x[:5], 10, 3, "l2") == 5
        check_search(ix, spec, x[:5], 128, 1, "l2")


# ---- surface --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,kind", [("l2", "f32"), ("cosine", "f16"), ("dot", "f32")])
def test_create_index_end_to_end(metric, kind):
    import lance_amd
    import oracle
    n, d, nlist = 3000, 32, 8
    x, q = S.gaussian(n, d, 33, seed=21, kind=kind)
    x[5, 3] = np.nan; x[9, 0] = np.inf                                   # rows without a partition are dropped
    ix = lance_amd.create_index(x, "IVF_SQ", metric=metric, num_partitions=nlist, num_bits=8, sample_rate=4, max_iters=5)
    assert isinstance(ix, lance_amd.IvfSqIndex) and ix.params.num_partitions == nlist and ix.params.metric == metric
    assert {"train_ivf", "train_sq", "transform", "build_partitions"} <= set(ix.stats.seconds)
    cent = ix.centroids
    b = ix.bounds
    xs, part = S.prepare_rows(oracle, x, cent, metric)
    assert (ix.part_ids.cpu().numpy().view(np.uint32) == part).all() and (part[[5, 9]] == S.NONE).all()      # under dot as well
    # the quantiser trained on the sample of sample_rate * 2^8 rows, normalised for cosine, non-finite rows removed
    sample = xs[lance_amd.vector.pq_sample_indices(n, ix.params)]
    assert b == S.bounds(sample[np.isfinite(sample.astype(f32)).all(axis=1)])
    codes = S.encode(xs, *b)
    for k, nprobes in ((10, 3), (128, nlist)):
        gi, gd = ix.nearest(q, k, nprobes)
        oi, od = S.search(oracle, codes, part, cent, q, k, nprobes, metric, *b)
        assert (gi == oi).all() and same_bits(gd, od), (k, nprobes)
    allow = np.random.default_rng(2).random(n) < 0.5
    oi, od = S.search(oracle, codes, part, cent, q, 10, 3, metric, *b, prefilter=allow)
    gi, gd = ix.nearest(q, 10, 3, prefilter=allow)
    assert (gi == oi).all() and same_bits(gd, od)
    gi, gd = ix.prefiltered(allow).nearest(q, 10, 3)
    assert (gi == oi).all() and same_bits(gd, od)


def test_refusals(tmp_path):
    import lance_amd
    x = np.zeros((64, 8), f32)
    with pytest.raises(ValueError, match="num_bits 4 not supported"):
        lance_amd.create_index(x, "IVF_SQ", num_partitions=2, num_bits=4)
    with pytest.raises(NotImplementedError, match="SQ builder: unsupported data type: int8"):
        lance_amd.create_index(x.astype(np.int8), "IVF_SQ", num_partitions=2)
    with pytest.raises(NotImplementedError):
        lance_amd.create_index(x, "IVF_HNSW_SQ", num_partitions=2)
    with pytest.raises(ValueError, match="unsupported data type"):
        eng().sq_bounds(np.zeros((4, 4), np.int8))
    ix, _ = built(300, 32, 4, "l2", "f32", seed=5)
    ivf = lance_amd.vector.IvfSqIndex(ix, None, None, None)
    q = np.zeros((1, 32), f32)
    with pytest.raises(NotImplementedError, match="refine_factor"):
        ivf.nearest(q, 5, 1, refine_factor=2)
    with pytest.raises(NotImplementedError, match="distance_range"):
        ivf.nearest(q, 5, 1, distance_range=(0.0, 1.0))
    with pytest.raises(NotImplementedError, match="index files"):
        ivf.save(tmp_path / "sq")
    with pytest.raises(lance_amd.LanceHipError):
        ix.search(q, 129, 1)                                             # k <= 128
    with pytest.raises(lance_amd.LanceHipError):                         # non-finite bounds cannot index
        lance_amd.engine.DeviceSqIndex.create(eng(), "l2", np.zeros((2, 8), f32), np.zeros((4, 8), np.uint8), np.zeros(4, np.int32), (0.0, np.inf))


def test_other_entry_points_refuse_an_sq_handle(tmp_path):
    import torch
    import lance_amd
    ix, _ = built(300, 32, 4, "l2", "f32", seed=5)
    e = eng()
    q = torch.zeros((2, 32), dtype=torch.float32, device="cuda")
    ids = torch.full((2, 5), -7, dtype=torch.int64, device="cuda")
    dists = torch.zeros((2, 5), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    lib = e.lib
    assert lib.lance_hip_ivfflat_search(e.h, ix.h, p(q), 2, 5, 1, p(ids), p(dists)) == lance_amd._lib.EINVAL
    assert lib.lance_hip_ivfflat_search_filtered(e.h, ix.h, p(q), 2, 5, 1, None, 0, p(ids), p(dists)) == lance_amd._lib.EINVAL
    assert lib.lance_hip_ivfpq_search(e.h, ix.h, p(q), 2, 5, 1, 0, p(ids), p(dists)) == lance_amd._lib.EINVAL
    assert lib.lance_hip_ivfpq_search_async(e.h, ix.h, p(q), 2, 5, 1, 0, p(ids), p(dists)) == lance_amd._lib.EINVAL
    assert lib.lance_hip_ivfpq_search_filtered(e.h, ix.h, p(q), 2, 5, 1, 0, None, 0, p(ids), p(dists)) == lance_amd._lib.EINVAL
    assert lib.lance_hip_index_save(e.h, ix.h, str(tmp_path / "sq").encode(), 0, 0.0) == lance_amd._lib.EINVAL
    assert (ids.cpu().numpy() == -7).all(), "a refused call writes nothing"
    # and the SQ entry refuses the other kinds
    x, _ = S.gaussian(300, 32, 1, seed=1)
    fx = lance_amd.create_index(x, "IVF_FLAT", num_partitions=2, max_iters=2)
    assert lib.lance_hip_ivfsq_search(e.h, fx._ix.h, p(q), 2, 5, 1, p(ids), p(dists)) == lance_amd._lib.EINVAL
