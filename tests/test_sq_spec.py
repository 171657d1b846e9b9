"""CPU checks of tests/sq_spec.py, the specification the GPU tests of IVF_SQ (tests/test_zz_gpu_sq.py, tests/test_zz_gpu_sq_scan.py) compare with bit for bit:
the reference's own recorded answers (lance-index sq.rs tests: test_f16_sq8 / test_f32_sq8 / test_f64_sq8 / test_scale_to_u8_with_nan),
the arithmetic rules of the specification, and the conditions the shared fixtures must meet to exercise what the GPU tests claim."""
import numpy as np
import pytest

import sq_spec as S

f32, f64 = np.float32, np.float64


# ---- the reference's recorded answers -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dt", [np.float16, np.float32, np.float64])
def test_codes_of_0_to_15_are_multiples_of_17(dt):
    v = np.arange(16).astype(dt).reshape(1, 16)
    start, end = S.bounds(v)
    assert (start, end) == (0.0, 15.0)
    assert S.encode(v, start, end).ravel().tolist() == [i * 17 for i in range(16)]


def test_nan_encodes_to_zero():
    v = np.array([0.0, 1.0, 2.0, 3.0, np.nan])
    assert S.encode(v, 0.0, 3.0).tolist() == [0, 85, 170, 255, 0]


# ---- bounds ---------------------------------------------------------------------------------------------------------------------
def test_bounds_start_fresh_skip_nan_and_fold():
    assert S.FRESH_BOUNDS == (np.finfo(f64).max, -np.finfo(f64).max)
    assert S.bounds(np.array([np.nan, np.nan], f32)) == S.FRESH_BOUNDS             # nothing folded
    x = np.array([[3.0, np.nan, -2.5], [7.25, 0.0, np.nan]], f32)
    assert S.bounds(x) == (-2.5, 7.25)
    assert S.bounds(x[1:], *S.bounds(x[:1])) == S.bounds(x)                         # retrain: the same fold
    assert S.bounds(np.array([np.inf, -np.inf, 1.0], np.float16)) == (-np.inf, np.inf)
    h = np.array([0.1], np.float16)                                                 # widened exactly, not re-rounded
    assert S.bounds(h) == (float(h[0]), float(h[0]))


# ---- encode ---------------------------------------------------------------------------------------------------------------------
def test_encode_truncates_saturates_and_degenerates():
    start, end = -1.5, 2.25
    v = np.array([start, end, start - 1e-3, end + 1e-3, -1e30, 1e30, np.inf, -np.inf, np.nan, -0.0], f32)
    assert S.encode(v, start, end).tolist() == [0, 255, 0, 255, 0, 255, 255, 0, 0, 102]
    # truncation toward zero, not rounding: 254.99.. stays 254, and t in (-1, 0) becomes 0
    assert S.encode(np.array([254.999, 0.999, -0.999]), 0.0, 255.0).tolist() == [254, 0, 0]
    assert (S.encode(np.array([1.0, np.nan, 5.0], f32), 2.0, 2.0) == 0).all()       # start == end
    # the three f64 operations in order: (v - start) * 255 / range, the divide last
    v, s, e = f64(0.7), f64(0.1), f64(0.9)
    assert int(S.encode(np.array([v]), s, e)[0]) == int((v - s) * f64(255.0) / (e - s))


def test_saturation_fixture_saturates_at_both_ends():
    x, (start, end) = S.saturation_fixture()
    codes = S.encode(x, start, end)
    below, above = x < start, x > end
    assert below.any() and above.any(), "the sample's bounds must not cover the column"
    assert (codes[below] == 0).all() and (codes[above] == 255).all()
    assert x[100, 3] < start and x[200, 5] > end


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_encode_fixture_holds_the_special_values(kind):
    x, (start, end) = S.encode_fixture(257, 16, kind, seed=3)
    v = x.astype(f64)
    assert np.isnan(v).any() and np.isposinf(v).any() and np.isneginf(v).any()
    assert (np.signbit(v) & (v == 0)).any(), "-0.0"
    tiny = np.finfo(x.dtype).tiny
    assert ((np.abs(v) < tiny) & (v != 0)).any(), "a subnormal"
    assert (v == start).any() and (v == end).any() and (v < start).any() and (v > end).any()


# ---- distances ------------------------------------------------------------------------------------------------------------------
def test_distance_formula():
    codes = np.array([[0, 255, 10, 3], [7, 7, 7, 7]], np.uint8)
    qc = np.array([255, 0, 12, 3], np.uint8)
    assert S.int_sums(codes, qc, "l2").tolist() == [2 * 65025 + 4, 248 * 248 + 49 + 25 + 16]
    assert S.int_sums(codes, qc, "cosine").tolist() == S.int_sums(codes, qc, "l2").tolist()      # no / 2 for cosine, unlike PQ
    assert S.int_sums(codes, qc, "dot").tolist() == [120 + 9, 7 * 270]
    start, end = -1.0, 2.0
    r2 = f32(3.0) * f32(3.0)
    assert S.scale(np.array([130054], np.uint32), "l2", start, end)[0] == (f32(130054) * r2) / f32(65025)
    assert S.scale(np.array([129], np.uint32), "dot", start, end)[0] == ((f32(1) - f32(129)) * r2) / f32(65025)
    assert S.scale(np.array([5], np.uint32), "l2", start, end).dtype == f32


def test_l2_sum_equals_the_norm_form_in_u32():
    """the kernels compute sum(x^2) + sum(q^2) - 2 sum(x q) in wrapping u32 arithmetic: the same integer as the reference's sum of
    squared differences for every d the engine accepts (2 d 255^2 < 2^32 up to d = 33025)"""
    rng = np.random.default_rng(0)
    for d in (1, 5, 1024, 16384):
        x = rng.integers(0, 256, (6, d)).astype(np.uint8)
        x[0] = 255; x[1] = 0
        for y in (rng.integers(0, 256, d).astype(np.uint8), np.zeros(d, np.uint8), np.full(d, 255, np.uint8)):
            xx = (x.astype(np.uint64) ** 2).sum(1); yy = (y.astype(np.uint64) ** 2).sum(); xy = (x.astype(np.uint64) * y).sum(1)
            assert (xx + yy < 2 ** 32).all()
            assert ((xx + yy - 2 * xy).astype(np.uint32) == S.int_sums(x, y, "l2")).all()
    assert 16384 * 65025 < 2 ** 32 and int(S.int_sums(np.full((1, 16384), 255, np.uint8), np.zeros(16384, np.uint8), "l2")[0]) == 16384 * 65025


def test_large_sum_fixture_merges_two_sums_into_one_float():
    x, q, (start, end) = S.large_sum_fixture()
    codes = S.encode(x, start, end)
    assert (codes == x.astype(np.uint8)).all() and (S.encode(q, start, end) == 0).all()      # code = value under 0 .. 255
    sums = S.int_sums(codes, S.encode(q, start, end)[0], "l2")
    assert len(set(sums.tolist())) == 4 and (sums > 2 ** 24).all()
    as_float = sums.astype(f32)
    assert sums[0] != sums[1] and as_float[0] == as_float[1], "two distinct integer sums must round to one f32"
    dist = S.distances(codes, q, "l2", start, end)[0]
    assert dist[0].view(np.uint32) == dist[1].view(np.uint32) and dist[3] > dist[0]


# ---- search ---------------------------------------------------------------------------------------------------------------------
def test_search_spec_on_a_small_index(oracle):
    x, q = S.gaussian(300, 20, 5, seed=1)
    cent = S.centroids_with_gaps(x, 4, seed=2)
    xs, part = S.prepare_rows(oracle, x, cent, "l2")
    offs, _ = oracle.partition_layout(part, 4)
    assert (np.diff(offs.astype(np.int64)) == 0).any(), "the fixture has an empty partition"
    start, end = S.bounds(xs[:64])
    codes = S.encode(xs, start, end)
    rid = S.permuted_ids(300, 9)
    ids, dists = S.search(oracle, codes, part, cent, q, 400, 4, "l2", start, end, row_ids=rid)
    # every partition probed and k above the row count: all rows, by (dist, rowid), the tail padded
    full = S.distances(codes, q, "l2", start, end)
    for qi in range(5):
        order = np.lexsort((rid, full[qi]))
        assert (ids[qi, :300] == rid[order]).all() and (dists[qi, :300] == full[qi][order]).all()
        assert (ids[qi, 300:] == np.iinfo(np.uint64).max).all() and np.isinf(dists[qi, 300:]).all()
    # a prefilter removes rows before the heap sees them
    allow = np.zeros(int(rid.max()) + 1, bool)
    allow[rid[::2]] = True
    fi, _ = S.search(oracle, codes, part, cent, q, 10, 4, "l2", start, end, row_ids=rid, prefilter=allow)
    assert allow[fi.astype(np.int64)].all()
    none_i, none_d = S.search(oracle, codes, part, cent, q, 10, 4, "l2", start, end, row_ids=rid, prefilter=np.zeros(4, bool))
    assert (none_i == np.iinfo(np.uint64).max).all() and np.isinf(none_d).all()


def test_tie_fixture_depends_on_heap_order(oracle):
    x, q, rid = S.tie_fixture()
    cent = S.centroids_with_gaps(x, 4, seed=3)
    xs, part = S.prepare_rows(oracle, x, cent, "l2")
    start, end = S.bounds(xs)
    codes = S.encode(xs, start, end)
    heap_i, _ = S.search(oracle, codes, part, cent, q, 10, 3, "l2", start, end, row_ids=rid)
    sort_i = S.sorted_search(oracle, codes, part, cent, q, 10, 3, "l2", start, end, row_ids=rid)
    differ = (heap_i != sort_i).any(axis=1)
    assert differ.any(), "at least one query's answer must depend on the heap's handling of ties"


# ---- large sums: the conditions tests/test_zz_gpu_sq_scan.py and tests/test_sq_kernels_cpu.py rely on, decided by the reference alone ------
LARGE = [(d, n, metric) for d, n in S.LARGE_SUM_DIMS for metric in ("l2", "dot")]


def kth_is_tied(keys, k):
    s = np.sort(keys)
    return len(s) > k and s[k - 1] == s[k]


@pytest.mark.parametrize("d,n,metric", LARGE)
def test_large_sum_partition_is_what_it_says(oracle, d, n, metric):
    f = S.large_sum_cached(d, metric, n)
    start, end = f["bounds"]
    assert f32(end - start) * f32(end - start) != f32(65025.0), "the scaling must not be a no-op"
    assert f["x"].dtype == f32 and (f["x"] != np.rint(f["x"])).mean() > 0.9, "real values, not the integers of the codes"
    assert (S.encode(f["x"], start, end) == f["codes"]).all() and (S.encode(f["q"], start, end) == f["qcodes"]).all()
    _, part = S.prepare_rows(oracle, f["x"], f["cent"], metric)
    assert (part[:n] == 0).all() and (part[n:] == 1).all() and len(part) == n + S.LARGE_SUM_OTHER
    probes, _ = oracle.find_partitions(f["q"], f["cent"], 2, metric)
    assert (probes[:, 0] == 0).all() and (probes[:, 1] == 1).all()
    rid = f["rid"]
    assert len(np.unique(rid)) == len(rid) and (np.diff(rid[:n].astype(np.int64)) < 0).sum() > n // 4, "row ids are no storage order"
    for qi in (0, 1):
        sums, _ = S.large_sum_keys(f, metric, qi)
        distinct = np.unique(sums)
        assert (np.diff(distinct.astype(np.int64)) == 1).sum() >= 8, "sums in steps of one"
        assert (distinct > 2 ** 24).all() == (d >= 516) and (distinct < 2 ** 24).all() == (d < 516)
    # the second partition's keys fall among the first's: two probes merge lists that interleave
    _, k0 = S.large_sum_keys(f, metric)
    k1 = S.order_key(S.scale(S.int_sums(f["codes"][n:], f["qcodes"][0], metric), metric, start, end))
    assert (k1 <= np.sort(k0)[127]).any() and (k1 >= np.sort(k0)[9]).any()


@pytest.mark.parametrize("d,n,metric", LARGE)
def test_large_sums_share_their_key(d, n, metric):
    """at least a quarter of the distinct sums of the design query end in the key of another sum.  At d = 259 every sum is below 2^24
    and is its own float: there the scaling alone merges them"""
    f = S.large_sum_cached(d, metric, n)
    sums, keys = S.large_sum_keys(f, metric)
    distinct, first = np.unique(sums, return_index=True)
    dk = keys[first]
    shared = np.array([(dk == v).sum() > 1 for v in dk])
    print(f"d={d} {metric}: {len(distinct)} sums, {len(np.unique(distinct.astype(f32)))} floats, {len(np.unique(dk))} keys, {shared.mean():.2f} shared")
    assert shared.mean() >= 0.25
    if d == 259:
        assert len(np.unique(distinct.astype(f32))) == len(distinct) and len(np.unique(dk)) < len(distinct)


@pytest.mark.parametrize("d,n,metric", LARGE)
def test_large_sum_lists_are_cut_with_a_tie(d, n, metric):
    """more rows are tied at the k-th key of the design query's partition than fit, at every k (and keff) the GPU file searches with:
    the cut-tie flag must be set and the query replayed"""
    f = S.large_sum_cached(d, metric, n)
    _, keys = S.large_sum_keys(f, metric)
    for k in S.LARGE_SUM_KS + dict(S.LARGE_SUM_WIDE).get(d, ()):
        assert kth_is_tied(keys, k), k


def mutant_differences(oracle, d, n, metric, k, nprobes=1):
    f = S.large_sum_cached(d, metric, n)
    _, part = S.prepare_rows(oracle, f["x"], f["cent"], metric)
    args = (oracle, f["codes"], part, f["cent"], f["q"][:2], k, nprobes, metric) + f["bounds"]
    ref, _ = S.search(*args, row_ids=f["rid"])
    return {"int_sum": (ref != S.search(*args, row_ids=f["rid"], select=S.int_sum_select)[0]).sum(),
            "unscaled": (ref != S.search(*args, row_ids=f["rid"], select=S.unscaled_select)[0]).sum(),
            "sorted": (ref != S.sorted_search(*args, row_ids=f["rid"])).sum()}


@pytest.mark.parametrize("d,n,metric", LARGE)
def test_large_sum_mutants_answer_differently(oracle, d, n, metric):
    """a selection keyed by the integer sum (from d = 516 on, where sums share a float), one keyed by f32(sum) before the scaling (at
    d = 259, where only the scaling merges), and the (dist, rowid) sort without the heap (everywhere) return other ids than the
    reference at k = 128, one probe"""
    diff = mutant_differences(oracle, d, n, metric, 128)
    print(f"d={d} {metric}: ids that differ at k = 128: {diff}")
    assert diff["sorted"] > 0
    if d >= 516:
        assert diff["int_sum"] > 0
    if d == 259:
        assert diff["unscaled"] > 0 and diff["int_sum"] > 0


def test_large_sum_mutants_differ_at_k_10(oracle):
    """... and at k = 10 from d = 1536 on, two probes (L2)"""
    for d, n in S.LARGE_SUM_DIMS:
        if d >= 1536:
            diff = mutant_differences(oracle, d, n, "l2", 10, 2)
            assert diff["int_sum"] > 0 and diff["sorted"] > 0, (d, diff)
