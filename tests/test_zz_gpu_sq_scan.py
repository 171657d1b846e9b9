"""IVF_SQ search on the GPU (lance_amd/csrc/sq.hip, pair_cand.cuh) where tests/test_zz_gpu_sq.py stops, against tests/sq_spec.py bit for
bit -- ids and distance bits, no tolerances:
  * every row length class of the search from d = 1 to 16384 (ld = d rounded up to 16: rows and the encoded query zero-padded; the
    query is 16 KiB of the scan's and the replay's LDS at the largest), Gaussian rows, an empty partition, L2 / dot / cosine, f16
    columns, permuted ids under a half mask and Lance row addresses without one, a query that is a centroid and one that is a row;
  * integer sums past 2^24 (sq_spec.large_sum_partition; its conditions are checked on the CPU by tests/test_sq_spec.py): distinct
    u32 sums are one f32 and one key, the heap decides which rows a partition keeps, and every cut tie must be replayed.  A kernel
    that keys on the integer sum, or on f32(sum) before the multiply and divide, or sorts by (dist, rowid) answers with other ids;
  * the same partitions and refine_spec.ordered_partition at d = 1536 through the wide capacity (keff = 129 and 768) with the raw rows
    attached, the candidates compared through k = keff and the refined answer through refine_spec.refine;
  * create_index end to end at d = 768 (f16, cosine) and d = 1536 (f32, dot), and one batch split at d = 1536.
Dynamic LDS of the launches here, by the library's sizing functions: scan ld + 8 cap + 16 <= 16384 + 32768 + 16 = 49,168 bytes (d = 16384,
wide); replay ld + cand_replay_bytes(768) = 32,048; merge 32,784; refine 16 P + 4 d = 81,920 (d = 16384, keff = 768) of the 160 KiB a
workgroup may ask for.

Wall time on an MI355X: 117 tests in 21.7 s -- the first test 2.1 s (it starts the engine), the d = 16384 cases 0.6 - 1.0 s each (the numpy
specification), every other test under 0.6 s."""
import functools

import numpy as np
import pytest

import refine_spec as F
import sq_spec as S
from test_zz_gpu_refine_sqrq import candidates, check_refined, sq_cap, sq_index
from test_zz_gpu_sq import built, check_search, eng, same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
KIND = {"f32": np.float32, "f16": np.float16}


def half_mask(rid, seed):
    half = np.zeros(int(rid.max()) + 1, bool)
    half[rid[np.random.default_rng(seed).random(len(rid)) < 0.5]] = True
    return half


def kth_is_tied(keys, k):
    s = np.sort(keys)
    return len(s) > k and s[k - 1] == s[k]


def flat_spec(spec):
    """sq_index's description of an index as check_search takes it"""
    _, _, (codes, part, cent, b), rid, _ = spec
    return codes, part, cent, b, rid


# ---- dimensions in search ---------------------------------------------------------------------------------------------------------------
DIMS = (1, 3, 15, 16, 17, 31, 48, 100, 128, 129, 255, 256, 272, 768, 1536, 4096, 4100, 16368, 16384)
F16_DIMS = (17, 768, 16384)
DIM_CASES = [(d, metric, "f32") for d in DIMS for metric in ("l2", "dot", "cosine")] + [(d, metric, "f16") for d in F16_DIMS for metric in ("l2", "dot", "cosine")]
NLIST = 4


def dim_rows(d):
    return 600 if d <= 4096 else 300


def dim_queries(d):
    """33; 9 past d = 4100, where the numpy specification of 33 queries takes seconds per case"""
    return 33 if d <= 4100 else 9


def dim_setup(d, metric, kind):
    """the index of test_zz_gpu_sq.built (permuted ids), a second one over the same rows, centroids and bounds under Lance row addresses,
    and dim_queries(d) queries: q[0] is a centroid, q[1] a stored row"""
    import rowid_fixtures
    n = dim_rows(d)
    ix, spec = built(n, d, NLIST, metric, kind)
    x, q = S.gaussian(n, d, dim_queries(d), seed=100 + n + d, kind=kind)          # the rows built() drew
    cent = spec[2]
    q[0] = cent[0]
    q[1] = x[7]
    addr = rowid_fixtures.row_addresses(n, d)
    ix2, spec2 = sq_index(x, cent, metric, addr, bounds=spec[3], raw=np.zeros((1, d), KIND[kind]))
    assert (spec2[2][0] == spec[0]).all() and (spec2[2][1] == spec[1]).all()
    return ix, spec, ix2, flat_spec(spec2), np.ascontiguousarray(q)


@pytest.mark.parametrize("d,metric,kind", DIM_CASES)
def test_search_dimensions(d, metric, kind):
    import oracle
    ix, spec, ix2, spec2, q = dim_setup(d, metric, kind)
    sizes = np.diff(oracle.partition_layout(spec[1], NLIST)[0].astype(np.int64))
    assert (sizes == 0).any() or metric == "dot"                 # (under dot the far centroid attracts rows instead)
    assert spec2[4].min() >= 2 ** 31 and spec2[4].max() >= 2 ** 32
    half = half_mask(spec[4], d)
    for nprobes in (1, NLIST):
        for k in (1, 10, 128):
            check_search(ix, spec, q, k, nprobes, metric, prefilter=half)
            check_search(ix2, spec2, q, k, nprobes, metric)
    if d <= 256:
        _, many = S.gaussian(dim_rows(d), d, 257, seed=100 + dim_rows(d) + d, kind=kind)
        check_search(ix, spec, many, 10, NLIST, metric)
        check_search(ix2, spec2, many, 128, 1, metric)


# ---- integer sums past 2^24 -------------------------------------------------------------------------------------------------------------
LARGE = [(d, n, metric) for d, n in S.LARGE_SUM_DIMS for metric in ("l2", "dot")]
WIDE_KEFF = dict(S.LARGE_SUM_WIDE)


@functools.lru_cache(maxsize=None)
def large_setup(d, n, metric):
    """the two-partition index of sq_spec.large_sum_partition; the raw rows are attached where the wide capacity is searched"""
    f = S.large_sum_cached(d, metric, n)
    raw = None if d in WIDE_KEFF else np.zeros((1, d), f32)
    ix, spec = sq_index(f["x"], f["cent"], metric, f["rid"], bounds=f["bounds"], raw=raw)
    assert (spec[2][0] == f["codes"]).all() and (spec[2][1][:n] == 0).all() and (spec[2][1][n:] == 1).all()
    return ix, spec, f


def design_query_is_replayed(f, metric, k, nprobes, allow, spec):
    """the rule of test_zz_gpu_rq_scan.test_threshold_and_ties: the design query's nearest partition cut a tie at its k-th key, so the
    query is replayed unless the other partition pushed that key out of the merged answer"""
    import oracle
    rid, n = f["rid"], f["n"]
    _, keys = S.large_sum_keys(f, metric)
    if allow is not None:
        keys = keys[allow[rid[:n]]]
    if not kth_is_tied(keys, k):
        return False
    if nprobes == 1:
        return True
    codes, part, cent, b, _ = spec
    _, od = S.search(oracle, codes, part, cent, f["q"][:1], k, nprobes, metric, *b, row_ids=rid, prefilter=allow)
    return S.order_key(od[0, k - 1:k])[0] >= np.sort(keys)[k - 1]


@pytest.mark.parametrize("mask", ["none", "all", "half"])
@pytest.mark.parametrize("d,n,metric", LARGE)
def test_large_sums(d, n, metric, mask):
    ix, spec, f = large_setup(d, n, metric)
    spec = flat_spec(spec)
    rid, q = f["rid"], f["q"]
    allow = None if mask == "none" else (np.ones(int(rid.max()) + 1, bool) if mask == "all" else half_mask(rid, 8))
    _, keys = S.large_sum_keys(f, metric)
    for k in S.LARGE_SUM_KS:
        if mask != "half":
            assert kth_is_tied(keys, k)                          # (what tests/test_sq_spec.py proved of the fixture)
        for nprobes in (1, 2):
            replays = check_search(ix, spec, q[:1], k, nprobes, metric, prefilter=allow)      # the design query alone: the count is its own
            if design_query_is_replayed(f, metric, k, nprobes, allow, spec):
                assert replays == 1, (k, nprobes)
            check_search(ix, spec, q[1:], k, nprobes, metric, prefilter=allow)


@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("d,keff", [(d, keff) for d in WIDE_KEFF for keff in (129, 768)])
def test_large_sums_through_the_wide_capacity(d, keff, metric):
    """keff = 129 and 768 candidates by the SQ distance -- compared through k = keff, refine_factor = 1: the refined ids are the
    candidates' -- and the answer re-ranked against the raw rows; scan, merge and replay run at the wide capacity (the kernel timers).
    300 rows at d = 16384 leave nothing to cut at keff = 768: there the query is 16 KiB of the largest scan and 64 KiB of the refine's LDS."""
    assert sq_cap(d) == 4096
    n = dict(S.LARGE_SUM_DIMS)[d]
    ix, spec, f = large_setup(d, n, metric)
    q = f["q"]
    e = eng()
    names = ["ivfsq_scan", "ivfsq_wide_scan", "ivfsq_wide_merge", "ivfsq_wide_exact", "refine"]
    for nprobes in (1, 2):
        cand = candidates(spec, q, keff, nprobes)
        e.timing(True)
        try:
            for name in names:
                e.timing_query(name)                             # (a query returns a timer's launches and resets it)
            oi = check_refined(ix, spec, q, keff, 1, nprobes, cand)
            ran = [e.timing_query(name)[1] for name in names]
        finally:
            e.timing(False)
        assert ran == [0, 1, 1, 1, 1]
        assert (np.sort(oi, axis=1) == np.sort(cand, axis=1)).all()
        check_refined(ix, spec, q[:1], keff, 1, nprobes, cand[:1])
        replayed = design_query_is_replayed(f, metric, keff, nprobes, None, flat_spec(spec))
        assert nprobes == 2 or replayed == (keff in WIDE_KEFF[d])
        if replayed:
            assert e.search_stats() == 1, nprobes
    check_refined(ix, spec, q, keff // 3, 3, 2, candidates(spec, q, keff // 3 * 3, 2))
    half = half_mask(f["rid"], 8)
    check_refined(ix, spec, q, 10, keff // 10, 2, candidates(spec, q, keff // 10 * 10, 2, allow=half), allow=half)


# ---- wide capacity at long rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,keff", [("descending", 129), ("descending", 768), ("tie_cut", 129), ("tie_cut", 768)])
def test_ordered_partitions_at_long_rows(order, keff):
    """test_zz_gpu_refine_sqrq.test_ordered_partitions at d = 1536: one partition longer than the scan's buffer plus two chunks, stored
    in an order chosen for the design query; the buffer holds 4096 entries at every d the engine accepts"""
    import oracle
    d = 1536
    assert [sq_cap(x) for x in (1, 64, d, 16368, 16384)] == [4096] * 5
    cap = sq_cap(d)
    n = (cap + 2 * F.CHUNK) // 32 * 32 + 32 + 1
    metric = "l2" if keff == 768 else "dot"
    f = F.ordered_partition(oracle, "sq", order, metric, keff, cap, n, d=d)
    q = np.ascontiguousarray(np.stack([f["q"], f["x"][5] + f32(0.1)]))
    rid = np.random.default_rng(3).permutation(len(f["x"])).astype(np.uint64)
    ix, spec = sq_index(f["x"], f["cent"], metric, rid, bounds=f["bounds"])
    cand = candidates(spec, q, keff, 2)
    oi = check_refined(ix, spec, q, keff, 1, 2, cand)
    replays = eng().search_stats()
    assert (np.sort(oi, axis=1) == np.sort(cand, axis=1)).all()
    assert replays >= 1 or not f["cut_tie"]
    assert f["cut_tie"] or order != "tie_cut"
    check_refined(ix, spec, q, keff // 3, 3, 2, candidates(spec, q, keff // 3 * 3, 2))


# ---- end to end -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,metric,kind", [(768, "cosine", "f16"), (1536, "dot", "f32")])
def test_create_index_end_to_end_at_long_rows(d, metric, kind):
    import lance_amd
    import oracle
    n, nlist = 2000, 8
    x, q = S.gaussian(n, d, 17, seed=23, kind=kind)
    x[5, 3] = np.nan; x[9, 0] = np.inf                                   # rows without a partition are dropped
    ix = lance_amd.create_index(x, "IVF_SQ", metric=metric, num_partitions=nlist, num_bits=8, sample_rate=4, max_iters=5, keep_raw=True)
    cent, b = ix.centroids, ix.bounds
    xs, part = S.prepare_rows(oracle, x, cent, metric)
    assert (ix.part_ids.cpu().numpy().view(np.uint32) == part).all() and (part[[5, 9]] == S.NONE).all()
    sample = xs[lance_amd.vector.pq_sample_indices(n, ix.params)]
    assert b == S.bounds(sample[np.isfinite(sample.astype(f32)).all(axis=1)])
    codes = S.encode(xs, *b)
    allow = np.random.default_rng(2).random(n) < 0.5
    for k, nprobes, mask in ((10, 3, None), (128, nlist, None), (10, 3, allow)):
        gi, gd = ix.nearest(q, k, nprobes, prefilter=mask)
        oi, od = S.search(oracle, codes, part, cent, q, k, nprobes, metric, *b, prefilter=mask)
        assert (gi == oi).all() and same_bits(gd, od), (k, nprobes)
    gi, gd = ix.prefiltered(allow).nearest(q, 10, 3)
    assert (gi == oi).all() and same_bits(gd, od)
    for k, rf, nprobes, mask in ((10, 5, 3, None), (10, 60, nlist, None), (10, 20, 3, allow)):
        gi, gd = ix.nearest(q, k, nprobes, refine_factor=rf, prefilter=mask)
        oi, od = F.sq_search_refine(oracle, codes, part, cent, q, k, rf, nprobes, metric, *b, raw=x, prefilter=mask)
        assert (gi == oi).all() and same_bits(gd, od), (k, rf, nprobes)


# ---- batch split --------------------------------------------------------------------------------------------------------------------------
def test_batch_split_at_long_rows():
    """k = 128 and 8 probes: 2^24 / (8 * 128) = 16384 queries per launch, so 16400 queries take two; the queries on both sides of the
    split are compared with the specification (64 distinct queries, repeated)"""
    import oracle
    d, n, nq = 1536, 2000, 16400
    x, q64 = S.gaussian(n, d, 64, seed=12)
    q = np.ascontiguousarray(np.tile(q64, (nq // 64 + 1, 1))[:nq])
    rid = np.random.default_rng(8).permutation(n).astype(np.uint64)
    cent = np.ascontiguousarray(x[np.random.default_rng(9).choice(n, 8, replace=False)])
    ix, spec = sq_index(x, cent, "l2", rid, raw=np.zeros((1, d), f32))
    gi, gd = ix.search(q, 128, 8)
    gi = gi.cpu().numpy().view(np.uint64); gd = gd.cpu().numpy()
    codes, part, cent, b, rid = flat_spec(spec)
    for lo, hi in ((0, 16), (16376, 16400)):
        oi, od = S.search(oracle, codes, part, cent, q[lo:hi], 128, 8, "l2", *b, row_ids=rid)
        assert (gi[lo:hi] == oi).all() and same_bits(gd[lo:hi], od), lo
