"""Flat KNN on REAL-VALUED data, and the single-pass kernel's running threshold (lance_amd/csrc/flat_small.hip, flat.hip, wide.hip).

The older flat tests use integer-valued rows, on which every order of additions gives the same bits
(tests/test_flat_order_spec.py::test_integer_fixtures_cannot_see_the_order), so they cannot hold a kernel to the reference's summation
order: 16 lane accumulators folded in lane order, the d % 16 tail summed first.  On the fixtures here (tests/flat_order_spec.py:
standard_normal * 3 in f32, * 0.7 in f16) a kernel that sums sequentially, folds the lanes pairwise or adds the tail last returns
other bits for 30-97 % of the answer (measured by the same spec test).  Everything is compared with the oracle bit for bit, ids as
uint64 and distances as uint32.  No fixture holds two equal rows unless its test says so: an overflow of the single-pass kernel's
lists (which hands the call to the batch path) cannot silently swap the route under test.

The second gap: flat_small_scan_kernel tightens its threshold inside the row loop only once a workgroup's list holds more than
FS_CAP - 128 = 896 entries, which needs slices of more than 1024 rows, i.e. a table of more than 1024 * 4 * CUs rows -- more than any
older test has (and than the benchmark's 1M rows on 256 CUs).  test_single_pass_running_threshold builds slices of 2048 rows and more.

Wall time on an MI355X: 71 tests in 22 s -- the two child-process tests 9.3 s and 4.9 s, every other test under 1 s (the running-threshold cases
0.2-0.8 s each); tests/test_zz_gpu_flat_small.py takes 8.6 s on the same machine."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import flat_order_spec as S

pytestmark = pytest.mark.gpu
f32 = np.float32

# the single-pass kernel answers one or two queries by default; LANCE_HIP_FLAT_SMALL_MAXQ=4 (read once per process) sends three and
# four there too: the child run of test_routes_* sets it and the tests below then ask with three and four queries
NQS = (3, 4) if os.environ.get("LANCE_HIP_FLAT_SMALL_MAXQ") else (1, 2)
IN_CHILD = bool(os.environ.get("LANCE_HIP_FLAT_SMALL_MAXQ") or os.environ.get("LANCE_HIP_NO_FLAT_SMALL"))


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _dev(a):
    import lance_amd.engine as E
    return E.to_device(a)


def _rids(n, seed):
    return np.random.default_rng(seed).permutation(n).astype(np.uint64) * 3 + 5          # ids unrelated to the storage order


def _same(eng, xd, qd, nq, k, metric, oi, od, rid=None, tag=None):
    """one call with the first nq queries; oi / od: the oracle's answer for at least nq queries and at least k neighbours (the
    (distance, row id) order is total, so a shorter answer is a prefix of a longer one)"""
    gi, gd = eng.flat_topk(xd, qd[:nq], k, metric, row_ids=rid)
    assert (gi.cpu().numpy().view(np.uint64) == oi[:nq, :k]).all(), tag
    assert (gd.cpu().numpy().view(np.uint32) == od[:nq, :k].view(np.uint32)).all(), tag


def _oracle_rows(x):
    return x if x.dtype == np.float16 else x.astype(f32)


# ---- B1: the single-pass kernel on real-valued f32 ------------------------------------------------------------------------------
# the tail (3, 17, 20, 100, 136, 200, 2047), no tail (16, 128, 144, 1536, 2048), the 128-element groups the two-query loop loads
# (128: one full group, 136 / 144: a group of one chunk behind it, 2047 / 2048: sixteen), the route's upper bound (2048) and the
# first dimension beyond it (2049: the batch path, which must be right as well)
B1_DIMS = (3, 16, 17, 20, 100, 128, 136, 144, 200, 1536, 2047, 2048, 2049)


@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("d", B1_DIMS)
def test_single_pass_real_f32(eng, oracle, metric, d, ns=(4224, 4097, 4096), ks=(1, 7, 10, 128)):
    """n = 4224: nine slices of 512 rows, the last one 128; 4097: the last slice is one row; 4096: the route's lower bound"""
    x, q = S.real_f32(max(ns), d, max(NQS), 1000 + d)
    qd = _dev(q)
    for n in ns:
        oi, od = oracle.flat_knn(x[:n], q, max(ks), metric)
        xd = _dev(x[:n])
        for nq in NQS:
            for k in ks:
                _same(eng, xd, qd, nq, k, metric, oi, od, tag=(metric, d, n, nq, k))


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_single_pass_real_f32_row_ids(eng, oracle, metric):
    n, d = 4224, 100
    x, q = S.real_f32(n, d, max(NQS), 1999)
    rid = _rids(n, 5)
    oi, od = oracle.flat_knn(x, q, 128, metric, row_ids=rid)
    xd, qd, rd = _dev(x), _dev(q), _dev(rid)
    for nq in NQS:
        for k in (1, 10, 128):
            _same(eng, xd, qd, nq, k, metric, oi, od, rid=rd, tag=(metric, nq, k))


# ---- B2: the other column types ---------------------------------------------------------------------------------------------------
# f16 dot above d = 16 sums in 32 lanes and is sent elsewhere by the dtype / metric gate: d = 40 is checked whichever route answers.
# int8 sums are exact: those cases check the tail's indexing, not the order.
B2_CASES = [("f16", "l2", d) for d in (8, 16, 20, 128, 136)] + [("f16", "dot", d) for d in (8, 16, 40)] + \
           [("int8", m, d) for m in ("l2", "dot") for d in (20, 136)]


@pytest.mark.parametrize("kind,metric,d", B2_CASES)
def test_single_pass_real_f16_and_int8(eng, oracle, kind, metric, d):
    n = 4224
    x, q = (S.real_f16 if kind == "f16" else S.int8_rows)(n, d, max(NQS), 2000 + d)
    oi, od = oracle.flat_knn(_oracle_rows(x), _oracle_rows(q), 128, metric)
    xd, qd = _dev(x), _dev(q)
    for nq in NQS:
        for k in (1, 10, 128):
            _same(eng, xd, qd, nq, k, metric, oi, od, tag=(kind, metric, d, nq, k))


# ---- B3: special values inside the answer ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_special_values_inside_the_answer(eng, oracle, metric):
    """70 finite rows among 4224, k = 128: the answer runs through the rows whose distance is +inf (one +inf element, or every
    element 1e20 so that the squared difference overflows) and into the rows whose distance is NaN (one canonical np.nan element).
    f32::total_cmp puts +inf behind every finite distance and the positive NaN behind +inf, ties by row id.  Under dot one +inf
    element times a query element (none is zero) gives a distance of -inf or +inf, and the 1e20 rows stay finite (twenty EQUAL rows:
    ties by row id).  The fixture holds no NaN that arithmetic GENERATES (inf - inf, 0 * inf): such a NaN's sign belongs to the host
    CPU (x86 produces the negative default NaN, which total_cmp sorts FIRST), not to the reference's arithmetic.  The thousands of
    rows tied at the NaN key overflow the single-pass kernel's lists, so the batch path may be the one that answers; the assertion is
    on the answer.  A plain call follows and must be right too: the overflow flag word is cleared behind the call that raised it."""
    n, d, k = 4224, 24, 128
    x, q = S.real_f32(n, d, 2, 77)
    assert (q != 0).all()
    rng = np.random.default_rng(78)
    p = rng.permutation(n)
    fin, infe, big, nan = p[:70], p[70:90], p[90:110], p[110:]
    x[infe, rng.integers(0, d, infe.size)] = np.inf
    x[big] = f32(1e20)
    x[nan, rng.integers(0, d, nan.size)] = np.nan
    rid = _rids(n, 79)
    oi, od = oracle.flat_knn(x, q, k, metric, row_ids=rid)
    # the test's own expectation, on the oracle's answer: sorted, ties by row id, the NaN rows last and positive
    isn = np.isnan(od)
    for qi in range(2):
        c = int((~isn[qi]).sum())
        assert not isn[qi, :c].any() and isn[qi, c:].all() and 0 < k - c
        assert (od[qi, c:].view(np.uint32) == 0x7FC00000).all()
        step = np.diff(S.keys(od[qi, :c]).astype(np.int64))
        assert (step >= 0).all()
        tie = step == 0
        assert (oi[qi, 1:c][tie] > oi[qi, :c - 1][tie]).all()
        assert (oi[qi, c:] == np.sort(rid[nan])[:k - c]).all()
        if metric == "l2":
            assert c == 110 and np.isfinite(od[qi, :70]).all() and set(oi[qi, :70]) == set(rid[fin])
            assert np.isposinf(od[qi, 70:110]).all() and (oi[qi, 70:110] == np.sort(rid[np.concatenate([infe, big])])).all()
    xd, qd, rd = _dev(x), _dev(q), _dev(rid)
    y, qy = S.real_f32(n, 20, 2, 1020)
    yi, yd = oracle.flat_knn(y, qy, 10, metric)
    yd_, qyd = _dev(y), _dev(qy)
    for nq in (1, 2):
        _same(eng, xd, qd, nq, k, metric, oi, od, rid=rd, tag=("special values", metric, nq))
        _same(eng, yd_, qyd, nq, 10, metric, yi, yd, tag=("plain call after the special values", metric, nq))


# ---- B4: the running threshold --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["random", "farthest-first", "nearest-first"])
@pytest.mark.parametrize("kind,metric,d", [("f32", "l2", 8), ("f32", "dot", 8), ("f16", "l2", 16)])
def test_single_pass_running_threshold(eng, oracle, kind, metric, d, order):
    """n = 2048 * 4 * CUs + 77 rows: every workgroup's slice has at least 2048 rows, so the capacity check inside the row loop fires,
    the threshold T[qi] is refreshed and `key <= T` filters for real.  farthest-first (rows sorted by descending distance to query 0):
    every row passes the stale threshold, the list fills and is tightened every few rounds, and the answer is the table's END;
    nearest-first: the threshold settles in the first slice.  Thirteen rows are copies of the rows at query 0's 1st, 10th and 128th
    distance (the only equal rows), so rows tied exactly at the k-th distance decide the answer by row id.  In the random order three of
    the four rows tied at the 1st distance are moved into ONE slice: one into its first 1024 rows (in the list when the loop first
    tightens: for k = 1 the threshold then IS that row's key) and two behind them, the first of which gets the group's smallest row
    id -- it is the answer for k = 1, and it enters the list only because the filter is `key <= T`, not `key < T`."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 2048 * 4 * cus + 77
    slice_rows = -(-(-(-n // (4 * cus))) // 128) * 128          # flat_topk_small: rows per workgroup, a multiple of the 128 rows of a round
    assert slice_rows == 2176
    x, q = (S.real_f32 if kind == "f32" else S.real_f16)(n, d, max(NQS), 4000 + d)
    rng = np.random.default_rng(41)
    key = S.keys(oracle.distance_batch(metric, q[0], x))
    for kk, copies in ((1, 3), (10, 5), (128, 5)):
        top = np.argpartition(key, kk + 40)[:kk + 40]
        top = top[np.argsort(key[top], kind="stable")]
        src = top[kk - 1]
        far = np.unique(rng.integers(0, n, 64))
        far = far[key[far] > key[top[-1]]][:copies]
        x[far] = x[src]; key[far] = key[src]
        assert (key == key[src]).sum() == copies + 1
    rid = _rids(n, 42)
    if order == "random":
        tied = np.flatnonzero(key == key.min())
        spots = 5 * slice_rows + np.array([100, 1500, 1800])
        for a, b in zip(tied[:3], spots):
            x[[a, b]] = x[[b, a]]; key[[a, b]] = key[[b, a]]
        group = np.flatnonzero(key == key.min())
        assert group.size == 4 and (group[:3] == spots).all()
        low = group[np.argmin(rid[group])]
        rid[[low, spots[1]]] = rid[[spots[1], low]]
    else:
        o = np.argsort(key, kind="stable")
        x = np.ascontiguousarray(x[o[::-1] if order == "farthest-first" else o])
    oi, od = oracle.flat_knn(_oracle_rows(x), _oracle_rows(q), 128, metric, row_ids=rid)
    assert od[0, 0] == od[0, 3] < od[0, 4] and od[0, 8] < od[0, 9] == od[0, 14] < od[0, 15]      # the ties straddle k = 1 and k = 10
    xd, qd, rd = _dev(x), _dev(q), _dev(rid)
    for nq in NQS:
        for k in (1, 10, 128):
            _same(eng, xd, qd, nq, k, metric, oi, od, rid=rd, tag=(kind, metric, order, nq, k))


# ---- B5: the batch path's exact kernels ---------------------------------------------------------------------------------------------
# fixed-dimension kernels: 8, 16, 32, 96; the any-dimension kernel: 20, 100, 200; k = 129 and 200 select the older kernels
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("d", [8, 16, 32, 96, 20, 100, 200])
def test_batch_path_real_f32(eng, oracle, metric, d, nqs=(3, 40), ks=None):
    if ks is None:
        ks = (10, 128) + ((129, 200) if d in (32, 20, 200) else ())
    x, q = S.real_f32(5000, d, max(nqs), 5000 + d)
    oi, od = oracle.flat_knn(x, q, max(ks), metric)
    xd, qd = _dev(x), _dev(q)
    for nq in nqs:
        for k in ks:
            _same(eng, xd, qd, nq, k, metric, oi, od, tag=(metric, d, nq, k))


# ---- B6: IVF_FLAT ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("d", [32, 40])
def test_ivf_flat_real_f32(eng, oracle, metric, d):
    from lance_amd.engine import DeviceFlatIndex
    n, nlist = 8000, 12
    x, q = S.real_f32(n, d, 32, 6000 + d)
    cent, _, _, _ = oracle.kmeans_train(x[:4096], nlist, max_iters=6, seed=2)
    part, _ = eng.assign(x, cent, metric)
    g = DeviceFlatIndex.create(eng, metric, cent, x, part)
    for k, nprobes in ((10, 4), (1, 3), (129, 12)):
        gi, gd = g.search(q, k, nprobes)
        oi, od = oracle.ivfflat_search(x, cent, q, k, nprobes, metric)
        assert (gi.cpu().numpy().view(np.uint64) == oi).all(), (metric, d, k, nprobes)
        assert (gd.cpu().numpy().view(np.uint32) == od.view(np.uint32)).all(), (metric, d, k, nprobes)


# ---- B7: the other routes, each in a fresh child process (both switches are read once per process) -----------------------------------
def _child(env, select):
    if IN_CHILD:
        pytest.skip("already inside the child run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-p", "no:cacheprovider", "-k", select],
                       cwd=root, env=dict(os.environ, **env), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-1000:]


def test_routes_three_and_four_queries_on_the_single_pass_kernel():
    """LANCE_HIP_FLAT_SMALL_MAXQ=4: the single-pass cases above (real-valued f32, the other column types, the running threshold) with
    three and four queries -- the instantiations whose chunk loads are issued eight at a time, like the two-query one"""
    _child({"LANCE_HIP_FLAT_SMALL_MAXQ": "4"}, "single_pass and not routes")


def test_routes_one_and_two_queries_on_the_batch_path():
    """LANCE_HIP_NO_FLAT_SMALL=1: the batch path answers the one- and two-query calls on the same data"""
    _child({"LANCE_HIP_NO_FLAT_SMALL": "1"}, "single_pass_real and not routes")


# ---- B4: rows with a NaN element behind the batch filters -------------------------------------------------------------------------------
# The reference's distance of such a row is the POSITIVE NaN (its CPU hands a NaN operand on with its sign) and sorts last.  The GPU's
# subtract returns a NaN subtrahend with the sign bit set: `q - x` in the exact evaluation behind the matrix-core filters, and the `1 - x`
# that ends a cosine distance, made it the negative NaN, which sorts FIRST (lance_amd/csrc/exact.cuh: dist_exact_rt's SWAP, cosine_finish).
# 5,000 NaN rows are more than a query's pool of 4,096: ranked first they overflow it, and the repair pass then finds nothing.
@pytest.mark.parametrize("kind,metric,d,nq,stage", [("f32", "l2", 128, 256, "flat_mfma"), ("f16", "l2", 128, 256, "flat_mfma"),
                                                    ("f32", "l2", 256, 256, "flat_mfma_wide"), ("f32", "cosine", 256, 256, "flat_mfma_wide"),
                                                    ("f32", "cosine", 256, 4, None), ("f32", "cosine", 128, 4, None), ("f32", "dot", 128, 256, "flat_mfma")])
def test_nan_rows_sort_last_behind_a_query_batch(eng, oracle, kind, metric, d, nq, stage):
    n = 40_000
    x, q = (S.real_f16 if kind == "f16" else S.real_f32)(n, d, nq, 4000 + d)
    x[3::8] = np.nan                                    # 5,000 rows, in every epoch of the scan
    assert np.isnan(x.astype(f32)).all(axis=1).sum() == 5000
    oi, od = oracle.flat_knn(_oracle_rows(x), _oracle_rows(q), 10, metric)
    assert not np.isnan(od).any()
    before = eng.timing_query("count:" + stage)[1] if stage else 0
    _same(eng, _dev(x), _dev(q), nq, 10, metric, oi, od, tag=(kind, metric, d, nq))
    assert stage is None or eng.timing_query("count:" + stage)[1] > before, f"the {stage} filter did not serve the call"
