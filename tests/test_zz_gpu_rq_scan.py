"""IVF_RQ on the GPU (lance_amd/csrc/rq.hip) where tests/test_zz_gpu_rq.py stops, against tests/rq_spec.py bit for bit -- ids and
distance bits, no tolerances:
  * partitions of ~800 rows stored in an order chosen for one query (rq_spec.ordered_partition, self-checked by tests/test_rq_spec.py):
    the scan passes its first truncation and then admits rows by its threshold alone; ties cut at one truncation and met again later;
  * k = 128 at d = 1024 and 1032, on either side of the dimension where the scan's candidate buffer doubles (the rotated query it borrows
    the buffer for fills 512 entries to the last byte at d = 1024), in partitions ordered for that buffer (refine_spec.ordered_partition);
  * search at d = 8, 24, 128 (16-byte row loads), 136 (full 16-blocks and a tail in the rotation) and 2048 (the largest: the rotated
    query fills the whole candidate buffer it borrows, ~48 KiB of LDS in the scan and ~52 KiB in the replay), one query a centroid;
  * the encoder at d >= 256 (one row per iteration) and at d that do not divide 256, and its grid-stride loop;
  * rq_distance with a real rotation beyond d = 128, and its grid-stride loop;
  * the query split of one search call (nq nprobes k > 2^24): equal to the same queries searched in two calls, replay counts included."""
import functools

import numpy as np
import pytest

import rq_spec as R
from test_zz_gpu_rq import check_distances, check_search, distance_queries, eng, same_bits, storage

pytestmark = pytest.mark.gpu
f32 = np.float32
UNSET = np.iinfo(np.uint64).max


def device_index(x, cent, P, metric, rid, built=None):
    """the rows encoded on the GPU and grouped into an index; the specification's build of the same rows next to it"""
    import oracle
    from lance_amd.engine import DeviceRqIndex
    part, codes, add, scale = built or R.build(oracle, x, cent, P, metric)
    dvc = oracle.assign(x, cent, metric)[1]
    e = eng()
    gc, ga, gs = e.rq_encode(x, part.view(np.int32), dvc, cent, P, metric)
    assert (gc.cpu().numpy() == codes).all() and same_bits(ga.cpu().numpy(), add) and same_bits(gs.cpu().numpy(), scale)
    ix = DeviceRqIndex.create(e, metric, cent, P, gc, ga, gs, part.view(np.int32), row_ids=rid)
    return ix, (codes, add, scale, part, cent, P, rid)


def row_ids(n, masked, seed):
    """permuted small ids where a mask is indexed by them, Lance row addresses (>= 2^32, permuted) otherwise"""
    import rowid_fixtures as F
    return R.permuted_ids(n, seed) if masked else F.row_addresses(n, seed)


def half_mask(rid, seed):
    half = np.zeros(int(rid.max()) + 1, bool)
    half[rid[np.random.default_rng(seed).random(len(rid)) < 0.5]] = True
    return half


# ---- threshold and ties ---------------------------------------------------------------------------------------------------------------
ORDERED = [(order, k) for order, (_, ks) in R.ORDERS.items() for k in ks]


@functools.lru_cache(maxsize=None)
def ordered(order, metric, k, prefiltered):
    """the layout is built for the branch in use: the u8 table without a prefilter, the f32 fold under one"""
    import oracle
    f = R.ordered_partition(oracle, order, metric, k, prefiltered=prefiltered)
    x = f["x"]
    ix, spec = device_index(x, f["cent"], f["P"], metric, row_ids(len(x), prefiltered, 3))
    rng = np.random.default_rng(13)
    others = (x[rng.integers(0, len(x), 2)] + rng.standard_normal((2, x.shape[1])) * 0.2).astype(f32)
    return ix, spec, np.ascontiguousarray(np.concatenate([f["q"][None], others])), f


@pytest.mark.parametrize("mask", ["none", "all", "half"])
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("order,k", ORDERED)
def test_threshold_and_ties(order, k, metric, mask):
    ix, spec, q, f = ordered(order, metric, k, mask != "none")
    rid, N = spec[6], f["N"]
    assert (rid.min() >= 2 ** 31 and rid.max() >= 2 ** 32) == (mask == "none")
    allow = None if mask == "none" else (np.ones(int(rid.max()) + 1, bool) if mask == "all" else half_mask(rid, 8))
    keys = f["keys"] if allow is None else f["keys"][allow[rid[:N]]]           # partition 0 is the first N rows, stored in input order
    cut = R.kth_is_tied(keys, k)
    if mask != "half":
        assert cut == f["cut_tie"]                               # what the builder proved holds for the rows this search sees
    for nprobes in (1, 2):
        replays, _, od = check_search(ix, spec, q, k, nprobes, metric, prefilter=allow)
        # the design query's nearest partition cut a tie at its k-th key: the query is replayed unless the other partition pushed
        # that key out of the merged answer
        if cut and (nprobes == 1 or R.order_key(od[0, k - 1]) >= np.sort(keys)[k - 1]):
            assert replays > 0, (order, k, metric, mask, nprobes)


# ---- k = 128 where the candidate buffer changes size ---------------------------------------------------------------------------------
# (d, entries of the scan's buffer at k = 128, rows of the ordered partition: past the buffer and two more chunks, N % 32 = 1)
K128_DIMS = [(1024, 512, 1409), (1032, 1024, 1569)]


@functools.lru_cache(maxsize=None)
def ordered_k128(d, cap, N, order, prefiltered):
    import oracle
    import refine_spec as F
    f = F.ordered_partition(oracle, "rq", order, "l2", 128, cap, N, d=d, prefiltered=prefiltered)
    ix, spec = device_index(f["x"], f["cent"], f["P"], "l2", row_ids(len(f["x"]), prefiltered, 3), f["built"])
    return ix, spec, f


@pytest.mark.parametrize("mask", ["none", "all"])
@pytest.mark.parametrize("order", ["descending", "tie_cut"])
@pytest.mark.parametrize("d,cap,N", K128_DIMS)
def test_k128_buffer_sizes(d, cap, N, order, mask):
    """descending: after the first cut every row enters, the buffer is cut again at every chunk; tie_cut: the first cut cuts a block of
    136 copies that still holds the 128th key at the end, so the design query is replayed"""
    ix, spec, f = ordered_k128(d, cap, N, order, mask == "all")
    rid = spec[6]
    allow = np.ones(int(rid.max()) + 1, bool) if mask == "all" else None
    assert f["cut_tie"] == (order == "tie_cut")
    q = np.ascontiguousarray(np.stack([f["q"], f["x"][5] + f32(0.1)]))
    for nprobes in (1, 2):
        replays, _, od = check_search(ix, spec, q, 128, nprobes, "l2", prefilter=allow)
        # replayed unless the other partition pushed the tied key out of the merged answer
        if f["cut_tie"] and (nprobes == 1 or R.order_key(od[0, 127]) >= np.sort(f["keys"])[127]):
            assert replays > 0, (d, order, mask, nprobes)


# ---- dimensions in search -------------------------------------------------------------------------------------------------------------
DIM_SIZES = [33, 0, 97]


@functools.lru_cache(maxsize=None)
def dim_rows(d, metric):
    import oracle
    x, cent = R.sized_partitions(DIM_SIZES, d, seed=d)
    rng = np.random.default_rng(d + 1)
    q = (x[rng.integers(0, len(x), 3)] + rng.standard_normal((3, d)) * 0.2).astype(f32)
    q[1] = cent[2]                                               # zero residual in partition 2 (qmin == qmax), not in partition 0
    P = R.rotation(d, d + 2)
    return x, cent, P, np.ascontiguousarray(q), R.build(oracle, x, cent, P, metric)      # (built once: at d = 2048 the numpy rotation takes seconds)


@functools.lru_cache(maxsize=None)
def dim_index(d, metric, masked):
    import oracle
    x, cent, P, q, built = dim_rows(d, metric)
    ix, spec = device_index(x, cent, P, metric, row_ids(len(x), masked, 5), built)
    assert list(np.diff(oracle.partition_layout(spec[3], 3)[0].astype(np.int64))) == DIM_SIZES
    return ix, spec, q


@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("k", [10, 128])
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("d", [8, 24, 128, 136, 2048])
def test_search_dimensions(d, metric, k, masked):
    ix, spec, q = dim_index(d, metric, masked)
    _, oi, _ = check_search(ix, spec, q, k, 3, metric, prefilter=half_mask(spec[6], 9) if masked else None)
    assert (oi[:, 0] != UNSET).all() and ((oi == UNSET).any() == (k == 128 and masked))      # 130 rows: k = 128 is filled unless masked


# ---- encode -----------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rot(d, name):
    return R.rotations(d, seed=d)[name]


def check_encode(x, cent, P, metric):
    import oracle
    part, dvc = R.prepare_rows(oracle, x, cent, metric)
    codes, add, scale = eng().rq_encode(x, part.view(np.int32), dvc, cent, P, metric)
    wc, wa, ws = R.encode(x, part, dvc, cent, P, metric)
    assert (codes.cpu().numpy() == wc).all()
    assert same_bits(add.cpu().numpy(), wa) and same_bits(scale.cpu().numpy(), ws)
    return part, wc, wa, ws


@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("name", ["qr", "signed_perm"])
@pytest.mark.parametrize("d,n", [(24, 301), (136, 67), (256, 67), (264, 67), (2048, 37)])
def test_encode_dimensions(d, n, name, metric):
    """d = 24: ten rows per iteration, 240 of 256 threads, n % 10 = 1; d = 136: one row per iteration with the rotated row at
    res + 256; d >= 256: one row per iteration, LDS of 2 d floats"""
    x, _ = R.clustered(n, d, 1, seed=d)
    own = (3, 20, 30, n - 1)
    cent = np.ascontiguousarray(x[list(own)])                    # four rows ARE centroids: zero residual, ip == 0
    x[7, 1] = np.nan                                             # a row without a partition: zeros out
    part, wc, wa, ws = check_encode(x, cent, rot(d, name), metric)
    assert part[7] == R.NONE and (wc[7] == 0).all() and wa[7] == 0 and ws[7] == 0
    own = [i for i in own if (x[i] == cent[part[i]]).all()]
    assert own or metric == "dot"                                # (under dot a centroid row may belong to another centroid)
    assert (ws[own] == 0).all() and (wc[own] == 255).all()


def test_encode_grid_stride():
    """d = 256, n = 8197: five rows past the 8192 blocks of the launch, taken by their second iteration"""
    x, _ = R.clustered(8197, 256, 1, seed=2)
    part, wc, _, _ = check_encode(x, np.ascontiguousarray(x[[5, 4000, 8196]]), rot(256, "qr"), "l2")
    assert (part[8192:] != R.NONE).all() and wc[8192:].any()


# ---- rq_distance ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("n", [33, 95])
@pytest.mark.parametrize("d", [24, 136, 2048])
def test_distances_rotated(d, n, metric):
    codes, add, scale = storage(n, d, seed=n + d)
    qr, dqc = distance_queries(d)
    check_distances(codes, add, scale, qr, dqc, rot(d, "qr"), metric)


def test_distances_grid_stride():
    """n = 16384 + 33: 65 blocks of rows for the 64 of the launch; the last 33 rows are one packed row short of a batch + remainder"""
    d, n = 8, 16384 + 33
    codes, add, scale = storage(n, d, seed=1)
    qr, dqc = distance_queries(d)
    check_distances(codes, add, scale, qr, dqc, rot(d, "qr"), "l2")


# ---- the query split of one call --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True])
def test_batch_split(masked):
    """nq nprobes k = 2051 * 64 * 128 > 2^24: the call scans 2048 queries, then 3.  150 copies of one row fill one partition past k = 128:
    unfiltered, that partition cuts a tie at its k-th key for every query and every query is replayed; under the half mask fewer than
    k of its rows are selected and none is (256 rows cannot hold a cut tie at k = 128 under a mask that selects half of them)"""
    import oracle
    d, n, nlist, k, nq = 8, 256, 64, 128, 2051
    x, _ = R.clustered(n, d, 1, seed=31)
    x[:150] = x[0]
    rng = np.random.default_rng(32)
    cent = np.ascontiguousarray(x[np.concatenate([[0], 150 + rng.choice(n - 150, nlist - 1, replace=False)])])
    q = np.ascontiguousarray((x[rng.integers(0, n, nq)] + rng.standard_normal((nq, d)) * 0.3).astype(f32))
    P = rot(d, "qr")
    rid = row_ids(n, masked, 6)
    ix, spec = device_index(x, cent, P, "l2", rid)
    allow = half_mask(rid, 7) if masked else None
    assert nq * nlist * k > 2 ** 24 and (2 ** 24) // (nlist * k) == 2048

    def run(qs):
        gi, gd = ix.search(qs, k, nlist, allow=allow)
        return gi.cpu().numpy().view(np.uint64), gd.cpu().numpy(), eng().search_stats()
    wi, wd, wr = run(q)
    ai, ad, ar = run(q[:1000])
    bi, bd, br = run(q[1000:])
    assert (wi == np.concatenate([ai, bi])).all() and same_bits(wd, np.concatenate([ad, bd]))
    assert wr == ar + br and (wr == 0) == masked, (wr, ar, br)
    some = [0, 2047, 2048, 2050]
    oi, od = R.search(oracle, *spec[:6], q[some], k, nlist, "l2", row_ids=rid, prefilter=allow)
    assert (wi[some] == oi).all() and same_bits(wd[some], od)
