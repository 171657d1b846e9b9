"""1-bit RaBitQ and IVF_RQ on the GPU (lance_amd/csrc/rq.hip) against tests/rq_spec.py, bit for bit: codes and factors, the three
distance branches (packed rows through the u8 table, the f32 remainder past the last full batch of 32, the f32 fold under a
prefilter), and searches -- ids and distance bits.  The specification is checked on the CPU by tests/test_rq_spec.py and the
kernels' source is run on the CPU by tests/test_rq_kernels_cpu.py.  Sorted last: newest device code last."""
import ctypes as C
import functools

import numpy as np
import pytest

import rq_spec as R

pytestmark = pytest.mark.gpu
f32 = np.float32
ROTS = ("identity", "signed_perm", "qr")


def eng():
    import lance_amd
    return lance_amd.default_engine()


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


# ---- encode -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("rot", ROTS)
@pytest.mark.parametrize("d", [8, 64, 128])
def test_encode(d, rot, metric):
    import oracle
    x, _ = R.clustered(300, d, 1, seed=d)
    cent = np.ascontiguousarray(x[[3, 50, 120, 299]])            # four rows ARE centroids: zero residual, ip == 0
    x[7, 1] = np.nan                                             # a row without a partition: zeros out
    P = R.rotations(d, seed=d)[rot]
    part, dvc = R.prepare_rows(oracle, x, cent, metric)
    assert part[7] == R.NONE
    codes, add, scale = eng().rq_encode(x, part.view(np.int32), dvc, cent, P, metric)
    wc, wa, ws = R.encode(x, part, dvc, cent, P, metric)
    assert (codes.cpu().numpy() == wc).all()
    assert same_bits(add.cpu().numpy(), wa) and same_bits(scale.cpu().numpy(), ws)
    own = [i for i in (3, 50, 120, 299) if (x[i] == cent[part[i]]).all()]
    assert own or metric == "dot"                                # (under dot a centroid row may belong to another centroid)
    assert (ws[own] == 0).all() and (wc[own] == 255).all()       # ip == 0 -> scale 0; every rotated component is +0.0
    assert (wc[7] == 0).all() and wa[7] == 0 and ws[7] == 0


def test_encode_signed_zero_components():
    """P = I: a residual component -0.0 (v = -0.0 against a +0.0 centroid) and one +0.0.  The rotation's dot starts its accumulators at
    +0.0 and (+0.0) + (-0.0) = +0.0, so both rotate to +0.0 and both set their bit -- on the GPU as in the specification."""
    d = 8
    cent = np.zeros((1, d), f32)
    x = np.array([[-0.0, 1.0, -1.0, 0.0, 2.0, -2.0, 0.5, -0.5],
                  [0.0, 1.0, -1.0, -0.0, 2.0, -2.0, 0.5, -0.5]], f32)
    assert np.signbit(x[0, 0] - cent[0, 0]) and not np.signbit(x[1, 0] - cent[0, 0])
    part = np.zeros(2, np.int32)
    dvc = np.array([10.5, 10.5], f32)
    codes, add, scale = eng().rq_encode(x, part, dvc, cent, np.eye(d, dtype=f32), "l2")
    wc, wa, ws = R.encode(x, part.view(np.uint32), dvc, cent, np.eye(d, dtype=f32), "l2")
    assert (codes.cpu().numpy() == wc).all() and same_bits(add.cpu().numpy(), wa) and same_bits(scale.cpu().numpy(), ws)
    assert list(wc[:, 0]) == [0b01011011, 0b01011011]


# ---- distances ----------------------------------------------------------------------------------------------------------------------
SIZES = (1, 31, 32, 33, 64, 95)


def storage(n, d, seed, all_bits_row=False):
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 256, (n, d // 8)).astype(np.uint8)
    if all_bits_row:
        codes[0] = 255
    return codes, rng.standard_normal(n).astype(f32), (-rng.random(n)).astype(f32)


def check_distances(codes, add, scale, qr, dqc, P, metric):
    for quantised in (True, False):
        got = eng().rq_distance(codes, add, scale, qr, dqc, P, metric, quantised).cpu().numpy()
        assert same_bits(got, R.distances(codes, add, scale, qr, dqc, P, metric, quantised)), (len(codes), metric, quantised)


@functools.lru_cache(maxsize=None)
def distance_queries(d):
    """residual queries [4][d]: all zero (qmin == qmax); one whose table is half-integers with qmax - qmin = 255 (factor exactly 1, so
    entries t - qmin = 0.5, 2.5, 4.5 ... sit on x.5 with x even: half-away rounds them up, half-even would round them down); a
    Gaussian one; a Gaussian one with a -0.0 component"""
    rng = np.random.default_rng(d)
    q = np.zeros((4, d), f32)
    q[1, :4] = [0.5, 2.0, 4.0, 8.0]
    q[1, 4] = 255.0
    q[2] = rng.standard_normal(d)
    q[3] = rng.standard_normal(d); q[3, 1] = -0.0
    return q, rng.standard_normal(4).astype(f32)


def test_half_way_table_entries_round_away_from_zero():
    q, _ = distance_queries(8)
    c = R.Query(q[1], 0.0, np.eye(8, dtype=f32), "l2")
    assert (c.qmin, c.qmax) == (0.0, 255.0) and c.table[0, 1] == 0.5 and c.table[0, 3] == 2.5
    assert c.e[0, 1] == 1 and c.e[0, 3] == 3 and c.e[0, 5] == 5            # round-half-even: 0, 2, 4
    z = R.Query(q[0], 0.0, np.eye(8, dtype=f32), "l2")
    assert z.qmin == z.qmax and not z.e.any()


@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("d", [8, 128])
def test_distances(d, n, metric):
    codes, add, scale = storage(n, d, seed=n + d)
    qr, dqc = distance_queries(d)
    check_distances(codes, add, scale, qr, dqc, np.eye(d, dtype=f32), metric)
    check_distances(codes, add, scale, qr[2:], dqc[2:], R.rotations(d, seed=1)["qr"], metric)


@pytest.mark.parametrize("n", SIZES)
def test_distances_saturate_the_u16_sum(n):
    """d = 1536, P = I, every query component 1: each of the 384 tables spans 0 .. 4, a row with every bit set picks 255 from each, and
    384 * 255 = 97920 saturates the u16 sum at 65535 -- in the packed rows only; the same row in the f32 branches sums to 1536"""
    d = 1536
    codes, add, scale = storage(n, d, seed=n, all_bits_row=True)
    qr = np.ones((1, d), f32)
    P = np.eye(d, dtype=f32)
    c = R.Query(qr[0], 0.0, P, "l2")
    assert int(c.e.max()) * (d // 4) == 97920 and c.raw_packed(codes[:1])[0] == f32(65535.0) * f32(f32(4.0) / f32(255.0)) and c.raw_f32(codes[:1], 0.0)[0] == 1536.0
    check_distances(codes, add, scale, qr, np.array([0.25], f32), P, "l2")


# ---- search -------------------------------------------------------------------------------------------------------------------------
NLIST = 5
DUP = 150


@functools.lru_cache(maxsize=None)
def built(metric, ids):
    """partitions of 31, 32, 33, 0 and 300 rows (forced by explicit centroids and constructed rows), the first 150 rows of the largest
    one vector repeated; ids: "addresses" = Lance row addresses (>= 2^32, permuted), "small" = small permuted ids (for masks)"""
    import oracle
    import rowid_fixtures as F
    from lance_amd.engine import DeviceRqIndex
    d = 64
    x, cent = R.sized_partitions([31, 32, 33, 0, 300], d, seed=11, dup_block=DUP)
    P = R.rotation(d, 5)
    part, codes, add, scale = R.build(oracle, x, cent, P, metric)
    sizes = np.diff(oracle.partition_layout(part, NLIST)[0].astype(np.int64))
    assert list(sizes) == [31, 32, 33, 0, 300]
    rid = F.row_addresses(len(x), 3) if ids == "addresses" else R.permuted_ids(len(x), 3)
    e = eng()
    dvc = oracle.assign(x, cent, metric)[1]
    gc, ga, gs = e.rq_encode(x, part.view(np.int32), dvc, cent, P, metric)
    ix = DeviceRqIndex.create(e, metric, cent, P, gc, ga, gs, part.view(np.int32), row_ids=rid)
    rng = np.random.default_rng(12)
    q = (x[rng.integers(0, len(x), 33)] + rng.standard_normal((33, d)) * 0.2).astype(f32)
    rows, counts = np.unique(x, axis=0, return_counts=True)
    assert counts.max() == DUP
    q[0] = rows[np.argmax(counts)]                                                   # the repeated vector itself: 150 rows tie at its nearest distance
    return ix, (codes, add, scale, part, cent, P, rid), np.ascontiguousarray(q)


def check_search(ix, spec, q, k, nprobes, metric, prefilter=None):
    import oracle
    codes, add, scale, part, cent, P, rid = spec
    gi, gd = ix.search(q, k, nprobes, allow=prefilter)
    gi = gi.cpu().numpy().view(np.uint64); gd = gd.cpu().numpy()
    oi, od = R.search(oracle, codes, add, scale, part, cent, P, q, k, nprobes, metric, row_ids=rid, prefilter=prefilter)
    assert (gi == oi).all(), (k, nprobes, np.argwhere(gi != oi)[:4])
    assert same_bits(gd, od), (k, nprobes)
    return eng().search_stats(), oi, od


def cut_tie(spec, q0, k, metric):
    """does the nearest partition of q0 hold more rows at its k-th smallest distance than fit into k?"""
    import oracle
    codes, add, scale, part, cent, P, _ = spec
    pr, pd = oracle.find_partitions(q0[None], cent, 1, metric)
    offs, perm = oracle.partition_layout(part, NLIST)
    rows = perm[int(offs[pr[0, 0]]):int(offs[pr[0, 0] + 1])]
    keys = np.sort(R.order_key(R.Query(q0 - cent[pr[0, 0]], pd[0, 0], P, metric).distance_all(codes[rows], add[rows], scale[rows])))
    return len(keys) > k and keys[k - 1] == keys[k]


@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("nprobes", [1, 3, NLIST])
@pytest.mark.parametrize("k", [1, 10, 128])
def test_search(k, nprobes, metric):
    ix, spec, q = built(metric, "addresses")
    assert spec[6].min() >= 2 ** 31 and spec[6].max() >= 2 ** 32
    replays, oi, _ = check_search(ix, spec, q, k, nprobes, metric)
    if k == 128 and nprobes == 1:
        assert (oi == np.iinfo(np.uint64).max).any()             # k larger than the probed rows: the tail stays unset
    if nprobes == 1 and cut_tie(spec, q[0], k, metric):
        assert replays > 0                                       # the duplicate block ties at the k-th distance: the heap decides
    if metric == "l2" and k == 10:
        assert cut_tie(spec, q[0], k, metric)                    # (the fixture does what it is for)


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_search_prefiltered(metric):
    ix, spec, q = built(metric, "small")
    rid = spec[6]
    size = int(rid.max()) + 1
    every = np.ones(size, bool)
    none = np.zeros(size, bool)
    half = none.copy(); half[rid[np.random.default_rng(8).random(len(rid)) < 0.5]] = True
    _, ai, ad = check_search(ix, spec, q, 10, NLIST, metric, prefilter=every)
    _, ui, ud = check_search(ix, spec, q, 10, NLIST, metric)
    # the all-selected mask takes the f32 fold, the unfiltered search the u8 table: the answers must differ somewhere, or this test
    # could not tell the two branches apart
    assert not same_bits(ad, ud)
    _, ni, _ = check_search(ix, spec, q, 10, NLIST, metric, prefilter=none)
    assert (ni == np.iinfo(np.uint64).max).all()
    check_search(ix, spec, q, 10, NLIST, metric, prefilter=half)
    check_search(ix, spec, q, 128, 3, metric, prefilter=half)
    check_search(ix, spec, q, 10, 3, metric, prefilter=half[: size // 2])          # a mask shorter than the largest row id


# ---- surface ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_create_index_end_to_end(metric):
    import lance_amd
    import oracle
    n, d, nlist = 2000, 64, 8
    x, q = R.clustered(n, d, 33, seed=21)
    x[5, 3] = np.nan; x[9, 0] = np.inf                           # rows without a partition are dropped
    ix = lance_amd.create_index(x, "IVF_RQ", metric=metric, num_partitions=nlist, max_iters=5, seed=3)
    assert isinstance(ix, lance_amd.IvfRqIndex) and ix.params.num_partitions == nlist and ix.params.metric == metric and ix.params.num_bits == 1
    assert {"train_ivf", "transform", "encode", "build_partitions"} <= set(ix.stats.seconds)
    cent, P = ix.centroids, ix.rotation
    assert P.shape == (d, d) and P.dtype == f32 and same_bits(P, lance_amd.vector.rq_rotation_matrix(d, 3))
    assert np.abs(P.astype(np.float64) @ P.astype(np.float64).T - np.eye(d)).max() < 1e-5
    part, codes, add, scale = R.build(oracle, x, cent, P, metric)
    assert (ix.part_ids.cpu().numpy().view(np.uint32) == part).all() and (part[[5, 9]] == R.NONE).all()
    for k, nprobes in ((10, 3), (128, nlist)):
        gi, gd = ix.nearest(q, k, nprobes)
        oi, od = R.search(oracle, codes, add, scale, part, cent, P, q, k, nprobes, metric)
        assert (gi == oi).all() and same_bits(gd, od), (k, nprobes)
    allow = np.random.default_rng(2).random(n) < 0.5
    oi, od = R.search(oracle, codes, add, scale, part, cent, P, q, 10, 3, metric, prefilter=allow)
    gi, gd = ix.nearest(q, 10, 3, prefilter=allow)
    assert (gi == oi).all() and same_bits(gd, od)
    # an explicit rotation is taken as given
    P2 = R.signed_permutation(d, 4)
    ix2 = lance_amd.create_index(x, "IVF_RQ", metric=metric, num_partitions=nlist, num_bits=1, ivf_centroids=cent, rq_rotation=P2)
    assert same_bits(ix2.rotation, P2) and same_bits(ix2.centroids, cent)
    part2, codes2, add2, scale2 = R.build(oracle, x, cent, P2, metric)
    gi, gd = ix2.nearest(q, 10, 3)
    oi, od = R.search(oracle, codes2, add2, scale2, part2, cent, P2, q, 10, 3, metric)
    assert (gi == oi).all() and same_bits(gd, od)


def test_refusals(tmp_path):
    import lance_amd
    x = np.zeros((64, 16), f32)
    with pytest.raises(ValueError, match="num_bits 8 not supported"):
        lance_amd.create_index(x, "IVF_RQ", num_partitions=2, num_bits=8)
    with pytest.raises(ValueError, match="num_bits 2 not supported"):
        lance_amd.create_index(x, "IVF_RQ", num_partitions=2, num_bits=2)
    with pytest.raises(ValueError, match="dimension 12 is not a multiple of 8"):
        lance_amd.create_index(np.zeros((64, 12), f32), "IVF_RQ", num_partitions=2)
    with pytest.raises(ValueError, match="not a multiple of 8"):
        eng().rq_encode(np.zeros((4, 12), f32), np.zeros(4, np.int32), np.zeros(4, f32), np.zeros((1, 12), f32), np.eye(12, dtype=f32))
    for dt in (np.float16, np.int8):
        with pytest.raises(NotImplementedError, match="unsupported data type: " + np.dtype(dt).name):
            lance_amd.create_index(x.astype(dt), "IVF_RQ", num_partitions=2)
    with pytest.raises(NotImplementedError, match="float16"):
        eng().rq_encode(x.astype(np.float16), np.zeros(64, np.int32), np.zeros(64, f32), x[:1], np.eye(16, dtype=f32))
    with pytest.raises(NotImplementedError, match="cosine is not supported"):
        lance_amd.create_index(x, "IVF_RQ", metric="cosine", num_partitions=2)
    with pytest.raises(NotImplementedError, match="cosine is not supported"):
        eng().rq_distance(np.zeros((2, 2), np.uint8), np.zeros(2, f32), np.zeros(2, f32), x[:1], np.zeros(1, f32), np.eye(16, dtype=f32), "cosine")
    with pytest.raises(ValueError, match="rq_rotation must be"):
        lance_amd.create_index(x, "IVF_RQ", num_partitions=2, ivf_centroids=x[:2], rq_rotation=np.eye(8, dtype=f32))
    ix, _, q = built("l2", "small")
    ivf = lance_amd.vector.IvfRqIndex(ix, None, None, None)
    with pytest.raises(NotImplementedError, match="refine_factor"):
        ivf.nearest(q, 5, 1, refine_factor=2)
    with pytest.raises(NotImplementedError, match="distance_range"):
        ivf.nearest(q, 5, 1, distance_range=(0.0, 1.0))
    with pytest.raises(NotImplementedError, match="index files"):
        ivf.save(tmp_path / "rq")
    for call, name in ((lambda: ivf.append(x), "append"), (lambda: ivf.remap({}), "remap"), (lambda: ivf.delete([1]), "delete"),
                       (lambda: lance_amd.merge_indices([ivf, ivf]), "merge_indices")):
        with pytest.raises(NotImplementedError, match=name + " is not supported"):
            call()
    with pytest.raises(lance_amd.LanceHipError, match="k=129 not supported"):
        ix.search(q, 129, 1)
    with pytest.raises(lance_amd.LanceHipError, match="k=129 not supported"):
        ix.search(q, 129, 1, allow=np.ones(8, bool))


def test_entry_points_refuse_each_others_handles(tmp_path):
    import torch
    import lance_amd
    rx, _, _ = built("l2", "small")
    e = eng()
    q = torch.zeros((2, 64), dtype=torch.float32, device="cuda")
    ids = torch.full((2, 5), -7, dtype=torch.int64, device="cuda")
    dists = torch.zeros((2, 5), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    lib, EINVAL = e.lib, lance_amd._lib.EINVAL
    assert lib.lance_hip_ivfflat_search(e.h, rx.h, p(q), 2, 5, 1, p(ids), p(dists)) == EINVAL
    assert lib.lance_hip_ivfflat_search_filtered(e.h, rx.h, p(q), 2, 5, 1, None, 0, p(ids), p(dists)) == EINVAL
    assert lib.lance_hip_ivfpq_search(e.h, rx.h, p(q), 2, 5, 1, 0, p(ids), p(dists)) == EINVAL
    assert lib.lance_hip_ivfpq_search_async(e.h, rx.h, p(q), 2, 5, 1, 0, p(ids), p(dists)) == EINVAL
    assert lib.lance_hip_ivfpq_search_filtered(e.h, rx.h, p(q), 2, 5, 1, 0, None, 0, p(ids), p(dists)) == EINVAL
    assert lib.lance_hip_ivfsq_search(e.h, rx.h, p(q), 2, 5, 1, p(ids), p(dists)) == EINVAL
    assert lib.lance_hip_ivfsq_search_filtered(e.h, rx.h, p(q), 2, 5, 1, None, 0, p(ids), p(dists)) == EINVAL
    assert lib.lance_hip_index_save(e.h, rx.h, str(tmp_path / "rq").encode(), 0, 0.0) == EINVAL
    out = C.c_void_p()
    handles = (C.c_void_p * 1)(rx.h)
    assert lib.lance_hip_index_merge(e.h, handles, 1, C.byref(out)) == EINVAL and not out.value
    assert lib.lance_hip_index_remap(e.h, rx.h, None, None, 0, C.byref(out)) == EINVAL and not out.value
    assert lib.lance_hip_index_export_rows(e.h, rx.h, None, None, None, None) == EINVAL
    assert (ids.cpu().numpy() == -7).all(), "a refused call writes nothing"
    # and the RQ entries refuse the other kinds
    x, _ = R.clustered(300, 64, 1, seed=1)
    for kind in ("IVF_FLAT", "IVF_SQ"):
        other = lance_amd.create_index(x, kind, num_partitions=2, max_iters=2, sample_rate=4)
        assert lib.lance_hip_ivfrq_search(e.h, other._ix.h, p(q), 2, 5, 1, p(ids), p(dists)) == EINVAL, kind
        assert lib.lance_hip_ivfrq_search_filtered(e.h, other._ix.h, p(q), 2, 5, 1, None, 0, p(ids), p(dists)) == EINVAL, kind
    assert (ids.cpu().numpy() == -7).all()
