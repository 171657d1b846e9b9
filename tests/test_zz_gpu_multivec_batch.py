"""Batched multivector flat KNN on the GPU (lance_amd/csrc/multivec_batch.hip) against the CPU specification -- per query
multivec_spec.topk(multivec_spec.distances(...)), ids as uint64 and distances as uint32 bits -- and against the single-query calls on
the same inputs.  The filter-route cases also assert WHICH route answered (count:multivec_mc_filter advanced, count:multivec_batch_loop
and count:multivec_batch_overflow did not) and that the rows evaluated exactly per query lie between k and the specification's
superset count {D_spec <= t_spec + 4 E} (tests/multivec_batch_spec.py).

The layout under test: the rows are cut into units by vector count and walked in tiles of 32 vectors (rows of 1, 2, 31, 32, 33, 64,
65, 200 and 1030 vectors end before, at and after tile boundaries and span many tiles); the query vectors of a batch are columns in
blocks of 32 (nqv of 1 .. 256 mixed in one batch start and end anywhere in a block, and a query of 256 spans eight); a chunk holds at
most 64 queries and 2048 columns.  Every case is a few hundred to a few thousand short rows."""
import ctypes as C

import numpy as np
import pytest

import multivec_batch_spec as B
import multivec_spec as M

pytestmark = pytest.mark.gpu
f32 = np.float32
U64_MAX = 0xFFFFFFFFFFFFFFFF


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _dev(a):
    import lance_amd.engine as E
    return E.to_device(a)


def _counts(eng):
    return tuple(eng.timing_query("count:" + s)[1] for s in ("multivec_mc_filter", "multivec_batch_loop", "multivec_batch_overflow"))


def _degenerate_rows(values, off):
    return ~np.logical_and.reduceat(B.split(values)[3], np.asarray(off, np.int64)[:-1])


def _run(eng, oracle, values, off, qs, k, metric="cosine", rid=None, route="filter", vd=None, qd=None, tag=None, spec=True, **rng):
    """one batch call against the specification and against the single-query calls; -> (ids, dists, survivors, spec distances)"""
    n = len(off) - 1
    qoff = np.concatenate([[0], np.cumsum([len(q) for q in qs])]).astype(np.int64)
    vd = _dev(values) if vd is None else vd
    qd = _dev(np.concatenate(qs)) if qd is None else qd
    rd = None if rid is None else _dev(rid)
    c0 = _counts(eng)
    ids, dists, surv = eng.multivec_topk_batch(vd, off, qd, qoff, k, metric, row_ids=rd, return_survivors=True, **rng)
    c1 = _counts(eng)
    ids, dists = ids.cpu().numpy().view(np.uint64), dists.cpu().numpy()
    want = [M.distances(oracle, values, off, q, metric) for q in qs]
    for b, q in enumerate(qs):
        if spec and not rng:
            oi, od = M.topk(want[b], k, rid)
            assert (ids[b] == oi).all(), (tag, "ids", b, ids[b][:8], oi[:8])
            assert spec == "ids" or (dists[b].view(np.uint32) == od.view(np.uint32)).all(), (tag, "dists", b)
        si, sd = eng.multivec_topk(vd, off, qd[int(qoff[b]):int(qoff[b + 1])], k, metric, row_ids=rd, **rng)
        assert (si.cpu().numpy().view(np.uint64) == ids[b]).all() and (sd.cpu().numpy().view(np.uint32) == dists[b].view(np.uint32)).all(), (tag, "single", b)
    if route == "filter":
        assert c1[0] > c0[0] and c1[1] == c0[1] and c1[2] == c0[2], (tag, c0, c1)
        degen = _degenerate_rows(values, off)
        for b, q in enumerate(qs):
            hi = B.superset_count(want[b], degen, k, B.margin(len(q), values.shape[1]))
            assert min(k, n) <= surv[b] <= hi, (tag, "survivors", b, int(surv[b]), hi)
    elif route == "loop":
        assert c1[1] == c0[1] + len(qs) and c1[2] == c0[2] and (surv == n).all(), (tag, c0, c1, surv)
    return ids, dists, surv, want


def _column(rows, lo, hi, d, seed, kind):
    return M.column(M.lengths(rows, lo, hi, seed), d, 1, seed, kind)[:2]


# ---- the filter route -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("d", [8, 20, 128, 136, 256])
def test_dimension(eng, oracle, kind, d):
    """d = 8 and 20 pad to K = 16 and 32, 128 fills its K, 136 pads to 256, 256 is the largest d served; 300 rows of 1..40 vectors,
    B = 2 (nqv = 5 and 32), permuted row ids"""
    values, off = _column(300, 1, 40, d, 100 + d, kind)
    _run(eng, oracle, values, off, B.queries([5, 32], d, 200 + d, kind), 10, rid=M.row_ids(300, d), tag=(kind, d))


def test_dimension_not_served_takes_the_loop(eng, oracle):
    values, off = _column(100, 1, 9, 260, 3, "f32")
    _run(eng, oracle, values, off, B.queries([4, 6], 260, 4), 10, route="loop")


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_query_vector_counts_mixed_in_one_batch(eng, oracle, kind):
    """nqv = 1, 5, 31, 32, 33, 64, 65 and 256 in one batch: queries that start and end inside a column block, one that fills a block
    exactly, and queries of 2, 3 and 8 pieces; k = 1 and 10"""
    values, off = _column(300, 1, 24, 20, 11, kind)
    qs = B.queries([1, 5, 31, 32, 33, 64, 65, 256], 20, 12, kind)
    for k in (1, 10):
        _run(eng, oracle, values, off, qs, k, rid=M.row_ids(300, 5), tag=(kind, k))


@pytest.mark.parametrize("nb", [1, 2, 7, 70])
def test_batch_sizes(eng, oracle, nb):
    """B = 1, 2, 7 and 70: the last is two chunks by the query count (64 + 6)"""
    values, off = _column(250, 1, 20, 16, 21, "f32")
    nqvs = [1 + (3 * i) % 9 for i in range(nb)]
    _run(eng, oracle, values, off, B.queries(nqvs, 16, 22), 5, tag=nb)


def test_two_chunks_by_columns(eng, oracle):
    """nine queries of 256 vectors: 2304 columns, the ninth query opens a second chunk"""
    values, off = _column(150, 1, 10, 8, 23, "f16")
    _run(eng, oracle, values, off, B.queries([256] * 9, 8, 24, "f16"), 5)


@pytest.mark.parametrize("kind,d", [("f32", 20), ("f16", 128)])
def test_row_length_boundaries(eng, oracle, kind, d):
    """rows of exactly 1, 2, 31, 32, 33, 64, 65, 200 and 1030 vectors among short ones (the boundary fixture of
    tests/test_zz_gpu_multivec.py::test_row_length_boundaries, with the 32-vector tile's own boundaries)"""
    rng = np.random.default_rng(77)
    lens = M.lengths(60, 1, 12, 5)
    lens[rng.permutation(60)[:18]] = [1, 2, 31, 32, 33, 64, 65, 200, 1030] * 2
    values, off, _ = M.column(lens, d, 1, 5000 + d, kind)
    _run(eng, oracle, values, off, B.queries([5, 33], d, 31, kind), 10, rid=M.row_ids(60, 8), tag=(kind, d))
    _run(eng, oracle, values, off, B.queries([5, 33], d, 31, kind), 60, rid=M.row_ids(60, 8), tag=(kind, d, 60))


def test_many_short_rows(eng, oracle):
    """5000 rows of 1..12 vectors: many units, several rows in every tile, the threshold taken in two rounds; k = 1, 10 and 1024"""
    values, off = _column(5000, 1, 12, 20, 6, "f32")
    qs = B.queries([6, 3], 20, 41)
    for k in (1, 10, 1024):
        _run(eng, oracle, values, off, qs, k, rid=M.row_ids(5000, 9), tag=k)


def test_k_above_the_row_count(eng, oracle):
    """k > n_rows: no threshold, every row is evaluated, the slots behind the rows are padding"""
    values, off = _column(40, 1, 9, 20, 51, "f32")
    ids, dists, surv, _ = _run(eng, oracle, values, off, B.queries([4, 7], 20, 52), 64)
    assert (ids[:, 40:] == U64_MAX).all() and np.isposinf(dists[:, 40:]).all() and (surv == 40).all()


def test_row_ids_above_2_32(eng, oracle):
    values, off = _column(200, 1, 9, 20, 61, "f32")
    rid = M.row_ids(200, 62) + np.uint64(1 << 33)
    _run(eng, oracle, values, off, B.queries([4, 7], 20, 63), 10, rid=rid)


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_pointers_off_the_16_byte_grid(eng, oracle, kind):
    """values and q are views that start 8 bytes into their buffers"""
    values, off = _column(150, 1, 9, 20, 71, kind)
    qs = B.queries([5, 9], 20, 72, kind)
    pad = 2 if kind == "f32" else 4
    vflat = _dev(np.concatenate([np.zeros(pad, values.dtype), values.reshape(-1)]))
    qflat = _dev(np.concatenate([np.zeros(pad, values.dtype), np.concatenate(qs).reshape(-1)]))
    vd, qd = vflat[pad:].reshape(-1, 20), qflat[pad:].reshape(-1, 20)
    assert vd.data_ptr() % 16 == 8 and qd.data_ptr() % 16 == 8 and vd.is_contiguous() and qd.is_contiguous()
    _run(eng, oracle, values, off, qs, 10, vd=vd, qd=qd, tag=kind)


def test_duplicated_row_straddling_k(eng, oracle):
    """seven copies of the row at the 10th distance, row ids permuted: the tie at position k goes by row id"""
    values, off = _column(300, 1, 20, 20, 81, "f32")
    qs = B.queries([6, 4], 20, 82)
    order = np.argsort(M.S.keys(M.distances(oracle, values, off, qs[0], "cosine")), kind="stable")
    src = [order[9]] * 7
    values = np.concatenate([values] + [values[off[r]:off[r + 1]] for r in src])
    off = M.offsets_of(np.concatenate([np.diff(off), [off[r + 1] - off[r] for r in src]]))
    for k in (8, 10, 12):
        _run(eng, oracle, values, off, qs, k, rid=M.row_ids(307, 13), tag=k)


def test_last_bit_neighbours_around_k(eng, oracle):
    """An all-positive column against an all-negative query: every similarity is negative, s lies in (-nqv, 0) and 1 - s rounds, so
    neighbouring f32 values occur.  48 copies of the row at the 10th distance with one component scaled by 1 + i 2^-21 sit around it:
    the specification has rows ONE ulp apart there (asserted), and the batch orders them as it does, for the k at and next to them"""
    values, off = _column(200, 1, 12, 20, 91, "f32")
    values = np.abs(values)
    qs = [-np.abs(q) for q in B.queries([6], 20, 92)]
    dist = M.distances(oracle, values, off, qs[0], "cosine")
    r = np.argsort(M.S.keys(dist), kind="stable")[9]
    row = values[off[r]:off[r + 1]]
    copies = []
    for i in range(48):
        c = row.copy()
        c[:, (7 * i) % 20] *= f32(1 + (i + 1) * 2.0 ** -21)
        copies.append(c)
    values = np.concatenate([values] + copies)
    off = M.offsets_of(np.concatenate([np.diff(off), [len(c) for c in copies]]))
    dist = M.distances(oracle, values, off, qs[0], "cosine")
    keys = np.sort(M.S.keys(dist))[:60].astype(np.int64)
    assert (np.diff(keys) == 1).any(), "the fixture holds no two rows one ulp apart"
    first = int(np.nonzero(np.diff(keys) == 1)[0][0])
    for k in (first + 1, first + 2, 10):
        _run(eng, oracle, values, off, qs, k, tag=k)


@pytest.mark.parametrize("scale", [2.0 ** -40, 2.0 ** 40])
def test_scaled_column(eng, oracle, scale):
    values, off = _column(200, 1, 12, 20, 95, "f32")
    _run(eng, oracle, (values * f32(scale)).astype(f32), off, B.queries([5, 8], 20, 96), 10, tag=scale)


# ---- degenerate inputs ----------------------------------------------------------------------------------------------------------
def _degenerate_column(which):
    lens = M.lengths(120, 2, 9, 31)
    values, off, _ = M.column(lens, 20, 1, 9000, "f32")
    rows = np.random.default_rng(3).permutation(120)[:8]
    for r in rows:
        if which == "zero":
            values[off[r] + 1] = 0
        elif which == "nan":
            values[off[r] + 1, 7] = np.nan
        elif which == "inf":
            values[off[r] + 1, 7] = np.inf
        else:                                   # a row of only such vectors
            values[off[r]:off[r + 1]] = 0
            values[off[r], 3] = np.nan
    return values, off, rows


@pytest.mark.parametrize("which", ["zero", "nan", "inf", "all"])
def test_degenerate_rows(eng, oracle, which):
    """a zero vector in a row, a NaN element, an inf element, a row of only such vectors: the rows survive the filter unconditionally and
    the exact arithmetic gives them the specification's bits; k = 10 and k = all the rows (the degenerate rows' own places).
    A ZERO vector's cosine is 0 / 0 and a vector with an inf element's is inf / inf: a NaN that the DIVISION makes, whose sign is the
    dividing machine's (x86, where the specification runs: -NaN, the minimum of the row's similarities, so the vector is as good as
    absent; this GPU: +NaN, the maximum, so the row scores NaN and sorts last -- exact.cuh's cosine_finish, and
    tests/test_zz_gpu_flat_wide.py::test_degenerate_rows for single-vector rows).  With k = 10 no such row is among the answers on
    either side and the bits are the specification's; with k = 120 the eight rows stand where their machine puts them (the
    specification: at their finite distances; the GPU, batch and single call alike: last), so those two calls are held to the
    single-query call alone.  A NaN ELEMENT is a NaN on every machine: `nan` and `all` are held to the specification at both k."""
    values, off, rows = _degenerate_column(which)
    assert _degenerate_rows(values, off)[rows].all()
    for k in (10, 120):
        _run(eng, oracle, values, off, B.queries([4, 7], 20, 97), k, rid=M.row_ids(120, 32), tag=(which, k),
             spec=not (which in ("zero", "inf") and k == 120))


def test_zero_query_vector_takes_the_loop(eng, oracle):
    """a query with a zero vector has no margin: it is answered by the loop, the other query of the batch by the filter.  Every
    distance of that query is 0 / 0 (the NaN's sign is the dividing machine's, test_degenerate_rows): its ids -- every row ties, so the
    lowest row ids -- are the specification's, its bits the single-query call's"""
    values, off = _column(150, 1, 9, 20, 98, "f32")
    qs = B.queries([4, 7], 20, 99)
    qs[1][2] = 0
    c0 = _counts(eng)
    _run(eng, oracle, values, off, qs[:1], 10)
    _, dists, surv, _ = _run(eng, oracle, values, off, qs, 10, route=None, spec="ids")
    c1 = _counts(eng)
    assert np.isnan(dists[1]).all() and np.isfinite(dists[0]).all()
    assert c1[0] > c0[0] and c1[1] == c0[1] + 1 and c1[2] == c0[2] and surv[1] == 150 and 10 <= surv[0] < 150


# ---- overflow -------------------------------------------------------------------------------------------------------------------
def test_overflow(eng, oracle):
    """2100 identical one-vector rows, d = 8: every row ties, every query's list overflows, the loop answers with the lowest row ids"""
    v = M.S.real_f32(1, 8, 1, 5)[0]
    values = np.repeat(v, 2100, 0)
    off = np.arange(2101, dtype=np.int64)
    qs = B.queries([3, 5], 8, 6)
    c0 = _counts(eng)
    ids, _, surv, _ = _run(eng, oracle, values, off, qs, 10, route=None)
    c1 = _counts(eng)
    assert c1[2] == c0[2] + 2 and c1[1] == c0[1] + 2 and (surv == 2100).all()
    assert (ids == np.arange(10, dtype=np.uint64)).all()


# ---- the loop -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", [("f32", "l2"), ("f32", "dot"), ("f16", "l2"), ("f16", "dot")])
def test_l2_and_dot_take_the_loop(eng, oracle, kind, metric):
    values, off = _column(200, 1, 12, 20, 111, kind)
    _run(eng, oracle, values, off, B.queries([5, 33, 1], 20, 112, kind), 10, metric=metric, rid=M.row_ids(200, 3), route="loop", tag=(kind, metric))


def test_ranged_cosine_batch_takes_the_loop(eng, oracle):
    """bounds that are returned distances: lower = the 3rd distance of query 0 (kept), upper = its 9th (left out)"""
    values, off = _column(200, 1, 12, 20, 121, "f32")
    qs = B.queries([5, 8], 20, 122)
    d0 = np.sort(M.distances(oracle, values, off, qs[0], "cosine"))
    lower, upper = float(d0[2]), float(d0[8])
    ids, dists, _, want = _run(eng, oracle, values, off, qs, 10, route="loop", lower=lower, upper=upper)
    for b in range(2):
        keep = (want[b] >= f32(lower)) & (want[b] < f32(upper))
        oi, od = M.topk(want[b][keep], 10, np.nonzero(keep)[0].astype(np.uint64))
        assert (ids[b] == oi).all() and (dists[b].view(np.uint32) == od.view(np.uint32)).all()
    assert (ids[0][:6] != U64_MAX).all() and (ids[0][6:] == U64_MAX).all()


@pytest.mark.parametrize("metric", ["cosine", "l2"])
def test_prefiltered_batch_through_the_public_function(eng, oracle, metric):
    """multivector_flat_knn with a list of queries, a prefilter and row ids: the sub-column is gathered once, the ids stay the table's"""
    import lance_amd
    values, off = _column(300, 1, 20, 20, 131, "f32")
    qs = B.queries([5, 9, 2], 20, 132)
    mask = np.random.default_rng(4).random(300) < 0.5
    rid = M.row_ids(300, 22)
    for ids_in in (None, rid):
        full = np.arange(300, dtype=np.uint64) if ids_in is None else ids_in
        gi, gd = lance_amd.multivector_flat_knn(values, off, qs, k=10, metric=metric, engine=eng, prefilter=mask, row_ids=ids_in)
        assert tuple(gi.shape) == (3, 10) and tuple(gd.shape) == (3, 10)
        for b, q in enumerate(qs):
            oi, od = M.topk(M.distances(oracle, values, off, q, metric)[mask], 10, full[mask])
            assert (gi[b].cpu().numpy().view(np.uint64) == oi).all() and (gd[b].cpu().numpy().view(np.uint32) == od.view(np.uint32)).all()
            si, sd = lance_amd.multivector_flat_knn(values, off, q, k=10, metric=metric, engine=eng, prefilter=mask, row_ids=ids_in)
            assert (si.cpu().numpy() == gi[b].cpu().numpy()).all() and (sd.cpu().numpy().view(np.uint32) == gd[b].cpu().numpy().view(np.uint32)).all()
    # a tuple of torch tensors, no prefilter, a range
    gi, gd = lance_amd.multivector_flat_knn(_dev(values), off, tuple(_dev(q) for q in qs), k=5, metric=metric, engine=eng, distance_range=(None, 1e9))
    for b, q in enumerate(qs):
        oi, od = M.topk(M.distances(oracle, values, off, q, metric), 5)
        assert (gi[b].cpu().numpy().view(np.uint64) == oi).all() and (gd[b].cpu().numpy().view(np.uint32) == od.view(np.uint32)).all()


# ---- the C boundary -------------------------------------------------------------------------------------------------------------
def test_c_boundary(oracle):
    """raw ctypes: NULLs, n_queries = 0 and 65536, bad q_offsets, k out of range, a zero-length row and decreasing offsets (refused
    through the flag word on the filter route and on the loop), n_rows = 0 (padding), survivors = NULL"""
    from lance_amd import _lib
    lib = _lib.load()
    values, off = _column(50, 1, 9, 20, 141, "f32")
    qs = B.queries([5, 3], 20, 142)
    qoff = np.array([0, 5, 8], np.uint64)
    k = 7
    ctx = C.c_void_p()
    assert lib.lance_hip_ctx_create(0, None, C.byref(ctx)) == 0
    held = []

    def dev(a):
        a = np.ascontiguousarray(a)
        p = C.c_void_p()
        assert lib.lance_hip_malloc(ctx, max(a.nbytes, 16), C.byref(p)) == 0
        assert lib.lance_hip_memcpy_h2d(ctx, p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
        held.append(p)
        return p

    def host(p, n, dtype):
        out = np.empty(n, dtype)
        assert lib.lance_hip_memcpy_d2h(ctx, out.ctypes.data_as(C.c_void_p), p, out.nbytes) == 0
        return out

    def call(metric=_lib.COSINE, vd=None, od=None, n=50, qd=None, qo=qoff, nq=2, kk=k, rng=(0, 0.0, 0, 0.0), ids=None, dists=None, surv=None):
        return lib.lance_hip_flat_multivec_topk_batch(ctx, _lib.F32, metric, vd, od, None, n, 20, qd, None if qo is None else qo.ctypes.data_as(C.c_void_p),
                                                      nq, kk, *rng, ids, dists, surv)
    try:
        vd, od, qd = dev(values), dev(off.astype(np.uint64)), dev(np.concatenate(qs))
        top_i, top_d = dev(np.zeros(2 * k, np.uint64)), dev(np.zeros(2 * k, f32))
        surv = np.zeros(2, np.uint32)
        ok = dict(vd=vd, od=od, qd=qd, ids=top_i, dists=top_d)
        for metric in (_lib.COSINE, _lib.DOT):
            name = "cosine" if metric == _lib.COSINE else "dot"
            for sv in (surv.ctypes.data_as(C.c_void_p), None):
                assert call(metric=metric, surv=sv, **ok) == 0, lib.lance_hip_last_error()
                gi, gd = host(top_i, 2 * k, np.uint64).reshape(2, k), host(top_d, 2 * k, np.uint32).reshape(2, k)
                for b in range(2):
                    oi, odd = M.topk(M.distances(oracle, values, off, qs[b], name), k)
                    assert (gi[b] == oi).all() and (gd[b] == odd.view(np.uint32)).all()
            assert (surv == 50).all() if metric == _lib.DOT else ((surv >= k) & (surv <= 50)).all()
        for missing in ("vd", "od", "qd", "ids", "dists"):
            assert call(**{**ok, missing: None}) == _lib.EINVAL and b"NULL" in lib.lance_hip_last_error()
        assert call(qo=None, **ok) == _lib.EINVAL and b"NULL" in lib.lance_hip_last_error()
        for nq in (0, 65536):
            assert call(nq=nq, qo=np.arange(65537, dtype=np.uint64), **ok) == _lib.EINVAL and b"1..65535" in lib.lance_hip_last_error()
        assert call(qo=np.array([0, 5, 5], np.uint64), **ok) == _lib.EINVAL and b"query 1 holds 0 vectors" in lib.lance_hip_last_error()
        assert call(qo=np.array([0, 5, 3], np.uint64), **ok) == _lib.EINVAL and b"decrease" in lib.lance_hip_last_error()
        assert call(qo=np.array([0, 5, 300], np.uint64), **ok) == _lib.EINVAL and b"1..256" in lib.lance_hip_last_error()
        for kk in (0, 1025):
            assert call(kk=kk, **ok) == _lib.EINVAL and b"k=" in lib.lance_hip_last_error()
        assert call(rng=(1, 2.0, 1, 1.0), **ok) == _lib.EINVAL and b"above the upper bound" in lib.lance_hip_last_error()
        empty = off.astype(np.uint64).copy(); empty[11] = empty[10]
        down = off.astype(np.uint64).copy(); down[11] = down[10] - 1
        for bad, word in ((empty, b"no vector"), (down, b"decrease")):
            bd = dev(bad)
            for metric in (_lib.COSINE, _lib.L2):
                assert call(metric=metric, **{**ok, "od": bd}) == _lib.EINVAL
                assert word in lib.lance_hip_last_error(), lib.lance_hip_last_error()
        # n_rows = 0: padding
        assert call(n=0, **ok) == 0, lib.lance_hip_last_error()
        assert (host(top_i, 2 * k, np.uint64) == U64_MAX).all() and np.isposinf(host(top_d, 2 * k, f32)).all()
        # and the context still answers
        assert call(surv=surv.ctypes.data_as(C.c_void_p), **ok) == 0
        oi, _ = M.topk(M.distances(oracle, values, off, qs[1], "cosine"), k)
        assert (host(top_i, 2 * k, np.uint64).reshape(2, k)[1] == oi).all()
    finally:
        for p in held:
            lib.lance_hip_free(ctx, p)
        lib.lance_hip_ctx_destroy(ctx)
