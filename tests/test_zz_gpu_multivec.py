"""Multivector (late-interaction) flat KNN on the GPU (lance_amd/csrc/multivec.hip) against the CPU specification of
tests/multivec_spec.py, bit for bit: ids as uint64, distances as uint32.

The layout under test: one wave per row; the 64 lanes are 64 / QP sub-slices of QP lanes (QP = the power of two >= min(nqv, 64)),
lane (sub, qi) owns query vector qi and the row's vectors sub, sub + 64 / QP, ...; the row's vectors stream through a wave-private
LDS tile of at most 64 vectors (fewer when 4096 floats do not hold 64: 31 at d = 128); nqv > 64 runs passes of 64 query vectors; four
rows are in flight per workgroup and the waves stride over the rows once there are more than 16 rows per CU.  d in {8, 16, 32, 64, 96,
128} with nqv <= 64 takes the kernels that hold the query vector in registers, everything else the run-time-dimension kernel, and rows
too long for LDS (d > 9916) are read where they lie.  Every case is a few hundred short rows: the properties are those of the kernel's
index arithmetic and summation order, not of a workload.  Every order-sensitive case has nqv >= 4 (tests/test_multivec_spec.py).

Wall time on an MI355X: 66 tests in 3 s, the slowest 0.3 s."""
import ctypes as C

import numpy as np
import pytest

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


def _same_topk(got, want, tag):
    gi, gd = got
    oi, od = want
    assert (gi.cpu().numpy().view(np.uint64) == oi).all(), tag
    assert (gd.cpu().numpy().view(np.uint32) == od.view(np.uint32)).all(), tag


def _check(eng, oracle, values, off, q, metric, ks=(1, 10, 128), rid=None, tag=None):
    """the full [n_rows] output of multivec_distance and the top k for every k, against the specification; -> the spec's distances"""
    dist = M.distances(oracle, values, off, q, metric)
    vd, qd = _dev(values), _dev(q)
    got = eng.multivec_distance(vd, off, qd, metric).cpu().numpy()
    bad = np.nonzero(got.view(np.uint32) != dist.view(np.uint32))[0]
    assert bad.size == 0, (tag, metric, "rows that differ:", bad[:8], got[bad[:8]], dist[bad[:8]])
    rd = None if rid is None else _dev(rid)
    for k in ks:
        _same_topk(eng.multivec_topk(vd, off, qd, k, metric, row_ids=rd), M.topk(dist, k, rid), (tag, metric, k))
    return dist


# ---- dimension and metric -------------------------------------------------------------------------------------------------------
# f32: 3 = a tail only, 16 = no tail (and cosine_once), 20 = a group and a tail, 128 = a fixed-dimension kernel, 136 = full groups and a tail
# f16: the 32-lane dot starts above 16 (40 = one group of 32 and a tail of 8, 136 = four groups and a tail); 8 and 16 are fixed-dimension kernels
CASES = [("f32", m, d) for m in ("l2", "dot", "cosine") for d in (3, 16, 20, 128, 136)] + \
        [("f16", m, d) for m in ("l2", "dot", "cosine") for d in (8, 16, 40, 136)]


@pytest.mark.parametrize("kind,metric,d", CASES)
def test_dimension_and_metric(eng, oracle, kind, metric, d):
    """300 rows of 1..40 vectors, nqv = 5 (eight sub-slices of eight lanes, three of them idle), permuted row ids"""
    values, off, q = M.column(M.lengths(300, 1, 40, d), d, 5, 3000 + d, kind)
    _check(eng, oracle, values, off, q, metric, rid=M.row_ids(300, d), tag=(kind, d))


# ---- query-vector count ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nqv", [1, 2, 4, 31, 32, 33, 64, 65, 100, 256])
def test_query_vector_count(eng, oracle, nqv):
    """1, 2, 4: many sub-slices; 31 / 32 / 33: the half-wave boundary (QP = 32 -> 64); 64 / 65: the second pass; 100: two passes, the second
    partly filled; 256: the documented limit, four full passes.  d = 20 is the run-time-dimension kernel, d = 16 the register kernel up
    to nqv = 64 and the run-time one beyond."""
    for kind, metric, d in (("f32", "cosine", 20), ("f32", "l2", 16), ("f16", "dot", 40)):
        values, off, q = M.column(M.lengths(200, 1, 24, nqv), d, nqv, 4000 + nqv, kind)
        _check(eng, oracle, values, off, q, metric, ks=(10,), tag=(kind, d, nqv))


def test_query_vector_limit(eng):
    from lance_amd import _lib
    values, off, _ = M.column(np.array([2, 3]), 20, 1, 1)
    with pytest.raises(ValueError, match="above the limit"):
        eng.multivec_topk(_dev(values), off, _dev(np.zeros((_lib.MULTIVEC_MAX_QUERY_VECTORS + 1, 20), f32)), 1, "l2")


# ---- row lengths ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric,d,nqv", [("f32", "cosine", 20, 5), ("f32", "l2", 20, 64), ("f32", "dot", 128, 5), ("f16", "cosine", 128, 33),
                                               ("f16", "l2", 16, 4)])
def test_row_length_boundaries(eng, oracle, kind, metric, d, nqv):
    """Rows of exactly 1, 2, 63, 64, 65, 200 and 1030 vectors among short ones.  At d = 20 / 16 a tile holds 64 vectors: 1 and 2 leave most
    sub-slices without a vector (nqv = 5: eight sub-slices; nqv = 4: sixteen), 63 / 64 / 65 end just before, at and just after the first
    tile, 200 is three tiles and a part, 1030 sixteen tiles and six vectors.  At d = 128 a tile holds 31 vectors: the same lengths are 2, 2
    and 3 tiles, 6 tiles + 14 and 33 tiles + 7.  nqv = 64 is one sub-slice (a lane per query vector, every vector of the tile in turn),
    nqv = 33 one sub-slice with 31 lanes idle."""
    rng = np.random.default_rng(77)
    lens = M.lengths(60, 1, 12, 5)
    lens[rng.permutation(60)[:14]] = [1, 2, 63, 64, 65, 200, 1030, 1, 2, 63, 64, 65, 200, 1030]
    values, off, q = M.column(lens, d, nqv, 5000 + d + nqv, kind)
    _check(eng, oracle, values, off, q, metric, ks=(1, 10, 60), rid=M.row_ids(60, 8), tag=(kind, d, nqv))


def test_many_short_rows(eng, oracle):
    """5000 rows of 1..12 vectors, d = 20: four rows share a workgroup at any time (a wave each), and with more than 16 rows per CU of a
    256-CU device the waves take a second row (the grid-stride loop); k = 1024 is the selection's upper bound and takes three rounds"""
    values, off, q = M.column(M.lengths(5000, 1, 12, 6), 20, 6, 6000, "f32")
    _check(eng, oracle, values, off, q, "cosine", ks=(1, 10, 1024), rid=M.row_ids(5000, 9))


@pytest.mark.parametrize("kind,metric", [("f32", "l2"), ("f32", "cosine"), ("f16", "dot")])
def test_rows_too_long_for_lds(eng, oracle, kind, metric):
    """d = 10300: four tile rows no longer fit the LDS, the kernel reads the vectors where they lie, in the column's own element type"""
    values, off, q = M.column(np.array([1, 3, 2, 9, 1, 2]), 10300, 4, 6100, kind)
    _check(eng, oracle, values, off, q, metric, ks=(1, 6))


def test_unaligned_column(eng, oracle):
    """a column that does not start on a 16-byte boundary (a view into a larger buffer, 8 bytes in) is staged element by element, and a
    fixed-dimension shape (f16 d = 8) then takes the run-time-dimension kernel"""
    for d in (20, 8):
        values, off, q = M.column(M.lengths(100, 1, 9, d), d, 5, 6200 + d, "f16")
        dist = M.distances(oracle, values, off, q, "l2")
        flat = _dev(np.concatenate([np.zeros(4, np.float16), values.reshape(-1)]))
        view = flat[4:].reshape(-1, d)
        assert view.data_ptr() % 16 == 8 and view.is_contiguous()
        got = eng.multivec_distance(view, off, _dev(q), "l2").cpu().numpy()
        assert (got.view(np.uint32) == dist.view(np.uint32)).all()


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("d", [8, 32, 64, 96, 128])
def test_every_register_kernel(eng, oracle, kind, d):
    """the fixed dimensions the other cases leave out, every metric: 100 rows of 1..70 vectors (past one tile at every d), nqv = 6"""
    values, off, q = M.column(M.lengths(100, 1, 70, d), d, 6, 6300 + d, kind)
    for metric in ("l2", "dot", "cosine"):
        _check(eng, oracle, values, off, q, metric, ks=(10,), tag=(kind, d))


# ---- ties and ids ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_ties_are_decided_by_row_id(eng, oracle, metric):
    """twenty rows that are copies of the rows at the 1st, 10th and 128th distance (the only equal rows of the fixture), row ids
    permuted: whichever of the tied rows falls at the k-th place, the answer takes the smaller row ids"""
    d, nqv = 20, 6
    values, off, q = M.column(M.lengths(300, 1, 20, 12), d, nqv, 7000, "f32")
    order = np.argsort(M.S.keys(M.distances(oracle, values, off, q, metric)), kind="stable")
    src = [order[0]] * 7 + [order[9]] * 7 + [order[127]] * 6
    values = np.concatenate([values] + [values[off[r]:off[r + 1]] for r in src])
    off = M.offsets_of(np.concatenate([np.diff(off), [off[r + 1] - off[r] for r in src]]))
    rid = M.row_ids(320, 13)
    dist = _check(eng, oracle, values, off, q, metric, ks=(1, 3, 10, 20, 128, 140), rid=rid, tag="ties")
    for r in (order[0], order[9], order[127]):
        assert (dist.view(np.uint32) == dist.view(np.uint32)[r]).sum() in (7, 8)


# ---- prefilter ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_prefilter(eng, oracle, kind):
    """a mask over about half the rows and one over fewer than k: the scan covers the selected rows, the ids are those of the full
    table (the row index, or row_ids), and the slots beyond the selected rows hold id 2^64 - 1 and +inf as flat_knn's do"""
    import lance_amd
    values, off, q = M.column(M.lengths(300, 1, 20, 21), 20, 5, 8000, kind)
    dist = M.distances(oracle, values, off, q, "cosine")
    rng = np.random.default_rng(4)
    half = rng.random(300) < 0.5
    few = np.zeros(300, bool); few[rng.permutation(300)[:6]] = True
    rid = M.row_ids(300, 22)
    for mask in (half, few):
        for ids in (None, rid):
            full = np.arange(300, dtype=np.uint64) if ids is None else ids
            got = lance_amd.multivector_flat_knn(values, off, q, k=10, metric="cosine", engine=eng, prefilter=mask, row_ids=ids)
            want = M.topk(dist[mask], 10, full[mask])
            _same_topk(got, want, (kind, int(mask.sum()), ids is None))
    assert (want[0][6:] == U64_MAX).all() and np.isposinf(want[1][6:]).all()
    # no prefilter, through the same public function, and the distances of every row
    _same_topk(lance_amd.multivector_flat_knn(values, off, q, k=10, metric="cosine", engine=eng), M.topk(dist, 10), kind)
    got = lance_amd.multivector_distance(values, off, q, metric="cosine", engine=eng).cpu().numpy()
    assert (got.view(np.uint32) == dist.view(np.uint32)).all()


# ---- special values -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d", [("f32", 20), ("f32", 128), ("f16", 16)])
def test_special_values_l2(eng, oracle, kind, d):
    """l2 only, so that arithmetic generates no NaN.  Rows whose single vector has one +inf element: distance +inf, behind every finite
    row.  Rows of several vectors one of which has a +inf element: that vector can never be the maximum, the row stays finite.  Rows one
    of whose vectors holds a canonical np.nan: the positive NaN is the maximum under total_cmp, the row's distance is NaN, positive, and
    sorts last.  A plain call on a clean column follows on the same engine and is right as well."""
    rng = np.random.default_rng(31)
    lens = M.lengths(120, 2, 9, 31)
    p = rng.permutation(120)
    inf1, infn, nan = p[:10], p[10:20], p[20:30]
    lens[inf1] = 1
    values, off, q = M.column(lens, d, 4, 9000 + d, kind)
    values[off[inf1], rng.integers(0, d, 10)] = np.inf
    values[off[infn] + 1, rng.integers(0, d, 10)] = np.inf
    values[off[nan] + 1, rng.integers(0, d, 10)] = np.nan
    rid = M.row_ids(120, 32)
    dist = _check(eng, oracle, values, off, q, "l2", ks=(1, 10, 100, 120), rid=rid, tag=("special", kind, d))
    # the test's own expectation, on the specification's answer
    assert np.isposinf(dist[inf1]).all() and np.isfinite(dist[infn]).all() and (dist[nan].view(np.uint32) == M.NAN_BITS).all()
    assert np.isfinite(np.delete(dist, np.concatenate([inf1, nan]))).all()
    oi, od = M.topk(dist, 120, rid)
    assert np.isfinite(od[:100]).all() and np.isposinf(od[100:110]).all() and (od[110:].view(np.uint32) == M.NAN_BITS).all()
    assert oi[100:110].tolist() == sorted(int(x) for x in rid[inf1]) and oi[110:].tolist() == sorted(int(x) for x in rid[nan])
    values, off, q = M.column(M.lengths(120, 1, 9, 33), d, 4, 9100 + d, kind)
    _check(eng, oracle, values, off, q, "l2", ks=(10,), tag=("clean", kind, d))


# ---- the C entry points, no torch -----------------------------------------------------------------------------------------------
def test_c_entry_points_through_ctypes(oracle):
    """both exports driven through raw ctypes with device pointers from lance_hip_malloc / memcpy_h2d; a zero-length row and
    decreasing offsets are LANCE_HIP_EINVAL from both, int8 columns and too many query vectors are refused before any launch"""
    from lance_amd import _lib
    lib = _lib.load()
    values, off, q = M.column(M.lengths(50, 1, 9, 41), 20, 5, 9500, "f32")
    dist = M.distances(oracle, values, off, q, "dot")
    rid = M.row_ids(50, 42)
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

    try:
        vd, od, qd, rd = dev(values), dev(off.astype(np.uint64)), dev(q), dev(rid)
        out_d, top_i, top_d = dev(np.zeros(50, f32)), dev(np.zeros(k, np.uint64)), dev(np.zeros(k, f32))
        assert lib.lance_hip_multivec_distance(ctx, _lib.F32, _lib.DOT, vd, od, 50, 20, qd, 5, out_d) == 0, lib.lance_hip_last_error()
        assert (host(out_d, 50, np.uint32) == dist.view(np.uint32)).all()
        assert lib.lance_hip_flat_multivec_topk(ctx, _lib.F32, _lib.DOT, vd, od, rd, 50, 20, qd, 5, k, top_i, top_d) == 0, lib.lance_hip_last_error()
        oi, odd = M.topk(dist, k, rid)
        assert (host(top_i, k, np.uint64) == oi).all() and (host(top_d, k, np.uint32) == odd.view(np.uint32)).all()
        # row_ids NULL -> the row index
        assert lib.lance_hip_flat_multivec_topk(ctx, _lib.F32, _lib.DOT, vd, od, None, 50, 20, qd, 5, k, top_i, top_d) == 0
        assert (host(top_i, k, np.uint64) == M.topk(dist, k)[0]).all()
        # a zero-length row, decreasing offsets
        empty = off.astype(np.uint64).copy(); empty[11] = empty[10]
        down = off.astype(np.uint64).copy(); down[11] = down[10] - 1
        for bad, word in ((empty, b"no vector"), (down, b"decrease")):
            bd = dev(bad)
            assert lib.lance_hip_multivec_distance(ctx, _lib.F32, _lib.DOT, vd, bd, 50, 20, qd, 5, out_d) == _lib.EINVAL
            assert word in lib.lance_hip_last_error()
            assert lib.lance_hip_flat_multivec_topk(ctx, _lib.F32, _lib.DOT, vd, bd, rd, 50, 20, qd, 5, k, top_i, top_d) == _lib.EINVAL
            assert word in lib.lance_hip_last_error()
        assert lib.lance_hip_multivec_distance(ctx, _lib.I8, _lib.DOT, vd, od, 50, 20, qd, 5, out_d) == _lib.EINVAL
        assert b"int8" in lib.lance_hip_last_error()
        assert lib.lance_hip_multivec_distance(ctx, _lib.F32, _lib.DOT, vd, od, 50, 20, qd, _lib.MULTIVEC_MAX_QUERY_VECTORS + 1, out_d) == _lib.EINVAL
        assert lib.lance_hip_flat_multivec_topk(ctx, _lib.F32, _lib.DOT, vd, od, rd, 50, 20, qd, 5, 1025, top_i, top_d) == _lib.EINVAL
        # and the context still answers
        assert lib.lance_hip_multivec_distance(ctx, _lib.F32, _lib.DOT, vd, od, 50, 20, qd, 5, out_d) == 0
        assert (host(out_d, 50, np.uint32) == dist.view(np.uint32)).all()
    finally:
        for p in held:
            lib.lance_hip_free(ctx, p)
        lib.lance_hip_ctx_destroy(ctx)
