"""Multivector ANN search on the GPU (lance_amd/csrc/multivec_ann.hip behind lance_hip_multivec_xtr_score /
lance_hip_ivfpq_multivec_search, create_multivector_index(...).nearest(...)) against the CPU specification of
tests/multivec_ann_spec.py, bit for bit: ids as uint64, distances as uint32.

The kernels under test: one workgroup per candidate list sorts a copy by (row id, position) in LDS (power-of-two padding: keff = 257
sorts 512 slots, 4096 is the largest list); one workgroup per list scores the rows it owns with one binary search per other list
(nqv = 65: one list more than a wave has lanes; 256: the limit); a batched block sort of 2048 candidates selects the k_out best
(8 x 4096 candidates: sixteen blocks, two rounds).  The end-to-end cases are 600 rows of 4..12 vectors, d = 32, 8 partitions, M = 8:
the candidate lists are those of the oracle's IVF_PQ search over the flattened index, repeated row ids included."""
import numpy as np
import pytest

import multivec_ann_spec as A
import multivec_spec as M

pytestmark = pytest.mark.gpu
f32 = np.float32
BIG = 1 << 40


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _score(eng, ids, dists, q_offsets, k_out):
    gi, gd = eng.multivec_xtr_score(ids, dists, q_offsets, k_out)
    return gi.cpu().numpy().view(np.uint64), gd.cpu().numpy()


def _check_score(eng, ids, dists, q_offsets, k_out, tag=None):
    gi, gd = _score(eng, ids, dists, q_offsets, k_out)
    for b in range(len(q_offsets) - 1):
        sl = slice(int(q_offsets[b]), int(q_offsets[b + 1]))
        oi, od = A.topk(ids[sl], dists[sl], k_out)
        assert (gi[b] == oi).all(), (tag, b, np.argwhere(gi[b] != oi)[:4])
        assert (gd[b].view(np.uint32) == od.view(np.uint32)).all(), (tag, b)
    return gi, gd


# ---- the join and score stage on synthetic lists ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nqv", [1, 5, 32, 65, 256])
@pytest.mark.parametrize("keff", [10, 100, 257])
def test_xtr_score(eng, nqv, keff):
    """rows fewer than entries (a row recurs inside a list and across lists), two short lists and an empty one, row ids >= 2^40"""
    short = () if nqv < 5 else (1, nqv - 1)
    ids, dists = A.random_lists(nqv, keff, max(30, nqv * keff // 6), seed=nqv * 1000 + keff, id_base=BIG + 5, id_step=3, short=short,
                                empty=(3,) if nqv >= 5 else ())
    _check_score(eng, ids, dists, [0, nqv], 10, (nqv, keff))
    _check_score(eng, ids, dists, [0, nqv], 1024, (nqv, keff, "all"))


def test_xtr_score_largest_list(eng):
    """keff = 4096, nqv = 8: 48 KiB of LDS in the sort; 32768 candidates over 20000 rows: sixteen selection blocks"""
    ids, dists = A.random_lists(8, 4096, 20000, seed=77, id_base=BIG, id_step=7, short=(2,), dup=0.1)
    _check_score(eng, ids, dists, [0, 8], 1024)
    _check_score(eng, ids, dists, [0, 8], 10)


def test_xtr_score_batch(eng):
    """three queries of 1, 5 and 32 vectors in one call equal the same queries one by one; the first joins fewer rows than k_out"""
    parts = [A.random_lists(n, 100, rows, seed=40 + n, id_base=BIG, short=(0,)) for n, rows in ((1, 20), (5, 300), (32, 900))]
    ids, dists = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    gi, gd = _check_score(eng, ids, dists, [0, 1, 6, 38], 40)
    assert (gi[0] == A.U64_MAX).any() and np.isinf(gd[0][gi[0] == A.U64_MAX]).all()
    for b, (pi, pd) in enumerate(parts):
        oi, od = _score(eng, pi, pd, [0, len(pi)], 40)
        assert (oi[0] == gi[b]).all() and (od[0].view(np.uint32) == gd[b].view(np.uint32)).all()


def test_xtr_score_empty_lists(eng):
    """every list empty: nothing is joined, the answer is padding"""
    ids, dists = A.pad_lists([(np.empty(0, np.uint64), np.empty(0, f32))] * 3, 16)
    gi, gd = _score(eng, ids, dists, [0, 3], 5)
    assert (gi == A.U64_MAX).all() and np.isinf(gd).all()


def test_xtr_score_order_fixture(eng):
    """the fixture on which another summation order changes bits (tests/test_multivec_ann_spec.py asserts that it does)"""
    ids, dists = A.order_fixture()
    _check_score(eng, ids, dists, [0, len(ids)], 400)


def test_xtr_score_refusals(eng):
    ids, dists = A.random_lists(2, 8, 20, seed=1)
    with pytest.raises(ValueError, match="above the limit of 256"):
        eng.multivec_xtr_score(np.zeros((257, 4), np.uint64), np.zeros((257, 4), f32), [0, 257], 1)
    with pytest.raises(ValueError, match="holds no vector"):
        eng.multivec_xtr_score(ids, dists, [0, 0, 2], 1)
    with pytest.raises(ValueError, match=r"keff = k \* overfetch = 4097 .*1\.\.4096"):
        eng.multivec_xtr_score(np.zeros((1, 4097), np.uint64), np.zeros((1, 4097), f32), [0, 1], 1)
    with pytest.raises(ValueError, match=r"k_out = k \* refine_factor = 1025 .*1\.\.1024"):
        eng.multivec_xtr_score(ids, dists, [0, 2], 1025)
    with pytest.raises(ValueError, match="one list per query vector"):
        eng.multivec_xtr_score(ids, dists, [0, 3], 1)


def test_c_abi_refusals(eng):
    """the same limits at the C boundary, each with a message naming it"""
    import ctypes as C
    import lance_amd.engine as E
    from lance_amd._lib import LanceHipError, check
    ids, dists = A.random_lists(2, 8, 20, seed=1)
    di, dd = E.to_device(ids), E.to_device(dists)
    oi, od = E.to_device(np.zeros((1, 2048), np.int64)), E.to_device(np.zeros((1, 2048), f32))

    def call(off, keff, k_out):
        off = np.asarray(off, np.uint64)
        check(eng.lib.lance_hip_multivec_xtr_score(eng.h, E._ptr(di), E._ptr(dd), off.ctypes.data_as(C.c_void_p), len(off) - 1, keff, k_out,
                                                   E._ptr(oi), E._ptr(od)))
    for off, keff, k_out, msg in (([0, 257], 8, 1, "1..256 vectors"), ([0, 0], 8, 1, "1..256 vectors"), ([0, 2], 4097, 1, r"1\.\.4096"),
                                  ([0, 2], 0, 1, r"1\.\.4096"), ([0, 2], 8, 1025, r"1\.\.1024"), ([0, 2], 8, 0, r"1\.\.1024"),
                                  ([1, 2], 8, 1, "start at 0")):
        with pytest.raises(LanceHipError, match=msg):
            call(off, keff, k_out)
    call([0, 2], 8, 4)       # and the same buffers are accepted within the limits


# ---- nearest, end to end ----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module", params=["f32", "f16"])
def built(request, engine, oracle):
    kind = request.param
    values, off, flat_rid = A.small_column(kind)
    idx = engine.create_multivector_index(values, off, num_partitions=8, num_sub_vectors=8, max_iters=8)
    oidx = oracle.build_index(values, idx.centroids, idx.codebook, "cosine", row_ids=flat_rid)
    yield kind, values, off, idx, oidx
    idx.close()


def _query(values, nqv, seed):
    rng = np.random.default_rng(seed)
    base = values[rng.integers(0, len(values), nqv)].astype(f32)
    return (base + 0.3 * rng.standard_normal(base.shape).astype(f32)).astype(values.dtype)


@pytest.mark.parametrize("nqv", [1, 5, 32])
@pytest.mark.parametrize("nprobes", [1, 8])
def test_nearest(built, oracle, nqv, nprobes):
    """k = 10 with and without a prefilter, refine_factor None / 1 / 5: ids and distance bits equal the specification"""
    kind, values, off, idx, oidx = built
    q = _query(values, nqv, 900 + nqv)
    mask = np.random.default_rng(nqv).random(len(off) - 1) < 0.5
    for pre in (None, mask):
        for rf in (None, 1, 5):
            gi, gd = idx.nearest(q, k=10, nprobes=nprobes, refine_factor=rf, prefilter=pre)
            oi, od = A.ann_spec(oracle, oidx, values, off, q, 10, nprobes, refine_factor=rf, prefilter=pre)
            tag = (kind, nqv, nprobes, rf, pre is not None)
            assert (gi == oi).all(), (tag, gi, oi)
            assert (gd.view(np.uint32) == od.view(np.uint32)).all(), (tag, gd, od)
            if pre is not None:
                assert mask[gi[gi != A.U64_MAX].astype(np.int64)].all(), tag


def test_candidate_lists(built):
    """what the join is fed: the index's own search with k = keff over the flattened vectors equals the oracle's, repeated row ids
    included (several vectors of a row are found by one query vector)"""
    kind, values, off, idx, oidx = built
    q = _query(values, 5, 17)
    gi, gd = idx._ix.search(q, 100, 8)
    oi, od = A.candidate_lists(oidx, q, 100, 8)
    gi = gi.cpu().numpy().view(np.uint64)
    assert (gi == oi).all() and (gd.cpu().numpy().view(np.uint32) == od.view(np.uint32)).all()
    assert any(np.unique(l[l != A.U64_MAX]).size < (l != A.U64_MAX).sum() for l in gi), "no row id recurs in a list: the fixture is too easy"


def test_batch_equals_one_by_one(built):
    kind, values, off, idx, oidx = built
    qs = [_query(values, n, 50 + n) for n in (3, 32, 1, 7)]
    for rf in (None, 5):
        bi, bd = idx.nearest(qs, k=10, nprobes=4, refine_factor=rf)
        assert bi.shape == (4, 10)
        for b, q in enumerate(qs):
            gi, gd = idx.nearest(q, k=10, nprobes=4, refine_factor=rf)
            assert (bi[b] == gi).all() and (bd[b].view(np.uint32) == gd.view(np.uint32)).all(), (rf, b)


def test_zero_query_vector_completes(built):
    """an all-zero query vector makes its list's distances NaN: outside the parity statement, but the call completes and returns rows"""
    kind, values, off, idx, oidx = built
    q = _query(values, 4, 3)
    q[2] = 0
    gi, gd = idx.nearest(q, k=10, nprobes=8)
    assert gi.shape == (10,) and (gi != A.U64_MAX).any()


def test_empty_rows_are_allowed(engine, oracle):
    """rows without vectors contribute nothing to the index and are never returned"""
    values, off, _ = A.small_column("f32", n_rows=200, seed=9)
    lens = np.diff(off)
    lens2 = np.insert(lens, [0, 50, 200], 0)                      # three empty rows, the first and the last among them
    off2 = M.offsets_of(lens2)
    idx = engine.create_multivector_index(values, off2, num_partitions=4, num_sub_vectors=8, max_iters=6)
    rid = np.repeat(np.arange(len(lens2), dtype=np.uint64), lens2)
    oidx = oracle.build_index(values, idx.centroids, idx.codebook, "cosine", row_ids=rid)
    q = _query(values, 5, 4)
    for rf in (None, 5):
        gi, gd = idx.nearest(q, k=10, nprobes=4, refine_factor=rf)
        oi, od = A.ann_spec(oracle, oidx, values, off2, q, 10, 4, refine_factor=rf)
        assert (gi == oi).all() and (gd.view(np.uint32) == od.view(np.uint32)).all()
        assert (lens2[gi.astype(np.int64)] > 0).all()
    idx.close()


def test_refusals(built, engine):
    kind, values, off, idx, oidx = built
    q = _query(values, 3, 1)
    for metric in ("l2", "dot", "euclidean"):
        with pytest.raises(ValueError, match="multivector type supports only cosine distance"):
            engine.create_multivector_index(values, off, metric=metric, num_partitions=8, num_sub_vectors=8)
    with pytest.raises(ValueError, match="unsupported multivector element type int8"):
        engine.create_multivector_index(np.zeros((4, 8), np.int8), [0, 2, 4], num_partitions=2, num_sub_vectors=2)
    with pytest.raises(ValueError, match="null rows"):
        engine.create_multivector_index(values, None, num_partitions=8, num_sub_vectors=8)
    with pytest.raises(ValueError, match="above the limit of 256"):
        idx.nearest(_query(values, 257, 2))
    with pytest.raises(ValueError, match="holds no vector"):
        idx.nearest(q[:0])
    with pytest.raises(ValueError, match=r"keff = k \* overfetch = 4100 .*1\.\.4096"):
        idx.nearest(q, k=410, overfetch=10)
    with pytest.raises(ValueError, match=r"k_out = k \* refine_factor = 1030 .*1\.\.1024"):
        idx.nearest(q, k=103, overfetch=2, refine_factor=10)
    with pytest.raises(ValueError, match="Refine factor cannot be zero"):
        idx.nearest(q, refine_factor=0)
    for name, val in (("distance_range", (0.0, 1.0)), ("minimum_nprobes", 2), ("maximum_nprobes", 4)):
        with pytest.raises(NotImplementedError, match=name):
            idx.nearest(q, **{name: val})
    with pytest.raises(ValueError, match="prefilter must be a boolean array over the 600 rows"):
        idx.nearest(q, prefilter=np.ones(5, bool))
    # the C entry point refuses an index of another metric with the reference's words
    from lance_amd._lib import LanceHipError
    l2 = engine.create_index(values, "IVF_PQ", metric="l2", num_partitions=8, num_sub_vectors=8, max_iters=4)
    with pytest.raises(LanceHipError, match="multivector type supports only cosine distance"):
        l2._ix.multivec_search(q, [0, 3], 10, 1)
