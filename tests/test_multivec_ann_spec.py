"""The specification of the multivector ANN search (tests/multivec_ann_spec.py) checked against itself on the CPU: the loop form against
a literal transcription of the reference's HashMap loop (knn.rs:1218-1298), the properties the GPU tests rely on (a fixture on which a
wrong list order or a tree sum changes bits, first occurrences, empty lists, ties), and the whole path end to end on a small column
whose candidate lists come from the oracle's IVF_PQ search over the flattened vectors with repeated row ids."""
import os
import re

import numpy as np
import pytest

import multivec_ann_spec as A
import multivec_spec as M
import oracle_engine as OE

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NONE = A.U64_MAX


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def lists_of(*ls, keff=None):
    ls = [(np.array(i, np.uint64), np.array(d, f32)) for i, d in ls]
    return A.pad_lists(ls, keff or max(1, max(len(i) for i, _ in ls)))


# ---- the formulation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", range(6))
def test_loop_form_equals_the_reference_loop(seed):
    """random lists with repeated rows, short and empty lists, in list order and in a shuffled one: identical rows and bits"""
    nqv = (1, 2, 7, 32, 5, 64)[seed]
    ids, dists = A.random_lists(nqv, 40, 90, seed=seed, id_base=(1 << 40), id_step=5, short=(0,) if nqv > 1 else (), empty=(1,) if nqv > 2 else ())
    for order in (None, list(np.random.default_rng(seed).permutation(nqv))):
        r1, d1 = A.scores(ids, dists, order)
        r2, d2 = A.reference_loop(ids, dists, order)
        assert (r1 == r2).all() and (bits(d1) == bits(d2)).all()


def test_order_fixture_discriminates():
    """32 lists x 100 candidates over 400 rows: taking the lists in reversed order, or adding a row's terms as a tree, changes the bits
    of many rows -- the GPU test on this fixture can see a wrong order"""
    ids, dists = A.order_fixture()
    rows, d = A.scores(ids, dists)
    rr, dr = A.scores(ids, dists, order=range(len(ids) - 1, -1, -1))
    rp, dp = A.scores_pairwise(ids, dists)
    assert (rows == rr).all() and (rows == rp).all() and rows.min() > (1 << 40)
    assert (bits(d) != bits(dr)).sum() >= 50 and (bits(d) != bits(dp)).sum() >= 50
    assert (ids[9] == NONE).all()                       # the empty list
    r2, d2 = A.reference_loop(ids, dists)
    assert (rows == r2).all() and (bits(d) == bits(d2)).all()


def test_duplicates_inside_a_list():
    """the FIRST occurrence in list order gives the row's sim; the last entry (a duplicate) still gives min_sim"""
    ids, dists = lists_of(([7, 9, 7, 9], [0.125, 0.25, 0.5, 0.75]), ([9, 9, 8], [0.1, 0.2, 0.3]), keff=4)
    rows, d = A.scores(ids, dists)
    assert rows.tolist() == [7, 8, 9]
    m0, m1 = f32(1) - f32(0.75), f32(1) - f32(0.3)
    want = {7: (f32(1) - f32(0.125)) + f32(0) + m1, 8: (f32(1) - f32(0.3)) + (f32(0) + m0), 9: ((f32(1) - f32(0.25)) + f32(0)) + (f32(1) - f32(0.1))}
    assert (bits(d) == bits([f32(2) - want[r] for r in (7, 8, 9)])).all()


def test_first_occurrence_is_by_list_position_not_distance():
    """a list out of distance order (not what a search returns): the entry EARLIEST in the list counts, as in the reference's loop"""
    ids, dists = lists_of(([4, 4], [0.6, 0.2]))
    _, d = A.scores(ids, dists)
    assert bits(d)[0] == bits([f32(1) - (f32(1) - f32(0.6))])[0]
    _, d2 = A.reference_loop(ids, dists)
    assert bits(d2)[0] == bits(d)[0]


def test_empty_list():
    """an empty list has min_sim 0: it adds +0 to every row and to missed"""
    full = ([3, 5], [0.25, 0.5])
    ids, dists = lists_of(full, ([], []), ([5], [0.125]))
    rows, d = A.scores(ids, dists)
    s3 = ((f32(0.75) + f32(0)) + f32(0)) + f32(0.875)
    s5 = ((f32(0.5) + f32(0)) + f32(0)) + f32(0.875)
    assert rows.tolist() == [3, 5] and (bits(d) == bits([f32(3) - s3, f32(3) - s5])).all()
    ids, dists = lists_of(([], []), ([], []), keff=3)
    rows, d = A.scores(ids, dists)
    assert rows.size == 0
    ti, td = A.topk(ids, dists, 4)
    assert (ti == NONE).all() and np.isinf(td).all()


def test_presence_patterns():
    """a row in every list, in exactly one (the middle), and only in the last"""
    l0 = ([1, 2], [0.1, 0.3])
    l1 = ([1, 3], [0.2, 0.6])
    l2 = ([1, 4], [0.05, 0.7])
    ids, dists = lists_of(l0, l1, l2)
    rows, d = A.scores(ids, dists)
    one = f32(1)
    m = [one - f32(0.3), one - f32(0.6), one - f32(0.7)]
    every = ((one - f32(0.1)) + f32(0)) + (one - f32(0.2)) + (one - f32(0.05))
    first_only = ((one - f32(0.3)) + f32(0)) + m[1] + m[2]
    middle = ((one - f32(0.6)) + (f32(0) + m[0])) + m[2]
    last = (one - f32(0.7)) + ((f32(0) + m[0]) + m[1])
    assert rows.tolist() == [1, 2, 3, 4]
    assert (bits(d) == bits([f32(3) - every, f32(3) - first_only, f32(3) - middle, f32(3) - last])).all()


def test_tie_is_broken_by_row_id():
    ids, dists = lists_of(([30, 10, 20], [0.25, 0.25, 0.25]))
    ti, td = A.topk(ids, dists, 2)
    assert ti.tolist() == [10, 20] and (bits(td) == bits([0.25, 0.25])).all()


# ---- end to end on a small column -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small(oracle):
    """600 rows x 4..12 vectors, d = 32, 8 partitions, M = 8; the flattened index through the device-index stand-in"""
    values, off, flat_rid = A.small_column("f32")
    cent, cb = A.train_model(oracle, values, 8, 8)
    o = oracle.build_index(values, cent, cb, "cosine", row_ids=flat_rid)
    ix = OE.OracleDeviceIndex.create(None, "cosine", cent, cb, o.part_ids, o.codes_rowmajor, flat_rid)
    return values, off, flat_rid, o, ix


def _query(values, nqv, seed):
    rng = np.random.default_rng(seed)
    base = values[rng.integers(0, len(values), nqv)].astype(f32)
    return (base + 0.3 * rng.standard_normal(base.shape).astype(f32)).astype(values.dtype)


def test_lists_come_with_repeated_row_ids(small):
    values, off, flat_rid, o, ix = small
    q = _query(values, 5, 17)
    ci, cd = ix.search(q, 100, 8)
    ci, cd = ci.numpy().view(np.uint64), cd.numpy()
    oi, od = A.candidate_lists(o, q, 100, 8)
    assert (ci == oi).all() and (bits(cd) == bits(od)).all()           # the stand-in and the oracle index agree: one definition of a list
    assert all(np.unique(l).size < l.size for l in ci) and ci.max() < 600
    assert (np.diff(M.S.keys(cd), axis=1) >= 0).all()


def test_every_row_in_every_list(small):
    """nprobes = nlist and keff >= the number of vectors: no imputation is left, the score is nqv - sum_j max_v (1 - pqdist(q_j, v)),
    the maxima added in query-vector order"""
    values, off, flat_rid, o, ix = small
    total = len(values)
    q = _query(values, 6, 23)
    ci, cd = A.candidate_lists(o, q, total, 8)
    assert (ci != NONE).all()
    rows, d = A.scores(ci, cd)
    assert rows.tolist() == list(range(600))
    s = np.zeros(600, f32)
    for j in range(6):
        best = np.full(600, -np.inf, f32)
        np.maximum.at(best, ci[j].astype(np.int64), f32(1) - cd[j])
        s = s + best
    assert (bits(d) == bits(f32(6) - s)).all()


def test_refine_over_all_rows_is_the_exact_answer(small, oracle):
    values, off, flat_rid, o, ix = small
    q = _query(values, 5, 31)
    total = len(values)
    gi, gd = A.ann_spec(oracle, o, values, off, q, 10, 8, overfetch=(total + 9) // 10, refine_factor=60)
    oi, od = M.topk(M.distances(oracle, values, off, q, "cosine"), 10, np.arange(600, dtype=np.uint64))
    assert (gi == oi).all() and (bits(gd) == bits(od)).all()


def test_prefilter_restricts_the_lists(small, oracle):
    values, off, flat_rid, o, ix = small
    q = _query(values, 5, 37)
    mask = np.random.default_rng(2).random(600) < 0.3
    for rf in (None, 5):
        gi, _ = A.ann_spec(oracle, o, values, off, q, 10, 8, refine_factor=rf, prefilter=mask)
        assert (gi != NONE).all() and mask[gi.astype(np.int64)].all()


# recall@10 of the specification against the exact flat answer, 20 queries of 8 vectors on clustered rows (600 rows, 8 partitions,
# nprobes = 2, overfetch 10), as the specification produces them here: a record, not a threshold -- the GPU must equal the specification
# bit for bit, so it has these recalls too
RECALL_NONE, RECALL_RF5 = 0.83, 0.985


def test_recall_record(oracle):
    values, off, flat_rid = A.small_column("f32", clustered=True, seed=21)
    cent, cb = A.train_model(oracle, values, 8, 8)
    o = oracle.build_index(values, cent, cb, "cosine", row_ids=flat_rid)
    hit = {None: 0, 5: 0}
    for i in range(20):
        r = int(np.random.default_rng(i).integers(0, 600))
        rows = values[off[r]:off[r + 1]]
        q = (rows[np.random.default_rng(i + 100).integers(0, len(rows), 8)] + 0.2 * np.random.default_rng(i + 200).standard_normal((8, 32))).astype(f32)
        exact, _ = M.topk(M.distances(oracle, values, off, q, "cosine"), 10, np.arange(600, dtype=np.uint64))
        for rf in hit:
            gi, _ = A.ann_spec(oracle, o, values, off, q, 10, 2, refine_factor=rf)
            hit[rf] += np.intersect1d(gi, exact).size
    got = (hit[None] / 200, hit[5] / 200)
    print("recall@10 without / with refine_factor = 5:", got)
    assert got == (RECALL_NONE, RECALL_RF5)


# ---- the boundary, without a device -------------------------------------------------------------------------------------------------
def test_entry_points_at_every_layer():
    """declared in include/lance_hip.h with the limits defined once, bound in lance_amd/_lib.py, declared in hip.rs, present on the Python
    surface and in the three documents"""
    import lance_amd
    from lance_amd import _lib, engine, vector
    read = lambda *p: open(os.path.join(ROOT, *p)).read()
    hdr, rs = read("include", "lance_hip.h"), read("integration", "rust", "lance-linalg", "src", "hip.rs")
    for name in ("lance_hip_multivec_xtr_score", "lance_hip_ivfpq_multivec_search"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\(" % name, hdr) and re.search(r"pub fn %s\(" % name, rs), name
        for doc in ("README.md", "DESIGN.md", "INTEGRATION.md"):
            assert name in read(doc), (name, doc)
    assert re.search(r"#define LANCE_HIP_MULTIVEC_ANN_MAX_KEFF 4096\b", hdr) and _lib.MULTIVEC_ANN_MAX_KEFF == A.MAX_KEFF == 4096
    assert re.search(r"#define LANCE_HIP_MULTIVEC_ANN_MAX_K_OUT 1024\b", hdr) and _lib.MULTIVEC_ANN_MAX_K_OUT == A.MAX_K_OUT == 1024
    assert _lib.MULTIVEC_MAX_QUERY_VECTORS == A.MAX_NQV
    src = read("lance_amd", "csrc", "multivec_ann.hip")
    assert "multivec_ann.hip" in read("lance_amd", "csrc", "Makefile") and "static_assert(MVA_MAX_NQV == LANCE_HIP_MULTIVEC_MAX_QUERY_VECTORS" in src
    assert callable(engine.Engine.multivec_xtr_score) and callable(engine.DeviceIndex.multivec_search)
    assert lance_amd.create_multivector_index is vector.create_multivector_index and lance_amd.IvfPqMultivectorIndex is vector.IvfPqMultivectorIndex


def test_argument_rules_need_no_device():
    """every refusal of create_multivector_index and of the size limits is raised before any device work"""
    import lance_amd
    from lance_amd.engine import check_multivector_ann_sizes, check_query_offsets
    v = np.zeros((4, 8), f32)
    for metric in ("l2", "dot", "euclidean"):
        with pytest.raises(ValueError, match="multivector type supports only cosine distance"):
            lance_amd.create_multivector_index(v, [0, 2, 4], metric=metric)
    with pytest.raises(ValueError, match="unsupported multivector element type int8"):
        lance_amd.create_multivector_index(v.astype(np.int8), [0, 2, 4])
    with pytest.raises(ValueError, match="null rows"):
        lance_amd.create_multivector_index(v, None)
    with pytest.raises(ValueError, match="end at len"):
        lance_amd.create_multivector_index(v, [0, 2, 5])
    with pytest.raises(ValueError, match=r"1\.\.4096"):
        check_multivector_ann_sizes(4097, 1)
    with pytest.raises(ValueError, match=r"1\.\.1024"):
        check_multivector_ann_sizes(10, 1025)
    with pytest.raises(ValueError, match="above the limit of 256"):
        check_query_offsets([0, 3, 260])
    assert check_query_offsets([0, 3, 259]).dtype == np.uint64
