"""The CPU specification of the multivector distance (tests/multivec_spec.py) checked on itself, the host-side validation of the
multivector entry points, and the Arrow helper.  No GPU: the kernels are held to this specification bit for bit by
tests/test_zz_gpu_multivec.py."""
import numpy as np
import pytest

import multivec_spec as M

f32 = np.float32

# two rows of two and three 2-d vectors, a query of two vectors; every operation below is exact
HAND_Q = [[1, 0], [0, 2]]
HAND_VALUES = [[1, 0], [0, 1],                 # row 0
               [-2, 0], [0, -3], [2, 0]]       # row 1
HAND_OFFSETS = [0, 2, 5]
# l2 (squared):  row 0: q0 -> sims 1 - 0, 1 - 2: best 1;  q1 -> 1 - 5, 1 - 1: best 0;   s = 1,  1 - s = 0
#                row 1: q0 -> 1 - 9, 1 - 10, 1 - 1: best 0;  q1 -> 1 - 8, 1 - 25, 1 - 8: best -7;   s = -7,  1 - s = 8
# dot:           sim = 1 - (1 - dot) = dot.  row 0: q0 -> 1, 0: 1;  q1 -> 0, 2: 2;   s = 3,  1 - s = -2
#                row 1: q0 -> -2, 0, 2: 2;  q1 -> 0, -6, 0: 0;   s = 2,  1 - s = -1
# cosine:        sim = the cosine.  row 0: q0 -> 1, 0: 1;  q1 -> 0, 1: 1;   s = 2,  1 - s = -1
#                row 1: q0 -> -1, 0, 1: 1;  q1 -> 0, -1, 0: 0;   s = 1,  1 - s = 0       (not nqv - s = 1)
HAND_EXPECTED = {"l2": [0.0, 8.0], "dot": [-2.0, -1.0], "cosine": [-1.0, 0.0]}


@pytest.mark.parametrize("dtype", [np.float32, np.float16])
@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_hand_computed_case(oracle, metric, dtype):
    values, q = np.array(HAND_VALUES, dtype), np.array(HAND_Q, dtype)
    got = M.distances(oracle, values, HAND_OFFSETS, q, metric)
    assert got.dtype == f32 and got.tolist() == HAND_EXPECTED[metric]
    assert M.distances_per_pair(oracle, values, HAND_OFFSETS, q, metric).tolist() == HAND_EXPECTED[metric]
    ids, d = M.topk(got, 3)
    order = np.argsort(np.array(HAND_EXPECTED[metric]), kind="stable")
    assert ids.tolist() == order.tolist() + [0xFFFFFFFFFFFFFFFF] and d[:2].tolist() == sorted(HAND_EXPECTED[metric]) and np.isposinf(d[2])


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
@pytest.mark.parametrize("d", [8, 20, 40])
def test_batch_composition_equals_per_pair_composition(oracle, metric, kind, d):
    """the segmented composition over oracle.distance_batch is the pair-by-pair one over oracle.l2 / dot / cosine, bit for bit
    (d = 40 on f16: the 32-lane dot)"""
    values, off, q = M.column(M.lengths(12, 1, 6, d), d, 5, 100 + d, kind)
    a = M.distances(oracle, values, off, q, metric)
    b = M.distances_per_pair(oracle, values, off, q, metric)
    assert (a.view(np.uint32) == b.view(np.uint32)).all()


def test_fixture_sees_the_order_of_the_sum(oracle):
    """The sum of the maxima is order-dependent and the fixture must be able to show it: on 3000 rows (lengths 1..39, d = 128,
    nqv = 32, cosine, f32) a pairwise-tree sum of the same maxima gives other final bits than the sequential sum for 1835 rows
    (measured).  At least one tenth must differ: a condition that the fixture is not blind, not a tolerance.  (Sums of fewer than
    four terms cannot show the order; every order-sensitive GPU case has nqv >= 4.)"""
    values, off, q = M.column(M.lengths(3000, 1, 39, 7), 128, 32, 7, "f32")
    best = M.maxima(oracle, values, off, q, "cosine")
    seq, tree = f32(1) - M.sum_sequential(best), f32(1) - M.sum_pairwise(best)
    differ = int((seq.view(np.uint32) != tree.view(np.uint32)).sum())
    print("rows whose bits differ between the sequential and the pairwise sum:", differ, "of", seq.size)
    assert differ >= seq.size // 10
    for nqv in (1, 2, 3):      # up to three terms every order is the same order
        b = best[:nqv]
        assert (M.sum_sequential(b).view(np.uint32) == M.sum_pairwise(b).view(np.uint32)).all()


def test_nan_is_the_maximum_and_sorts_last(oracle):
    """f32::total_cmp makes the positive NaN the maximum of a row's similarities (fmaxf would drop it): a row whose second of three
    vectors holds one canonical np.nan scores NaN, positive, and sorts behind every other row, ties by row id"""
    lens = np.full(40, 3, np.int64)
    values, off, q = M.column(lens, 20, 4, 11, "f32")
    bad = [5, 17, 30]
    for r in bad:
        values[off[r] + 1, 7] = np.nan
    dist = M.distances(oracle, values, off, q, "l2")
    assert (dist[bad].view(np.uint32) == M.NAN_BITS).all()
    assert np.isfinite(np.delete(dist, bad)).all()
    rid = M.row_ids(40, 3)
    ids, d = M.topk(dist, 40, rid)
    assert (d[-3:].view(np.uint32) == M.NAN_BITS).all() and np.isfinite(d[:-3]).all() and (np.diff(d[:-3]) >= 0).all()
    assert ids[-3:].tolist() == sorted(int(x) for x in rid[bad])


# ---- host validation: every problem is a ValueError before any device call ------------------------------------------------------
def _good():
    values, off, q = M.column(np.array([2, 1, 3]), 8, 4, 5, "f32")
    return values, off, q


def _both(values, off, q, match, **kw):
    import lance_amd
    with pytest.raises(ValueError, match=match):
        lance_amd.multivector_flat_knn(values, off, q, k=2, **kw)
    kw.pop("prefilter", None); kw.pop("row_ids", None)
    with pytest.raises(ValueError, match=match):
        lance_amd.multivector_distance(values, off, q, **kw)


def test_validation_offsets():
    values, off, q = _good()
    _both(values, off + 1, q, "start at 0")
    _both(values, np.array([0, 4, 3, 6]), q, "decrease")
    _both(values, np.array([0, 2, 3, 5]), q, "end at len")
    _both(values, np.array([0, 2, 2, 6]), q, "row 1 is empty")
    _both(values, np.array([[0, 6]]), q, "1-D integer")
    _both(values, np.array([0.0, 6.0]), q, "1-D integer")


def test_validation_query_shape():
    values, off, q = _good()
    _both(values, off, q[:, :7], r"\[nqv\]\[d\] with d = 8")
    _both(values, off, q[0], r"\[nqv\]\[d\]")
    _both(values, off, q[:0], "no vector")
    _both(values.reshape(-1), off, q, "flattened")


def test_validation_dtype_and_metric():
    values, off, q = _good()
    for t in (np.int8, np.uint8):
        _both(values.astype(t), off, q.astype(t), f"unsupported multivector element type {np.dtype(t).name}")
    _both(values.astype(np.uint8), off, q.astype(np.uint8), "hamming", metric="hamming")
    _both(values, off, q, "hamming", metric="hamming")
    _both(values, off, q, "not supported", metric="manhattan")


def test_validation_query_vector_limit():
    from lance_amd import _lib
    values, off, _ = _good()
    limit = _lib.MULTIVEC_MAX_QUERY_VECTORS
    assert limit >= 256
    _both(values, off, np.zeros((limit + 1, 8), f32), f"above the limit of {limit}")


def test_validation_k_prefilter_row_ids():
    import lance_amd
    values, off, q = _good()
    for k in (0, 1025):
        with pytest.raises(ValueError, match="k="):
            lance_amd.multivector_flat_knn(values, off, q, k=k)
    with pytest.raises(ValueError, match="prefilter"):
        lance_amd.multivector_flat_knn(values, off, q, k=2, prefilter=np.ones(4, bool))
    with pytest.raises(ValueError, match="prefilter"):
        lance_amd.multivector_flat_knn(values, off, q, k=2, prefilter=np.ones(3, np.int32))
    with pytest.raises(ValueError, match="row_ids"):
        lance_amd.multivector_flat_knn(values, off, q, k=2, row_ids=np.arange(4, dtype=np.uint64))


def test_header_declares_the_limit():
    """the Python-side limit is the header's"""
    import os
    import re
    from lance_amd import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "lance_hip.h")).read()
    assert int(re.search(r"#define LANCE_HIP_MULTIVEC_MAX_QUERY_VECTORS (\d+)", hdr).group(1)) == _lib.MULTIVEC_MAX_QUERY_VECTORS
    for name in ("lance_hip_multivec_distance", "lance_hip_flat_multivec_topk"):
        assert name in _lib.SYMBOLS and re.search(r"\b%s\(" % name, hdr)


# ---- the Arrow helper -----------------------------------------------------------------------------------------------------------
def _arrow_column(values, off, large=False):
    import pyarrow as pa
    fsl = pa.FixedSizeListArray.from_arrays(pa.array(values.reshape(-1)), values.shape[1])
    if large:
        return pa.LargeListArray.from_arrays(pa.array(off.astype(np.int64)), fsl)
    return pa.ListArray.from_arrays(pa.array(off.astype(np.int32)), fsl)


@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_multivector_from_arrow(kind):
    import pyarrow as pa
    from lance_amd.arrow_io import multivector_from_arrow
    values, off, _ = M.column(np.array([2, 1, 3, 4, 1]), 6, 1, 9, kind)
    for large in (False, True):
        col = _arrow_column(values, off, large)
        v, o = multivector_from_arrow(col)
        assert v.dtype == values.dtype and v.shape == values.shape and (v == values).all()
        assert o.dtype == np.int64 and (o == off).all()
        # a slice: rows 1..3; the values are those rows' vectors, the offsets start at 0
        v, o = multivector_from_arrow(col.slice(1, 3))
        assert (v == values[off[1]:off[4]]).all() and (o == off[1:5] - off[1]).all()
        # chunks, the second one itself a slice
        v, o = multivector_from_arrow(pa.chunked_array([col.slice(0, 2), col.slice(2, 3)]))
        assert (v == values).all() and (o == off).all()


def test_multivector_from_arrow_refuses_nulls_and_other_types():
    import pyarrow as pa
    from lance_amd.arrow_io import multivector_from_arrow
    t = pa.list_(pa.list_(pa.float32(), 2))
    with pytest.raises(ValueError, match="null rows"):
        multivector_from_arrow(pa.array([[[1.0, 2.0]], None, [[3.0, 4.0], [5.0, 6.0]]], type=t))
    with pytest.raises(ValueError, match="null"):
        multivector_from_arrow(pa.array([[[1.0, 2.0]], [None, [5.0, 6.0]]], type=t))
    with pytest.raises(ValueError, match="unsupported multivector element type"):
        multivector_from_arrow(pa.array([[[1, 2]]], type=pa.list_(pa.list_(pa.uint8(), 2))))
    with pytest.raises(ValueError, match="List<FixedSizeList"):
        multivector_from_arrow(pa.array([[1.0, 2.0]], type=pa.list_(pa.float32(), 2)))
