"""CPU side of the large-column tests (tests/large_column_spec.py): at a scaled-down n, where the oracle can process the WHOLE materialised
column, the tiled expectation equals the oracle's output bit for bit for every transform of the table, and the planted-window expectation
equals the oracle's top k over the whole column, ids and distance bits, for every search of the table.  The conditions that make the
planted answer THE answer depend only on the base rows, the planted rows and the queries, not on n: they are asserted here for the
full-size parameters.  Last, the table's own arithmetic: every case's n really lies past the boundaries it claims."""
import os
import subprocess

import numpy as np
import pytest

import large_column_spec as L
import refine_spec
import rq_spec
import sq_spec

f32 = np.float32
K = 10
SEARCHES = [("f32-128", m, nq) for m in ("l2", "dot") for nq in (1, 4, 256)] + [("f32-256", m, nq) for m in ("l2", "dot", "cosine") for nq in (4, 256)] + \
           [("f16-128", "l2", nq) for nq in (1, 4, 256)] + [("f16-128", "dot", 4)] + [("i8-128", m, nq) for m in ("l2", "dot") for nq in (1, 4, 256)]
PER_ROW = [(name, op) for name in ("f32-128", "chunk-m96", "f16-128") for op in L.per_row_ops(L.Column.of_case(L.CASES[name]))]


def _rows(a):
    return a if a.dtype == np.float16 else a.astype(f32)


# ---- the table ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(L.CASES))
def test_case_table_arithmetic(name):
    c = L.CASES[name]
    es = L.ELEM[c.kind]
    assert c.n < 1 << 32
    assert c.column_bytes == c.n * c.d * es
    for what, value, unit, row in c.crosses:
        assert row + 1500 // 2 <= c.n - 3000, "no room for rows past the boundary ahead of the last window"
        if what == "bytes":
            assert unit == es and row * c.d * es == value, "the first byte of this row is the boundary"
            assert c.column_bytes > value
        elif what == "elements":
            assert row * c.d == value and c.n * c.d > value
        elif what == "copy":
            assert row * c.d * unit == value and c.n * c.d * unit > value, "the one-byte copy of the column passes the boundary at this row"
        else:
            m = {"chunk-m32": 32, "chunk-m96": 96}[name]
            assert row == 2 * L.chunk_rows(c.n, m) == value and c.n > row, "a third row chunk exists"
            assert L.chunk_rows(c.n, m) < c.n and L.chunk_rows(c.n, m) % 128 == 0
    assert c.need == sum(c.peak_of.values()) and c.peak_of["column"] == c.column_bytes
    assert c.need <= L.MEM_LIMIT, f"{c.need / L.GIB:.1f} GiB"
    col = L.refine_column(c) if name == "refine-raw" else L.Column.of_case(c)      # (asserts that the windows do not overlap)
    assert col.starts[0] == 0 and col.starts[-1] + col.sizes[-1] == c.n
    for b, s, w in zip(c.boundary_rows, col.starts[1:-1], col.sizes[1:-1]):
        assert s < b < s + w, "the window straddles the boundary row"


def test_chunk_counts_of_the_big_column():
    """the 5 and 9 row chunks the f32-128 column takes through the fused transform at M = 16 and M = 32"""
    n = L.CASES["f32-128"].n
    assert -(-n // L.chunk_rows(n, 16)) == 5 and -(-n // L.chunk_rows(n, 32)) == 9
    assert L.chunk_rows(1 << 30, 16) == 4194304 and L.chunk_rows(1 << 30, 32) == 2097152 and L.chunk_rows(1 << 30, 96) == 699008


def test_the_wide_plane_is_above_4_gib():
    c = L.CASES["f32-256"]
    assert c.n * c.d * 2 > 4 << 30


@pytest.mark.parametrize("kind,d", [("f32", 128), ("f32", 256), ("f32", 384), ("f16", 128), ("i8", 128)])
def test_a_wrapped_offset_lands_on_another_row(kind, d):
    """row r + 2^j / d (an offset that lost bit j) is another base row, and that row differs"""
    base = L.base_rows(kind, d)
    es = L.ELEM[kind]
    for j in range(24, 40):
        for unit in (1, es):                     # the lost bit counted in elements or in bytes
            if (1 << j) % (d * unit):
                continue
            shift = ((1 << j) // (d * unit)) % L.P
            assert shift != 0
            same = (base.view(f"u{es}") == np.roll(base, shift, axis=0).view(f"u{es}")).all(axis=1)
            assert same.sum() <= 2, "only the duplicated pair may meet itself"


def test_spoilers_are_in_the_base():
    b = L.base_rows("f32", 128)
    assert np.isnan(b[L.NAN_ROW]).all() and (b[L.ZERO_ROW] == 0).all() and (b[L.DUP_ROWS[0]] == b[L.DUP_ROWS[1]]).all()
    assert not np.isnan(L.base_rows("i8", 128).astype(f32)).any()


# ---- periodic column: per-row operations ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,op", PER_ROW)
def test_tiled_expectation_equals_the_oracle_on_the_whole_column(oracle, name, op):
    small = L.scaled_down(L.CASES[name])
    fn, _ = L.per_row_ops(small)[op]
    whole = fn(small.rows(0, small.n))
    exp = L.expected_rows(small, fn)
    assert len(whole) == len(exp)
    for w, (eb, ov) in zip(whole, exp):
        bad = np.nonzero(~L.same_bits(w, L.assemble(small.n, eb, ov)).reshape(small.n, -1).all(axis=1))[0]
        assert bad.size == 0, (name, op, "first differing row", bad[:1], "r mod P", bad[:1] % L.P)


def test_sq_distance_expectation_equals_the_spec_on_the_whole_column(oracle):
    small = L.scaled_down(L.CASES["sq-codes"])
    codes, bounds = L.sq_codes_of(small)
    q = L.queries(small, 2)
    for metric in ("l2", "dot"):
        fn = lambda c: (np.ascontiguousarray(sq_spec.distances(c, q, metric, *bounds).T),)
        whole = fn(codes.rows(0, codes.n))[0]
        (eb, ov), = L.expected_rows(codes, fn)
        assert L.same_bits(whole, L.assemble(codes.n, eb, ov)).all()


# ---- planted windows: searches ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,metric,nq", SEARCHES)
def test_planted_answer_equals_the_oracle_on_the_whole_column(oracle, name, metric, nq):
    small = L.scaled_down(L.CASES[name])
    q = L.queries(small, nq)
    pi, pd = L.planted_answer(small, q, K, metric)
    oi, od = oracle.flat_knn(_rows(small.rows(0, small.n)), _rows(q), K, metric)
    assert (oi == pi).all() and (od.view(np.uint32) == pd.view(np.uint32)).all()


@pytest.mark.parametrize("name,metric,nq", SEARCHES)
def test_conditions_hold_at_full_size(oracle, name, metric, nq):
    col = L.Column.of_case(L.CASES[name])
    oi, _ = L.planted_answer(col, L.queries(col, nq), K, metric)      # asserts the conditions
    for b in col.boundary_rows:
        assert (oi >= b).any(axis=1).all()
    assert ((oi >= col.last_window()).sum(axis=1) * 4 >= K).all()
    assert (oi < L.WIN).any() or metric != "dot", "under dot window 0 contributes as well: its rows must keep their own places"


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_last_list_answer_equals_the_search_of_the_whole_column(oracle, metric):
    """IVF_FLAT by position (list_ids): the last list is the last window, in order, and the queries probe it"""
    small = L.scaled_down(L.CASES["f32-128"])
    cent = L.list_centroids(small, L.NLIST)
    q = L.queries(small, 33)
    assert L.probes_last_list(q, cent, metric)
    offs, perm = oracle.partition_layout(L.list_ids(small, L.NLIST), L.NLIST)
    rows = perm[int(offs[L.NLIST - 1]):int(offs[L.NLIST])]
    lrows, lrid = L.last_list_rows(small)
    whole = small.rows(0, small.n)
    assert (rows == lrid.astype(np.int64)).all() and (whole[rows].view(np.uint32) == lrows.view(np.uint32)).all()
    allow = np.arange(len(lrid)) % 3 != 0
    for a in (None, allow):
        gi, gd = L.flat_list_answer(whole[rows], rows.astype(np.uint64), q, K, metric, a)
        ei, ed = L.flat_list_answer(lrows, lrid, q, K, metric, a)
        assert (gi == ei).all() and (gd.view(np.uint32) == ed.view(np.uint32)).all()
    assert L.probes_last_list(L.queries(L.Column.of_case(L.CASES["f32-128"]), 33), cent, metric)


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_sq_last_list_answer_equals_the_search_of_the_whole_column(oracle, metric):
    small = L.scaled_down(L.CASES["sq-codes"])
    codes, bounds = L.sq_codes_of(small)
    cent = L.list_centroids(small, L.NLIST)
    q = L.queries(small, 33)
    assert L.probes_last_list(q, cent, metric)
    whole = codes.rows(0, codes.n)
    lcodes, lrid = L.last_list_rows(codes)
    allow = np.arange(len(lrid)) % 3 != 0
    for a in (None, allow):
        pre = None
        if a is not None:
            pre = np.ones(small.n, bool)
            pre[lrid[~a].astype(np.int64)] = False
        oi, od = sq_spec.search(oracle, whole, L.list_ids(small, L.NLIST), cent, q, K, 1, metric, bounds[0], bounds[1], prefilter=pre)
        ei, ed = L.sq_list_answer(lcodes, lrid, cent, q, K, metric, bounds, a)
        assert (oi == ei).all() and (od.view(np.uint32) == ed.view(np.uint32)).all()
        assert (ei >= small.last_window()).all() and not np.isnan(ed).any()


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_rq_expectations_equal_the_spec_on_the_whole_column(oracle, metric):
    """rq_encode with lists by position, rq_distance (the last n % 32 rows take the f32 path) and the IVF_RQ search of the last list"""
    small = L.scaled_down(L.CASES["f32-128"])
    assert small.n % rq_spec.BATCH and L.CASES["f32-128"].n % rq_spec.BATCH
    outs, cent, rot = L.rq_expected(small, metric)
    whole = L.rq_encode_rows(small.rows(0, small.n), L.rq_lists(small), cent, rot, metric)
    for w, (eb, ov) in zip(whole, outs):
        assert L.same_bits(w, L.assemble(small.n, eb, ov)).all()
    q, qr = L.rq_queries(small, cent, 3)
    dqc = oracle.assign(q, np.ascontiguousarray(cent[1:2]), metric)[1]
    eb, ov = L.rq_distance_expected(small, outs, qr, dqc, rot, metric)
    part, _, codes, add, scale = whole
    dist = rq_spec.distances(codes, add, scale, qr, dqc, rot, metric, True)
    assert L.same_bits(dist.T, L.assemble(small.n, eb, ov)).all()
    q33 = L.queries(small, 33).astype(f32)
    assert L.probes_last_list(q33, cent, metric)
    keep = np.arange(L.LAST) % 3 != 0
    for a in (None, keep):
        pre = None
        if a is not None:
            pre = np.ones(small.n, bool)
            pre[small.pos[small.pstart[-2]:][~a].astype(np.int64)] = False
        oi, od = rq_spec.search(oracle, codes, add, scale, part, cent, rot, q33, K, 1, metric, prefilter=pre)
        ei, ed = L.rq_list_answer(small, outs, cent, rot, q33, K, metric, a)
        assert (oi == ei).all() and (od.view(np.uint32) == ed.view(np.uint32)).all()
        assert (ei >= small.last_window()).all() and not np.isnan(ed).any()


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_multivec_expectations_equal_the_spec_on_the_whole_column(oracle, metric):
    import multivec_spec
    small = L.scaled_down(L.CASES["f32-128"])
    off, R = L.multivec_offsets(small)
    q = L.multivec_query(small)
    eb, ov = L.multivec_expected(small, off, R, q, metric)
    whole = multivec_spec.distances(oracle, small.rows(0, small.n), off, q, metric)
    exp = np.array(eb[np.arange(len(off) - 1) % R])
    for r0, d_ in ov:
        exp[r0:r0 + len(d_)] = d_
    assert L.same_bits(whole, exp).all()
    ids, d_ = L.multivec_planted_answer(eb, ov, K)
    wi, wd = multivec_spec.topk(whole, K)
    assert (wi == ids).all() and (wd.view(np.uint32) == d_.view(np.uint32)).all()
    big = L.Column.of_case(L.CASES["f32-128"])                      # the conditions at full size (the offsets alone are 30 MB)
    boff, bR = L.multivec_offsets(big)
    assert boff[-1] == big.n and bR == R
    bi, _ = L.multivec_planted_answer(*L.multivec_expected(big, boff, bR, L.multivec_query(big), metric), K)
    assert (boff[bi.astype(np.int64)] >= big.boundary_rows[-1]).any()


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_refine_answer_conditions_and_the_whole_column(oracle, metric):
    """full size: the conditions (asserted by refine_answer).  Scaled down: the same answer with the WHOLE materialised column as the
    refine source and the positions as row ids"""
    case = L.CASES["refine-raw"]
    col = L.refine_column(case)
    assert sum(L.REFINE_SIZES[1:]) == 6000 and ((col.base >= 0) & (col.base <= 255) & (col.base == np.rint(col.base))).all()
    q = L.refine_queries(col, 64)
    for k, rf in ((10, 10), (13, 10)):
        L.refine_answer(col, q, k, rf, metric)
    n = 3 * L.P + 6000
    small = L.refine_column(case, n, [3000, 6001])
    x, pos = L.refine_index_rows(small)
    cent, cb = L.refine_models(case.d, metric)
    oi, od = oracle.build_index(x, cent, cb, metric, row_ids=pos).search(q, 10, L.REFINE_NLIST, refine=10, raw=small.rows(0, n))
    ei, ed = L.refine_answer(small, q, 10, 10, metric)
    assert (oi == ei).all() and (od.view(np.uint32) == ed.view(np.uint32)).all()
    # the IVF_SQ index over the same rows, refined from the same column
    L.sq_refine_answer(col, q, 10, 10, metric)
    codes, part, cent, bounds = L.sq_refine_index(small, metric)
    oi, od = refine_spec.sq_search_refine(oracle, codes, part, cent, q, 10, 10, L.REFINE_NLIST, metric, bounds[0], bounds[1], small.rows(0, n), row_ids=pos)
    ei, ed = L.sq_refine_answer(small, q, 10, 10, metric)
    assert (oi == ei).all() and (od.view(np.uint32) == ed.view(np.uint32)).all()


# ---- what the GPU run found: a launch of 2^32 work-items ---------------------------------------------------------------------------------
def test_grid_stride_launches_stay_below_2_32_work_items(tmp_path):
    """lance_amd/csrc/grid.h compiled alone (tests/c/grid_main.cpp): the gather of an IVF_SQ index over 2^25 + P rows asked for one thread
    per code byte, 2^32 + 524,800 work-items, and left the last list unwritten (tests/test_zz_gpu_large_columns.py::test_sq_codes_index)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "grid")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(root, "lance_amd", "csrc"), os.path.join(root, "tests", "c", "grid_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr
