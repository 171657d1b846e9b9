"""Columns past 2^31 elements and 4 GiB on the row-indexed kernels (tests/large_column_spec.py has the construction and the table).

Every case builds its column ON THE DEVICE (base.repeat(...)[:n] with the planted windows written over it), calls the entry point with
device tensors -- engine.py passes a contiguous CUDA tensor through without a copy --, compares the WHOLE output on the device against
the oracle's output for the base and planted rows, tiled the same way (bit for bit; first differing row and its r mod P reported), and
copies back only k-sized answers.  Searches are compared with the oracle's answer over the planted rows alone, ids and distance bits.
Routes that have a `count:<stage>` counter are asserted, so that a case cannot pass on a fallback kernel.

Memory: one column is alive at a time (`_column` releases the previous one: f32-128, then the chunk columns, f32-256, f16-128, i8-128,
sq-codes), every case runs on an Engine of its own that is closed with the case (the context's scratch arena goes with it), and no case
may hold more than 24 GiB: torch's share is asserted against the table's figure through torch.cuda.max_memory_allocated(), the device's
(arena included) through mem_get_info.  A case skips, with both numbers, if less than its need + 4 GiB is free.  Nothing above a few MB
lives on the host.

Wall time and peak memory per test on an MI355X: DESIGN.md section 3b."""
import contextlib
import time

import numpy as np
import pytest
import torch

import large_column_spec as L

pytestmark = pytest.mark.gpu
f32 = np.float32
K = 10
P = L.P
_LIVE = {}


# ---- memory discipline -----------------------------------------------------------------------------------------------------------------
def _release():
    for _, t, _ in _LIVE.values():
        t.untyped_storage().resize_(0)      # (a failed test's traceback may still hold the tensor: its memory goes back all the same)
    _LIVE.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


@pytest.fixture(scope="module", autouse=True)
def _finaliser():
    yield
    _release()


def _column(name):
    """(spec column, device tensor) of a table row: built once, shared by the row's cases, released before the next row's is built"""
    if name not in _LIVE:
        _release()
        case = L.CASES[name]
        free, _ = torch.cuda.mem_get_info()
        if free < case.need + L.FREE_MARGIN:
            pytest.skip(f"{name}: {free} bytes free on the device, the case needs {case.need} + {L.FREE_MARGIN}")
        col = L.refine_column(case) if name == "refine-raw" else L.Column.of_case(case)
        if case.kind == "u8":
            codes, bounds = L.sq_codes_of(col)
            _LIVE[name] = (codes, codes.device(torch), dict(raw=col, bounds=bounds))
        else:
            _LIVE[name] = (col, col.device(torch), {})
        assert _LIVE[name][1].shape == (case.n, case.d) and _LIVE[name][1].numel() * _LIVE[name][1].element_size() == case.column_bytes
    return _LIVE[name]


@contextlib.contextmanager
def held(name):
    """one case: the row's column, a fresh Engine, the memory checks of the module docstring"""
    from lance_amd.engine import Engine
    case = L.CASES[name]
    col, dev, extra = _column(name)
    torch.cuda.synchronize()
    free, _ = torch.cuda.mem_get_info()
    rest = case.need - case.column_bytes
    if free < rest + L.FREE_MARGIN:
        pytest.skip(f"{name}: {free} bytes free on the device beside the column, the case needs {rest} + {L.FREE_MARGIN}")
    torch.cuda.reset_peak_memory_stats()
    eng = Engine()
    t0 = time.perf_counter()
    st = dict(extra, held=0, free0=free)
    try:
        yield col, dev, eng, st
    finally:
        torch.cuda.synchronize()
        st["held"] = max(st["held"], free - torch.cuda.mem_get_info()[0])      # tensors still alive + the context's arena
        eng.close()
        peak = torch.cuda.max_memory_allocated()
        torch.cuda.empty_cache()
        print(f"[large-column] {name}: {time.perf_counter() - t0:.2f} s, torch peak {peak / L.GIB:.2f} GiB, "
              f"device beside the column {st['held'] / L.GIB:.2f} GiB, table {case.need / L.GIB:.2f} GiB")
    assert peak <= case.need, f"torch held {peak} bytes at its peak, the table says {case.need}"
    assert case.column_bytes + st["held"] <= L.MEM_LIMIT, f"{case.column_bytes + st['held']} bytes on the device"


class counted:
    """the stage counter moves inside the block"""

    def __init__(self, eng, stage):
        self.eng, self.stage = eng, stage

    def __enter__(self):
        self.before = self.eng.timing_query("count:" + self.stage)[1]

    def __exit__(self, *a):
        if a[0] is None:
            assert self.eng.timing_query("count:" + self.stage)[1] > self.before, f"the {self.stage} stage did not serve this call"


# ---- whole-output comparison on the device -----------------------------------------------------------------------------------------------
def _bits(t):
    if t.dtype == torch.float32:
        return t.view(torch.int32)
    if t.dtype == torch.float16:
        return t.view(torch.int16)
    return t


def _dev(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def _row_diff(got, exp):
    """[rows] bool: the row differs in some bit (two NaNs count as equal: a NaN's sign and payload belong to the machine that made it)"""
    g, e = got.reshape(got.shape[0], -1), exp.reshape(exp.shape[0], -1)
    assert g.dtype == e.dtype and g.shape == e.shape, (g.dtype, e.dtype, g.shape, e.shape)
    bad = _bits(g) != _bits(e)
    if g.dtype.is_floating_point:
        bad &= ~(torch.isnan(g) & torch.isnan(e))
    return bad.any(dim=1)


def same_everywhere(got, exp_base, overrides, what, periods=64, leave_out=None):
    """got [n][...] on the device == exp_base tiled with the overrides written over it, over the WHOLE output (leave_out: rows, as a
    device index tensor, whose value is not pinned)"""
    n, period = got.shape[0], len(exp_base)
    eb = _dev(exp_base)
    tile = eb.repeat(periods, *([1] * (eb.dim() - 1)))
    bad = torch.empty(n, dtype=torch.bool, device=got.device)
    step = periods * period
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        bad[r0:r1] = _row_diff(got[r0:r1], tile[:r1 - r0])
    for s, rows in overrides:
        bad[s:s + len(rows)] = _row_diff(got[s:s + len(rows)], _dev(rows))
    if leave_out is not None:
        bad[leave_out] = False
    nbad = int(bad.sum())
    if nbad:
        first = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {nbad} of {n} rows differ, the first is row {first} (r mod {period} = {first % period})")


def tiled(exp_base, overrides, n):
    """the expected rows as a device tensor (inputs of a later stage)"""
    eb = _dev(exp_base)
    out = eb.repeat(-(-n // len(exp_base)), *([1] * (eb.dim() - 1)))[:n]
    for s, rows in overrides:
        out[s:s + len(rows)] = _dev(rows)
    return out


def same_answer(gi, gd, oi, od, what):
    gi, gd = gi.cpu().numpy().view(np.uint64), gd.cpu().numpy()
    bad = np.nonzero((gi != oi).any(axis=1))[0]
    assert bad.size == 0, (what, f"ids differ in {bad.size} queries, the first is query {bad[0]}", gi[bad[0]].astype(np.int64), gd[bad[0]], oi[bad[0]].astype(np.int64), od[bad[0]])
    assert (gd.view(np.uint32) == od.view(np.uint32)).all(), (what, "distance bits differ")


# ---- per-row operations ----------------------------------------------------------------------------------------------------------------
def run_assign(name, op):
    with held(name) as (col, x, eng, st):
        fn, mo = L.per_row_ops(col)[op]
        (ib, iov), (db, dov) = L.expected_rows(col, fn)
        if col.kind == "f32" and col.d <= 128:
            with counted(eng, "xf_assign"):
                ids, dists = eng.assign(x, mo["cent"], mo["metric"])
        else:
            ids, dists = eng.assign(x, mo["cent"], mo["metric"])
        same_everywhere(ids, ib.view(np.int32), [(s, r.view(np.int32)) for s, r in iov], f"{name} {op} ids")
        same_everywhere(dists, db, dov, f"{name} {op} distances")


def run_ivfpq_encode(name, op, stage):
    with held(name) as (col, x, eng, st):
        fn, mo = L.per_row_ops(col)[op]
        (pb, pov), (cb, cov) = L.expected_rows(col, fn)
        with counted(eng, stage):
            part, codes, loss = eng.ivfpq_encode(x, mo["cent"], mo["cb"], mo["metric"], want_loss=False)
        assert loss is None
        same_everywhere(part, pb.view(np.int32), [(s, r.view(np.int32)) for s, r in pov], f"{name} {op} partition ids")
        codes[part == -1] = 0               # (rows without a partition: their codes are unspecified)
        same_everywhere(codes, cb, cov, f"{name} {op} codes")


F32_128_ENCODES = [f"ivfpq_encode-m{m}-{metric}" for m in (16, 32) for metric in ("l2", "dot", "cosine")]


def test_f32_128_normalize():
    with held("f32-128") as (col, x, eng, st):
        fn, _ = L.per_row_ops(col)["normalize"]
        (eb, ov), = L.expected_rows(col, fn)
        same_everywhere(eng.normalize(x), eb, ov, "normalize")


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_f32_128_assign(metric):
    run_assign("f32-128", f"assign-{metric}")


@pytest.mark.parametrize("op", F32_128_ENCODES)
def test_f32_128_ivfpq_encode(op):
    """5 row chunks at M = 16, 9 at M = 32 (tests/test_large_column_spec.py::test_chunk_counts_of_the_big_column)"""
    run_ivfpq_encode("f32-128", op, "xform_fused")


def test_f32_128_residual_pq_encode():
    with held("f32-128") as (col, x, eng, st):
        fn, mo = L.per_row_ops(col)["residual+pq_encode"]
        (pb, pov), (rb, rov), (cb, cov) = L.expected_rows(col, fn)
        part, _ = eng.assign(x, mo["cent"], "l2")
        same_everywhere(part, pb.view(np.int32), [(s, r.view(np.int32)) for s, r in pov], "assign ahead of residual")
        res = eng.residual(x, mo["cent"], part)
        same_everywhere(res, rb, rov, "residual")
        codes = eng.pq_encode(res, mo["cb"], "l2")
        same_everywhere(codes, cb, cov, "pq_encode of the residuals")


def test_f32_128_sq_encode():
    with held("f32-128") as (col, x, eng, st):
        fn, mo = L.per_row_ops(col)["sq_encode"]
        (eb, ov), = L.expected_rows(col, fn)
        codes = eng.sq_encode(x, mo["bounds"])
        assert int(codes.min()) == 0 and int(codes.max()) == 255, "the bounds were chosen so that codes saturate at both ends"
        same_everywhere(codes, eb, ov, "sq_encode")


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_f32_128_rq_encode(metric):
    """the partition ids and distances are inputs here: the oracle's, tiled (Engine.assign has its own cases above)"""
    with held("f32-128") as (col, x, eng, st):
        fn, mo = L.per_row_ops(col)[f"rq_encode-{metric}"]
        (pb, pov), (vb, vov), (cb, cov), (ab, aov), (sb, sov) = L.expected_rows(col, fn)
        part = tiled(pb.view(np.int32), [(s, r.view(np.int32)) for s, r in pov], col.n)
        dvc = tiled(vb, vov, col.n)
        with counted(eng, "rq_encode"):
            codes, add, scale = eng.rq_encode(x, part, dvc, mo["cent"], mo["rot"], metric)
        same_everywhere(codes, cb, cov, "rq_encode codes")
        same_everywhere(add, ab, aov, "rq_encode add")
        same_everywhere(scale, sb, sov, "rq_encode scale")


# ---- flat KNN --------------------------------------------------------------------------------------------------------------------------
def run_flat(name, metric, nq, stage=None, calls=1):
    with held(name) as (col, x, eng, st):
        q = L.queries(col, nq)
        oi, od = L.planted_answer(col, q, K, metric)
        qd = _dev(q)
        for c in range(calls):
            if stage:
                with counted(eng, stage):
                    gi, gd = eng.flat_topk(x, qd, K, metric)
            else:
                gi, gd = eng.flat_topk(x, qd, K, metric)
            same_answer(gi, gd, oi, od, f"{name} flat_topk {metric} nq={nq} call {c}")


@pytest.mark.parametrize("nq,stage", [(1, None), (4, "flat_scan"), (256, "flat_mfma")])
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_f32_128_flat_topk(metric, nq, stage):
    """1 query: the single-pass kernel; 4: the batch filter; 256: the matrix-core filter"""
    run_flat("f32-128", metric, nq, stage)


# ---- IVF_FLAT over the whole column --------------------------------------------------------------------------------------------------
def _list_ids(col):
    part = (torch.arange(col.n, device="cuda") % (L.NLIST - 1)).to(torch.int32)
    part[col.last_window():] = L.NLIST - 1
    return part


def _allow(col, lrid, keep):
    allow = torch.ones(col.n, dtype=torch.bool, device="cuda")
    allow[_dev(lrid[~keep])] = False
    return allow


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_f32_128_ivfflat(metric):
    """the probed list is the last one: its storage and the rows its gather read both lie past the boundaries"""
    from lance_amd.engine import DeviceFlatIndex
    with held("f32-128") as (col, x, eng, st):
        cent = L.list_centroids(col, L.NLIST)
        q = L.queries(col, 33)
        assert L.probes_last_list(q, cent, metric)
        lrows, lrid = L.last_list_rows(col)
        idx = DeviceFlatIndex.create(eng, metric, cent, x, _list_ids(col))
        try:
            gi, gd = idx.search(q, K, 1)
            same_answer(gi, gd, *L.flat_list_answer(lrows, lrid, q, K, metric), f"IVF_FLAT {metric}")
            if metric == "l2":
                keep = np.arange(len(lrid)) % 3 != 0
                gi, gd = idx.search(q, K, 1, allow=_allow(col, lrid, keep))
                same_answer(gi, gd, *L.flat_list_answer(lrows, lrid, q, K, metric, keep), "IVF_FLAT filtered")
            torch.cuda.synchronize()
            st["held"] = st["free0"] - torch.cuda.mem_get_info()[0]          # (the index goes before the case's own reading)
        finally:
            idx.close()


# ---- RQ codes of the same column: 2^31 input elements ----------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_rq_codes(oracle, metric):
    """rq_encode with the lists given by position (every row but the last window in list 0, the last window in list 1), rq_distance over
    all codes (the last n % 32 rows take the f32 path), and the IVF_RQ search of the last list, unfiltered and filtered"""
    from lance_amd.engine import DeviceRqIndex
    with held("f32-128") as (col, x, eng, st):
        outs, cent, rot = L.rq_expected(col, metric)
        (pb, pov), (vb, vov), (cb, cov), (ab, aov), (sb, sov) = outs
        part = tiled(pb.view(np.int32), [(s, r.view(np.int32)) for s, r in pov], col.n)
        dvc = tiled(vb, vov, col.n)
        with counted(eng, "rq_encode"):
            codes, add, scale = eng.rq_encode(x, part, dvc, cent, rot, metric)
        same_everywhere(codes, cb, cov, "rq_encode codes")
        same_everywhere(add, ab, aov, "rq_encode add")
        same_everywhere(scale, sb, sov, "rq_encode scale")
        q, qr = L.rq_queries(col, cent, 2)
        dqc = oracle.assign(q, np.ascontiguousarray(cent[1:2]), metric)[1]
        eb, ov = L.rq_distance_expected(col, outs, qr, dqc, rot, metric)
        with counted(eng, "rq_distance"):
            got = eng.rq_distance(codes, add, scale, qr, dqc, rot, metric, quantised=True)
        for j in range(q.shape[0]):
            same_everywhere(got[j], np.ascontiguousarray(eb[:, j]), [(s, np.ascontiguousarray(r[:, j])) for s, r in ov], f"rq_distance {metric} query {j}")
        del got
        q33 = L.queries(col, 33).astype(f32)
        assert L.probes_last_list(q33, cent, metric)
        idx = DeviceRqIndex.create(eng, metric, cent, rot, codes, add, scale, part)
        try:
            gi, gd = idx.search(q33, K, 1)
            same_answer(gi, gd, *L.rq_list_answer(col, outs, cent, rot, q33, K, metric), f"IVF_RQ {metric}")
            keep = np.arange(L.LAST) % 3 != 0
            gi, gd = idx.search(q33, K, 1, allow=_allow(col, col.pos[col.pstart[-2]:], keep))
            same_answer(gi, gd, *L.rq_list_answer(col, outs, cent, rot, q33, K, metric, keep), f"IVF_RQ {metric} filtered")
            torch.cuda.synchronize()
            st["held"] = st["free0"] - torch.cuda.mem_get_info()[0]
        finally:
            idx.close()


# ---- multivector rows over the same vectors: 2^31 elements of `values` -------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_multivec(metric):
    """rows of 1 .. 8 vectors in a pattern with the filler's period: multivec_distance of every row, multivec_topk of the planted rows"""
    with held("f32-128") as (col, x, eng, st):
        off, R = L.multivec_offsets(col)
        q = L.multivec_query(col)
        eb, ov = L.multivec_expected(col, off, R, q, metric)
        with counted(eng, "multivec_scan"):
            got = eng.multivec_distance(x, off, q, metric)
        assert got.shape[0] == len(off) - 1
        leave_out = None
        if metric == "cosine":
            # a row that holds the all-zero vector: its cosine similarity is 0 / 0, a NaN whose sign is the dividing machine's -- as the
            # maximum (+NaN) it makes the row's distance NaN, as the minimum (-NaN) it is as if the vector were not there
            zeros = torch.arange(L.ZERO_ROW, col.n, P, device="cuda")
            leave_out = torch.searchsorted(_dev(off), zeros, right=True) - 1
            assert leave_out.numel() == -(-(col.n - L.ZERO_ROW) // P)
        same_everywhere(got, eb, ov, f"multivec_distance {metric}", leave_out=leave_out)
        ei, ed = L.multivec_planted_answer(eb, ov, K)
        gi, gd = eng.multivec_topk(x, off, q, K, metric)
        same_answer(gi[None], gd[None], ei[None], ed[None], f"multivec_topk {metric}")


# ---- the transform's row chunks alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_chunk_only_m32(metric):
    """d = 128, M = 32: three row chunks of xf_kernel, nothing else large"""
    run_ivfpq_encode("chunk-m32", f"ivfpq_encode-m32-{metric}", "xform_fused")


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_chunk_only_m96(metric):
    """d = 384, M = 96: three row chunks of xf_tail_kernel behind the K-tiled coarse quantiser"""
    run_ivfpq_encode("chunk-m96", f"ivfpq_encode-m96-{metric}", "xform_tail")


# ---- refine from a raw column past 2^31 elements (and 2^31 bytes in its u8 copy) -------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_refine_raw(oracle, metric):
    """an IVF_PQ index over the 6,000 planted rows of the high windows, row ids = their positions in the raw column: the u8 copy of the
    WHOLE column is made and read (keff 100: refine_rows_u8_kernel, keff 130: refine_u8_kernel), then, with one raw element spoiled by a
    fraction, the f32 refine kernels read the column itself"""
    from lance_amd.engine import DeviceIndex
    from test_zz_gpu_refine_u8 import _u8_used
    with held("refine-raw") as (col, x, eng, st):
        xh, pos = L.refine_index_rows(col)
        cent, cb = L.refine_models(col.d, metric)
        q = L.refine_queries(col, 64)
        gpart, gcodes, _ = eng.ivfpq_encode(xh, cent, cb, metric)
        gidx = DeviceIndex.create(eng, metric, cent, cb, gpart, gcodes, pos.view(np.int64), raw=x)
        try:
            for k, rf, whole_rows in ((10, 10, True), (13, 10, False)):
                before = eng.timing_query("count:refine_rows")[1]
                with _u8_used(eng, True):
                    gi, gd = gidx.search(q, k, L.REFINE_NLIST, rf)
                assert (eng.timing_query("count:refine_rows")[1] > before) == whole_rows, "the other u8 refine kernel answered"
                same_answer(gi, gd, *L.refine_answer(col, q, k, rf, metric), f"refine from the u8 copy {metric} k={k} refine={rf}")
            torch.cuda.synchronize()
            st["held"] = st["free0"] - torch.cuda.mem_get_info()[0]          # (with the u8 copy of the whole column alive)
            keep = x[5, 3].clone()
            try:
                x[5, 3] += 0.5                  # a filler row no query is near: the column is no longer a column of bytes
                gidx.set_raw(x)
                for k, rf in ((10, 10), (13, 10)):
                    with _u8_used(eng, False):
                        gi, gd = gidx.search(q, k, L.REFINE_NLIST, rf)
                    same_answer(gi, gd, *L.refine_answer(col, q, k, rf, metric), f"refine from the f32 column {metric} k={k} refine={rf}")
            finally:
                x[5, 3] = keep                  # the column is shared with the cases after this one
        finally:
            gidx.close()


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_refine_raw_sq_index(oracle, metric):
    """the same 6,000 rows under an IVF_SQ index whose row ids are their positions in the raw column: DeviceSqIndex.set_raw +
    refine_factor -- the candidates' ids (past 2^24) go from sq.hip's own lists into raw + id * d"""
    from lance_amd.engine import DeviceSqIndex
    with held("refine-raw") as (col, x, eng, st):
        _, pos = L.refine_index_rows(col)
        codes, part, cent, bounds = L.sq_refine_index(col, metric)
        q = L.refine_queries(col, 64)
        idx = DeviceSqIndex.create(eng, metric, cent, codes, part, bounds, row_ids=pos.view(np.int64))
        try:
            idx.set_raw(x)
            with counted(eng, "refine"):
                gi, gd = idx.search(q, 10, L.REFINE_NLIST, refine_factor=10)
            same_answer(gi, gd, *L.sq_refine_answer(col, q, 10, 10, metric), f"IVF_SQ refine {metric}")
        finally:
            idx.close()


# ---- f32, d = 256: 2^31 elements, a bf16 plane above 4 GiB -----------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_f32_256_assign(metric):
    run_assign("f32-256", f"assign-{metric}")


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_f32_256_flat_topk_plane_released_and_allocated_again(metric):
    """twice on one context: the plane above 4 GiB goes back through the guard after the first call, the second allocates it again"""
    run_flat("f32-256", metric, 256, "flat_mfma_wide", calls=2)


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_f32_256_flat_topk_exact(metric):
    """4 queries: the exact kernel (cosine: cosine_rownorm_kernel's grid over the whole column)"""
    run_flat("f32-256", metric, 4)


# ---- f16, d = 128 ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric,nq,stage", [("l2", 1, None), ("l2", 4, "flat_scan"), ("l2", 256, "flat_mfma"), ("dot", 4, None)])
def test_f16_128_flat_topk(metric, nq, stage):
    """l2: the kernels read the f16 rows as they are; dot: the 32-lane order on the widened copy"""
    run_flat("f16-128", metric, nq, stage)


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_f16_128_assign(metric):
    run_assign("f16-128", f"assign-{metric}")


@pytest.mark.parametrize("m", [16, 32])
def test_f16_128_ivfpq_encode(m):
    """l2: the transform kernel reads the f16 rows as they are (cosine normalises into an f32 copy first -- the f32 route, and beside
    the widened copy it would not fit the 24 GiB of this file; dot keeps the 32-lane kernels)"""
    run_ivfpq_encode("f16-128", f"ivfpq_encode-m{m}-l2", "xform_fused")


# ---- int8, d = 128: 2^31 and 2^32 elements = bytes ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nq,stage", [(1, None), (4, "flat_scan"), (256, "flat_mfma")])
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_i8_128_flat_topk(metric, nq, stage):
    run_flat("i8-128", metric, nq, stage)


# ---- SQ codes past 2^32 bytes --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_sq_codes_distance(metric):
    import sq_spec
    with held("sq-codes") as (codes, cd, eng, st):
        q = L.queries(st["raw"], 2)
        bounds = st["bounds"]
        (eb, ov), = L.expected_rows(codes, lambda c: (np.ascontiguousarray(sq_spec.distances(c, q, metric, *bounds).T),))
        with counted(eng, "sq_distance"):
            got = eng.sq_distance(cd, q, bounds, metric)
        for j in range(q.shape[0]):
            same_everywhere(got[j], np.ascontiguousarray(eb[:, j]), [(s, np.ascontiguousarray(r[:, j])) for s, r in ov], f"sq_distance {metric} query {j}")


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_sq_codes_index(metric):
    """nprobes = 1 into the last list, stored past 2^32 bytes of codes; unfiltered and filtered"""
    from lance_amd.engine import DeviceSqIndex
    with held("sq-codes") as (codes, cd, eng, st):
        raw, bounds = st["raw"], st["bounds"]
        cent = L.list_centroids(raw, L.NLIST)
        q = L.queries(raw, 33)
        assert L.probes_last_list(q, cent, metric)
        lcodes, lrid = L.last_list_rows(codes)
        idx = DeviceSqIndex.create(eng, metric, cent, cd, _list_ids(codes), bounds)
        try:
            gi, gd = idx.search(q, K, 1)
            same_answer(gi, gd, *L.sq_list_answer(lcodes, lrid, cent, q, K, metric, bounds), f"IVF_SQ {metric}")
            keep = np.arange(len(lrid)) % 3 != 0
            gi, gd = idx.search(q, K, 1, allow=_allow(codes, lrid, keep))
            same_answer(gi, gd, *L.sq_list_answer(lcodes, lrid, cent, q, K, metric, bounds, keep), f"IVF_SQ {metric} filtered")
            torch.cuda.synchronize()
            st["held"] = st["free0"] - torch.cuda.mem_get_info()[0]
        finally:
            idx.close()
