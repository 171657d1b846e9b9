"""Characterisation of the four device index handles (lance_amd/engine.py: DeviceIndex, DeviceFlatIndex, DeviceSqIndex, DeviceRqIndex) on the
CPU: which library symbol every method calls, with which scalar arguments, after which synchronisation, and what the objects that
merge / remap / split / join hand back carry.  `engine.lib` is a recording stand-in, `_dev` is the CPU device, and the two kinds of
waiting (device-wide torch.cuda.synchronize, torch's current stream) append "device" / "stream" to the same log.  The expected logs are
literals recorded once from the implementation this file was first written against; they are not computed from the code under test."""
import ctypes as C
import inspect
import numbers
import types

import numpy as np
import pytest
import torch

from lance_amd import engine as E

D, NLIST, N_ROWS = 8, 4, 6


def _fmt(a):
    """one argument of a library call as the log shows it: scalars as they are, handles as h<value>, any other address as ptr"""
    if a is None:
        return "None"
    if isinstance(a, C.c_void_p):
        return "None" if a.value is None else (f"h{a.value}" if a.value < 1000 else "ptr")
    if isinstance(a, C.Array):
        return "[" + ", ".join(_fmt(v) for v in a) + "]"
    if isinstance(a, bool) or isinstance(a, numbers.Integral):
        return str(int(a))
    if isinstance(a, float):
        return repr(a)
    if isinstance(a, bytes):
        return repr(a)
    return "ref" if type(a).__name__ == "CArgObject" else type(a).__name__


class _Lib:
    """every attribute is a function that logs (symbol, arguments) and returns 0; a handle asked for through byref gets the next
    number, lance_hip_index_info answers n = N_ROWS (nlist, m, d when asked), `fill[symbol]` may write into the output arrays"""

    def __init__(self, log):
        self._log, self._next, self.fill = log, 20, {}

    def __getattr__(self, name):
        def fn(*args):
            self._log.append(f"{name}({', '.join(_fmt(a) for a in args)})")
            if name == "lance_hip_index_info":
                for ref, v in zip(args[1:], (N_ROWS, NLIST, 2, D)):
                    if ref is not None:
                        ref._obj.value = v
            elif args and type(args[-1]).__name__ == "CArgObject" and isinstance(args[-1]._obj, C.c_void_p):
                args[-1]._obj.value = self._next
                self._next += 1
            if name in self.fill:
                self.fill[name](*args)
            return 0
        return fn


@pytest.fixture
def rec(monkeypatch):
    log = []
    lib = _Lib(log)
    monkeypatch.setattr(E, "_dev", lambda: torch.device("cpu"))
    monkeypatch.setattr(torch.cuda, "synchronize", lambda *a, **kw: log.append("device"))
    monkeypatch.setattr(E, "_torch_inputs_ready", lambda: log.append("stream"))
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a, **kw: types.SimpleNamespace(synchronize=lambda: log.append("stream")))
    eng = types.SimpleNamespace(lib=lib, h=C.c_void_p(1), device=0, use_torch_stream=False)
    held = []          # every index made here lives to the end of the test: a collected one would log its destroy in the middle

    def hold(ix):
        held.append(ix)
        return ix
    return types.SimpleNamespace(log=log, lib=lib, eng=eng, hold=hold)


def _cent(dtype=torch.float32):
    return torch.zeros(NLIST, D, dtype=dtype)


def _make(rec, kind, handle=10):
    h = C.c_void_p(handle)
    if kind == "flat":
        return rec.hold(E.DeviceFlatIndex(rec.eng, h, "l2", _cent(torch.float16), torch.float16))
    if kind == "sq":
        return rec.hold(E.DeviceSqIndex(rec.eng, h, "cosine", _cent(), torch.float32, (-1.5, 2.5)))
    if kind == "rq":
        return rec.hold(E.DeviceRqIndex(rec.eng, h, "dot", _cent(), torch.eye(D)))
    return rec.hold(E.DeviceIndex(rec.eng, h, "l2", _cent(), torch.zeros(2, 256, 4), None, torch.float32))


def _q(nq=3, dtype=np.float64):
    return np.arange(nq * D, dtype=dtype).reshape(nq, D)


ALLOW = np.array([True, False] * 5)


def _take(rec):
    out = list(rec.log)
    del rec.log[:]
    return out


def _shape(ids, dists):
    return (tuple(ids.shape), ids.dtype, tuple(dists.shape), dists.dtype)


OUT35 = ((3, 5), torch.int64, (3, 5), torch.float32)


# ---- search arms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, sym", [("sq", "ivfsq"), ("rq", "ivfrq")])
def test_sq_rq_search_arms(rec, kind, sym):
    ix = _make(rec, kind)
    q = _q(dtype=np.float32 if kind == "rq" else np.float64)
    assert _shape(*ix.search(q, 5, 2)) == OUT35
    assert _take(rec) == ["device", f"lance_hip_{sym}_search(h1, h10, ptr, 3, 5, 2, ptr, ptr)"]
    assert _shape(*ix.search(q, 5, 2, allow=ALLOW)) == OUT35
    assert _take(rec) == ["device", f"lance_hip_{sym}_search_filtered(h1, h10, ptr, 3, 5, 2, ptr, 10, ptr, ptr)"]
    assert _shape(*ix.search(q, 5, 2, refine_factor=3)) == OUT35
    assert _take(rec) == ["device", f"lance_hip_{sym}_search_refine(h1, h10, ptr, 3, 5, 2, 3, None, 0, ptr, ptr)"]
    assert _shape(*ix.search(q, 5, 2, allow=torch.from_numpy(ALLOW), refine_factor=3)) == OUT35
    assert _take(rec) == ["device", f"lance_hip_{sym}_search_refine(h1, h10, ptr, 3, 5, 2, 3, ptr, 10, ptr, ptr)"]
    assert _shape(*ix.search(q[0], 1, 4)) == ((1, 1), torch.int64, (1, 1), torch.float32)      # one query given as [d]
    assert _take(rec) == ["device", f"lance_hip_{sym}_search(h1, h10, ptr, 1, 1, 4, ptr, ptr)"]


def test_rq_refuses_queries_that_are_not_float32(rec):
    ix = _make(rec, "rq")
    with pytest.raises(NotImplementedError, match="IVF_RQ: queries must be float32, got float16"):
        ix.search(_q(dtype=np.float16), 5, 2)
    assert _take(rec) == []


def test_flat_search_arms(rec):
    ix = _make(rec, "flat")
    q = _q()
    assert _shape(*ix.search(q, 5, 2)) == OUT35
    assert _take(rec) == ["device", "lance_hip_ivfflat_search(h1, h10, ptr, 3, 5, 2, ptr, ptr)"]
    assert _shape(*ix.search(q, 5, 2, allow=ALLOW)) == OUT35
    assert _take(rec) == ["device", "lance_hip_ivfflat_search_filtered(h1, h10, ptr, 3, 5, 2, ptr, 10, ptr, ptr)"]
    assert _shape(*ix.search(q, 5, 2, lower=0.1)) == OUT35
    assert _take(rec) == ["device", "lance_hip_ivfflat_search_range(h1, h10, ptr, 3, 5, 2, None, 0, 0.10000000149011612, 3.4028234663852886e+38, ptr, ptr)"]
    assert _shape(*ix.search(q, 5, 2, allow=ALLOW, upper=2.3)) == OUT35
    assert _take(rec) == ["device", "lance_hip_ivfflat_search_range(h1, h10, ptr, 3, 5, 2, ptr, 10, -3.4028234663852886e+38, 2.299999952316284, ptr, ptr)"]
    assert _shape(*ix.search(q, 5, 2, allow=ALLOW, lower=-1, upper=7)) == OUT35
    assert _take(rec) == ["device", "lance_hip_ivfflat_search_range(h1, h10, ptr, 3, 5, 2, ptr, 10, -1.0, 7.0, ptr, ptr)"]


def test_queries_take_the_element_type_of_the_index(rec, monkeypatch):
    """a float32 batch goes to a float32 index as it is (same storage) and is converted for the float16 one"""
    q = torch.from_numpy(_q(dtype=np.float32))
    seen = []
    real = E._ptr

    def spy(t):
        if t is not None and tuple(t.shape) == (3, D):          # the query batch; the outputs are [3][5]
            seen.append((t.dtype, t.data_ptr() == q.data_ptr()))
        return real(t)
    monkeypatch.setattr(E, "_ptr", spy)
    for kind in ("flat", "sq", "rq", "pq"):
        _make(rec, kind).search(q, 5, 2)
    assert seen == [(torch.float16, False), (torch.float32, True), (torch.float32, True), (torch.float32, True)]


def test_pq_search_sync_sliced_async(rec):
    ix = _make(rec, "pq")
    q = _q()
    assert _shape(*ix.search(q, 5, 2)) == OUT35
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search(h1, h10, ptr, 3, 5, 2, 0, ptr, ptr)"]
    assert _shape(*ix.search(q, 5, 2, refine_factor=4)) == OUT35
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search(h1, h10, ptr, 3, 5, 2, 4, ptr, ptr)"]
    # slices: 3 queries x 2 probes above 4 pairs per call -> 2 queries per call
    ix.MAX_PAIRS_PER_CALL = 4
    ids = torch.zeros(3, 5, dtype=torch.int64)
    dists = torch.zeros(3, 5)
    got = ix.search(q, 5, 2, 1, out=(ids, dists))
    assert got[0] is ids and got[1] is dists
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search(h1, h10, ptr, 2, 5, 2, 1, ptr, ptr)",
                          "lance_hip_ivfpq_search(h1, h10, ptr, 1, 5, 2, 1, ptr, ptr)"]
    ix.search(q[:1], 5, 9)                  # one query is never sliced
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search(h1, h10, ptr, 1, 5, 9, 0, ptr, ptr)"]
    ix.search(q, 5, 2, sync=False)          # nor is an asynchronous batch
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_async(h1, h10, ptr, 3, 5, 2, 0, ptr, ptr)"]
    del ix.MAX_PAIRS_PER_CALL
    assert E.DeviceIndex.MAX_PAIRS_PER_CALL == 1_500_000
    # asynchronous: waits on torch's stream only when torch converted the batch or allocated the outputs
    ready = torch.from_numpy(_q(dtype=np.float32))
    got = ix.search(ready, 5, 2, out=(ids, dists), sync=False)
    assert got[0] is ids and got[1] is dists
    assert _take(rec) == ["lance_hip_ivfpq_search_async(h1, h10, ptr, 3, 5, 2, 0, ptr, ptr)"]
    ix.search(ready, 5, 2, sync=False)
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_async(h1, h10, ptr, 3, 5, 2, 0, ptr, ptr)"]
    ix.search(q, 5, 2, out=(ids, dists), sync=False)            # a float64 numpy batch: converted
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_async(h1, h10, ptr, 3, 5, 2, 0, ptr, ptr)"]
    other = types.SimpleNamespace(lib=rec.lib, h=C.c_void_p(2), device=0, use_torch_stream=True)
    ix.search(q, 5, 2, sync=False, engine=other)                # an engine on torch's stream never waits
    assert _take(rec) == ["lance_hip_ivfpq_search_async(h2, h10, ptr, 3, 5, 2, 0, ptr, ptr)"]
    ix.search(q, 5, 2, engine=other)
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search(h2, h10, ptr, 3, 5, 2, 0, ptr, ptr)"]


def test_pq_search_filtered(rec):
    ix = _make(rec, "pq")
    assert _shape(*ix.search_filtered(_q(), 5, 2, ALLOW)) == OUT35
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_filtered(h1, h10, ptr, 3, 5, 2, 0, ptr, 10, ptr, ptr)"]
    out = (torch.zeros(3, 5, dtype=torch.int64), torch.zeros(3, 5))
    got = ix.search_filtered(_q(), 5, 2, torch.from_numpy(ALLOW), refine_factor=2, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_filtered(h1, h10, ptr, 3, 5, 2, 2, ptr, 10, ptr, ptr)"]


def _fill_candidates(ids_col, dists_col):
    """the stand-in's answer of a re-ranking range call: per query the row ids 0 .. k-1 (query 1: the odd ones missing) at the
    distances 0.0, 0.5, 1.0, ... shifted by the query's number"""
    def fill(*args):
        nq, k = args[3], args[4]
        ids = np.ctypeslib.as_array((C.c_int64 * (nq * k)).from_address(args[ids_col].value)).reshape(nq, k)
        dists = np.ctypeslib.as_array((C.c_float * (nq * k)).from_address(args[dists_col].value)).reshape(nq, k)
        ids[:] = np.arange(k)
        ids[1, 1::2] = -1
        dists[:] = 0.5 * np.arange(k) + np.arange(nq)[:, None]
    return fill


def test_pq_search_range(rec):
    ix = _make(rec, "pq")
    q = _q()
    assert _shape(*ix.search_range(q, 5, 2, lower=0.1)) == OUT35
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_range(h1, h10, ptr, 3, 5, 2, 0, 0.10000000149011612, 3.4028234663852886e+38, ptr, ptr)"]
    out = (torch.zeros(3, 5, dtype=torch.int64), torch.zeros(3, 5))
    got = ix.search_range(q, 5, 2, upper=2.3, out=out)
    assert got[0] is out[0] and got[1] is out[1]
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_range(h1, h10, ptr, 3, 5, 2, 0, -3.4028234663852886e+38, 2.299999952316284, ptr, ptr)"]
    assert _shape(*ix.search_range(q, 5, 2, lower=0.1, allow=ALLOW)) == OUT35
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_filtered_range(h1, h10, ptr, 3, 5, 2, 0, ptr, 10, 0.10000000149011612, "
                          "3.4028234663852886e+38, ptr, ptr)"]
    # a refine factor: k * refine_factor candidates come back re-ranked (flag 1) and the range is applied to them on the host
    rec.lib.fill = {"lance_hip_ivfpq_search_range": _fill_candidates(9, 10), "lance_hip_ivfpq_search_filtered_range": _fill_candidates(11, 12)}
    inf = float("inf")
    want_ids = [[1, 2, 3], [0, 2, -1], [0, -1, -1]]
    want_dists = [[0.5, 1.0, 1.5], [1.0, 2.0, inf], [2.0, inf, inf]]
    ids, dists = ix.search_range(q, 3, 2, lower=0.5, upper=2.25, refine_factor=2)
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_range(h1, h10, ptr, 3, 6, 2, 1, 0.5, 2.25, ptr, ptr)"]
    assert ids.tolist() == want_ids and dists.tolist() == want_dists
    ids, dists = ix.search_range(q, 3, 2, lower=0.5, upper=2.25, refine_factor=2, allow=ALLOW)
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_filtered_range(h1, h10, ptr, 3, 6, 2, 1, ptr, 10, 0.5, 2.25, ptr, ptr)"]
    assert ids.tolist() == want_ids and dists.tolist() == want_dists
    ids, dists = ix.search_range(q, 2, 2, upper=0.75, refine_factor=2)          # open lower end on the host side too
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_range(h1, h10, ptr, 3, 4, 2, 1, -3.4028234663852886e+38, 0.75, ptr, ptr)"]
    assert ids.tolist() == [[0, 1], [-1, -1], [-1, -1]] and dists.tolist() == [[0.0, 0.5], [inf, inf], [inf, inf]]


def test_pq_search_candidates_and_multivec(rec):
    ix = _make(rec, "pq")
    ids, pq, ex = ix.search_candidates(_q(), 7, 9)
    assert _shape(ids, pq) == ((3, 7), torch.int64, (3, 7), torch.float32) and _shape(ids, ex) == _shape(ids, pq)
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_candidates(h1, h10, ptr, 3, 7, 4, ptr, ptr, ptr)"]
    other = types.SimpleNamespace(lib=rec.lib, h=C.c_void_p(2), device=0, use_torch_stream=False)
    ids, pq, ex = ix.search_candidates(_q(), 7, 2, exact=False, engine=other)
    assert ex is None
    assert _take(rec) == ["stream", "lance_hip_ivfpq_search_candidates(h2, h10, ptr, 3, 7, 2, ptr, ptr, None)"]
    ids, dists = ix.multivec_search(_q(5), [0, 2, 5], 3, 9, overfetch=4)
    assert _shape(ids, dists) == ((2, 3), torch.int64, (2, 3), torch.float32)
    assert _take(rec) == ["stream", "lance_hip_ivfpq_multivec_search(h1, h10, ptr, ptr, 2, 3, 4, 4, 3, None, 0, ptr, ptr)"]
    ids, dists = ix.multivec_search(_q(5), [0, 2, 5], 3, 2, k_out=6, allow=ALLOW)
    assert _shape(ids, dists) == ((2, 6), torch.int64, (2, 6), torch.float32)
    assert _take(rec) == ["stream", "lance_hip_ivfpq_multivec_search(h1, h10, ptr, ptr, 2, 3, 2, 10, 6, ptr, 10, ptr, ptr)"]
    with pytest.raises(ValueError, match="q holds 4 vectors, q_offsets end at 5"):
        ix.multivec_search(_q(4), [0, 2, 5], 3, 2)
    assert _take(rec) == []


# ---- maintenance and export -----------------------------------------------------------------------------------------------------
def _attrs(ix):
    out = {"type": type(ix).__name__, "h": ix.h.value, "metric": ix.metric, "data_dtype": ix.data_dtype, "centroids": tuple(ix.centroids.shape),
           "cent_dtype": ix.centroids.dtype}
    if hasattr(ix, "bounds"):
        out["bounds"] = ix.bounds
    if hasattr(ix, "codebook"):
        out["codebook"] = tuple(ix.codebook.shape)
    raw = getattr(ix, "_raw", None)
    out["raw"] = None if raw is None else tuple(raw.shape)
    return out


_KIND_ATTRS = {
    "flat": {"type": "DeviceFlatIndex", "metric": "l2", "data_dtype": torch.float16, "cent_dtype": torch.float16, "raw": None},
    "sq": {"type": "DeviceSqIndex", "metric": "cosine", "data_dtype": torch.float32, "cent_dtype": torch.float32, "bounds": (-1.5, 2.5), "raw": None},
    "pq": {"type": "DeviceIndex", "metric": "l2", "data_dtype": torch.float32, "cent_dtype": torch.float32, "codebook": (2, 256, 4), "raw": None},
}


@pytest.mark.parametrize("kind", ["flat", "sq", "pq"])
def test_merge_remap_split_join(rec, kind):
    ix, ix2 = _make(rec, kind, 10), _make(rec, kind, 11)
    raw = np.ones((9, D), np.float32)
    same = dict(_KIND_ATTRS[kind], centroids=(NLIST, D))

    m = rec.hold(type(ix).merge([ix, ix2]))
    assert _take(rec) == ["device", "lance_hip_index_merge(h1, [10, 11], 2, ref)"]
    assert _attrs(m) == dict(same, h=20) and m.centroids is ix.centroids and m.engine is rec.eng
    m = rec.hold(type(ix).merge([ix2, ix], raw=raw))          # raw: attached by the IVF_PQ handle, accepted and ignored by the others
    want = ["device", "lance_hip_index_merge(h1, [11, 10], 2, ref)"] + (["lance_hip_index_set_raw(h21, ptr, 9)"] if kind == "pq" else [])
    assert _take(rec) == want
    assert _attrs(m) == dict(same, h=21, **({"raw": (9, D)} if kind == "pq" else {}))

    r = rec.hold(ix.remap([3, 5, 7], np.array([4, -1, 9])))
    assert _take(rec) == ["device", "lance_hip_index_remap(h1, h10, ptr, ptr, 3, ref)"]
    assert _attrs(r) == dict(same, h=22) and r.centroids is ix.centroids
    with pytest.raises(ValueError, match="remap: 2 old ids but 3 new ids"):
        ix.remap([3, 5], [4, 5, 6])
    assert _take(rec) == []
    if kind == "pq":
        r = rec.hold(ix.remap([3], [4], raw=raw))
        assert _take(rec) == ["device", "lance_hip_index_remap(h1, h10, ptr, ptr, 1, ref)", "lance_hip_index_set_raw(h23, ptr, 9)"]
        assert _attrs(r) == dict(same, h=23, raw=(9, D))
    else:
        with pytest.raises(TypeError):
            ix.remap([3], [4], raw=raw)
        rec.lib._next += 1          # (the handle numbers below stay the same for the three kinds)
    assert _take(rec) == []

    s = rec.hold(ix.split(1, np.ones((2, D)), raw))
    assert _take(rec) == ["device", "lance_hip_index_split(h1, h10, 1, ptr, ptr, 9, ref)"]
    assert _attrs(s) == dict(same, h=24, centroids=(NLIST + 1, D))      # (no raw attached, IVF_PQ included)
    assert s.centroids[1].tolist() == [1.0] * D and s.centroids[NLIST].tolist() == [1.0] * D and s.centroids[2].tolist() == [0.0] * D
    j = rec.hold(ix.join(2, raw))
    assert _take(rec) == ["device", "lance_hip_index_join(h1, h10, 2, ptr, 9, ref)"]
    assert _attrs(j) == dict(same, h=25, centroids=(NLIST - 1, D))
    with pytest.raises(ValueError, match="split / join: the raw vectors are required"):
        ix.join(2, None)
    with pytest.raises(ValueError, match="split / join: raw vectors must be float32, got float16"):
        ix.split(2, np.ones((2, D)), raw.astype(np.float16))
    assert _take(rec) == []


def test_export_rows_arity_and_pq_exports(rec):
    offs, rows, rid = _make(rec, "flat").export_rows()
    assert (offs.shape, rows.shape, rows.dtype, rid.shape, rid.dtype) == ((NLIST + 1,), (N_ROWS, D), np.float32, (N_ROWS,), np.uint64)
    want = ["lance_hip_index_info(h10, ref, None, None, None)", "device"]
    assert _take(rec) == want + ["lance_hip_index_export_rows(h1, h10, ptr, ptr, None, ptr)"]
    offs, rows, xx, rid = _make(rec, "sq").export_rows()
    assert (offs.shape, rows.shape, rows.dtype, xx.shape, xx.dtype, rid.shape) == ((NLIST + 1,), (N_ROWS, D), np.uint8, (N_ROWS,), np.uint32, (N_ROWS,))
    assert _take(rec) == want + ["lance_hip_index_export_rows(h1, h10, ptr, ptr, ptr, ptr)"]
    ix = _make(rec, "pq")
    offs, rows, rid = ix.export_rows()
    assert (offs.shape, rows.shape, rows.dtype, rid.shape) == ((NLIST + 1,), (N_ROWS, 2), np.uint8, (N_ROWS,))
    assert _take(rec) == want + ["lance_hip_index_export_rows(h1, h10, ptr, ptr, None, ptr)"]
    offs, rid = E._export_ids(rec.eng, ix.h, NLIST)
    assert (offs.shape, rid.shape) == ((NLIST + 1,), (N_ROWS,))
    assert _take(rec) == want + ["lance_hip_index_export_rows(h1, h10, ptr, None, None, ptr)"]
    assert ix.info() == {"n": N_ROWS, "nlist": NLIST, "m": 2, "d": D}
    offs, codes, rid = ix.export()
    assert (offs.shape, codes.shape, rid.shape) == ((NLIST + 1,), (N_ROWS * 2,), (N_ROWS,))
    assert ix.part_offsets().shape == (NLIST + 1,)
    ix.prewarm()
    info = "lance_hip_index_info(h10, ref, ref, ref, ref)"
    assert _take(rec) == [info, info, "lance_hip_index_export(h1, h10, ptr, ptr, ptr)", info, "lance_hip_index_export(h1, h10, ptr, None, None)",
                          "lance_hip_index_prewarm(h1, h10)"]


def test_set_raw(rec):
    raw = np.ones((9, D), np.float64)
    for kind in ("sq", "rq", "pq"):
        ix = _make(rec, kind)
        ix.set_raw(raw)
        assert _take(rec) == ["lance_hip_index_set_raw(h10, ptr, 9)"]
        assert ix._raw.dtype == torch.float32 and tuple(ix._raw.shape) == (9, D)
    for kind in ("sq", "rq"):
        with pytest.raises(ValueError, match=r"raw vectors must be \[rows\]\[d\], got shape \(72,\)"):
            _make(rec, kind).set_raw(raw.reshape(-1))
        assert _take(rec) == []
    ix = _make(rec, "pq")
    ix.set_raw(raw.reshape(-1))             # the IVF_PQ handle does not check the number of dimensions
    assert _take(rec) == ["lance_hip_index_set_raw(h10, ptr, 72)"]
    assert not hasattr(E.DeviceFlatIndex, "set_raw")
    ix = rec.hold(E.DeviceIndex(rec.eng, C.c_void_p(12), "l2", _cent(torch.float16), torch.zeros(2, 16, 4), raw))       # raw= of the constructor
    assert _take(rec) == ["lance_hip_index_set_raw(h12, ptr, 9)"]
    assert ix._raw.dtype == torch.float16 and ix.data_dtype == torch.float16


def test_create(rec):
    part = np.array([0, 1, -1, 3, 2, 0])
    ix = rec.hold(E.DeviceFlatIndex.create(rec.eng, "cosine", np.zeros((NLIST, D)), np.zeros((N_ROWS, D), np.float16), part))
    assert _take(rec) == ["device", "lance_hip_ivfflat_create(h1, 1, 1, 8, ptr, 4, ptr, ptr, None, 6, ref)"]
    assert _attrs(ix) == {"type": "DeviceFlatIndex", "h": 20, "metric": "cosine", "data_dtype": torch.float16, "centroids": (NLIST, D),
                          "cent_dtype": torch.float16, "raw": None}
    ix = rec.hold(E.DeviceSqIndex.create(rec.eng, "l2", np.zeros((NLIST, D), np.float32), np.zeros((N_ROWS, D), np.uint8), part, (-1, 2), row_ids=np.arange(6)))
    assert _take(rec) == ["device", "lance_hip_ivfsq_create(h1, 0, 0, 8, ptr, 4, ptr, ptr, ptr, 6, [-1.0, 2.0], ref)"]
    assert _attrs(ix) == {"type": "DeviceSqIndex", "h": 21, "metric": "l2", "data_dtype": torch.float32, "centroids": (NLIST, D),
                          "cent_dtype": torch.float32, "bounds": (-1.0, 2.0), "raw": None}
    ix = rec.hold(E.DeviceRqIndex.create(rec.eng, "dot", np.zeros((NLIST, D)), np.eye(D), np.zeros((N_ROWS, 1), np.uint8), np.zeros(6), np.zeros(6), part))
    assert _take(rec) == ["device", "lance_hip_ivfrq_create(h1, 2, 8, ptr, 4, ptr, ptr, ptr, ptr, ptr, None, 6, ref)"]
    assert _attrs(ix) == {"type": "DeviceRqIndex", "h": 22, "metric": "dot", "data_dtype": torch.float32, "centroids": (NLIST, D),
                          "cent_dtype": torch.float32, "raw": None}
    assert tuple(ix.rotation.shape) == (D, D) and ix.rotation.dtype == torch.float32
    with pytest.raises(NotImplementedError, match="IVF_RQ: centroids must be float32, got float16"):
        E.DeviceRqIndex.create(rec.eng, "dot", np.zeros((NLIST, D), np.float16), np.eye(D), None, None, None, None)
    ix = rec.hold(E.DeviceIndex.create(rec.eng, "l2", np.zeros((NLIST, D)), np.zeros((2, 16, 4)), part, np.zeros((6, 1), np.uint8), dtype="int8"))
    assert _take(rec) == ["device", "lance_hip_index_create(h1, 2, 0, 8, ptr, 4, ptr, 2, 4, ptr, ptr, None, 6, ref)"]
    assert _attrs(ix) == {"type": "DeviceIndex", "h": 23, "metric": "l2", "data_dtype": torch.int8, "centroids": (NLIST, D),
                          "cent_dtype": torch.float32, "codebook": (2, 16, 4), "raw": None}
    ix = rec.hold(E.DeviceIndex.from_storage(rec.eng, "l2", np.zeros((NLIST, D), np.float16), np.zeros((2, 256, 4)), [0, 2, 3, 5, 6], np.zeros((6, 2)),
                                    np.arange(6), raw=np.ones((9, D))))
    assert _take(rec) == ["device", "lance_hip_index_from_storage(h1, 1, 0, 8, ptr, 4, ptr, 2, 8, ptr, ptr, 1, ptr, 6, ref)",
                          "lance_hip_index_set_raw(h24, ptr, 9)"]
    assert _attrs(ix) == {"type": "DeviceIndex", "h": 24, "metric": "l2", "data_dtype": torch.float16, "centroids": (NLIST, D),
                          "cent_dtype": torch.float16, "codebook": (2, 256, 4), "raw": (9, D)}


def test_save(rec):
    for kind in ("flat", "pq"):
        ix = _make(rec, kind)
        ix.save("/somewhere")
        ix.save("/somewhere", loss=1.5)
        assert _take(rec) == ["device", "lance_hip_index_save(h1, h10, b'/somewhere', 0, 0.0)", "device", "lance_hip_index_save(h1, h10, b'/somewhere', 1, 1.5)"]
    with pytest.raises(NotImplementedError, match=r"IVF_SQ index files are not supported \(IVF_PQ and IVF_FLAT are\)"):
        _make(rec, "sq").save("/somewhere")
    with pytest.raises(NotImplementedError, match=r"IVF_RQ index files are not supported \(IVF_PQ and IVF_FLAT are\)"):
        _make(rec, "rq").save("/somewhere")
    assert _take(rec) == []


# ---- lifecycle and class shape ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["flat", "sq", "rq", "pq"])
def test_close_destroys_once(rec, kind):
    ix = _make(rec, kind)
    ix.close()
    assert _take(rec) == ["lance_hip_index_destroy(h10)"] and ix.h is None
    ix.close()
    ix.__del__()
    assert _take(rec) == []
    ix = _make(rec, kind, 11)
    ix.__del__()
    assert _take(rec) == ["lance_hip_index_destroy(h11)"]
    ix.__del__()
    assert _take(rec) == []
    half = object.__new__(type(ix))         # a constructor that raised before `h` was set
    half.__del__()
    assert _take(rec) == []


def test_rq_handle_has_no_maintenance():
    for name in ("merge", "remap", "split", "join", "export_rows", "load"):
        assert not hasattr(E.DeviceRqIndex, name), name
    for cls in (E.DeviceIndex, E.DeviceFlatIndex, E.DeviceSqIndex):
        for name in ("merge", "remap", "split", "join", "export_rows"):
            assert hasattr(cls, name), (cls.__name__, name)
    assert hasattr(E.DeviceIndex, "load") and hasattr(E.DeviceFlatIndex, "load") and not hasattr(E.DeviceSqIndex, "load")


_PUBLIC = {
    "DeviceFlatIndex": ["close", "export_rows", "join", "remap", "save", "search", "split"],
    "DeviceSqIndex": ["close", "export_rows", "join", "remap", "save", "search", "set_raw", "split"],
    "DeviceRqIndex": ["close", "save", "search", "set_raw"],
    "DeviceIndex": ["close", "export", "export_rows", "info", "join", "multivec_search", "part_offsets", "prewarm", "remap", "save", "search",
                    "search_candidates", "search_filtered", "search_range", "set_raw", "split"],
}
_CLASSMETHODS = {"DeviceFlatIndex": ["create", "load", "merge"], "DeviceSqIndex": ["create", "merge"], "DeviceRqIndex": ["create"],
                 "DeviceIndex": ["create", "from_storage", "load", "merge"]}


@pytest.mark.parametrize("name", sorted(_PUBLIC))
def test_methods_run_under_the_device_guard(name):
    cls = getattr(E, name)
    methods, classmethods = [], []
    for attr in dir(cls):
        if attr.startswith("_"):
            continue
        static = inspect.getattr_static(cls, attr)
        if isinstance(static, classmethod):
            classmethods.append(attr)
        elif callable(static):
            methods.append(attr)
    assert methods == _PUBLIC[name] and classmethods == _CLASSMETHODS[name]
    exempt = {"close"} | ({"save"} if name in ("DeviceSqIndex", "DeviceRqIndex") else set())
    for attr in methods:
        assert hasattr(getattr(cls, attr), "__wrapped__") == (attr not in exempt), attr
    for attr in classmethods:
        assert not hasattr(getattr(cls, attr).__func__, "__wrapped__"), attr


def test_guard_makes_the_engines_device_current(rec, monkeypatch):
    """a method found on a base class runs with the engine's device current, as one defined in the class itself"""
    entered = []

    current = [0]

    class Ctx:
        def __init__(self, dev):
            self.dev = dev

        def __enter__(self):
            entered.append(self.dev)
            self.before, current[0] = current[0], self.dev

        def __exit__(self, *a):
            current[0] = self.before
            return False
    monkeypatch.setattr(torch.cuda, "is_available", lambda: True)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: current[0])
    monkeypatch.setattr(torch.cuda, "device", Ctx)
    rec.eng.device = 3
    raw = np.ones((9, D), np.float32)
    for kind in ("flat", "sq", "rq", "pq"):
        ix = _make(rec, kind)
        ix.search(_q(dtype=np.float32), 5, 2)
        if kind != "flat":
            ix.set_raw(raw)
        if kind != "rq":
            ix.remap([1], [2])
            ix.split(1, np.ones((2, D)), raw)
            ix.join(1, raw)
            ix.export_rows()
        if kind in ("flat", "pq"):
            ix.save("/somewhere")
        ix.close()
    assert entered == [3] * (6 + 6 + 2 + 7)
