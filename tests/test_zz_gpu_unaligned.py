"""Device pointers off the 16-byte grid on every audited entry point ("Pointer alignment").

A slice of an Arrow FixedSizeList column starts on an element boundary only: 4 bytes for f32, 2 for f16, 1 for int8 and code bytes.
The library tests the pointers it is handed (`& 15`, `& 7`, `& 3`, `% (4 * es)`) and then takes a vector / matrix-core kernel or one
that reads element by element.  Every other GPU test passes fresh torch allocations (256-byte aligned), so only the first kind ran.

Each case here runs a call on aligned buffers, again with ONE operand moved off the grid, and once with all of them moved, and wants
ids, codes, partition ids and the bits of every distance equal to the aligned run's and to the CPU oracle / specification the
neighbouring test files use.  Where the library counts the fast kernel's launches (`count:<stage>`: every ScopedTimer name counts),
the aligned call must have launched it and the moved call must not -- otherwise a fallback would be compared with itself; where
there is no counter the gate is named in a comment.

Offsets: f32 4, 8, 12 (8 separates the `& 7` gates from the `& 15` ones); f16 2 and 8; int8 / code bytes 1 and 4.  No case hands a
kernel a pointer that the audited code neither gates nor reads element-wise.  Sorted last: newest device code last."""
import functools

import numpy as np
import pytest

import refine_spec as F
import rq_spec as RQ
import sq_spec as SQ

pytestmark = pytest.mark.gpu
f32 = np.float32
OFFSETS = {"float32": (4, 8, 12), "float16": (2, 8), "int8": (1, 4), "uint8": (1, 4), "int32": (4, 8, 12), "int64": (8,)}


def eng():
    import lance_amd
    return lance_amd.default_engine()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint32:
        a = a.view(np.int32)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    return torch.from_numpy(a).cuda()


def off_view(t, nbytes):
    """a copy of the contiguous device tensor t that starts `nbytes` after a 256-byte boundary"""
    import torch
    assert t.is_cuda and t.is_contiguous() and nbytes % t.element_size() == 0
    size = t.numel() * t.element_size()
    buf = torch.empty(size + 512, dtype=torch.uint8, device=t.device)
    start = (-buf.data_ptr()) % 256 + nbytes
    v = buf[start:start + size].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 256 == nbytes % 256 and v.data_ptr() % 16 == nbytes % 16 and v.is_contiguous()
    return v


def offsets(t):
    return OFFSETS[str(t.dtype).replace("torch.", "")]


def moved(operands, movable=None):
    """operands: {name: device tensor}.  -> [(label, {name: tensor})]: aligned first, then one movable operand at a time at each of its
    offsets, then all of them at their first offset"""
    movable = list(operands) if movable is None else movable
    out = [("aligned", dict(operands))]
    for name in movable:
        for o in offsets(operands[name]):
            out.append((f"{name}+{o}", dict(operands, **{name: off_view(operands[name], o)})))
    if len(movable) > 1:
        out.append(("all", dict(operands, **{name: off_view(operands[name], offsets(operands[name])[0]) for name in movable})))
    return out


def misaligned(t, a):
    return t.data_ptr() % a != 0


def counted(names, fn):
    """-> (fn(), {name: launches of stage `name` enqueued by the call})"""
    e = eng()
    before = [e.timing_query("count:" + n)[1] for n in names]
    out = fn()
    e.synchronize()
    return out, {n: int(e.timing_query("count:" + n)[1] - b) for n, b in zip(names, before)}


def bits(t):
    a = t.cpu().numpy() if hasattr(t, "cpu") else np.ascontiguousarray(t)
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}.get(a.dtype.itemsize, np.uint8))


def same(a, b):
    a, b = bits(a), bits(b)
    return a.shape == b.shape and bool((a == b).all())


def rows(n, d, seed, kind="float32"):
    rng = np.random.default_rng(seed)
    centers = rng.normal(0, 4, (24, d))
    x = centers[rng.integers(0, 24, n)] + rng.normal(0, 1, (n, d))
    if kind == "int8":
        return np.clip(np.rint(x * 8), -127, 127).astype(np.int8)
    return x.astype(kind)


def model_kind(kind):
    return "float32" if kind == "int8" else kind


# ---- the helper and the engine's plumbing ---------------------------------------------------------------------------------------------
def test_views_reach_the_library_unchanged():
    """engine.py hands contiguous device views on as they are: what a test moves off the grid is what the kernels are given"""
    import torch
    from lance_amd import engine as E
    for kind, o in (("float32", 4), ("float32", 8), ("float32", 12), ("float16", 2), ("float16", 8), ("int8", 1), ("int8", 4)):
        t = dev(rows(33, 20, 1, kind))
        v = off_view(t, o)
        assert torch.equal(v, t) and v.data_ptr() % 16 == o
        assert E.to_device(v).data_ptr() == v.data_ptr() and E._vec(v)[0].data_ptr() == v.data_ptr()
        assert E._like(v, v).data_ptr() == v.data_ptr() and E._raw_column(v, v.dtype).data_ptr() == v.data_ptr()
        if kind != "int8":
            assert E._model(v, v).data_ptr() == v.data_ptr()
    c = off_view(dev(np.arange(64, dtype=np.uint8).reshape(4, 16)), 1)
    assert E.to_device(c, torch.uint8).data_ptr() == c.data_ptr()


# ---- assign -----------------------------------------------------------------------------------------------------------------------------
# d = 16 / 128, k = 32, n = 2048: the matrix-core sweep (xform_fused.hip:1218-1219, mfma_assign.hip:783-790: x_aligned && cent_aligned);
# d = 144, k = 64: the K-tiled matrix-core route has NO pointer gate (mfma_assign.hip:771-776): rows and centroids go through ld_elem;
# d = 20: wide.hip:61 (vec_ok = x_aligned && cent_aligned) -- no counter separates its two stagings.
# f16 / int8 rows and f16 centroids are widened element by element into scratch first (dtype.hip:11-20): the kernels see an aligned f32
# copy of those, and the caller's pointer of f32 rows and f32 centroids (the model of an Int8 column is f32).
@pytest.mark.parametrize("kind", ["float32", "float16", "int8"])
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("d,k", [(16, 32), (128, 32), (144, 64), (20, 32)])
def test_assign(oracle, d, k, metric, kind):
    x = rows(2048, d, 3 + d, kind)
    cent = rows(k, d, 4 + d, model_kind(kind))
    oi, od = oracle.assign(x, cent, metric)
    e = eng()
    # what the kernels are handed: f32 rows and f32 centroids (an Int8 column's model is f32) as they are, everything else as a widened copy
    seen_moved = lambda label: (label.startswith("x") and kind == "float32") or (label.startswith("cent") and kind != "float16") or \
        (label == "all" and kind != "float16")
    for label, op in moved({"x": dev(x), "cent": dev(cent)}):
        (gi, gd), ran = counted(["ma_sweep"], lambda: e.assign(op["x"], op["cent"], metric))
        assert same(gi, oi) and same(gd, od), label
        if label == "aligned":
            first = ran
            assert ran["ma_sweep"] == int(d in (16, 128)), ran
        else:
            assert ran["ma_sweep"] == (0 if seen_moved(label) else first["ma_sweep"]), (label, ran)


# ---- find_partitions -------------------------------------------------------------------------------------------------------------------
# mfma_assign.hip:1479 (q | cent) & 15, then the size gate of :1486-1487 (nq * nlist * d >= 2^27; d > 128: nq * nlist >= 2^23): the
# smallest batches that cross it.  Aligned: the fused kernel (nlist 32, d 16: count:coarse_fused) / the K-tiled sweep, whose selection
# is the only one timed as select_probes from this entry point; moved: the exact distance matrix (pairwise.hip:207-209).
# (Far more rows than the other cases, forced by that gate: 16 MB / 69 MB of queries, eight calls each; a case measured under 0.1 s on an
# MI355X, the oracle about 0.1 s.)
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("nlist,d,nq,stage", [(32, 16, 1 << 18, "coarse_fused"), (64, 132, 1 << 17, "select_probes")])
def test_find_partitions(oracle, nlist, d, nq, stage, metric):
    q = np.tile(rows(4096, d, 11 + d), (nq // 4096, 1)) + np.arange(nq, dtype=f32)[:, None] * f32(2.0 ** -12)
    q = np.ascontiguousarray(q, f32)
    cent = rows(nlist, d, 12 + d)
    oi, od = oracle.find_partitions(q, cent, 4, metric)
    e = eng()
    for label, op in moved({"q": dev(q), "cent": dev(cent)}):
        (gi, gd), ran = counted([stage], lambda: e.find_partitions(op["q"], op["cent"], 4, metric))
        assert same(gi, oi) and same(gd, od), label
        assert ran[stage] == (1 if label == "aligned" else 0), label


# ---- ivfpq_encode / pq_encode ---------------------------------------------------------------------------------------------------------
def encode_oracle(oracle, x, cent, cb, metric):
    part, _ = oracle.assign(x, cent.astype(np.float16) if x.dtype == np.float16 else cent, metric)
    res = oracle.residual(x, cent, np.where(part == oracle.NONE, 0, part)) if metric == "l2" else x
    return part, oracle.pq_encode(res, cb, "l2")


def xform_ok(op, m):        # xform_fused.hip:975-976
    es = op["x"].element_size()
    return not (misaligned(op["x"], 4 * es) or misaligned(op["cent"], 16) or misaligned(op["cb"], 16) or misaligned(op["codes"], 4))


def lane_encode_ok(op, m):  # encode_fused.hip:111-114: the rows, the model, and the codes a lane stores as 16-byte pieces or 4-byte words
    es = op["x"].element_size()
    return not (misaligned(op["x"], 4 * es) or misaligned(op["cent"], 16) or misaligned(op["cb"], 16) or misaligned(op["codes"], 16 if m % 16 == 0 else 4))


def pq_mfma_ok(op):         # pq_mfma.hip:342-345 (n >= 2048 is the caller's): the rows and the model; the codes are stored byte by byte
    es = op["x"].element_size()
    return not (misaligned(op["x"], 4 * es) or misaligned(op["cent"], 16) or misaligned(op["cb"], 16))


# n = 2048: the single-kernel transform (xform_fused); when it refuses the codes alone (1 byte off) the matrix-core encoder takes the
# rows natively and stores code bytes one by one (pq_mfma.hip:223,279; timed as encode_fused).  n = 300 is below pq_mfma's n >= 2048
# (pq_mfma.hip:342) and below the transform's: the lane-per-row encoder answers (encode_fused.hip), whose code stores are 16 bytes wide
# at M = 16 and 4 bytes wide at M = 8.  Whatever refuses, the staged route (assign, residual, pq_encode: element-wise) answers.
@pytest.mark.parametrize("kind", ["float32", "float16", "int8"])
@pytest.mark.parametrize("d,m,n", [(128, 16, 2048), (64, 16, 2048), (64, 8, 300), (128, 16, 300)])
def test_ivfpq_encode(oracle, d, m, n, kind):
    import torch
    from lance_amd import _lib
    nlist = 32
    x = rows(n, d, 20 + d + m, kind)
    mk = model_kind(kind)
    cent = rows(nlist, d, 21 + d, mk)
    cb = np.random.default_rng(22 + d + m).normal(0, 1, (m, 256, d // m)).astype(mk)
    part, codes = encode_oracle(oracle, x, cent, cb, "l2")
    e = eng()
    dt = {"float32": _lib.F32, "float16": _lib.F16, "int8": _lib.I8}[kind]
    ops = {"x": dev(x), "cent": dev(cent), "cb": dev(cb), "part": torch.empty(n, dtype=torch.int32, device="cuda"),
           "codes": torch.empty((n, m), dtype=torch.uint8, device="cuda")}
    stages = ["xform_fused", "encode_fused"]
    for label, op in moved(ops):
        op["part"].fill_(-7); op["codes"].fill_(255)
        torch.cuda.synchronize()
        call = lambda: _lib.check(e.lib.lance_hip_ivfpq_encode(e.h, dt, _lib.L2, op["x"].data_ptr(), n, d, op["cent"].data_ptr(), nlist,
                                                               op["cb"].data_ptr(), m, 8, op["part"].data_ptr(), op["codes"].data_ptr(), None))
        _, ran = counted(stages, call)
        assert same(op["part"], part) and same(op["codes"], codes), label
        model_moves = kind != "float16"         # f16 centroids / codebook are widened into scratch: the kernels see an aligned model
        chk = dict(op) if model_moves else dict(op, cent=ops["cent"], cb=ops["cb"])
        if n >= 2048:
            assert ran["xform_fused"] == int(xform_ok(chk, m)), (label, ran)
            assert label != "aligned" or ran["xform_fused"] == 1
            # the transform refused: the matrix-core encoder (codes 1 byte off: no gate on them) or the lane-per-row one, both timed
            # as encode_fused -- or, with the rows / the model moved, the staged route, which is not
            assert ran["encode_fused"] == int(not xform_ok(chk, m) and (pq_mfma_ok(chk) or lane_encode_ok(chk, m))), (label, ran)
            assert not label.startswith("codes+1") or ran["encode_fused"] == 1, (label, ran)
        else:
            assert ran["xform_fused"] == 0 and ran["encode_fused"] == int(lane_encode_ok(chk, m)), (label, ran)
            assert label != "aligned" or ran["encode_fused"] == 1


# pq_encode widens / takes f32 rows and runs launch_assign per sub-quantiser: pq_mfma (pq_mfma.hip:289: x_aligned && cent_aligned) at
# n >= 2048, else the exact kernels (pairwise.hip:207-209); codes are stored byte by byte everywhere (pairwise.hip:136, wide.hip:307)
@pytest.mark.parametrize("d,m,n", [(64, 16, 2048), (64, 8, 300)])
def test_pq_encode(oracle, d, m, n):
    import torch
    from lance_amd import _lib
    x = rows(n, d, 30 + d + m)
    cb = np.random.default_rng(31 + d + m).normal(0, 1, (m, 256, d // m)).astype(f32)
    codes = oracle.pq_encode(x, cb, "l2")
    e = eng()
    ops = {"x": dev(x), "cb": dev(cb), "codes": torch.empty((n, m), dtype=torch.uint8, device="cuda")}
    for label, op in moved(ops):
        op["codes"].fill_(255)
        torch.cuda.synchronize()
        _, ran = counted(["pq_mfma_estep"], lambda: _lib.check(e.lib.lance_hip_pq_encode(e.h, _lib.F32, _lib.L2, op["x"].data_ptr(), n, d,
                                                                                          op["cb"].data_ptr(), m, 8, op["codes"].data_ptr())))
        assert same(op["codes"], codes), label
        fast = n >= 2048 and not misaligned(op["x"], 16) and not misaligned(op["cb"], 16)
        assert ran["pq_mfma_estep"] == int(fast), (label, ran)


# ---- pq_train -----------------------------------------------------------------------------------------------------------------------------
# kmeans.hip:1092: the sliced layout (16-byte loads of the residual matrix) needs (residuals & 15) == 0; otherwise the row-major matrix
# is trained in place by kernels that read it element-wise (x_aligned = false: pairwise.hip:207).  No counter: the gate is that line.
def test_pq_train(oracle):
    res = rows(1024, 16, 40)
    want, _ = oracle.pq_train(res, 4, nbits=8, max_iters=4, seed=5)
    e = eng()
    for label, op in moved({"res": dev(res)}):
        cb, _ = e.pq_train(op["res"], 4, nbits=8, max_iters=4, seed=5)
        assert same(cb, want), label


# ---- flat KNN -----------------------------------------------------------------------------------------------------------------------------
# d = 16 / 96, nq = 128: flat.hip:392-393 (fixed: (x | q) & 15) and flat_mfma.hip:273; d = 96 is a fixed dimension, so moved operands go to
# the any-dimension filter (wide.hip:350-351); d = 128, nq = 4: the fixed-dimension filter alone; d = 160, nq = 128: flat_mfma_wide.hip:316
# (count:flat_mfma_wide); f16 rows at d = 8: flat.hip:1164-1165, the native-row path, else the widened copy.
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("kind,d,nq", [("float32", 16, 128), ("float32", 96, 128), ("float32", 128, 4), ("float32", 160, 128), ("float16", 8, 128),
                                       ("int8", 16, 4)])
def test_flat_topk(oracle, kind, d, nq, metric):
    n = 3000
    x = rows(n, d, 50 + d, kind)
    q = rows(nq, d, 51 + d, kind)
    oi, od = oracle.flat_knn(x, q, 10, metric)
    e = eng()
    for label, op in moved({"x": dev(x), "q": dev(q)}):
        (gi, gd), ran = counted(["flat_mfma_wide"], lambda: e.flat_topk(op["x"], op["q"], 10, metric))
        assert same(gi, oi) and same(gd, od), label
        if d == 160:
            assert (ran["flat_mfma_wide"] >= 1) == (label == "aligned"), (label, ran)


# k > 128, and f16 columns under dot / cosine, keep the older query-per-lane route (flat.hip:1169-1216): launch_flat_fixed at the fixed
# dimensions, flat_scan_generic_kernel otherwise.  Both read q and x one element at a time (flat.hip:66-68, :82, :110, :123): no gate.
@pytest.mark.parametrize("kind,metric,d", [("float32", "l2", 32), ("float32", "dot", 20), ("float16", "dot", 24), ("float16", "cosine", 32)])
def test_flat_topk_query_per_lane_route(oracle, kind, metric, d):
    x = rows(3000, d, 55 + d, kind)
    q = rows(8, d, 56 + d, kind)
    k = 200 if kind == "float32" else 10
    oi, od = oracle.flat_knn(x, q, k, metric)
    e = eng()
    for label, op in moved({"x": dev(x), "q": dev(q)}):
        gi, gd = e.flat_topk(op["x"], op["q"], k, metric)
        assert same(gi, oi) and same(gd, od), label


# ---- IVF-PQ search: the routes of the plan with the queries moved -------------------------------------------------------------------------
# search_plan.h:127-129: the matrix-core bound pass reads queries and centroids as 8-byte pairs (search_ms.hip:750,757) and is refused at
# 4 bytes off -- L2 keeps the integer bound pass, dot leaves the quantised flow for the exact pair scan; at 8 bytes off it stays.  The
# refine loses its pair kernel and the u8 copy whenever q is off the 16-byte grid (search.hip:1337-1339).  integer_scan / tiled_pt /
# small_batch: the only query gate is a.vec4 (search_q.hip:1333), which has no counter; select_probes: mfma_assign.hip:1479.
@pytest.mark.parametrize("name", ["mscan_pm", "integer_scan", "tiled_pt", "small_batch", "dot_mscan"])
def test_ivfpq_search_routes(oracle, name):
    import torch
    import search_routes_spec as R
    e = eng()
    index, nq, k, nprobes, rf, _ = R.CASES[name]
    gidx, oidx, raw, q = R.build(e, oracle, index)
    q = q[:nq]
    oi, od = oidx.search(q, k, nprobes, refine=rf, raw=raw if rf else None)
    stages = ["ivfpq_msbound", "ivfpq_mscan", "refine", "refine_u8"]
    for label, op in moved({"q": dev(q)}):
        if label == "q+12":
            continue
        # (engine=: the spec caches its indices per process, and the context they were built through may be closed by now)
        (gi, gd), ran = counted(stages, lambda: gidx.search(op["q"], k, nprobes, rf, engine=e))
        assert same(gi, oi) and same(gd, od), (name, label)
        if label == "aligned":
            first = ran
            assert ran["ivfpq_msbound"] == int(name in ("mscan_pm", "dot_mscan")) and ran["refine"] == int(rf > 0)
            assert ran["refine_u8"] == int(name == "mscan_pm")
        else:
            assert ran["refine"] == first["refine"] and ran["refine_u8"] == 0, (name, label, ran)
            assert ran["ivfpq_msbound"] == (first["ivfpq_msbound"] if label == "q+8" else 0), (name, label, ran)
            if name == "dot_mscan" and label == "q+4":
                assert ran["ivfpq_mscan"] == 0
            else:
                assert ran["ivfpq_mscan"] == first["ivfpq_mscan"]


# lance_hip_pq_scan_topk copies what it is given into an index of its own -- the codes byte by byte (build.hip:192-202), the codebook and
# row ids with hipMemcpy / the element-wise widen (build.hip:515-519, :600) -- so the alignment branches of launch_scan
# (search.hip:1271-1282) never see a caller's pointer: moved operands run the kernels the aligned ones run.
def test_pq_scan_topk(oracle):
    rng = np.random.default_rng(60)
    d, m, n_p = 32, 8, 700
    cb = rng.normal(0, 1, (m, 256, d // m)).astype(f32)
    codes_t = rng.integers(0, 256, (m, n_p)).astype(np.uint8)
    rid = rng.permutation(n_p).astype(np.uint64) * np.uint64(3)
    qr = rng.normal(0, 1, d).astype(f32)
    lut = oracle.build_lut(qr, cb, "l2")
    wi, wd = oracle.heap_topk(oracle.pq_scan(lut, codes_t, "l2"), rid, 10)
    wi, wd = oracle.sort_fetch(wi, wd, 10)
    e = eng()
    for label, op in moved({"q": dev(qr), "cb": dev(cb), "codes": dev(codes_t), "rid": dev(rid)}):
        gi, gd = e.pq_scan_topk(op["q"], op["cb"], op["codes"], op["rid"], 10, "l2")
        assert same(gi, wi) and same(gd, wd), label


# ---- refine: IVF_PQ over f32 / f16 / int8 raw vectors ---------------------------------------------------------------------------------------
# search.hip:1337-1339: f32 rows of whole 16-element chunks with raw and q on the 16-byte grid take the pair kernel, integer-valued ones
# its u8 copy (raw_compact_prepare: search.hip:1073-1074); otherwise refine_kernel, which reads raw through ld_elem (exact.cuh:123-125)
# for every element type.  keff = 20.
@functools.lru_cache(maxsize=None)
def refine_setup(kind):
    import oracle
    from lance_amd.engine import DeviceIndex
    n, d, m, nlist = 3000, 64, 16, 8
    rng = np.random.default_rng(70)
    centers = rng.uniform(0, 100, (24, d))
    x = np.clip(np.rint(centers[rng.integers(0, 24, n)] + rng.normal(0, 15, (n, d))), 0, 120)
    q = np.clip(np.rint(centers[rng.integers(0, 24, 64)] + rng.normal(0, 15, (64, d))), 0, 120)
    x, q = (x.astype(kind), q.astype(kind)) if kind != "float16" else ((x * 0.05).astype(np.float16), (q * 0.05).astype(np.float16))
    cent, _, _, _ = oracle.kmeans_train(x[:2048].astype(f32), nlist, max_iters=4, seed=1)
    cent = cent.astype(model_kind(kind))
    part, _ = oracle.assign(x, cent, "l2")
    cb, _ = oracle.pq_train(oracle.residual(x, cent, part)[:2048], m, max_iters=3, seed=2)
    cb = np.asarray(cb).astype(model_kind(kind))
    wide = (lambda a: a.astype(f32)) if kind == "int8" else (lambda a: a)      # Int8 columns are widened exactly: the oracle takes the f32 values
    oidx = oracle.build_index(wide(x), cent, cb, "l2")
    e = eng()
    gpart, gcodes, _ = e.ivfpq_encode(x, cent, cb, "l2")
    gidx = DeviceIndex.create(e, "l2", cent, cb, gpart, gcodes, None, raw=x, dtype=kind)
    oi, od = oidx.search(wide(q), 10, 4, refine=2, raw=x.astype(f32))
    return gidx, x, q, oi, od


@pytest.mark.parametrize("kind", ["float32", "float16", "int8"])
def test_ivfpq_refine(kind):
    gidx, x, q, oi, od = refine_setup(kind)
    try:
        for label, op in moved({"raw": dev(x), "q": dev(q)}):
            gidx.set_raw(op["raw"])
            (gi, gd), ran = counted(["refine", "refine_u8"], lambda: gidx.search(op["q"], 10, 4, 2))
            assert same(gi, oi) and same(gd, od), label
            assert ran["refine"] == 1 and ran["refine_u8"] == int(kind == "float32" and label == "aligned"), (label, ran)
    finally:
        gidx.set_raw(dev(x))


# ---- IVF_SQ and IVF_RQ: search and refine with q and raw moved; IVF_FLAT with q moved -----------------------------------------------------
@functools.lru_cache(maxsize=None)
def sqrq_setup(kind):
    import oracle
    import test_zz_gpu_refine_sqrq as T
    n, d, nlist, nq = 2000, 64, 8, 64
    rid = np.random.default_rng(17).permutation(n).astype(np.uint64)
    if kind == "rq":
        x, q = RQ.clustered(n, d, nq, 3)
        cent = np.ascontiguousarray(x[np.random.default_rng(1).choice(n, nlist, replace=False)])
        ix, spec = T.rq_index(x, cent, RQ.rotation(d, 7), "l2", rid)
    else:
        x, q = SQ.gaussian(n, d, nq, seed=31)
        cent = SQ.centroids_with_gaps(x, nlist, seed=2)
        ix, spec = T.sq_index(x, cent, "l2", rid)
    cand = T.candidates(spec, q, 20, 4)
    s = spec[2]      # the unrefined search at k = 10: ids and distances of the index type's specification
    if kind == "rq":
        plain = RQ.search(oracle, s[0], s[1], s[2], s[3], s[4], s[5], q, 10, 4, "l2", row_ids=rid)
    else:
        plain = SQ.search(oracle, s[0], s[1], s[2], q, 10, 4, "l2", *s[3], row_ids=rid)
    return ix, spec, q, cand, plain


@pytest.mark.parametrize("kind", ["sq", "rq"])
def test_ivf_sq_rq_search_and_refine(oracle, kind):
    """the queries go through the element-wise encoders / rq_prepare (sq.hip:84-91, rq.hip:163-167) and the coarse quantiser's gate
    (mfma_assign.hip:1479); the refine is IVF_PQ's (search.hip:1337: raw | q)"""
    ix, spec, q, cand, plain = sqrq_setup(kind)
    raw = spec[4]
    want_i, want_d = F.refine(oracle, cand, raw, q, 10, "l2")
    try:
        for label, op in moved({"raw": dev(raw), "q": dev(q)}):
            ix.set_raw(op["raw"])
            gi, gd = ix.search(op["q"], 10, 4)
            assert same(gi, plain[0]) and same(gd, plain[1]), label
            (gi, gd), ran = counted(["refine"], lambda: ix.search(op["q"], 10, 4, refine_factor=2))
            assert same(gi, want_i) and same(gd, want_d), label
            assert ran["refine"] == 1
    finally:
        ix.set_raw(dev(raw))


# flat.hip:1034-1035: the partition-major kernels read four query elements at a time and need (q & 15) == 0; the query-major kernel
# stages the query element by element (flat.hip:583-586, :695).  No counter: the gate is that line.
@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_ivfflat_search(oracle, metric):
    from lance_amd.engine import DeviceFlatIndex
    n, d, nlist = 3000, 32, 8
    x, q = rows(n, d, 80), rows(200, d, 81)
    cent = rows(nlist, d, 82)
    part, _ = oracle.assign(x, cent, metric)
    oi, od = oracle.ivfflat_search(x, cent, q, 10, 4, metric)
    ix = DeviceFlatIndex.create(eng(), metric, cent, x, part.view(np.int32))
    for label, op in moved({"q": dev(q)}):
        gi, gd = ix.search(op["q"], 10, 4)
        assert same(gi, oi) and same(gd, od), label


# ---- scalar quantiser building blocks --------------------------------------------------------------------------------------------------
# sq.hip:611: rows of whole 16-byte words at an aligned base are read 16 bytes per lane, anything else word by word from bytes
# (sq.hip:147-157).  Both run under the one sq_distance timer: the gate is that line.  Bounds and encode read x element by element.
@pytest.mark.parametrize("kind", ["float32", "float16"])
@pytest.mark.parametrize("d", [16, 20])
def test_sq_blocks(d, kind):
    x, q = SQ.gaussian(700, d, 5, seed=90 + d, kind="f16" if kind == "float16" else "f32")
    b = SQ.bounds(np.asarray(x, f32)[100:164])
    codes = SQ.encode(np.asarray(x, f32), *b)
    want = SQ.distances(codes, np.asarray(q, f32), "l2", *b)
    e = eng()
    for label, op in moved({"x": dev(x), "q": dev(q), "codes": dev(codes)}):
        assert e.sq_bounds(op["x"]) == SQ.bounds(np.asarray(x, f32)), label
        assert same(e.sq_encode(op["x"], b), codes), label
        got, ran = counted(["sq_distance"], lambda: e.sq_distance(op["codes"], op["q"], b, "l2"))
        assert same(got, want) and ran["sq_distance"] == 1, label


# ---- RaBitQ building blocks -------------------------------------------------------------------------------------------------------------
# rq.hip:617: rows of whole 16-byte words (d % 128 == 0) are read as such (rq.hip:218-228, :239-249) and REFUSED off the grid; shorter
# rows are read byte by byte from any base.  rq_encode reads x, the centroids and the rotation element by element (rq.hip:102-116).
@pytest.mark.parametrize("d", [64, 128])
def test_rq_blocks(oracle, d):
    import lance_amd
    x, q = RQ.clustered(600, d, 4, 5)
    cent = np.ascontiguousarray(x[:4])
    P = RQ.rotation(d, 9)
    part, codes, add, scale = RQ.build(oracle, x, cent, P, "l2")
    dvc = oracle.assign(x, cent, "l2")[1]
    e = eng()
    for label, op in moved({"x": dev(x), "cent": dev(cent), "rot": dev(P)}):
        gc, ga, gs = e.rq_encode(op["x"], part.view(np.int32), dvc, op["cent"], op["rot"], "l2")
        assert same(gc, codes) and same(ga, add) and same(gs, scale), label
    sel = np.flatnonzero(part == 0)
    qr = np.ascontiguousarray(q - cent[0])
    dqc = np.linspace(0.5, 2.0, len(q)).astype(f32)                  # (an input of the calculator: any value serves)
    for quantised in (True, False):
        want = RQ.distances(codes[sel], add[sel], scale[sel], qr, dqc, P, "l2", quantised)
        for label, op in moved({"codes": dev(codes[sel]), "qr": dev(qr), "rot": dev(P)}):
            call = lambda: e.rq_distance(op["codes"], add[sel], scale[sel], op["qr"], dqc, op["rot"], "l2", quantised)
            if d % 128 == 0 and misaligned(op["codes"], 16):
                with pytest.raises(lance_amd.LanceHipError, match="codes of 16-byte rows must be 16-byte aligned") as ei:
                    call()
                assert ei.value.code == lance_amd._lib.EINVAL, label
                continue                                        # ... and the context serves the next call
            assert same(call(), want), (label, quantised)


# ---- rebalance: raw is the caller's -----------------------------------------------------------------------------------------------------
# rebalance.hip:114,119 (the decision kernel) and :307 (the gather of arriving rows) read raw[id * d + c] one element at a time: no gate.
def test_reassign_rows():
    import test_zz_gpu_rebalance as T
    c, want = T.case(1, 5, 20, "l2")
    e = eng()
    for label, op in moved({"raw": dev(c["raw"])}):
        dest, ran = counted(["rebalance_reassign"], lambda: e.reassign_rows("l2", op["raw"], c["ids"][want["pos"]], want["seg_offs"], want["seg_cent"],
                                                                             np.asarray(want["cands"], np.uint32), c["c12"], c["part"], len(c["centroids"])))
        assert same(dest, want["dest"]) and ran["rebalance_reassign"] == 1, label


@pytest.mark.parametrize("kind,nbits", [("IVF_PQ", 8), ("IVF_FLAT", 8), ("IVF_SQ", 8)])
def test_split_and_join_with_raw_moved(kind, nbits):
    import rebalance_spec as R
    import test_zz_gpu_rebalance as T
    b = T.built(kind, nbits, 1, 5, 20, "l2")
    c = b.c
    cent, offs, ids, cols, _ = R.split_storage(kind, "l2", c["centroids"], c["offs"], c["ids"], b.cols, c["part"], c["raw"], c["c12"], **b.model)
    jcent, joffs, jids, jcols, _ = R.join_storage(kind, "l2", c["centroids"], c["offs"], c["ids"], b.cols, 0, c["raw"], **b.model)
    for label, op in moved({"raw": dev(c["raw"])}):
        got = b.ix.split(c["part"], c["c12"], op["raw"])
        assert T.same_storage(T.stored(got), offs, ids, cols) and same(got.centroids, cent), label
        got = b.ix.join(0, op["raw"])
        assert T.same_storage(T.stored(got), joffs, jids, jcols) and same(got.centroids, jcent), label


# ---- normalize, residual ----------------------------------------------------------------------------------------------------------------
# build.hip:34-53, :61-106 (normalize: element loads; d = 70 takes the tiled kernel) and build.hip:151-163 (residual): no gate
@pytest.mark.parametrize("kind", ["float32", "float16"])
@pytest.mark.parametrize("d", [20, 70])
def test_normalize_and_residual(oracle, d, kind):
    import torch
    from lance_amd import _lib
    x = rows(500, d, 100 + d, kind)
    cent = rows(8, d, 101 + d, kind)
    part, _ = oracle.assign(x, cent, "l2")
    want_n, want_r = oracle.normalize(x), oracle.residual(x, cent, part)
    e = eng()
    dt = _lib.F16 if kind == "float16" else _lib.F32
    ops = {"x": dev(x), "cent": dev(cent), "out": torch.empty_like(dev(x))}
    part_d = dev(part)
    for label, op in moved(ops):
        assert same(e.normalize(op["x"]), want_n), label
        op["out"].zero_()
        torch.cuda.synchronize()
        _lib.check(e.lib.lance_hip_normalize(e.h, dt, op["x"].data_ptr(), 500, d, op["out"].data_ptr()))
        assert same(op["out"], want_n), label
        _lib.check(e.lib.lance_hip_residual(e.h, dt, op["x"].data_ptr(), 500, d, op["cent"].data_ptr(), part_d.data_ptr(), op["out"].data_ptr()))
        assert same(op["out"], want_r), label
