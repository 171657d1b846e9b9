"""Re-ranking for IVF_SQ and IVF_RQ on the GPU (lance_hip_ivfsq_search_refine / lance_hip_ivfrq_search_refine) against
tests/refine_spec.py, ids exactly and distances as bits: keff = k * refine_factor candidates through the scan / merge / replay of
pair_cand.cuh at its narrow capacity (keff <= 128) or its wide one (128 < keff <= 768), then the exact refine against the raw vectors
with the original query.  The specification is checked on the CPU by tests/test_refine_spec.py and the kernels' source is run on the
CPU by tests/test_wide_cand_kernels_cpu.py.  Sorted last: newest device code last."""
import ctypes as C
import functools

import numpy as np
import pytest

import refine_spec as F
import rq_spec as R
import sq_spec as S

pytestmark = pytest.mark.gpu
f32 = np.float32
UNSET = F.UNSET


def eng():
    import lance_amd
    return lance_amd.default_engine()


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


def wide_cap(fixed):
    """cand_scan_cap above 128 candidates (pair_cand.cuh): the largest power of two whose 8-byte entries fit beside `fixed` bytes in 64 KiB"""
    cap = 1024
    while fixed + cap * 16 <= 65536:
        cap *= 2
    return cap


def rq_cap(d):
    return wide_cap(20 * d + 24 + 16)


def sq_cap(d):
    return wide_cap((d + 15) // 16 * 16 + 16)


# ---- indices next to what the specification needs ----------------------------------------------------------------------------------
def rq_index(x, cent, P, metric, rid, raw=None, built=None):
    import oracle
    from lance_amd.engine import DeviceRqIndex
    part, codes, add, scale = built or R.build(oracle, x, cent, P, metric)
    e = eng()
    gc, ga, gs = e.rq_encode(x, part.view(np.int32), oracle.assign(x, cent, metric)[1], cent, P, metric)
    assert (gc.cpu().numpy() == codes).all() and same_bits(ga.cpu().numpy(), add) and same_bits(gs.cpu().numpy(), scale)
    ix = DeviceRqIndex.create(e, metric, cent, P, gc, ga, gs, part.view(np.int32), row_ids=rid)
    raw = F.raw_by_row_id(x, rid) if raw is None else raw
    ix.set_raw(raw)
    return ix, ("rq", metric, (codes, add, scale, part, cent, P), rid, raw)


def sq_index(x, cent, metric, rid, bounds=None, raw=None):
    import oracle
    from lance_amd.engine import DeviceSqIndex
    xs, part = S.prepare_rows(oracle, x, cent, metric)
    b = S.bounds(xs[:64]) if bounds is None else bounds
    ix = DeviceSqIndex.create(eng(), metric, cent, eng().sq_encode(xs, b), part, b, row_ids=rid)
    raw = F.raw_by_row_id(x, rid) if raw is None else raw
    ix.set_raw(raw)                                              # the ORIGINAL rows: xs is their normalised copy under cosine
    return ix, ("sq", metric, (S.encode(xs, *b), part, cent, b), rid, raw)


def candidates(spec, q, keff, nprobes, allow=None):
    """the keff candidates of every query: the index type's specification at k = keff"""
    import oracle
    kind, metric, s, rid, _ = spec
    if kind == "rq":
        codes, add, scale, part, cent, P = s
        return R.search(oracle, codes, add, scale, part, cent, P, q, keff, nprobes, metric, row_ids=rid, prefilter=allow)[0]
    codes, part, cent, b = s
    return S.search(oracle, codes, part, cent, q, keff, nprobes, metric, *b, row_ids=rid, prefilter=allow)[0]


@functools.lru_cache(maxsize=None)
def spec_candidates(key, keff, nprobes, mask_key=None):
    """of a cached setup (the slow part of the specification: shared by the (k, refine_factor) cases with the same keff)"""
    _, spec, q = SETUPS[key]()
    return candidates(spec, q, keff, nprobes, None if mask_key is None else MASKS[mask_key](spec[3]))


def search(ix, q, k, nprobes, rf, allow=None):
    gi, gd = ix.search(q, k, nprobes, allow=allow, refine_factor=rf)
    return gi.cpu().numpy().view(np.uint64), gd.cpu().numpy()


def check_refined(ix, spec, q, k, rf, nprobes, cand, allow=None):
    import oracle
    gi, gd = search(ix, q, k, nprobes, rf, allow)
    oi, od = F.refine(oracle, cand, spec[4], q, k, spec[1])
    assert (gi == oi).all(), (k, rf, np.argwhere(gi != oi)[:4])
    assert same_bits(gd, od), (k, rf)
    return oi


# ---- both routes, and the 128 / 129 boundary -----------------------------------------------------------------------------------------
N, D, NLIST, NPROBES, NQ = 4000, 64, 16, 4, 100


@functools.lru_cache(maxsize=None)
def routes_setup(kind, metric, dtype):
    import oracle
    rid = np.random.default_rng(17).permutation(N).astype(np.uint64)         # permuted row ids below n
    if kind == "rq":
        x, q = R.clustered(N, D, NQ, 3)
        cent = np.ascontiguousarray(x[np.random.default_rng(1).choice(N, NLIST, replace=False)])
        ix, spec = rq_index(x, cent, R.rotation(D, 7), metric, rid)
    else:
        x, q = S.gaussian(N, D, NQ, seed=31, kind=dtype)
        cent = S.centroids_with_gaps(oracle.normalize(x) if metric == "cosine" else x, NLIST, seed=2)
        ix, spec = sq_index(x, cent, metric, rid)
    return ix, spec, q


CONFIGS = [("rq", "l2", "f32"), ("rq", "dot", "f32"), ("sq", "l2", "f32"), ("sq", "dot", "f32"), ("sq", "cosine", "f32"), ("sq", "l2", "f16"),
           ("sq", "cosine", "f16")]
SETUPS = {"/".join(c): functools.partial(routes_setup, *c) for c in CONFIGS}
MASKS = {"half": lambda rid: np.random.default_rng(23).random(int(rid.max()) + 1) < 0.5,
         "few": lambda rid: np.isin(np.arange(int(rid.max()) + 1), np.sort(rid)[[5, 900, 2100, 3300, 3999]])}


@pytest.mark.parametrize("k,rf", [(10, 2), (128, 1), (129, 1), (10, 50), (768, 1), (96, 8)])
@pytest.mark.parametrize("config", CONFIGS, ids="/".join)
def test_both_routes(config, k, rf):
    """keff = 20 and 128 run scan / merge / replay at the narrow capacity, 129, 500 and 768 at the wide one (asserted by the kernel timers)"""
    key = "/".join(config)
    ix, spec, q = SETUPS[key]()
    e = eng()
    names = ["ivf%s_scan" % config[0], "ivf%s_wide_scan" % config[0], "refine"]
    e.timing(True)
    try:
        for n in names:
            e.timing_query(n)                                    # (a query returns a timer's launches and resets it)
        check_refined(ix, spec, q, k, rf, NPROBES, spec_candidates(key, k * rf, NPROBES))
        ran = [e.timing_query(n)[1] for n in names]
    finally:
        e.timing(False)
    assert ran == ([1, 0, 1] if k * rf <= 128 else [0, 1, 1])


def test_refine_factor_one_and_python_surface():
    """refine_factor = 1 keeps the unrefined id set; IvfRqIndex / IvfSqIndex.nearest forward refine_factor and prefilter"""
    import lance_amd
    for key in ("rq/l2/f32", "sq/cosine/f16"):
        ix, spec, q = SETUPS[key]()
        ui, _ = ix.search(q, 10, NPROBES)
        ri, _ = search(ix, q, 10, NPROBES, 1)
        assert (np.sort(ui.cpu().numpy().view(np.uint64), axis=1) == np.sort(ri, axis=1)).all()
        wrap = (lance_amd.vector.IvfRqIndex if key.startswith("rq") else lance_amd.vector.IvfSqIndex)(ix, None, None, None)
        ni, nd = wrap.nearest(q, 10, NPROBES, refine_factor=50)
        gi, gd = search(ix, q, 10, NPROBES, 50)
        assert (ni == gi).all() and same_bits(nd, gd)
        m = MASKS["half"](spec[3])
        ni, nd = wrap.nearest(q, 10, NPROBES, refine_factor=5, prefilter=m)
        gi, gd = search(ix, q, 10, NPROBES, 5, allow=m)
        assert (ni == gi).all() and same_bits(nd, gd)


def test_create_index_keeps_the_original_column():
    """create_index(keep_raw=True) attaches x itself -- under cosine not the normalised rows the codes are made from"""
    import lance_amd
    import oracle
    x, q = S.gaussian(1500, 32, 20, seed=8)
    for itype, metric in (("IVF_SQ", "cosine"), ("IVF_RQ", "l2")):
        idx = lance_amd.create_index(x, itype, metric=metric, num_partitions=4, max_iters=5)
        ids, dists = idx.nearest(q, k=10, nprobes=4, refine_factor=50)       # what comes back carries the exact distances to x, in order
        for qi in range(len(q)):
            ei, ed = oracle.flat_knn(np.ascontiguousarray(x[ids[qi].astype(np.int64)]), q[qi:qi + 1], 10, metric, row_ids=ids[qi])
            assert (ei[0] == ids[qi]).all() and same_bits(ed[0], dists[qi])
        bare = lance_amd.create_index(x, itype, metric=metric, num_partitions=4, max_iters=5, keep_raw=False)
        with pytest.raises(NotImplementedError, match="refine_factor.*set_raw"):
            bare.nearest(q, k=10, nprobes=4, refine_factor=2)
        bare.set_raw(x)
        bi, bd = bare.nearest(q, k=10, nprobes=4, refine_factor=50)
        assert (bi == ids).all() and same_bits(bd, dists)


# ---- prefilter with refine ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,rf", [(10, 5), (10, 50)])
@pytest.mark.parametrize("key", ["rq/dot/f32", "sq/l2/f32", "sq/cosine/f16"])
def test_prefilter_with_refine(key, k, rf):
    ix, spec, q = SETUPS[key]()
    rid = spec[3]
    check_refined(ix, spec, q, k, rf, NPROBES, spec_candidates(key, k * rf, NPROBES, "half"), allow=MASKS["half"](rid))
    oi = check_refined(ix, spec, q, k, rf, NLIST, spec_candidates(key, k * rf, NLIST, "few"), allow=MASKS["few"](rid))
    assert (oi[:, :5] != UNSET).all() and (oi[:, 5:] == UNSET).all()      # five rows selected, all partitions probed: padded with ~0 / +inf


# ---- fewer candidates than keff --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,metric", [("rq", "l2"), ("rq", "dot"), ("sq", "l2"), ("sq", "cosine")])
def test_fewer_candidates_than_keff(kind, metric):
    """300 rows, every partition probed, keff = 768: every row is a candidate, the answer is the flat one"""
    import oracle
    x, q = R.clustered(300, 32, 9, seed=5)
    rid = np.random.default_rng(2).permutation(300).astype(np.uint64)
    cent = np.ascontiguousarray(x[[1, 50, 100, 150, 200]])
    if kind == "rq":
        ix, spec = rq_index(x, cent, R.rotation(32, 1), metric, rid)
    else:
        ix, spec = sq_index(x, oracle.normalize(cent) if metric == "cosine" else cent, metric, rid)
    for k, rf in ((768, 1), (16, 48)):
        gi, gd = search(ix, q, k, 5, rf)
        oi, od = oracle.flat_knn(x, q, k, metric, row_ids=rid)
        assert (gi == oi).all() and same_bits(gd, od)
        assert ((gi == UNSET).sum(axis=1) == max(0, k - 300)).all()


# ---- threshold logic at the wide capacity ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rq", "sq"])
@pytest.mark.parametrize("order,keff,rem", [("descending", 129, 0), ("descending", 768, 1), ("ascending", 768, 31), ("staircase", 129, 1),
                                            ("staircase", 768, 0), ("tie_cut", 129, 31), ("tie_cut", 768, 1)])
def test_ordered_partitions(kind, order, keff, rem):
    """one partition longer than the scan's buffer plus two chunks, stored in an order chosen for the design query
    (refine_spec.ordered_partition at the capacity the library picks for d = 64); the candidates are compared through k = keff,
    refine_factor = 1 -- the refined ids are the candidates' -- and through k = keff / 3 of them.  A cut tie is replayed."""
    import oracle
    cap = rq_cap(64) if kind == "rq" else sq_cap(64)
    n = (cap + 2 * F.CHUNK) // 32 * 32 + 32 + rem
    metric = "l2" if keff == 768 else "dot"
    f = F.ordered_partition(oracle, kind, order, metric, keff, cap, n)
    q = np.ascontiguousarray(np.stack([f["q"], f["x"][5] + f32(0.1)]))
    rid = np.random.default_rng(3).permutation(len(f["x"])).astype(np.uint64)
    ix, spec = rq_index(f["x"], f["cent"], f["P"], metric, rid) if kind == "rq" else sq_index(f["x"], f["cent"], metric, rid, bounds=f["bounds"])
    cand = candidates(spec, q, keff, 2)
    oi = check_refined(ix, spec, q, keff, 1, 2, cand)
    replays = eng().search_stats()
    assert (np.sort(oi, axis=1) == np.sort(cand, axis=1)).all()
    assert replays >= 1 or not f["cut_tie"]
    assert f["cut_tie"] or order != "tie_cut"
    check_refined(ix, spec, q, keff // 3, 3, 2, candidates(spec, q, keff // 3 * 3, 2))


def test_rq_largest_dimension_replays_at_768():
    """d = 2048, keff = 768: the scan's tables leave room for 2048 candidates (57,384 bytes of LDS), the replay's tables, its heap of 768
    and its merged list take 64,840 of the 65,536 bytes.  900 copies of one row tie at the design query's 768-th key, so the replay
    runs.  (The specification encodes the 141 distinct rows; a row's code does not depend on its neighbours.)"""
    import oracle
    d = 2048
    base, cent = R.sized_partitions([100, 40], d, seed=3)
    P = R.rotation(d, 4)
    part, codes, add, scale = R.build(oracle, base, cent, P, "l2")
    src = int(np.nonzero(part == 0)[0][0])
    pick = np.concatenate([np.arange(len(base)), np.full(900, src)])
    pick = pick[np.random.default_rng(6).permutation(len(pick))]
    x = np.ascontiguousarray(base[pick])
    built = (part[pick], codes[pick], add[pick], scale[pick])
    rid = np.random.default_rng(7).permutation(len(x)).astype(np.uint64)
    assert rq_cap(d) == 2048
    ix, spec = rq_index(x, cent, P, "l2", rid, built=built)
    q = np.ascontiguousarray(np.stack([base[src] + f32(0.01), base[3]]))
    cand = candidates(spec, q, 768, 2)
    check_refined(ix, spec, q, 768, 1, 2, cand)
    assert eng().search_stats() >= 1
    check_refined(ix, spec, q, 10, 76, 2, candidates(spec, q, 760, 2))


# ---- the u8 refine source --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rq", "sq"])
@pytest.mark.parametrize("k,rf", [(10, 5), (10, 30)])
def test_u8_refine_source(kind, k, rf):
    """an integer-valued f32 column (values 0..218) is re-ranked from the index's lossless u8 copy (refine_u8_kernel); the same values
    + 0.5 -- same differences, same codes, no u8 copy -- give the same ids and the same distance bits under L2"""
    import oracle
    from lance_amd.testing import sift_like
    x = sift_like(2000, 64, seed=9)
    q = sift_like(40, 64, seed=10)
    assert x.dtype == f32 and (x == np.rint(x)).all() and x.min() >= 0 and x.max() <= 218
    rid = np.random.default_rng(4).permutation(len(x)).astype(np.uint64)
    cent = np.ascontiguousarray(x[np.random.default_rng(5).choice(len(x), 8, replace=False)])
    out, took_u8 = [], []
    e = eng()
    for shift in (f32(0.0), f32(0.5)):
        xs, qs, cs = x + shift, q + shift, cent + shift
        if kind == "rq":
            ix, spec = rq_index(xs, cs, R.rotation(64, 3), "l2", rid)
        else:
            ix, spec = sq_index(xs, cs, "l2", rid, bounds=(float(shift), 218.0 + float(shift)))
        e.timing(True)
        try:
            e.timing_query("refine_u8")                          # (resets the timer)
            out.append(search(ix, qs, k, 3, rf))
            took_u8.append(e.timing_query("refine_u8")[1])
        finally:
            e.timing(False)
        if shift == 0:
            check_refined(ix, spec, qs, k, rf, 3, candidates(spec, qs, k * rf, 3))
    assert took_u8 == [1, 0]
    assert (out[0][0] == out[1][0]).all() and same_bits(out[0][1], out[1][1])


# ---- batch split ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,k,rf", [("rq", 768, 1), ("sq", 96, 8)])
def test_batch_split(kind, k, rf):
    """keff = 768 and 8 probes: 2^24 / (8 * 768) = 2730 queries per launch, so 2800 queries take two; the queries on both sides of
    the split are compared with the specification (all 2800 would take the numpy specification minutes)"""
    import oracle
    x, q = R.clustered(2000, 16, 2800, seed=12)
    rid = np.random.default_rng(8).permutation(len(x)).astype(np.uint64)
    cent = np.ascontiguousarray(x[np.random.default_rng(9).choice(len(x), 8, replace=False)])
    ix, spec = rq_index(x, cent, R.rotation(16, 2), "l2", rid) if kind == "rq" else sq_index(x, cent, "l2", rid)
    gi, gd = search(ix, q, k, 8, rf)
    for lo, hi in ((0, 32), (2700, 2800)):
        qs = np.ascontiguousarray(q[lo:hi])
        oi, od = F.refine(oracle, candidates(spec, qs, k * rf, 8), spec[4], qs, k, "l2")
        assert (gi[lo:hi] == oi).all() and same_bits(gd[lo:hi], od)


# ---- refusals --------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    import lance_amd
    from lance_amd import _lib
    from lance_amd.engine import DeviceRqIndex, DeviceSqIndex
    import oracle
    e = eng()
    lib = e.lib
    x, q = R.clustered(400, 32, 2, seed=2)
    rid = np.arange(400, dtype=np.uint64)
    cent = np.ascontiguousarray(x[[0, 100, 200, 300]])
    rq, _ = rq_index(x, cent, R.rotation(32, 1), "l2", rid)
    sq, _ = sq_index(x, cent, "l2", rid)
    pq = lance_amd.create_index(x, "IVF_PQ", num_partitions=4, num_sub_vectors=4, max_iters=4)
    qt = torch.from_numpy(q).cuda()
    ids = torch.full((2, 768), -7, dtype=torch.int64, device="cuda")
    dists = torch.zeros((2, 768), dtype=torch.float32, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    err = lambda: lib.lance_hip_last_error().decode()
    entries = {"rq": (lib.lance_hip_ivfrq_search_refine, rq), "sq": (lib.lance_hip_ivfsq_search_refine, sq)}

    def call(kind, handle, k, rf):
        return entries[kind][0](e.h, handle, p(qt), 2, k, 2, rf, None, 0, p(ids), p(dists))
    for kind, (_, ix) in entries.items():
        assert call(kind, ix.h, 10, 2) == _lib.OK
        assert call(kind, ix.h, 10, 0) == _lib.EINVAL and "refine_factor" in err()                      # scanner.rs:2869
        assert call(kind, ix.h, 769, 1) == _lib.EINVAL and "768" in err()
        assert call(kind, ix.h, 77, 10) == _lib.EINVAL and "768" in err()
        assert call(kind, ix.h, 0, 3) == _lib.EINVAL
        assert call(kind, ix.h, 384, 2) == _lib.OK
        other = entries["sq" if kind == "rq" else "rq"][1]
        assert call(kind, other.h, 10, 2) == _lib.EINVAL and "not an IVF_" in err()
        assert call(kind, pq._ix.h, 10, 2) == _lib.EINVAL and "not an IVF_" in err()
    # the four entry points without refine keep their limit
    for ix in (rq, sq):
        with pytest.raises(lance_amd.LanceHipError, match="k=129 not supported"):
            ix.search(q, 129, 1)
        with pytest.raises(lance_amd.LanceHipError, match="k=129 not supported"):
            ix.search(q, 129, 1, allow=np.ones(400, bool))
    # a stored row id beyond the raw vectors: reported, not ranked
    for kind, (_, ix) in entries.items():
        ix.set_raw(x[:200])
        assert call(kind, ix.h, 10, 60) == _lib.EINVAL and "lance_hip_index_set_raw" in err() and "row ids beyond" in err()
        assert call(kind, ix.h, 10, 5) == _lib.EINVAL and "row ids beyond" in err()
        with pytest.raises(lance_amd.LanceHipError, match="row ids beyond"):
            ix.search(q, 10, 2, refine_factor=5)
    # no raw vectors: from C, and through nearest
    part, codes, add, scale = R.build(oracle, x, cent, R.rotation(32, 1), "l2")
    gc, ga, gs = e.rq_encode(x, part.view(np.int32), oracle.assign(x, cent, "l2")[1], cent, R.rotation(32, 1), "l2")
    bare_rq = DeviceRqIndex.create(e, "l2", cent, R.rotation(32, 1), gc, ga, gs, part.view(np.int32))
    b = S.bounds(x)
    bare_sq = DeviceSqIndex.create(e, "l2", cent, e.sq_encode(x, b), part.view(np.int32), b)
    torch.cuda.synchronize()
    for kind, ix, wrap in (("rq", bare_rq, lance_amd.vector.IvfRqIndex), ("sq", bare_sq, lance_amd.vector.IvfSqIndex)):
        assert call(kind, ix.h, 10, 2) == _lib.EINVAL and "lance_hip_index_set_raw" in err()
        with pytest.raises(NotImplementedError, match="refine_factor"):
            wrap(ix, None, None, None).nearest(q, 5, 1, refine_factor=2)
        with pytest.raises(NotImplementedError, match="distance_range"):
            wrap(ix, None, None, None).nearest(q, 5, 1, refine_factor=2, distance_range=(0.0, 1.0))
