"""Row ids as a table of several fragments has them -- row ADDRESSES, fragment << 32 | offset, at and above 2^32, up to fragment 2^31 - 1,
unrelated to the storage order (tests/rowid_fixtures.py) -- through every entry point that returns ids: the flat scans, IVF_FLAT,
IVF_PQ (every scan flow, refine, prefilter, range, candidates, export / from_storage / save / load), IVF_SQ, the multivector scan,
pq_scan_topk and merge_topk.  Ids and distance bits must equal the CPU oracle's, which orders by the full 64-bit id
(SortExec(dist, rowid).fetch(k), scanner.rs:3440-3468).

Every case holds each row three times, so exact ties sit at and around the k-th distance, and tests/test_rowid_fixtures.py shows for
every case that the oracle's answer changes when ties are broken by the low word, the high word or the storage position: a kernel that
compares, carries, packs or shuffles half an id cannot pass.  Shapes are the smallest that still take the path named in each case (the
routing constants are quoted in rowid_fixtures.IVFPQ_CASES / FLAT_CASES); where the suite has a path assertion it is reused.

Refine reads the raw column BY ID: with ids that are a permutation of the rows and the column laid out by id the answers are the
oracle's; with addresses (all beyond the column) every refine kernel must refuse -- "refine met row ids beyond the ... raw vectors" --
and leave no finite distance behind.  A prefilter mask is indexed by id: ids beyond the mask are unselected, so an all-True mask of n
entries over addresses fragment << 32 | i (i < n) selects exactly the fragment-0 rows."""
import numpy as np
import pytest
import torch

import rowid_fixtures as R
from test_gpu_pm_scan import _np, _pm_used
from test_zz_gpu_dot_flow import _dot_flow_used
from test_zz_gpu_mscan import _ms_used

pytestmark = pytest.mark.gpu
f32 = np.float32
u64 = np.uint64


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def same(got, want, tag):
    gi, gd = _np(got[0]).view(u64), _np(got[1])
    oi, od = want
    assert gi.shape == oi.shape, tag
    bad = np.nonzero((gi != oi).reshape(gi.shape[0], -1).any(axis=1))[0] if gi.ndim == 2 else np.nonzero(gi != oi)[0]
    assert bad.size == 0, (tag, f"ids differ in {bad.size} places, first {bad[:5]}")
    assert (gd.view(np.uint32) == od.view(np.uint32)).all(), (tag, "distance bits differ")


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)) if a.dtype in (np.float16, np.int8) else a


class _paths:
    """the path assertions of the neighbouring files, by case name"""

    def __init__(self, eng, name):
        self.eng, self.name, self.ctx = eng, name, []

    def __enter__(self):
        e = self.eng
        self.ctx = {"partition_major": [_pm_used(e)], "mscan": [_ms_used(e)], "tiled_m48": [_pm_used(e)],
                    "dot_flow": [_dot_flow_used(e)], "overflow": [_pm_used(e)]}.get(self.name, [])
        for t in ("ivfpq_scan_c1", "ivfpq_mscan", "ivfpq_msbound"):
            e.timing_query(t)          # a query returns the launches since the one before it and starts again from 0
        if self.name in ("query_major", "four_bit"):
            e.timing(True)
        for c in self.ctx:
            c.__enter__()
        return self

    def __exit__(self, *a):
        for c in reversed(self.ctx):
            c.__exit__(*a)
        if self.name in ("query_major", "four_bit"):
            self.eng.synchronize()
            after = self.eng.timing_query("ivfpq_scan_c1")[1]
            self.eng.timing(False)
            if a[0] is None:
                assert after == 0, "the query-major scan was expected, the partition-major one ran"


# ---- flat KNN -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(R.FLAT_CASES))
def test_flat(eng, oracle, name):
    """small_1q / small_2q: the streaming kernel (flat_small.hip); filter_v2: the exact fixed-dimension filter; mfma_batch: the bf16x3
    matrix-core filter (flat_mfma.hip, >= 128 queries); mfma_wide: the K-tiled one for long rows (flat_mfma_wide.hip, counter asserted);
    generic_cosine: d = 20 under cosine, the any-dimension kernel; large_k: k = 200, the lanes-own-queries kernel; f16_dot: the 32-lane
    order of a Float16 column; f16_native / int8_native: rows read in the column's element type (exact and matrix-core filter).
    Only mfma_wide has a counter to assert.  The other names say where the dispatch of flat.hip sends the shape; in particular the
    streaming kernel may give a call up (more candidates at its bound than it keeps) and the batch path then answers it: with
    rows in three copies small_1q / small_2q are not known to stay in flat_small.hip, whichever kernel answers must equal the oracle"""
    c = R.flat_case(name)
    want = R.flat_answers(oracle, c, c.rid)
    wide = eng.timing_query("count:flat_mfma_wide")[1]
    for k, w in zip(c.ks, want):
        same(eng.flat_topk(_dev(c.x), _dev(c.q), k, c.metric, row_ids=c.rid), w, (name, k))
    assert (eng.timing_query("count:flat_mfma_wide")[1] > wide) == (name == "mfma_wide"), "long-row matrix-core filter"


# ---- IVF_FLAT -----------------------------------------------------------------------------------------------------------------
def test_ivf_flat_search_replay_save_load(eng, oracle, tmp_path):
    from lance_amd import index_file as IF
    from lance_amd.engine import DeviceFlatIndex
    c = R.ivfflat_case()
    want = R.ivfflat_answers(oracle, c, c.rid)
    ix = DeviceFlatIndex.create(eng, c.metric, c.cent, c.x, c.part, row_ids=c.rid)
    for (k, nprobes), w in zip(c.runs, want):
        same(ix.search(c.q, k, nprobes), w, (k, nprobes))
    # a mask shorter than every address selects nothing
    gi, gd = ix.search(c.q, 10, 6, allow=np.ones(c.x.shape[0], bool))
    assert (_np(gi) == -1).all() and np.isinf(_np(gd)).all()
    ix.save(tmp_path / "f")
    _, perm = oracle.partition_layout(c.part, c.cent.shape[0])
    stored = IF.read_index_files(tmp_path / "f")
    assert stored.row_ids.dtype == u64 and (stored.row_ids == c.rid[perm]).all()
    ix2 = DeviceFlatIndex.load(eng, tmp_path / "f")
    for (k, nprobes), w in zip(c.runs, want):
        same(ix2.search(c.q, k, nprobes), w, ("loaded", k, nprobes))
    ix.close(); ix2.close()


# ---- IVF_PQ -------------------------------------------------------------------------------------------------------------------
def _build(eng, c, raw=None):
    from lance_amd.engine import DeviceIndex
    int8 = c.kind == "int8"
    xg = torch.from_numpy(c.x.astype(np.int8)) if int8 else c.x
    gpart, gcodes, _ = eng.ivfpq_encode(xg, c.cent, c.cb, c.metric)
    if raw is not None and int8:
        raw = torch.from_numpy(raw.astype(np.int8))
    return DeviceIndex.create(eng, c.metric, c.cent, c.cb, gpart, gcodes, c.rid, raw=raw, dtype="int8" if int8 else None)


def _q(c, nq):
    return torch.from_numpy(c.q[:nq].astype(np.int8)) if c.kind == "int8" else c.q[:nq]


@pytest.mark.parametrize("name", sorted(R.IVFPQ_CASES))
def test_ivfpq_unrefined(eng, oracle, name, tmp_path):
    """query_major: one workgroup per query (520 queries) and the probes split over several (3 and 1 queries); partition_major: the
    partition-major flow at a batch too small for the matrix-core scan's own threshold; mscan: the matrix-core scan; tiled_m48: the per-query-table kernels; four_bit; dot_flow; overflow: more ties
    inside one partition than a candidate buffer holds -> the exact replay"""
    from lance_amd.engine import DeviceIndex
    c = R.ivfpq_case(name)
    oidx = R.ivfpq_oracle_index(oracle, c, c.rid)
    gidx = _build(eng, c)
    # export: the ids in stored order; from_storage with them answers identically; save -> load keeps them
    offs, codes_t, rid = gidx.export()
    assert (offs == oidx.part_offsets).all() and (codes_t == oidx.codes_t).all()
    assert rid.dtype == u64 and (rid == oidx.row_ids).all() and (rid == c.rid[oidx.perm]).all()
    g2 = DeviceIndex.from_storage(eng, c.metric, c.cent, c.cb, offs, codes_t, rid, transposed=True)
    gidx.save(tmp_path / "i")
    g3 = DeviceIndex.load(eng, tmp_path / "i")
    assert (g3.export()[2] == rid).all()
    replays = 0
    for nq, k, nprobes in c.runs:
        want = oidx.search(c.q[:nq], k, nprobes)
        with _paths(eng, name if nq >= 100 else ""):
            got = gidx.search(c.q[:nq], k, nprobes)
        replays += eng.search_stats()
        same(got, want, (name, nq, k, nprobes))
        same(g2.search(c.q[:nq], k, nprobes), want, (name, "from_storage", nq, k, nprobes))
        same(g3.search(c.q[:nq], k, nprobes), want, (name, "loaded", nq, k, nprobes))
    if name == "overflow":
        assert replays > 0, "no query was replayed by the exact kernel"
    for g in (gidx, g2, g3):
        g.close()


@pytest.mark.parametrize("name", R.OTHER_SEARCHES)
def test_ivfpq_filtered_range_candidates(eng, oracle, name):
    """the other searches over the same ids: a mask shorter than every address selects nothing; a distance range; the candidate lists
    of a list-sharded search (ids and PQ distances of search(k = keff))"""
    c = R.ivfpq_case(name)
    oidx = R.ivfpq_oracle_index(oracle, c, c.rid)
    gidx = _build(eng, c)
    nq, k, nprobes = c.runs[0]
    q = c.q[:nq]
    mask = np.ones(c.x.shape[0], bool)
    same(gidx.search_filtered(q, k, nprobes, mask), oidx.search(q, k, nprobes, prefilter=mask), (name, "filtered"))
    assert (_np(gidx.search_filtered(q, k, nprobes, mask)[0]) == -1).all()
    lo, hi = R.range_bounds(oidx, c)
    same(gidx.search_range(q, k, nprobes, lo, hi), oidx.search(q, k, nprobes, lower=lo, upper=hi), (name, "range"))
    ci, cd, _ = gidx.search_candidates(q, R.CANDIDATES_KEFF, nprobes, exact=False)
    same((ci, cd), oidx.search(q, R.CANDIDATES_KEFF, nprobes), (name, "candidates"))
    gidx.close()


# ---- refine -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f32_frac", "int8"])
@pytest.mark.parametrize("name", sorted(R.REFINE_RUNS))
def test_refine_reads_the_raw_column_by_id(eng, oracle, name, kind):
    """f32: integer-valued, refined from the lossless u8 copy (refine_u8_kernel); f32_frac: one element is a fraction, so the column
    stays f32 (refine_pair_kernel); int8: an Int8 column (refine_kernel<.., int8_t>)"""
    c = R.ivfpq_case(name, "raw", kind)
    raw = R.raw_by_id(c.x, c.rid)
    assert (raw != c.x).any()
    oidx = R.ivfpq_oracle_index(oracle, c, c.rid)
    gidx = _build(eng, c, raw=raw)
    nq, k, nprobes = R.REFINE_RUNS[name]
    for rf in R.REFINE_FACTORS:
        with _paths(eng, name):
            got = gidx.search(_q(c, nq), k, nprobes, rf)
        same(got, oidx.search(c.q[:nq], k, nprobes, refine=rf, raw=raw), (name, kind, rf))
    # the candidate call: ids / PQ distances of search(k = keff), and each candidate's exact distance next to it
    cq, keff = R.REFINE_CANDIDATES
    ci, cp, ce = gidx.search_candidates(_q(c, cq), keff, nprobes)
    same((ci, cp), oidx.search(c.q[:cq], keff, nprobes), (name, kind, "candidates"))
    oi, od = oidx.search(c.q[:cq], keff, nprobes, refine=1, raw=raw)
    ci, ce = _np(ci).view(u64), _np(ce)
    for r in range(cq):
        assert {(int(a), int(b)) for a, b in zip(ci[r], ce[r].view(np.uint32)) if a != R.NONE_ID} == \
               {(int(a), int(b)) for a, b in zip(oi[r], od[r].view(np.uint32)) if a != R.NONE_ID}, (name, kind, "exact distances", r)
    gidx.close()


@pytest.mark.parametrize("kind", ["f32", "f32_frac", "int8"])
@pytest.mark.parametrize("name", sorted(R.REFINE_RUNS))
def test_refine_refuses_ids_beyond_the_raw_column(eng, oracle, name, kind):
    """what every table of several fragments meets when the raw column is handed over in storage order: every address lies beyond it"""
    from lance_amd._lib import LanceHipError
    c = R.ivfpq_case(name, "addresses", kind)
    gidx = _build(eng, c, raw=c.x)
    nq, k, nprobes = R.REFINE_RUNS[name]
    for rf in R.REFINE_FACTORS:
        ids = torch.full((nq, k), -1, dtype=torch.int64, device="cuda")
        dists = torch.full((nq, k), float("nan"), dtype=torch.float32, device="cuda")
        with pytest.raises(LanceHipError, match="raw vectors"):
            gidx.search(_q(c, nq), k, nprobes, rf, out=(ids, dists))
        # the contract of a refusal: whatever the kernels wrote before they met the id, no slot holds a finite distance -- and so no
        # (id, distance) pair that reads as a result; an id next to a non-finite distance is the "no row" form of every search
        assert not torch.isfinite(dists).any(), (name, kind, rf, "a finite distance was left behind by a refused refine")
        assert not ((ids != -1) & torch.isfinite(dists)).any(), (name, kind, rf, "an id with a finite distance was left behind")
    oidx = R.ivfpq_oracle_index(oracle, c, c.rid)
    same(gidx.search(_q(c, nq), k, nprobes), oidx.search(c.q[:nq], k, nprobes), (name, kind, "unrefined, after the refusals"))
    gidx.close()


# ---- prefilter by id ----------------------------------------------------------------------------------------------------------
def _only_fragment_0(got, n):
    ids = _np(got[0])
    assert ((ids == -1) | ((ids >= 0) & (ids < n))).all() and (ids >= 0).any(), "a row outside fragment 0 was admitted"


@pytest.mark.parametrize("name", ["query_major", "four_bit"])
def test_prefilter_by_id_ivfpq(eng, oracle, name):
    c = R.ivfpq_case(name, "small")
    n = c.x.shape[0]
    oidx = R.ivfpq_oracle_index(oracle, c, c.rid)
    gidx = _build(eng, c)
    mask = np.ones(n, bool)
    for nq, k, nprobes in c.runs:
        got = gidx.search_filtered(c.q[:nq], k, nprobes, mask)
        same(got, oidx.search(c.q[:nq], k, nprobes, prefilter=mask), (name, nq, k, nprobes))
        _only_fragment_0(got, n)
    gidx.close()


def test_prefilter_by_id_ivf_flat(eng, oracle):
    from lance_amd.engine import DeviceFlatIndex
    c = R.ivfflat_case("small")
    n = c.x.shape[0]
    ix = DeviceFlatIndex.create(eng, c.metric, c.cent, c.x, c.part, row_ids=c.rid)
    some = np.ones(n, bool)
    some[::3] = False
    for mask in (np.ones(n, bool), some):
        want = R.ivfflat_answers(oracle, c, c.rid, keep=R.selected_rows(mask, c.rid))
        for (k, nprobes), w in zip(c.runs, want):
            got = ix.search(c.q, k, nprobes, allow=mask)
            same(got, w, (k, nprobes))
            _only_fragment_0(got, n)
    ix.close()


def _sq_index(eng, c):
    from lance_amd.engine import DeviceSqIndex
    return DeviceSqIndex.create(eng, c.metric, c.cent, eng.sq_encode(c.xs, c.bounds), c.part, c.bounds, row_ids=c.rid)


def test_prefilter_by_id_ivf_sq(eng, oracle):
    c = R.sq_case("gaussian", "small")
    n = c.x.shape[0]
    ix = _sq_index(eng, c)
    mask = np.ones(n, bool)
    for (k, nprobes), w in zip(c.runs, R.sq_answers(oracle, c, c.rid, prefilter=mask)):
        got = ix.search(c.q, k, nprobes, allow=mask)
        same(got, w, (k, nprobes))
        _only_fragment_0(got, n)
    ix.close()


# ---- the other entry points ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["gaussian", "ties"])
def test_ivf_sq(eng, oracle, name):
    """gaussian: k = 9 is answered by the fast path (sq_merge_kernel), k = 10 / 128 partly or wholly by the heap replay; ties: every query
    replayed through the heap (sq_exact_kernel)"""
    c = R.sq_case(name)
    ix = _sq_index(eng, c)
    for (k, nprobes), w in zip(c.runs, R.sq_answers(oracle, c, c.rid)):
        same(ix.search(c.q, k, nprobes), w, (name, k, nprobes))
        replays = eng.search_stats()
        # (the CPU emulation of these kernels, tests/test_sq_kernels_cpu.py's run_case, replays every query of the k = 10 run and none at k = 9)
        if name == "ties" or k == 10:
            assert replays > 0, (name, k, nprobes, "no query went through the heap replay")
        elif k == 9:
            assert replays == 0, (name, k, nprobes, replays, "the fast path was to answer every query")
    gi, gd = ix.search(c.q, 10, c.nlist, allow=np.ones(1000, bool))         # a mask far shorter than every address
    assert (_np(gi) == -1).all() and np.isinf(_np(gd)).all()
    ix.close()


def test_pq_scan_topk(eng, oracle):
    c = R.pq_partition_case()
    ct = oracle.transpose(c.codes)
    for k, w in zip(c.ks, R.pq_partition_answers(oracle, c, c.rid)):
        same(eng.pq_scan_topk(c.qr, c.cb, ct, c.rid, k), w, k)


def test_multivec_topk(eng, oracle):
    import lance_amd.engine as E
    c = R.multivec_case()
    vd, qd, rd = E.to_device(c.values), E.to_device(c.q), E.to_device(c.rid)
    for k, w in zip(c.ks, R.multivec_answers(oracle, c, c.rid)):
        same(eng.multivec_topk(vd, c.off, qd, k, c.metric, row_ids=rd), w, k)


@pytest.mark.parametrize("exact", [False, True])
def test_merge_topk(eng, oracle, exact):
    c = R.merge_case()
    (oi, od), = R.merge_answers(oracle, c, c.ids, exact)
    gi, gd = eng.merge_topk(c.ids.view(np.int64), c.dists, c.k, exact=c.exact if exact else None, keff=c.keff if exact else None)
    same((gi, gd), (oi, od), exact)
