"""The 4-bit IVF_PQ scan on the GPU against the oracle, whole outputs: ids as uint64, distances as uint32 views, no tolerance
(tests/pq4_spec.py holds the fixtures and a numpy model of the arithmetic; tests/test_pq4_spec.py shows on the CPU that model == oracle on
every case here, that each modelled kernel mistake changes the answer of a named case, and that the cases reach their regimes).

What runs: `pq_scan_topk` on single partitions of 1 .. 1008 rows x k 1 .. 5000 (k_hint below, at and above 200 and above the partition);
IVF search through ivfpq_scan4_kernel (k * refine <= 128; 40 queries: several workgroups share a query's probes; 600: one each) and through
ivfpq_exact_kernel<*, 4> alone (k * refine 129 .. 5000, up to the largest LDS request the library accepts, and the first it refuses); the
prefilter arithmetic at selectivity 0.5 and 0.01 with k * refine above 200; ranges whose bounds ARE returned distances (inclusive below,
exclusive above, empty, one-sided, +inf, negative under dot, fewer than k rows) on the 4-bit index and on an 8-bit index of the same rows;
L2, cosine and dot in both table regimes; saturating and many-level layouts; zero / NaN / inf codebooks and a NaN query; an f16 column;
M 2 .. 32 with d / M 2 .. 16; adaptive probing through IvfPqIndex.nearest.

Wall time on an MI355X: 85 tests in 6.4 s -- engine start-up and the first index 1.6 s, the exact-kernel sweep 0.9 s, each
pq_scan_topk grid (about 170 calls) 0.6 s, every other test under 0.4 s (the oracle's CPU searches at k = 5000 included)."""
import numpy as np
import pytest

import pq4_spec as S

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    for g in e.__dict__.pop("_pq4_indices", {}).values():
        g.close()
    e.close()


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


def device_index(eng, name, nbits=4):
    """the fixture's index on the device, built once per engine from the hand-assigned partition ids and the spec's codes"""
    import lance_amd.engine as E
    cache = eng.__dict__.setdefault("_pq4_indices", {})      # kept on the engine they live on
    if (name, nbits) not in cache:
        fx = S.index_fixture(name, nbits)
        ix = fx.ix
        cache[name, nbits] = E.DeviceIndex.create(eng, ix.metric, ix.cent, ix.cb, ix.part.view(np.int32), ix.codes, None, raw=fx.x)
    return cache[name, nbits]


class Counters:
    """what a block of calls raised: launches of the query-major scan and of the exact kernel, queries the exact kernel answered"""
    NAMES = ("ivfpq_scan", "ivfpq_exact", "ivfpq_mscan")

    def __init__(self, eng, on=True):
        self.eng, self.on, self.rose = eng, on, {}

    def __enter__(self):
        if self.on:
            self.before = {s: self.eng.timing_query("count:" + s)[1] for s in self.NAMES}
        return self

    def __exit__(self, *a):
        if self.on:
            self.eng.synchronize()
            self.rose = {s: int(self.eng.timing_query("count:" + s)[1] - b) for s, b in self.before.items()}
            self.rose["replayed"] = self.eng.search_stats()


def differs(got, want):
    """-> None or (what, first differing query, position)"""
    gi, gd = _np(got[0]).view(np.uint64).reshape(want[0].shape), np.ascontiguousarray(_np(got[1]), f32).reshape(want[1].shape)
    for what, a, b in (("ids", gi, want[0]), ("distances", gd.view(np.uint32), np.ascontiguousarray(want[1], f32).view(np.uint32))):
        bad = np.argwhere(a != b)
        if bad.size:
            return what, tuple(int(v) for v in bad[0]), int(len(bad))
    return None


def run_search(gidx, q, k, nprobes, refine, allow, lo, hi):
    if lo is not None or hi is not None:
        return gidx.search_range(q, k, nprobes, lo, hi, refine_factor=refine, allow=allow)
    if allow is not None:
        return gidx.search_filtered(q, k, nprobes, allow, refine)
    return gidx.search(q, k, nprobes, refine)


def oracle_search(fx, q, k, nprobes, refine, allow, lo, hi):
    with np.errstate(all="ignore"):
        return fx.ix.oracle().search(q, k, nprobes, refine=refine, raw=fx.x.astype(f32) if refine else None, prefilter=allow, lower=lo, upper=hi)


# ---- every case of the specification through DeviceIndex.search / search_filtered / search_range -----------------------------------------
def case_body(eng, name, nbits=4):
    c = S.CASE[name]
    fx = S.index_fixture(c.index, nbits)
    _, q, nprobes, allow = S.case_inputs(c)
    lo = hi = None
    if c.bounds is not None:      # from the oracle's own distances on THIS index, so that rows sit exactly on the bounds
        lo, hi = S.resolve_bounds(c, oracle_search(fx, q, c.k, nprobes, c.refine, allow, None, None)[1])
    want = oracle_search(fx, q, c.k, nprobes, c.refine, allow, lo, hi)
    got = run_search(device_index(eng, c.index, nbits), q, c.k, nprobes, c.refine, allow, lo, hi)
    assert differs(got, want) is None, (name, nbits, lo, hi, differs(got, want))
    return want, (lo, hi)


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_case(eng, oracle, name):
    case_body(eng, name)


@pytest.mark.parametrize("name", S.RANGE_CASES)
def test_range_case_on_the_8bit_index_of_the_same_rows(eng, oracle, name):
    """the same rows, partitions and queries under an 8-bit codebook; bounds from that index's own distances"""
    (ids, d), (lo, hi) = case_body(eng, name, nbits=8)
    c = S.CASE[name]
    found = ids != S.NOID
    if "on_lower" in c.regime and not c.refine:
        assert (d[found] == lo).any(), name
    if "on_upper" in c.regime:
        assert not (d[found] >= hi).any(), name


# ---- pq_scan_topk: one partition, the full grid of sizes x k ------------------------------------------------------------------------------
def scan_grid_body(eng, oracle, index, keffs=S.KEFFS):
    fx = S.index_fixture(index)
    ix = fx.ix
    q = S.queries(fx, 3, seed=9)
    fails = []
    for p in range(ix.cent.shape[0]):
        codes_t, rids = ix.partition(p)
        n_p = rids.size
        if n_p == 0:
            continue
        qr = q[p % 3] - ix.cent[p] if ix.metric == "l2" else q[p % 3]
        lut = oracle.build_lut(qr, ix.cb, ix.metric, nbits=4)
        for k in sorted(set(keffs) | {n_p}):          # k = n_p: every row exact
            hi_, hd_ = oracle.heap_topk(oracle.pq_scan4(lut, codes_t, k, ix.metric), rids, k)
            want = oracle.sort_fetch(hi_, hd_, k)
            got = eng.pq_scan_topk(qr, ix.cb, codes_t, rids, k, ix.metric)
            if _np(got[0]).size != want[0].size or differs(got, want) is not None:
                fails.append((index, "n_p", n_p, "k", k, _np(got[0]).size, want[0].size))
    assert not fails, f"{len(fails)} (partition, k) pairs differ from the oracle: {fails[:10]}"


@pytest.mark.parametrize("index", ["l2-m8", "l2-m32", "dot-signs"])
def test_pq_scan_topk_grid(eng, oracle, index):
    scan_grid_body(eng, oracle, index)


# ---- the two kernels, by route ---------------------------------------------------------------------------------------------------------------
SCAN4_SEARCHES = (("l2-m32", 1, 0), ("l2-m32", 10, 0), ("l2-m32", 128, 0), ("l2-m32", 25, 5), ("dot-signs", 10, 0), ("dot-signs", 32, 4),
                  ("cosine-m8", 128, 0), ("dot-low", 10, 0), ("l2-m2", 100, 0))


def scan4_route_body(eng, nq, counters=True, searches=SCAN4_SEARCHES):
    for index, k, refine in searches:
        fx = S.index_fixture(index)
        q = S.queries(fx, nq, seed=3)
        nprobes = fx.ix.cent.shape[0]
        want = oracle_search(fx, q, k, nprobes, refine, None, None, None)
        with Counters(eng, counters) as st:
            got = run_search(device_index(eng, index), q, k, nprobes, refine, None, None, None)
        print(f"[pq4] scan4 route {index} nq={nq} k={k} refine={refine}: {st.rose}")
        assert differs(got, want) is None, (index, nq, k, refine, differs(got, want))
        if counters:
            assert st.rose["ivfpq_scan"] >= 1 and st.rose["ivfpq_mscan"] == 0, (index, k, refine, st.rose)
            if fx.layout == "gauss":      # real-valued rows, no ties: the scan's own answer stands for most queries
                assert st.rose["replayed"] < nq, (index, k, refine, st.rose)


@pytest.mark.parametrize("nq", [40, 600])
def test_search_through_the_scan4_kernel(eng, oracle, nq):
    """k * refine <= 128: ivfpq_scan4_kernel answers (its stage counter rises, the matrix-core scan's does not).  40 queries: below twice
    the number of compute units, so several workgroups split one query's probes; 600: one workgroup per query"""
    scan4_route_body(eng, nq)


EXACT_SEARCHES = ((129, 0), (200, 0), (201, 0), (250, 0), (60, 5), (1000, 0), (5000, 0), (500, 10))


def exact_lds_bytes(d, m, keff):
    """the exact kernel's LDS as the host bounds it next to the launch (search.hip, the LH_REQUIRE `exact kernel does not fit`): the dynamic
    request plus the 16 bytes the kernel's static variables take in front of it"""
    dpad = (d + 3) & ~3
    return dpad * 4 + m * 256 * 4 + keff * 12 + (keff + 1) * 8 + 64 * 4 + 16 + 16 + max(200, keff) * 4 + m * 16 + 16 + 16


def exact_route_body(eng, index="l2-m32", counters=True, searches=EXACT_SEARCHES, nq=12):
    fx = S.index_fixture(index)
    q = S.queries(fx, nq, seed=4)
    nprobes = fx.ix.cent.shape[0]
    gidx = device_index(eng, index)
    for k, refine in searches:
        want = oracle_search(fx, q, k, nprobes, refine, None, None, None)
        with Counters(eng, counters) as st:
            got = run_search(gidx, q, k, nprobes, refine, None, None, None)
        print(f"[pq4] exact route {index} k={k} refine={refine}: {st.rose}")
        assert differs(got, want) is None, (index, k, refine, differs(got, want))
        if counters:
            assert st.rose["replayed"] == nq and st.rose["ivfpq_scan"] == 0 and st.rose["ivfpq_mscan"] == 0, (k, refine, st.rose)


def test_search_through_the_exact_kernel_alone(eng, oracle):
    """k * refine above 128 on the index with the largest M (32): every query is answered by ivfpq_exact_kernel<*, 4>, whose `fd` region
    and LDS request grow with k * refine"""
    exact_route_body(eng)


def test_exact_kernel_lds_limit(eng, oracle):
    """the largest k the host's LDS bound accepts for d 64, M 32 (160 KiB) answers like the oracle; the next one comes back as the
    library's own error, not as a failed launch.  (The bound once left the kernel's static LDS out: k = 5416 was accepted with a group
    segment of 163848 bytes, the queue refused the dispatch and every later call on the device failed.)"""
    from lance_amd._lib import LanceHipError
    fx = S.index_fixture("l2-m32")
    d, m = fx.ix.cent.shape[1], fx.ix.cb.shape[0]
    largest = max(k for k in range(129, 8193) if exact_lds_bytes(d, m, k) <= 160 * 1024)
    assert largest == 5415 and exact_lds_bytes(d, m, largest + 1) > 160 * 1024
    exact_route_body(eng, searches=((largest, 0),), nq=2)
    q = S.queries(fx, 2, seed=4)
    with pytest.raises(LanceHipError, match="exact kernel does not fit in LDS"):
        device_index(eng, "l2-m32").search(q, largest + 1, fx.ix.cent.shape[0], 0)
    exact_route_body(eng, searches=((10, 0),), nq=2, counters=False)      # the engine answers on after the refusal


# ---- adaptive probing through the Python surface -------------------------------------------------------------------------------------------------
def adaptive_body(eng, index="l2-m8", k=20):
    """minimum_nprobes 1, maximum_nprobes all: a query beside a partition of 1, 15, 16 or 17 rows (or the empty one) finds fewer than k
    rows and goes on, the number of partitions doubling; each returned list is the oracle's at the number of partitions it ended with"""
    from lance_amd.vector import IvfPqIndex, IvfPqParams
    fx = S.index_fixture(index)
    nlist, m = fx.ix.cent.shape[0], fx.ix.cb.shape[0]
    q = S.queries(fx, 2 * nlist, seed=6)
    ix = IvfPqIndex(device_index(eng, index), IvfPqParams(nlist, m, 4, fx.ix.metric))
    ids, dists = ix.nearest(q, k=k, minimum_nprobes=1, maximum_nprobes=nlist)
    per_np, npb = {}, 1
    while True:
        per_np[npb] = oracle_search(fx, q, k, npb, 0, None, None, None)
        if npb >= nlist:
            break
        npb = min(nlist, npb * 2)
    ended = []
    for i in range(q.shape[0]):
        for npb in sorted(per_np):
            oi, od = per_np[npb]
            if (oi[i] != S.NOID).all() or npb == nlist:
                assert (ids[i].view(np.uint64) == oi[i]).all() and (dists[i].view(np.uint32) == od[i].view(np.uint32)).all(), (i, npb)
                ended.append(npb)
                break
    assert min(ended) == 1 and max(ended) > 1, ended


def test_adaptive_probing_on_a_4bit_index(eng, oracle):
    adaptive_body(eng)
