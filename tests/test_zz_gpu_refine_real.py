"""The exact refine (lance_amd/csrc/search.hip launch_refine) on REAL-VALUED columns, every kernel instantiation and row length, against the
CPU oracle: row ids as uint64, distances as their bits.  The fixtures, the reason for them (an integer-valued column cannot see the order
of a sum) and the wrong sums they tell apart are in tests/refine_real_spec.py; tests/test_refine_real_spec.py checks on the CPU that every
fixture does tell them apart.

The grid (refine_real_spec.ARMS; n = 3000, eight lists of which one is empty and one holds 12 rows, 37 queries):
  f32 l2, dot   refine_pair_kernel              d = 16: one chunk; 48: three; 128: exactly one round of eight; 144: a round and one chunk;
                                                272: two rounds and one; 1536: the flagship cosine length
  f32 l2, dot   refine_kernel<.., float>        d = 8: all tail; 24: a chunk and a tail of 8; 40: chunks and 8; 100: chunks and a tail of 4
  f32 cosine    refine_kernel<COSINE, float>    d = 8, 16: cosine_once; 40, 100, 240; 264: >= 256 but no multiple of 16, stays narrow
  f32 cosine    the four-lane path              d = 256: the threshold; 272: one chunk more; 1536
  f16 l2        <L2, __half>                    d = 16, 40, 272 (16 lanes)
  f16 dot, cos  <.., __half, true>              d = 16: all tail; 40: 32 + 8; 64: two chunks; 72: two + 8; 272: eight + 16 (32 lanes)
  int8          <.., int8_t>                    d = 16, 40, 128; l2 / dot also 1024, where the sums pass 2^24
At the shortest and the longest row of each arm keff = k * refine_factor runs through 1, 33, 64, 65, 128, 129, 256, 257 and 1000, i.e.
P = 64 .. 1024: both sides of refine_emit_topk's switch at P = 256 and a P below the pair kernel's 128 slots per round.  Every length
also runs k = 10 x 10 with 4 and 8 probes and with one probe: q[0] then meets only the list of 12 rows and q[1] only the empty one (all
padding), each also alone (nq = 1).  search_candidates is compared position by position: ids and PQ distances with the oracle's
search(k = keff), exact distance j with the oracle's distance of the query to raw[id_j], +inf in an empty slot.  Every search must have
enqueued the refine once and never the u8 copy's kernels (count:refine, count:refine_u8, count:refine_rows).

Spoiled rows (NaN, +inf, a subnormal, -0.0, a row of 1e-30) and the 41 equal rows: refine_real_spec.spoiled_fixture.  IVF_SQ re-ranking
(the same launch_refine, up to 768 candidates): an f16 column at d = 72.  LANCE_HIP_REFINE_V1=1 (the one-lane kernel in place of the pair
kernel, read once per process): the pair kernel's lengths once more in a child process.

Found by this file: refine_pair_kernel took the L2 difference as q - row.  The GPU's subtract returns a NaN subtrahend with the sign bit
set, so a row with a NaN element got the NEGATIVE NaN for a distance and was returned first, where the reference returns it last
(test_spoiled_and_duplicate_rows[f32-l2-144]; the one-lane kernels take row - q, lance_amd/csrc/exact.cuh SWAP).

Wall time on an MI355X: 64 tests in 17 s -- the child process 4.3 s, the keff = 5000 sort 1.9 s, the d = 1536 and d = 1024 cases 0.4 - 0.6 s,
every other test under 0.35 s."""
import os
import subprocess
import sys

import numpy as np
import pytest

import refine_real_spec as S

pytestmark = pytest.mark.gpu
f32 = np.float32
u64 = np.uint64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "LANCE_HIP_REFINE_V1"
COUNTERS = ("refine", "refine_u8", "refine_rows")
# (k, refine_factor): keff = 1, 33, 64, 65, 128, 129, 256, 257, 1000 -> P = 64, 64, 64, 128, 128, 256, 256, 512, 1024
KEFF_RUNS = ((1, 1), (11, 3), (64, 1), (13, 5), (16, 8), (43, 3), (64, 4), (257, 1), (100, 10))
# pair kernel (l2, dot), the one-lane f32 kernel, narrow and wide cosine, f16 l2 and cosine
SPOILED = (("f32", "l2", 144), ("f32", "dot", 128), ("f32", "l2", 100), ("f32", "cosine", 100), ("f32", "cosine", 272), ("f16", "l2", 40),
           ("f16", "cosine", 72))


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _np(t):
    return t.cpu().numpy()


def _dev(a):
    """f16 / int8 arrays go in as tensors of that element type (numpy f32 is taken as it is)"""
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)) if a is not None and a.dtype in (np.float16, np.int8) else a


class _refined_once:
    """the searches inside enqueued the refine `times` times, and never from the u8 copy"""

    def __init__(self, eng, counters, times=1):
        self.eng, self.on, self.times = eng, counters, times

    def _read(self):
        return [self.eng.timing_query("count:" + c)[1] for c in COUNTERS]

    def __enter__(self):
        self.before = self._read() if self.on else None
        return self

    def __exit__(self, *a):
        if self.on and a[0] is None:
            got = [x - y for x, y in zip(self._read(), self.before)]
            assert got == [self.times, 0, 0], f"launches of {COUNTERS}: {got}, expected {[self.times, 0, 0]}"


def build(eng, fx, raw):
    """the device index from the oracle's models; the encode's partition ids and codes must be the oracle's before anything is searched"""
    from lance_amd.engine import DeviceIndex
    gpart, gcodes, _ = eng.ivfpq_encode(_dev(fx.x), fx.cent, fx.cb, fx.metric)
    assert (_np(gpart).view(np.uint32) == fx.oidx.part_ids).all(), "partition ids differ from the oracle's"
    assert (_np(gcodes) == fx.oidx.codes_rowmajor).all(), "PQ codes differ from the oracle's"
    return DeviceIndex.create(eng, fx.metric, fx.cent, fx.cb, gpart, gcodes, None, raw=_dev(raw), dtype="int8" if fx.kind == "int8" else None)


def check_search(eng, gidx, fx, q, k, nprobes, rf, raw, counters, tag):
    with _refined_once(eng, counters):
        gi, gd = gidx.search(_dev(q), k, nprobes, rf)
    oi, od = fx.oidx.search(S.oracle_rows(q), k, nprobes, refine=rf, raw=raw.astype(f32))
    gi, gd = _np(gi).view(u64), _np(gd)
    bad_i = np.nonzero((gi != oi).any(axis=1))[0]
    bad_d = np.nonzero((gd.view(np.uint32) != od.view(np.uint32)).any(axis=1))[0]
    if bad_i.size or bad_d.size:
        ci, cd, _ = gidx.search_candidates(_dev(q), k * rf, nprobes, exact=False)
        wi, wd = fx.oidx.search(S.oracle_rows(q), k * rf, nprobes)
        lists = (_np(ci).view(u64) == wi).all() and (_np(cd).view(np.uint32) == wd.view(np.uint32)).all()
        raise AssertionError(f"{tag} k={k} refine={rf} nprobes={nprobes} nq={len(q)}: ids differ for queries {bad_i[:5]} ({bad_i.size}), distance bits for "
                             f"{bad_d[:5]} ({bad_d.size}); the candidate lists " + ("agree: the REFINE differs" if lists else "differ: the SCAN differs"))


def check_candidates(gidx, fx, q, keff, nprobes, raw, tag):
    """position by position: ids, PQ distances, each candidate's exact distance, +inf in an empty slot"""
    ci, cp, ce = gidx.search_candidates(_dev(q), keff, nprobes)
    ci, cp, ce = _np(ci).view(u64), _np(cp), _np(ce)
    oi, od = fx.oidx.search(S.oracle_rows(q), keff, nprobes)
    assert (ci == oi).all(), (tag, "candidate ids differ from the oracle's search(k = keff)")
    assert (cp.view(np.uint32) == od.view(np.uint32)).all(), (tag, "candidate PQ distances differ")
    want = np.full(oi.shape, np.inf, f32)
    for r in range(len(q)):
        ok = oi[r] != S.NONE_ID
        if ok.any():
            want[r, ok] = S.oracle_distances(fx.metric, q[r], raw[oi[r][ok].astype(np.int64)])
    bad = np.argwhere(ce.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (tag, f"exact distance bits differ at {len(bad)} (query, position) places, first {bad[:4].tolist()}; the lists agree: the REFINE differs")
    return oi


def case(eng, arm, d, counters=True, full=None):
    kind, metric, dims = S.ARMS[arm]
    fx = S.fixture(kind, metric, d)
    raw = fx.x
    gidx = build(eng, fx, raw)
    tag = f"{arm} d={d}"
    if full is None:
        full = d in (min(dims), max(dims))
    for nprobes in (4, S.NLIST):
        check_search(eng, gidx, fx, fx.q, S.K, nprobes, S.RF, raw, counters, tag)
    if full:
        for k, rf in KEFF_RUNS:
            check_search(eng, gidx, fx, fx.q, k, S.NLIST, rf, raw, counters, tag)
    # one probe: q[0] meets only the list of 12 rows, q[1] only the empty one
    check_search(eng, gidx, fx, fx.q, S.K, 1, S.RF, raw, counters, tag + " one probe")
    for qi in (S.Q_SHORT, S.Q_EMPTY, S.Q_DUP):
        check_search(eng, gidx, fx, fx.q[qi:qi + 1], S.K, 1, S.RF, raw, counters, tag + f" query {qi} alone")
    oi = check_candidates(gidx, fx, fx.q, S.KEFF, 1, raw, tag + " one probe")
    cnt = (oi != S.NONE_ID).sum(axis=1)
    assert cnt[S.Q_SHORT] == S.NOUT and cnt[S.Q_EMPTY] == 0, "the short and the empty list are not what the two queries met"
    oi = check_candidates(gidx, fx, fx.q, S.KEFF, S.NLIST, raw, tag)
    assert 0 < np.isin(oi[S.Q_DUP], fx.block).sum() < S.NDUP, "the equal rows do not lie across keff"
    gidx.close()


CASES = [(arm, d) for arm, _, _, d in S.GRID]


@pytest.mark.parametrize("arm,d", CASES, ids=[f"{a}-{d}" for a, d in CASES])
def test_refine_real(eng, oracle, arm, d):
    if arm.endswith("-pair"):
        assert os.environ.get(SWITCH) is None, f"{SWITCH} is set: this process cannot reach the pair kernel"
    case(eng, arm, d)


def spoiled_case(eng, kind, metric, d, counters=True):
    fx, raw, rows, what, qs = S.spoiled_fixture(kind, metric, d)
    gidx = build(eng, fx, raw)
    tag = f"spoiled {kind} {metric} d={d}"
    check_search(eng, gidx, fx, qs, S.K, S.NLIST, S.RF, raw, counters, tag)
    check_search(eng, gidx, fx, qs, S.KEFF, S.NLIST, 1, raw, counters, tag)         # every candidate returned: the NaN rows last
    oi = check_candidates(gidx, fx, qs, S.KEFF, S.NLIST, raw, tag)
    assert np.isin(rows, oi).all(), "a changed row is no candidate"
    gidx.close()


@pytest.mark.parametrize("kind,metric,d", SPOILED)
def test_spoiled_and_duplicate_rows(eng, oracle, kind, metric, d):
    """the index stores the clean rows' codes, the refine reads the column as it is now: one element NaN / +inf / subnormal / -0.0, a row of
    1e-30, and at the ids of the 41 equal rows the row of the duplicate query's nearest candidate (a tie for the first place)"""
    spoiled_case(eng, kind, metric, d)


def sort_case(eng, counters=True, n=9000, k=2500, rf=2, nq=4):
    fx = S.fixture("f32", "l2", 64, n)
    gidx = build(eng, fx, fx.x)
    check_search(eng, gidx, fx, fx.q[:nq], k, S.NLIST, rf, fx.x, counters, f"keff={k * rf}")
    gidx.close()


def test_sort_over_the_whole_lds_array(eng, oracle):
    """k = 2500 x 2: keff = 5000, P = 8192 -- the bitonic sort of refine_emit_topk over the largest array the launch allows"""
    sort_case(eng)


@pytest.mark.parametrize("metric", ["l2", "cosine"])
def test_ivf_sq_reranking_real_f16(oracle, metric):
    """IVF_SQ re-ranking goes through the same launch_refine with up to 768 candidates: an f16 real-valued column at d = 72 (the 32-lane
    forms: two chunks and a tail of 8 under cosine; 16 lanes under l2), keff = 300 and 768, against refine_spec.sq_search_refine"""
    import refine_spec as F
    import sq_spec
    import test_zz_gpu_refine_sqrq as Q
    n, d, nlist, nprobes = 3000, 72, 8, 4
    x, q = sq_spec.gaussian(n, d, 20, seed=72, kind="f16")
    assert (x.astype(f32) != np.rint(x.astype(f32))).any()
    cent = sq_spec.centroids_with_gaps(oracle.normalize(x) if metric == "cosine" else x, nlist, seed=3)
    rid = np.random.default_rng(5).permutation(n).astype(u64)
    ix, (_, _, (codes, part, _, b), _, raw) = Q.sq_index(x, cent, metric, rid)
    e = Q.eng()
    for k, rf in ((300, 1), (30, 10), (768, 1), (96, 8)):
        with _refined_once(e, True):
            gi, gd = Q.search(ix, q, k, nprobes, rf)
        oi, od = F.sq_search_refine(oracle, codes, part, cent, q, k, rf, nprobes, metric, b[0], b[1], raw, row_ids=rid)
        assert (gi == oi).all(), (metric, k, rf, np.argwhere(gi != oi)[:4].tolist())
        assert Q.same_bits(gd, od), (metric, k, rf)
    ix.close()


def _pair_lengths_on_the_one_lane_kernel():
    """in the child process: the pair kernel's lengths, answered by refine_kernel<.., float>"""
    import oracle as orc
    from lance_amd.engine import Engine
    assert os.environ.get(SWITCH) is not None
    orc.lib()
    e = Engine()
    cases = [(arm, d) for arm, d in CASES if arm.endswith("-pair")]
    for arm, d in cases:
        case(e, arm, d)
    e.close()
    print(f"one-lane kernel cases ok: {len(cases)}")


def test_one_lane_kernel_by_the_switch():
    env = dict(os.environ, **{SWITCH: "1"})
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_zz_gpu_refine_real as t; "
                        "t._pair_lengths_on_the_one_lane_kernel()" % (ROOT, os.path.join(ROOT, "tests"))],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "one-lane kernel cases ok: 12" in r.stdout
