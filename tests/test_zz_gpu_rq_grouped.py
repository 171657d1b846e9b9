"""The partition-major scan of IVF_RQ batches (lance_amd/csrc/rq_pm.cuh: ivfrq_pm_scan_kernel, 32 pairs of a partition per i8 MFMA tile,
the u8 table lookups as a product with the rows' one-hot expansion) against tests/rq_spec.py bit for bit -- ids and distance bits, no
tolerances -- and against the pair-major scan of the same call in a child process that switches the route off.  Every search runs under
`on_route`: `ivfrq_pm_scan` served it and `ivfrq_scan` / `ivfrq_wide_scan` did not, or the reverse where the case must stay pair-major;
and every case first asks lance_hip_ivfrq_plan what it expects.

The route takes batches of at least G pairs per partition on average.  A block geometry case puts `n1` pairs (QB - 1, QB, QB + 1,
2 QB + 3) on partition 0 with n1 queries between centroids 0 and 1 and fills the batch with FILL queries between centroid 1 and
centroid 2, whose partition is empty (those pairs scan nothing and must report empty lists); one of them IS centroid 1 (zero residual:
qmin == qmax for that pair only).  Sorted last: newest device code last."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import refine_spec as F
import rq_spec as R
from test_zz_gpu_rq import check_search, eng, same_bits
from test_zz_gpu_rq_scan import device_index, half_mask, row_ids

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = 128                                            # rq_pm.cuh: RQPM_MIN_PAIRS_PER_LIST, the gate
QB, TILE, BUF, FILL = 32, 128, 256, 3 * G // 2      # rq_pm.cuh: RQPM_QB, RQPM_TILE, RQPM_CAP; 2 * FILL pairs >= G * 3 partitions
DMAX = 584                                         # the last d whose block of tables fits one workgroup's LDS
TIMERS = ("ivfrq_pm_scan", "ivfrq_scan", "ivfrq_wide_scan")
COPIES = -(-2 * G // 3)                            # of three design queries: 3 COPIES pairs per probe >= G * 2 partitions


def planned(nq, nprobes, nlist, keff, d, filtered=False):
    from lance_amd import _lib
    return _lib.load().lance_hip_ivfrq_plan(nq, min(nprobes, nlist), nlist, keff, d, int(filtered), 0) == 1


def on_route(call, route="grouped"):
    """call() with the kernel timers on: only the scan of `route` (grouped | pair | wide) served it"""
    e = eng()
    e.timing(True)
    try:
        for name in TIMERS:
            e.timing_query(name)                                 # (a query returns a timer's launches and resets it)
        out = call()
        ran = [e.timing_query(name)[1] for name in TIMERS]
    finally:
        e.timing(False)
    assert [r >= 1 for r in ran] == [route == "grouped", route == "pair", route == "wide"], dict(zip(TIMERS, ran))
    return out


# ---- partition and block geometry -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry(d, na, nb, n1, ids, metric):
    """partitions of na and nb rows at 4 e_0 and 4 e_1, an empty one at 4 e_2 + e_1; n1 queries probe {0, 1}, the other FILL probe {1, 2}"""
    import oracle
    x, cent = R.sized_partitions([na, nb, 0], d, seed=d + na)
    cent[2, 1] = 1.0                                             # centroid 1's second probe is partition 2 under both metrics
    rng = np.random.default_rng([d, na, nb, n1])
    noise = lambda n: (rng.standard_normal((n, d)) * 0.3 / np.sqrt(d / 8)).astype(f32)
    q = np.concatenate([(cent[0] + cent[1]) / 2 + noise(n1), (cent[1] + cent[2]) / 2 + noise(FILL)]).astype(f32)
    q[n1 + 5] = cent[1]
    q = np.ascontiguousarray(q[rng.permutation(len(q))])
    ix, spec = device_index(x, cent, R.rotation(d, d + 2), metric, row_ids(na + nb, ids == "permuted", d))
    probes = oracle.find_partitions(q, cent, 2, metric)[0]
    assert [(probes == p).sum() for p in range(3)] == [n1, n1 + FILL, FILL]
    assert list(np.diff(oracle.partition_layout(spec[3], 3)[0].astype(np.int64))) == [na, nb, 0]
    return ix, spec, q


GEOMETRY = [
    # d, rows of partitions 0 and 1, pairs on partition 0, k, ids, metric
    (8, 31, TILE - 1, QB - 1, 1, "permuted", "l2"),              # all remainder, no tile | three waves and a remainder
    (24, 32, TILE + 1, QB, 10, "permuted", "dot"),
    (128, BUF + 2 * TILE + 30, 33, QB + 1, 128, "permuted", "l2"),      # past one truncation; 16-byte row loads
    (136, TILE, BUF + 2 * TILE + 30, 2 * QB + 3, 10, "addresses", "dot"),
    (256, 33, TILE, 2 * QB + 3, 10, "addresses", "l2"),          # two sub-blocks of 16 prepared pairs
    (DMAX, 32, TILE + 1, QB + 1, 10, "permuted", "l2"),          # the largest block of tables: sub-blocks of 7
]


@pytest.mark.parametrize("d,na,nb,n1,k,ids,metric", GEOMETRY)
def test_block_geometry(d, na, nb, n1, k, ids, metric):
    ix, spec, q = geometry(d, na, nb, n1, ids, metric)
    rid = spec[6]
    assert (rid.min() >= 2 ** 31 and rid.max() >= 2 ** 32) == (ids == "addresses")
    for kk in [k] + sorted({1, 10, 128} - {k}) * (d <= 128):
        assert planned(len(q), 2, 3, kk, d)
        on_route(lambda: check_search(ix, spec, q, kk, 2, metric))


# ---- ties and the falling threshold: the same call on both routes -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_cases():
    """name -> (index, spec, queries [3 COPIES], k, cut_tie): design queries whose lists pass a truncation or are cut on a tie, tiled"""
    import oracle
    out = {}
    fixtures = [(f"{order}/10", R.ordered_partition(oracle, order, "l2", 10), 10) for order in ("descending", "staircase", "tie_then_closer")]
    fixtures += [(f"{order}/128", F.ordered_partition(oracle, "rq", order, "l2", 128, 2 * BUF, 2 * BUF + 2 * F.CHUNK + 33), 128) for order in ("descending", "tie_cut")]
    for name, f, k in fixtures:
        x = f["x"]
        assert f["N"] % 32 in (1, 13, 0) and len(x) < 2000
        ix, spec = device_index(x, f["cent"], f["P"], "l2", row_ids(len(x), False, 3), f.get("built"))
        q = np.tile(np.stack([f["q"], x[5] + f32(0.1), x[9]]), (COPIES, 1))
        out[name] = (ix, spec, np.ascontiguousarray(q), k, bool(f["cut_tie"]))
    assert out["tie_then_closer/10"][4] and out["tie_cut/128"][4] and not out["descending/10"][4]
    return out


def run_tie_cases(path=None):
    """-> name/nprobes -> (ids, distances, replayed queries); the child process saves them to `path`"""
    got = {}
    for name, (ix, _, q, k, _) in tie_cases().items():
        for nprobes in (1, 2):
            gi, gd = ix.search(q, k, nprobes)
            got[f"{name}/{nprobes}"] = (gi.cpu().numpy().view(np.uint64), gd.cpu().numpy(), np.uint32(eng().search_stats()))
    if path:
        np.savez(path, **{f"{name}|{i}": v for name, t in got.items() for i, v in enumerate(t)})
    return got


def test_ties_replay_like_the_pair_major_route(tmp_path):
    """partitions stored in an order chosen for the design query (descending: every row enters after the first cut; staircase: every later
    row is exactly the new k-th; a tie block cut at a truncation that still holds the k-th key at the end) on both routes: same ids, same
    bits, and the same number of replayed queries -- the cut-tie flag of every pair is the pair-major scan's.  The other route runs in a
    child process with LANCE_HIP_NO_RQ_GROUPED=1 (the switch is read once per process)."""
    path = str(tmp_path / "pair_major.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_zz_gpu_rq_grouped as t; t.run_tie_cases(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, LANCE_HIP_NO_RQ_GROUPED="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    import oracle
    other = np.load(path)
    cases = tie_cases()
    assert all(planned(3 * COPIES, nprobes, 2, k, 64) for _, _, _, k, _ in cases.values() for nprobes in (1, 2))
    got = on_route(run_tie_cases)
    for key, (gi, gd, replays) in got.items():
        name, nprobes = key.rsplit("/", 1)
        assert (gi == other[key + "|0"]).all() and same_bits(gd, other[key + "|1"]), key
        assert replays == other[key + "|2"], (key, replays, other[key + "|2"])
        ix, spec, q, k, cut = cases[name]
        if cut and nprobes == "1":
            assert replays >= COPIES, key                          # the design query's list is cut on a tie: replayed in every copy
        oi, od = R.search(oracle, *spec[:6], q[:3], k, int(nprobes), "l2", row_ids=spec[6])
        assert (gi == np.tile(oi, (COPIES, 1))).all() and same_bits(gd, np.tile(od, (COPIES, 1))), key


# ---- refine through the grouped scan, and what stays pair-major ------------------------------------------------------------------------------
def test_refine_and_what_stays_pair_major():
    from test_zz_gpu_refine_sqrq import D, NLIST, NPROBES, SETUPS, candidates, check_refined
    ix, spec, q100 = SETUPS["rq/l2/f32"]()
    q = np.ascontiguousarray(np.concatenate([q100 + f32(0.01 * i) for i in range(6)])[:G * NLIST // NPROBES])      # 512 x 4 pairs = G x 16 partitions
    assert planned(len(q), NPROBES, NLIST, 128, D) and not planned(len(q), NPROBES, NLIST, 129, D) and not planned(len(q), NPROBES, NLIST, 50, D, True)
    half = np.random.default_rng(23).random(int(spec[3].max()) + 1) < 0.5
    cand50 = candidates(spec, q, 50, NPROBES)
    on_route(lambda: check_refined(ix, spec, q, 10, 5, NPROBES, cand50))
    on_route(lambda: check_refined(ix, spec, q, 64, 2, NPROBES, candidates(spec, q, 128, NPROBES)))
    on_route(lambda: check_refined(ix, spec, q, 43, 3, NPROBES, candidates(spec, q, 129, NPROBES)), "wide")      # keff = 129: the wide capacity
    on_route(lambda: check_refined(ix, spec, q, 10, 5, NPROBES, candidates(spec, q, 50, NPROBES, allow=half), allow=half), "pair")      # the f32 fold


def test_past_the_lds_limit_stays_pair_major():
    """d = 592: a block's tables no longer fit one workgroup's LDS"""
    d = DMAX + 8
    ix, spec, q = geometry(d, 33, 40, QB, "permuted", "l2")
    assert planned(len(q), 2, 3, 10, DMAX) and not planned(len(q), 2, 3, 10, d)
    on_route(lambda: check_search(ix, spec, q, 10, 2, "l2"), "pair")
