"""The partition-major scan of IVF_SQ batches (lance_amd/csrc/sq_pm.cuh: ivfsq_pm_scan_kernel, 32 queries of a partition per i8 MFMA
tile) against tests/sq_spec.py bit for bit -- ids and distance bits, no tolerances -- and against the pair-major scan of the same call
in a child process that switches the route off.  Every search here must be served by `ivfsq_pm_scan` and never by `ivfsq_scan`.

The route takes batches of at least 64 pairs per partition on average, so every case has that many: a block geometry case puts `n1` pairs
(QB - 1, QB, QB + 1, 2 QB + 3) on partition 0 with n1 queries between centroids 0 and 1 and fills the batch with FILL queries between
centroid 1 and the far centroid 2, whose partition is empty (those pairs scan nothing and must report empty lists).  The fixtures of three design
queries (sq_spec.large_sum_partition, refine_spec.ordered_partition) are tiled to 129.  Sorted last: newest device code last."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import refine_spec as F
import sq_spec as S
from test_zz_gpu_refine_sqrq import candidates, check_refined, sq_index
from test_zz_gpu_sq import built, check_search, eng, same_bits
from test_zz_gpu_sq_scan import flat_spec, half_mask

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QB, TILE, BUF, FILL = 32, 128, 256, 128            # sq_pm.cuh: SQPM_QB, SQPM_TILE, SQPM_CAP; 2 * 128 pairs >= 64 * 3 partitions
TIMERS = ("ivfsq_pm_scan", "ivfsq_scan", "ivfsq_wide_scan")


def on_route(call, wide=False):
    """call() with the kernel timers on: the grouped scan served it and the pair-major scan did not (wide: the other way round)"""
    e = eng()
    e.timing(True)
    try:
        for name in TIMERS:
            e.timing_query(name)                                 # (a query returns a timer's launches and resets it)
        out = call()
        ran = [e.timing_query(name)[1] for name in TIMERS]
    finally:
        e.timing(False)
    assert (ran[0] == 0 and ran[2] >= 1) if wide else (ran[0] >= 1 and ran[1] == 0 and ran[2] == 0), dict(zip(TIMERS, ran))
    return out


# ---- partition and block geometry -------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def geometry(d, na, nb, n1, ids):
    """partitions of na and nb rows around centroids -2 and +2 (every component), an empty one at 60; n1 queries probe {0, 1}, the
    other FILL probe {1, 2}"""
    import oracle
    import rowid_fixtures
    rng = np.random.default_rng([d, na, nb, n1])
    cent = np.ascontiguousarray(np.stack([np.full(d, -2.0, f32), np.full(d, 2.0, f32), np.full(d, 60.0, f32)]))
    noise = lambda n, s: (rng.standard_normal((n, d)) * s).astype(f32)
    x = np.ascontiguousarray(np.concatenate([cent[0] + noise(na, 0.5), cent[1] + noise(nb, 0.5)]))
    q = np.ascontiguousarray(np.concatenate([noise(n1, 0.3), f32(30.0) + noise(FILL, 0.3)]))
    q = q[rng.permutation(len(q))]
    rid = rowid_fixtures.row_addresses(na + nb, d) if ids == "addresses" else S.permuted_ids(na + nb, d)
    ix, spec = sq_index(x, cent, "l2", rid, bounds=(-4.0, 4.0), raw=np.zeros((1, d), f32))
    probes = oracle.find_partitions(q, cent, 2, "l2")[0]
    assert [(probes == p).sum() for p in range(3)] == [n1, n1 + FILL, FILL]
    assert (spec[2][1] == np.repeat([0, 1], [na, nb])).all()
    return ix, flat_spec(spec), q


GEOMETRY = [
    # d, rows of partitions 0 and 1, pairs on partition 0, k, ids
    (1, 1, TILE - 1, QB - 1, 1, "permuted"),
    (17, TILE, TILE + 1, QB, 10, "permuted"),
    (128, BUF + 2 * TILE + 30, 1, QB + 1, 128, "permuted"),
    (1000, TILE + 1, BUF + 2 * TILE + 30, 2 * QB + 3, 10, "permuted"),
    (128, TILE - 1, 3 * TILE, 2 * QB + 3, 10, "addresses"),
]


@pytest.mark.parametrize("d,na,nb,n1,k,ids", GEOMETRY)
def test_block_geometry(d, na, nb, n1, k, ids):
    ix, spec, q = geometry(d, na, nb, n1, ids)
    rid = spec[4]
    on_route(lambda: check_search(ix, spec, q, k, 2, "l2"))
    if ids == "addresses":
        assert rid.min() >= 2 ** 31 and rid.max() >= 2 ** 32
        return
    nothing = np.zeros(int(rid.max()) + 1, bool)
    only_1 = nothing.copy(); only_1[rid[na:]] = True              # empties partition 0
    for allow in (half_mask(rid, d), nothing, only_1):
        on_route(lambda: check_search(ix, spec, q, k, 2, "l2", prefilter=allow))
    for other_k in {1, 10, 128} - {k}:
        on_route(lambda: check_search(ix, spec, q, other_k, 2, "l2"))


# ---- metrics and element types --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,metric,kind", [(17, "dot", "f32"), (128, "cosine", "f32"), (1000, "dot", "f32"), (1, "cosine", "f32"), (128, "l2", "f16"),
                                           (1000, "cosine", "f16")])
def test_metrics_and_f16_columns(d, metric, kind):
    """Gaussian rows in four partitions (one empty), 140 queries: the pairs fall on the partitions as they may"""
    n = 600
    ix, spec = built(n, d, 4, metric, kind)
    _, q = S.gaussian(n, d, 140, seed=100 + n + d, kind=kind)
    half = half_mask(spec[4], d)
    for k, nprobes in ((10, 2), (128, 4), (1, 2)):
        on_route(lambda: check_search(ix, spec, q, k, nprobes, metric))
        on_route(lambda: check_search(ix, spec, q, k, nprobes, metric, prefilter=half))


# ---- ties and the falling threshold: the same call on both routes -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tie_cases():
    """name -> (index, spec, queries [129], k, nprobes, metric): design queries whose lists are cut on a tie, tiled"""
    import oracle
    out = {}
    for metric in ("l2", "dot"):
        f = S.large_sum_cached(516, metric, 900)
        ix, spec = sq_index(f["x"], f["cent"], metric, f["rid"], bounds=f["bounds"], raw=np.zeros((1, 516), f32))
        for k in S.LARGE_SUM_KS:
            for nprobes in (1, 2):
                out[f"large/{metric}/{k}/{nprobes}"] = (ix, flat_spec(spec), np.tile(f["q"], (43, 1)), k, nprobes, metric)
    for order, k in (("descending", 10), ("tie_cut", 128), ("tie_cut", 10)):
        f = F.ordered_partition(oracle, "sq", order, "l2", k, 2 * BUF, (2 * BUF + 2 * F.CHUNK) // 32 * 32 + 33)
        assert f["cut_tie"] or order != "tie_cut"
        q = np.tile(np.stack([f["q"], f["x"][5] + f32(0.1), f["x"][9]]), (43, 1))
        rid = np.random.default_rng(3).permutation(len(f["x"])).astype(np.uint64)
        ix, spec = sq_index(f["x"], f["cent"], "l2", rid, bounds=f["bounds"], raw=np.zeros((1, 64), f32))
        out[f"{order}/{k}"] = (ix, flat_spec(spec), np.ascontiguousarray(q), k, 2, "l2")
    return out


def run_tie_cases(path=None):
    """-> name -> (ids, distances, replayed queries); the child process saves them to `path`"""
    got = {}
    for name, (ix, _, q, k, nprobes, _) in tie_cases().items():
        gi, gd = ix.search(q, k, nprobes)
        got[name] = (gi.cpu().numpy().view(np.uint64), gd.cpu().numpy(), np.uint32(eng().search_stats()))
    if path:
        np.savez(path, **{f"{name}|{i}": v for name, t in got.items() for i, v in enumerate(t)})
    return got


def test_ties_replay_like_the_pair_major_route(tmp_path):
    """cut ties (integer sums past 2^24 that share one f32 key; k + 8 copies of one row) on both routes: same ids, same bits, and the same
    number of replayed queries -- the cut-tie flag of every pair is the pair-major scan's.  The other route runs in a child process
    with LANCE_HIP_NO_SQ_GROUPED=1 (the switch is read once per process)."""
    path = str(tmp_path / "pair_major.npz")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_zz_gpu_sq_grouped as t; t.run_tie_cases(%r)" % (ROOT, os.path.join(ROOT, "tests"), path)
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, LANCE_HIP_NO_SQ_GROUPED="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    import oracle
    other = np.load(path)
    cases = tie_cases()
    got = on_route(run_tie_cases)
    for name, (gi, gd, replays) in got.items():
        assert (gi == other[name + "|0"]).all() and same_bits(gd, other[name + "|1"]), name
        assert replays == other[name + "|2"], (name, replays, other[name + "|2"])
        ix, spec, q, k, nprobes, metric = cases[name]
        if name.startswith("tie_cut") or (name.startswith("large") and nprobes == 1):
            assert replays >= 43, name                            # the design query's list is cut on a tie: replayed in every copy
        codes, part, cent, b, rid = spec
        oi, od = S.search(oracle, codes, part, cent, q[:3], k, nprobes, metric, *b, row_ids=rid)
        assert (gi == np.tile(oi, (43, 1))).all() and same_bits(gd, np.tile(od, (43, 1))), name


# ---- refine: candidates through the grouped scan, and the wide capacity beside it --------------------------------------------------------
def test_refine_and_the_wide_capacity():
    from test_zz_gpu_refine_sqrq import NPROBES, SETUPS
    ix, spec, q100 = SETUPS["sq/l2/f32"]()
    q = np.ascontiguousarray(np.concatenate([q100, q100 + f32(0.05), q100[:60] + f32(0.1)]))      # 260 x 4 pairs >= 64 x 16 partitions
    half = np.random.default_rng(23).random(int(spec[3].max()) + 1) < 0.5
    on_route(lambda: check_refined(ix, spec, q, 10, 5, NPROBES, candidates(spec, q, 50, NPROBES)))
    on_route(lambda: check_refined(ix, spec, q, 10, 5, NPROBES, candidates(spec, q, 50, NPROBES, allow=half), allow=half))
    on_route(lambda: check_refined(ix, spec, q, 64, 2, NPROBES, candidates(spec, q, 128, NPROBES)))
    on_route(lambda: check_refined(ix, spec, q, 43, 3, NPROBES, candidates(spec, q, 129, NPROBES)), wide=True)      # keff = 129: today's wide route
