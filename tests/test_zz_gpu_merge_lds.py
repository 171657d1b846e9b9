"""The merge kernels of the quantised IVF-PQ flow (lance_amd/csrc/search_q.hip: ivfpq_qmerge1g_kernel for nprobes <= 16,
ivfpq_qmerge_kernel above) keep the histogram of pass A and the compacted survivors of pass B in the SAME LDS (QmCutOverlay): the
histogram is dead once the cut is written, the compaction starts behind the barrier that follows.  These cases walk the windows that
overlay opens; each compares ids and distance bits with the CPU oracle and asserts that the batch took the matrix-core scan, whose
survivors these kernels merge (the `ivfpq_mscan` timer).

  two chunks     More than 512 survivors per query: pass A has to run through EVERY chunk before the cut is taken, and pass B re-reads
                 them and writes the compaction over the histogram chunk after chunk.  24 overlapping lists (centres 64 +- 12.5 per
                 component, rows sigma 14: a row of a neighbouring list is about as far from a query as one of its own), six of them with
                 101 .. 160 rows: at k * refine = 100 the bound of a query whose nearest list is one of those is that list's 100th
                 distance, i.e. nearly its largest, and most rows of the other probed lists pass it.  By exact distances (computed
                 below and asserted, so that the case cannot quietly stop being one) over a third of the 700 queries have more than 512
                 rows under their bound at nprobes 8, and some more than 1,024 at nprobes 16; segments over 256 rows overflow into the
                 rescan, so the same batch also holds queries whose pool entries arrive in `ckey` before the histogram is zeroed.  At
                 k * refine = 128 the six lists are too short for a bound: class B queries, pool only.
  ties           Rows duplicated ~80 times (the data of test_mscan_many_ties): overflowed segments together with class-A survivors
                 of the same query; with refine on a tie lies across the k * refine boundary, so the selection cannot stop at the
                 tightening rounds and takes the sort over the dynamic region (which held the staged residuals until then).
  sizes          k * refine = 1 and 128, refine on and off; nprobes 1 (4,200 queries, what the route asks for), 16 (the largest
                 dynamic region of the one-group kernel: 8 KB at d = 128) and 17 (the general kernel).
  shapes         (d, M) = (64, 16) and (128, 32), cosine, an f16 column: the other instantiations of both kernels."""
import numpy as np
import pytest

from test_gpu_pm_scan import _models, clustered
from test_zz_gpu_mscan import _check

pytestmark = pytest.mark.gpu
f32 = np.float32


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _pair(eng, oracle, x, cent, cb, metric="l2"):
    from lance_amd.engine import DeviceIndex
    oidx = oracle.build_index(x, cent, cb, metric)
    gpart, gcodes, _ = eng.ivfpq_encode(x, cent, cb, metric)
    return DeviceIndex.create(eng, metric, cent, cb, gpart, gcodes, None, raw=x), oidx


def _sq_dists(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return (a * a).sum(1)[:, None] - 2.0 * (a @ b.T) + (b * b).sum(1)[None, :]


_mixed_cache = {}


def _mixed(oracle):
    """lists of mixed size that overlap: built once, never changed"""
    if not _mixed_cache:
        rng = np.random.default_rng(1)
        d, m, nlist, nq = 128, 16, 24, 700
        sizes = np.concatenate([[101, 104, 110, 129, 135, 160], rng.integers(300, 1400, nlist - 6)])
        centres = 64.0 + rng.uniform(-12.5, 12.5, (nlist, d))
        x = np.clip(np.rint(np.concatenate([centres[i] + rng.normal(0, 14.0, (s, d)) for i, s in enumerate(sizes)])), 0, 218).astype(f32)
        which = np.where(rng.random(nq) < 0.5, rng.integers(0, 6, nq), rng.integers(0, nlist, nq))      # half of the queries at the short lists
        q = np.clip(np.rint(centres[which] + rng.normal(0, 14.0, (nq, d))), 0, 218).astype(f32)
        cent = centres.astype(f32)
        part, _ = oracle.assign(x, cent)
        res = oracle.residual(x, cent, part)
        cb, _ = oracle.pq_train(res[rng.choice(len(x), 4096, replace=False)], m, max_iters=3, seed=5)
        _mixed_cache["v"] = (x, q, cent, cb, np.asarray(part).astype(np.int64))
    return _mixed_cache["v"]


def _rows_under_bound(x, q, cent, part, keff, nprobes):
    """per query, by exact distances: rows of its probed lists at or under the keff-th distance of its nearest list, in segments of at
    most 256 (longer ones overflow into the rescan); -1 where the nearest list is shorter than keff (no bound: class B)"""
    order = np.argsort(_sq_dists(q, cent), axis=1)
    dx = _sq_dists(q, x)
    out = np.empty(len(q), np.int64)
    overflowed = np.zeros(len(q), bool)
    for i in range(len(q)):
        own = np.sort(dx[i, part == order[i, 0]])
        if own.size < keff:
            out[i] = -1
            continue
        under = np.isin(part, order[i, :nprobes]) & (dx[i] <= own[keff - 1])
        per = np.bincount(part[under], minlength=len(cent))
        overflowed[i] = per.max() > 256
        out[i] = np.where(per > 256, 0, per).sum()
    return out, overflowed


def test_two_chunks_of_survivors(eng, oracle):
    x, q, cent, cb, part = _mixed(oracle)
    sizes = np.bincount(part, minlength=len(cent))
    assert ((sizes > 100) & (sizes < 200)).sum() >= 4, "no list barely above k * refine rows"
    r8, o8 = _rows_under_bound(x, q, cent, part, 100, 8)
    r16, o16 = _rows_under_bound(x, q, cent, part, 100, 16)
    assert (r8 > 512).sum() >= 100 and (r16 > 1024).sum() >= 50, "not the case of several chunks any more"
    assert (o8 & (r8 > 0)).sum() >= 50, "no query with overflowed segments beside class-A survivors"
    assert (_rows_under_bound(x, q, cent, part, 128, 16)[0] == -1).sum() >= 50, "no class-B queries at k * refine = 128"
    gidx, oidx = _pair(eng, oracle, x, cent, cb)
    # (k, nprobes, refine): keff 100 with refine (the set of the tightening rounds) and without (the sort), keff 128 (class B beside class A)
    _check(eng, gidx, oidx, q, q, x, [(10, 8, 10), (10, 16, 10), (100, 8, 0), (100, 16, 0), (16, 16, 8), (128, 16, 0), (30, 8, 0)])
    gidx.close()


def test_sizes_and_probe_counts(eng, oracle):
    x, q, cent, cb, _ = _mixed(oracle)
    gidx, oidx = _pair(eng, oracle, x, cent, cb)
    _check(eng, gidx, oidx, q, q, x, [(1, 8, 0), (1, 8, 1), (1, 16, 10), (10, 16, 0), (10, 17, 10), (100, 17, 0), (128, 24, 0), (64, 17, 2)])
    q1 = np.tile(q, (6, 1))                            # 4,200 queries: nprobes = 1 reaches the partition-major route from 4,096 pairs
    _check(eng, gidx, oidx, q1, q1, x, [(10, 1, 10), (100, 1, 0), (1, 1, 1)])
    gidx.close()


def test_ties_overflow_and_sort_path(eng, oracle):
    rng = np.random.default_rng(5)
    d, m, nlist, nq = 128, 16, 16, 600
    base = clustered(300, d, 8)
    x = base[rng.integers(0, 300, 24000)]
    q = base[rng.integers(0, 300, nq)] + rng.integers(0, 2, (nq, d)).astype(f32)
    cent, cb = _models(oracle, x, nlist, m, "l2", seed=4)
    gidx, oidx = _pair(eng, oracle, x, cent, cb)
    before = eng.search_stats()
    # refine on with ~80 copies of every row: the k * refine boundary cuts through a group of equal keys
    _check(eng, gidx, oidx, q, q, x, [(10, 8, 4), (10, 8, 10), (10, 16, 10), (1, 16, 1), (40, nlist, 0), (16, 16, 8)])
    print(f"exact replays of the last call: {eng.search_stats()} (before: {before})")
    gidx.close()


@pytest.mark.parametrize("metric,d,m", [("l2", 64, 16), ("l2", 128, 32), ("cosine", 128, 16), ("cosine", 64, 16)])
def test_other_instantiations(eng, oracle, metric, d, m):
    n, nlist, nq = 20000, 24, 700
    x = clustered(n, d, 900 + d + m) + (1.0 if metric == "cosine" else 0.0)
    q = clustered(nq, d, 950 + d + m) + (1.0 if metric == "cosine" else 0.0)
    cent, cb = _models(oracle, x, nlist, m, metric, seed=d + m + 3)
    gidx, oidx = _pair(eng, oracle, x, cent, cb, metric)
    _check(eng, gidx, oidx, q, q, x, [(10, 8, 10), (10, 16, 0), (10, 17, 10), (100, 16, 0), (128, 17, 0), (1, 8, 1)])
    gidx.close()


def test_f16_column(eng, oracle):
    rng = np.random.default_rng(23)
    n, d, m, nlist, nq = 30000, 128, 16, 64, 800
    c = rng.standard_normal((64, d)) * 2
    x = (c[rng.integers(0, 64, n)] + rng.standard_normal((n, d)) * 0.7).astype(np.float16)
    q = (c[rng.integers(0, 64, nq)] + rng.standard_normal((nq, d)) * 0.7).astype(np.float16)
    cent = x[rng.choice(n, nlist, replace=False)].copy()
    part, _ = oracle.assign(x, cent)
    cb, _ = oracle.pq_train(oracle.residual(x, cent, part)[:4096], m, max_iters=3, seed=2)
    gidx, oidx = _pair(eng, oracle, x, cent, cb)
    _check(eng, gidx, oidx, q, q, x.astype(f32), [(10, 10, 10), (10, 16, 0), (10, 17, 10), (100, 16, 0)])
    gidx.close()
