"""refine_rows_u8_kernel (lance_amd/csrc/search.hip) passes a query's loaded rows through a 32-row LDS tile in four rounds of 32
candidate slots: write the round's registers, consume, and the next round overwrites the tile.  A round, a write inside a round (8 rows
per instruction) and the consume pass are each skipped by the candidate count, so the counts at every round boundary are what can go
wrong: 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127 and 128 candidates.

The index: twelve lists of exactly those sizes (and a thirteenth of 2,000 rows, for the PQ training and a full list), far apart, so
that a query aimed at a list and searched with nprobes = 1 has that list's rows as its candidates and nothing else: count < k * refine,
dead slots from there to 128.  The candidate counts are read back (search_candidates) and asserted.  d = 16 / 48 / 64 (rows shorter than
a 128-byte block), 128 (one block), 144 / 272 (a last block of one piece: the d > 128 instantiation, accumulators live across blocks);
L2 and dot; ids and distance bits against the CPU oracle, the kernel asserted through `refine_u8` and `count:refine_rows`; the same
cases answered by the pair kernel (LANCE_HIP_REFINE_U8_V1=1) in a child process; a stored row id beyond the attached column is refused
with the error and the query count of the pair kernel's day."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_pm_scan import _np
from test_zz_gpu_refine_rows import ROWS_DEFAULT, SWITCH, _kernel_used
from test_zz_gpu_refine_u8 import _equal

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COUNTS = [1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 127, 128]
BIG = 2000
DIMS = {16: 4, 48: 12, 64: 16, 128: 16, 144: 9, 272: 17}      # d -> M
METRICS = ["l2", "dot"]
PER_LIST = 2                                   # queries aimed at each list; one more at the big list: 27, not a multiple of a workgroup's four
# (k, refine_factor): keff 128 (every count is short of it or meets it), 100 (the flagship: lists of 127 / 128 rows fill it), 33 and 1
RUNS = [(16, 8), (10, 10), (11, 3), (1, 1)]


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


_cache = {}


def _fixture(oracle, metric, d):
    """rows, queries, models and the oracle's index: built once per (metric, d), never changed.  List i's centre is 200 on its own
    d / 16 coordinates and 20 elsewhere: the nearest centre under L2 and the largest product under dot for anything close to it."""
    if (metric, d) not in _cache:
        rng = np.random.default_rng(4100 + d)
        sizes = COUNTS + [BIG]
        nlist, w = len(sizes), d // 16
        cent = np.full((nlist, d), 20.0, f32)
        for i in range(nlist):
            cent[i, i * w:(i + 1) * w] = 200.0
        x = np.concatenate([cent[i] + rng.integers(0, 8, (s, d)) for i, s in enumerate(sizes)]).astype(f32)
        x[-1, :] = cent[-1] + 55.0                       # the column's last row reaches the top of the byte range: 255
        aim = np.r_[np.repeat(np.arange(len(COUNTS)), PER_LIST), nlist - 1]
        q = (cent[aim] + rng.uniform(0, 8, (aim.size, d))).astype(f32)      # queries need not be integers
        part, _ = oracle.assign(x, cent, metric)
        assert (np.bincount(np.asarray(part).astype(np.int64), minlength=nlist) == sizes).all(), "a row left its list"
        res = oracle.residual(x, cent, part) if metric == "l2" else x
        cb, _ = oracle.pq_train(res[-BIG:], DIMS[d], max_iters=3, seed=d + 1)
        _cache[(metric, d)] = (x, q, cent, cb, aim, oracle.build_index(x, cent, cb, metric))
    return _cache[(metric, d)]


def _gpu_index(eng, metric, x, cent, cb, rid=None):
    from lance_amd.engine import DeviceIndex
    gpart, gcodes, _ = eng.ivfpq_encode(x, cent, cb, metric)
    return DeviceIndex.create(eng, metric, cent, cb, gpart, gcodes, rid, raw=x)


def case_counts(eng, oracle, metric, d, rows):
    x, q, cent, cb, aim, oidx = _fixture(oracle, metric, d)
    gidx = _gpu_index(eng, metric, x, cent, cb)
    want = np.minimum(np.r_[np.repeat(COUNTS, PER_LIST), BIG], 128)
    cnt = (_np(gidx.search_candidates(q, 128, 1, exact=False)[0]) >= 0).sum(axis=1)
    assert (cnt == want).all(), f"candidate counts {cnt.tolist()}: not one query per round boundary"
    for k, rf in RUNS:
        with _kernel_used(eng, rows):
            gi, gd = gidx.search(q, k, 1, rf)
        oi, od = oidx.search(q, k, 1, refine=rf, raw=x)
        _equal(gi, gd, oi, od, f"{metric} d={d} k={k} refine={rf}")
    # two lists per query: counts that are sums across a boundary (1 + 31 = 32, 32 + 33 = 65, 63 + 64 = 127 ... as the probes fall)
    with _kernel_used(eng, rows):
        gi, gd = gidx.search(q[:-1], 16, 2, 8)
    oi, od = oidx.search(q[:-1], 16, 2, refine=8, raw=x)
    _equal(gi, gd, oi, od, f"{metric} d={d} two lists")
    gidx.close()


def case_bad_row(eng, oracle, metric, d, rows):
    import torch
    from lance_amd._lib import LanceHipError
    x, q, cent, cb, aim, _ = _fixture(oracle, metric, d)
    n, k, rf = x.shape[0], 16, 8
    victim = int(np.cumsum(COUNTS)[COUNTS.index(65)] - 1)      # the last row of the list of 65: slot 64 or below, in the third round
    rid = np.arange(n, dtype=np.uint64)
    rid[victim] = n                                           # one id beyond the attached column
    oidx = oracle.build_index(x, cent, cb, metric, row_ids=rid)
    gidx = _gpu_index(eng, metric, x, cent, cb, rid=rid.view(np.int64))
    met = (_np(gidx.search_candidates(q, k * rf, 1, exact=False)[0]) == n).any(axis=1)
    assert met.sum() == PER_LIST and met[aim == COUNTS.index(65)].all(), "the queries aimed at the victim's list do not meet it"
    ids = torch.full((q.shape[0], k), -1, dtype=torch.int64, device="cuda")
    dists = torch.full((q.shape[0], k), float("nan"), dtype=torch.float32, device="cuda")
    with pytest.raises(LanceHipError, match="raw vectors") as err:
        with _kernel_used(eng, rows):
            gidx.search(q, k, 1, rf, out=(ids, dists))
    assert int(re.search(r"\((\d+) queries\)", str(err.value)).group(1)) == met.sum(), "not exactly the queries that met the id are flagged"
    gi, gd = _np(ids), _np(dists)
    assert not ((gi == n) & np.isfinite(gd)).any(), "the id beyond the column was ranked"
    oi, od = oidx.search(q, k, 1, refine=rf, raw=np.vstack([x, x[victim:victim + 1]]))
    keep = ~met
    assert (gi.view(np.uint64)[keep] == oi[keep]).all() and (gd.view(np.uint32)[keep] == od.view(np.uint32)[keep]).all(), "an unflagged query changed"
    gidx.close()


CASES = [(case_counts, m, d) for m in METRICS for d in DIMS] + [(case_bad_row, "l2", 128), (case_bad_row, "dot", 48), (case_bad_row, "l2", 144)]


@pytest.mark.parametrize("case,metric,d", CASES, ids=[f"{c.__name__[5:]}-{m}-{d}" for c, m, d in CASES])
def test_rounds_of_the_tile(eng, oracle, case, metric, d):
    assert ROWS_DEFAULT, f"{SWITCH} is set: this process cannot reach the whole-row kernel"
    case(eng, oracle, metric, d, True)


def _all_cases_pair_kernel():
    """in the child process: every case above, answered by the pair kernel"""
    import oracle as orc
    from lance_amd.engine import Engine
    assert not ROWS_DEFAULT
    orc.lib()
    e = Engine()
    for case, metric, d in CASES:
        case(e, orc, metric, d, False)
    e.close()
    print(f"pair kernel cases ok: {len(CASES)}")


def test_pair_kernel_agrees_on_the_same_cases():
    env = dict(os.environ, **{SWITCH: "1"})
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_zz_gpu_refine_rows_tile as t; t._all_cases_pair_kernel()"
                        % (ROOT, os.path.join(ROOT, "tests"))], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"pair kernel cases ok: {len(CASES)}" in r.stdout
