"""The u8 refine kernel that reads whole rows, a wave per query (lance_amd/csrc/search.hip refine_rows_u8_kernel), against the CPU oracle:
ids and distance bits, both metrics, and the pair kernel it replaces (refine_u8_kernel, LANCE_HIP_REFINE_U8_V1=1) on the same cases in a
child process -- the switch is read once per process.  Every case asserts through the `refine_u8` stage that the u8 copy answered and
through `count:refine_rows` which of the two kernels did.

What each case is there for (the layout: eight lanes x 16 bytes load one 128-byte block of a row, a wave-instruction covers 8 rows, the
blocks pass through a swizzled 64-row LDS tile in two halves and are consumed by two lanes per row in passes of 32 rows; lane l keeps
the keys and ids of slots l and l + 64 for the selection):
  d = 16    a row is ONE 16-byte piece: seven of a group's eight lanes must stay idle -- a lane that does not would read the next rows
  d = 48    three pieces, 48-byte rows: groups straddle 128-byte lines, five idle lanes
  d = 128   the full block (the flagship shape)
  d = 144   nine chunks: a full block and then a block of one piece -- the accumulators live across blocks, the tile is reused
  d = 272   seventeen chunks: two full blocks and one piece
  keff 1    one live slot: one load instruction, one pass, a selection of one
  keff 33   one row into the second pass of 32 and the fifth load instruction
  keff 100  the flagship; the second half of the tile holds 36 rows, the fourth pass four
  keff 128  every slot live: both halves, all four passes, the last lane's high slot
  keff 130  the next dispatch class: the pair kernel answers, whatever the switch says
  k = 64 of keff 128: a selection that keeps half the slots (the bit search stops at a key in the middle)
  short lists: an index of 61 rows and one list more, which stays empty, so every query has count < keff (dead slots in the middle of
            a load instruction, of a pass and of the selection), and one query probes only the empty list: count 0, nothing loaded,
            all outputs padding
  nq 1, 5, 257: not multiples of the four queries of a workgroup -- the idle waves of the last workgroup must leave without a barrier
  last rows: the column's last row is a candidate (big index: a query next to it, every list probed; short index: every row is one) --
            at d = 16 and 48 a lane that read past its row would read past the allocation
  duplicate rows: 41 copies of one row under different ids lie across the k-th place and across keff: the (distance, row id) order
            decides, through the equal-key branch of the selection
  bad row id: one stored id lies beyond the attached column: the queries that meet it are flagged (the call is refused and says how
            many), the id is not ranked, and every other query's answer is the oracle's"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_pm_scan import _models, _np, clustered
from test_zz_gpu_refine_u8 import _equal, _u8_used

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "LANCE_HIP_REFINE_U8_V1"
ROWS_DEFAULT = os.environ.get(SWITCH) is None      # which kernel this process dispatches to for keff <= 128

N, NLIST, NQ = 6000, 12, 257
DIMS = {16: 4, 48: 12, 128: 16, 144: 9, 272: 17}      # d -> M
METRICS = ["l2", "dot"]
DUP0, DUPS = 50, slice(100, 140)
# (k, refine_factor, nprobes, nq)
RUNS = [(1, 1, 3, NQ), (11, 3, 4, NQ), (10, 10, 4, NQ), (16, 8, NLIST, NQ), (64, 2, NLIST, 5), (10, 10, NLIST, 1), (13, 10, 4, NQ)]
SHORT_RUNS = [(10, 10, 1, NQ), (10, 10, NLIST + 1, NQ), (16, 8, 2, 5), (1, 1, 1, 1)]


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


class _kernel_used:
    """the searches inside read the u8 copy, and the whole-row kernel answered them (or did not)"""

    def __init__(self, eng, rows):
        self.eng, self.rows, self.u8 = eng, rows, _u8_used(eng, True)

    def __enter__(self):
        self.before = self.eng.timing_query("count:refine_rows")[1]
        self.u8.__enter__()
        return self

    def __exit__(self, *a):
        self.u8.__exit__(*a)
        if a[0] is None:
            took = self.eng.timing_query("count:refine_rows")[1] > self.before
            assert took == self.rows, "the whole-row kernel " + ("did not answer" if self.rows else "answered unexpectedly")


_cache = {}


def _fixture(oracle, metric, d):
    """the column, the queries, the models and the oracle's index: built once per (metric, d), never changed"""
    if (metric, d) not in _cache:
        x = clustered(N, d, 1300 + d, hi=255.0)
        x[0, :] = 0.0
        x[1, :] = 255.0                 # both ends of the byte range
        x[DUP0, :] = 218.0              # under dot the rows of largest norm come first for positive queries
        x[DUPS, :] = x[DUP0]            # 41 copies under different ids
        x[N - 1, :] = 217.0             # the column's last row: next in line under dot
        q = clustered(NQ, d, 1301 + d, integer=False)
        q[0, :] = x[N - 1] + f32(0.25)
        q[1, :] = x[DUP0] + f32(0.25)
        cent, cb = _models(oracle, x, NLIST, DIMS[d], metric, seed=d + 7)
        # one more list that no row falls into: far from every row under L2, the smallest product with every (non-negative) row under dot
        empty = np.full((1, d), 1000.0, f32) if metric == "l2" else np.zeros((1, d), f32)
        centS = np.vstack([cent, empty]).astype(f32)
        q[2, :] = 1000.0 if metric == "l2" else -q[2]     # probes the empty list first
        xs = np.ascontiguousarray(np.vstack([x[2:62], x[N - 1:]]))      # (without the all-zero row: under dot it ties between all lists)
        _cache[(metric, d)] = (x, q, cent, cb, oracle.build_index(x, cent, cb, metric), xs, centS, oracle.build_index(xs, centS, cb, metric))
    return _cache[(metric, d)]


def _gpu_index(eng, metric, x, cent, cb, rid=None):
    from lance_amd.engine import DeviceIndex
    gpart, gcodes, _ = eng.ivfpq_encode(x, cent, cb, metric)
    return DeviceIndex.create(eng, metric, cent, cb, gpart, gcodes, rid, raw=x)


def case_shapes(eng, oracle, metric, d, rows):
    x, q, cent, cb, oidx, _, _, _ = _fixture(oracle, metric, d)
    gidx = _gpu_index(eng, metric, x, cent, cb)
    for k, rf, nprobes, nq in RUNS:
        keff = k * rf
        with _kernel_used(eng, rows and keff <= 128):
            gi, gd = gidx.search(q[:nq], k, nprobes, rf)
        oi, od = oidx.search(q[:nq], k, nprobes, refine=rf, raw=x)
        _equal(gi, gd, oi, od, f"{metric} d={d} k={k} refine={rf} nprobes={nprobes} nq={nq}")
        if nprobes == NLIST and nq >= 2:
            ci = _np(gidx.search_candidates(q[:2], keff, nprobes, exact=False)[0])
            assert (ci[0] == N - 1).any(), "the column's last row is not among the candidates of the query next to it"
            dups = np.r_[DUP0, np.arange(DUPS.start, DUPS.stop)]
            assert np.isin(ci[1], dups).sum() == 41, "the duplicated rows are not all candidates"
            if k < 41:
                took = oi[1][np.isin(oi[1], dups)]
                assert 0 < took.size < 41 and (took == dups[:took.size]).all(), "the duplicated rows do not lie across the k-th place in row-id order"
    gidx.close()


def case_short_lists(eng, oracle, metric, d, rows):
    _, q, _, cb, _, xs, centS, oidx = _fixture(oracle, metric, d)
    gidx = _gpu_index(eng, metric, xs, centS, cb)
    for k, rf, nprobes, nq in SHORT_RUNS:
        keff = k * rf
        qq = q[2:3] if nq == 1 else q[:nq]            # the single query is the one that probes the empty list
        cnt = (_np(gidx.search_candidates(qq, keff, nprobes, exact=False)[0]) >= 0).sum(axis=1)
        if keff > 1:
            assert (cnt < keff).all(), "a candidate list is full: not the short-list case"
        if nprobes == 1:
            assert cnt[0 if nq == 1 else 2] == 0, "the query aimed at the empty list found rows"
        if nprobes == NLIST + 1:
            assert (cnt == xs.shape[0]).all(), "not every row (the last one included) is a candidate"
        with _kernel_used(eng, rows):
            gi, gd = gidx.search(qq, k, nprobes, rf)
        oi, od = oidx.search(qq, k, nprobes, refine=rf, raw=xs)
        _equal(gi, gd, oi, od, f"short lists {metric} d={d} k={k} refine={rf} nprobes={nprobes} nq={nq}")
    gidx.close()


def case_bad_row(eng, oracle, metric, d, rows):
    import torch
    from lance_amd._lib import LanceHipError
    x, q, cent, cb, _, _, _, _ = _fixture(oracle, metric, d)
    k, rf, nprobes, victim = 10, 10, 4, 7
    rid = np.arange(N, dtype=np.uint64)
    rid[victim] = N                                  # one id beyond the attached column of N rows
    qq = np.array(q[:64]); qq[3] = x[victim] + f32(0.25)
    if metric == "dot":
        nprobes = NLIST                              # (the victim need not rank high under dot: every list, so that it is met at all)
    oidx = oracle.build_index(x, cent, cb, metric, row_ids=rid)
    gidx = _gpu_index(eng, metric, x, cent, cb, rid=rid.view(np.int64))
    met = (_np(gidx.search_candidates(qq, k * rf, nprobes, exact=False)[0]) == N).any(axis=1)
    if metric == "l2":
        assert met[3]
    ids = torch.full((qq.shape[0], k), -1, dtype=torch.int64, device="cuda")
    dists = torch.full((qq.shape[0], k), float("nan"), dtype=torch.float32, device="cuda")
    if met.any():
        with pytest.raises(LanceHipError, match="raw vectors") as err:
            with _kernel_used(eng, rows):
                gidx.search(qq, k, nprobes, rf, out=(ids, dists))
        assert int(re.search(r"\((\d+) queries\)", str(err.value)).group(1)) == met.sum(), "not exactly the queries that met the id are flagged"
    else:
        gidx.search(qq, k, nprobes, rf, out=(ids, dists))
    gi, gd = _np(ids), _np(dists)
    assert not ((gi == N) & np.isfinite(gd)).any(), "the id beyond the column was ranked"
    # the other queries: the oracle reads a column with one more row, which no unflagged query touches
    oi, od = oidx.search(qq, k, nprobes, refine=rf, raw=np.vstack([x, x[victim:victim + 1]]))
    keep = ~met
    assert keep.sum() > 0
    assert (gi.view(np.uint64)[keep] == oi[keep]).all() and (gd.view(np.uint32)[keep] == od.view(np.uint32)[keep]).all(), "an unflagged query changed"
    gidx.close()


CASES = [(case_shapes, m, d) for m in METRICS for d in DIMS] + [(case_short_lists, m, d) for m in METRICS for d in (16, 48, 128, 144)] + \
        [(case_bad_row, m, d) for m in METRICS for d in (48, 128)]


@pytest.mark.parametrize("case,metric,d", CASES, ids=[f"{c.__name__[5:]}-{m}-{d}" for c, m, d in CASES])
def test_whole_row_kernel(eng, oracle, case, metric, d):
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


def test_pair_kernel_by_the_switch():
    env = dict(os.environ, **{SWITCH: "1"})
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_zz_gpu_refine_rows as t; t._all_cases_pair_kernel()"
                        % (ROOT, os.path.join(ROOT, "tests"))], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert f"pair kernel cases ok: {len(CASES)}" in r.stdout
