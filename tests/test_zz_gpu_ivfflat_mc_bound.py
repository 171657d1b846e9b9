"""The bound pass of a batched IVF_FLAT search on the matrix cores (lance_amd/csrc/flat_ivf_mc.hip: ivfflat_mc_bound_kernel,
ivfflat_mc_bound_eval_kernel) against the CPU specification (tests/ivfflat_range_spec.py, un-ranged), bit for bit: ids and distance
bits through IvfFlatIndex.nearest, on the fixture of tests/test_zz_gpu_ivfflat_mc.py (partitions of 300, 513, 129, 128, 127, 0, 77
and 1 real-valued rows; most queries are nearest to partition 0, queries 1 .. 12 to the 513 rows, query 0 to the single row).
Every case asserts that the bound pass took the new route.  Sorted last: newest device code last."""
import numpy as np
import pytest

import ivfflat_range_spec as V
import rowid_fixtures as F
import test_zz_gpu_ivfflat_mc as M

pytestmark = pytest.mark.gpu
COUNTERS = ("count:ivfflat_mc_bound", "count:ivfflat_mc_queued")


def check(metric, d, **kw):
    """M.check (ids and distance bits against the specification) -> rows the main pass queued; the bound pass ran on the matrix cores"""
    e = M.eng()
    before = [e.timing_query(c)[1] for c in COUNTERS]
    M.check(metric, d, **kw)
    bound, queued = (e.timing_query(c)[1] - b for c, b in zip(COUNTERS, before))
    assert bound > 0, "the bound pass did not run on the matrix cores"
    return queued


@pytest.mark.parametrize("d", [36, 200])                        # less than one stage with a tail; stages plus a tail
@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_route_and_bits(metric, d):
    check(metric, d)


@pytest.mark.parametrize("k", [1, 10, 128])                     # 128: partitions of 127 and 1 rows give no bound, 128 rows exactly k classes, 129 / 513 wrap
def test_k(k):
    check("l2", 36, k=k)


def test_one_class_gives_no_bound():
    """of the 513-row partition only rows 0, 256 and 512 are allowed: three rows, one class, k = 2 -- no bound, the specification's answer"""
    mask = np.ones(sum(M.SIZES), bool)
    mask[M.SIZES[0]:M.SIZES[0] + M.SIZES[1]] = False
    mask[M.SIZES[0] + np.array([0, 256, 512])] = True
    check("l2", 36, k=2, prefilter=mask)


def test_prefilter_and_row_ids():
    mask = np.random.default_rng(8).random(sum(M.SIZES)) < 0.3
    check("l2", 200, ids="permuted", prefilter=F.mask_by_id(mask, M.build("l2", 200, ids="permuted")[4]))


@pytest.mark.parametrize("scale", [1e-3, 1e4])
@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_magnitude_and_degenerate_rows(metric, scale):
    check(metric, 36, scale=scale, odd=True)


def test_chunk_crossing():
    check("l2", 36, nq=M.QCHUNK + 1)


def test_bound_is_not_vacuous():
    """L2, d = 200: the main pass queues fewer than half of the N_all = 154,493 (query, row) cells of the probed partitions.  With no
    bound at all it queues every one of them (no queue overflows: 1,070 rows a query at the most), so an answer that is right says nothing
    about the bound.  Computed on the CPU from the specification's distances: 5,529 cells (3.6 % of N_all) lie at or under their query's
    exact k-th distance within its nearest partition -- the tightest bound this pass can give; the five queries whose nearest partition
    holds 0 or 1 rows have none and count with all their cells --, and the filter's margin and the surrogate's choice of rows add to that."""
    import oracle
    _, x, q, cent, _ = M.build("l2", 200)
    _, _, offs, _, probes = V._prepare(oracle, x, cent, q, M.NPROBES, "l2")
    n_all = int(np.diff(offs.astype(np.int64))[probes].sum())
    queued = check("l2", 200)
    print("queued", queued, "of", n_all)
    assert 0 < queued < n_all / 2
