"""The CPU specification of IVF_SQ / IVF_RQ searches with a refine_factor (tests/refine_spec.py): what re-ranking is worth (recall pins),
that full coverage is the flat answer, that refine_factor = 1 re-scores without re-selecting, and the ordered partitions at any k that the
kernel tests (tests/test_wide_cand_kernels_cpu.py, tests/test_zz_gpu_refine_sqrq.py) run."""
import functools

import numpy as np
import pytest

import refine_spec as F
import rq_spec as R
import sq_spec as S

f32 = np.float32


def same_bits(a, b):
    return a.shape == b.shape and (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


# ---- (a) what re-ranking is worth --------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def recall_setup():
    x, q = R.clustered(4000, 64, 100, 3)
    cent = np.ascontiguousarray(x[np.random.default_rng(1).choice(4000, 16, replace=False)])
    return x, q, cent, R.rotation(64, 7)


# recall@10 at nprobes 4 of 16: (unrefined, refine_factor 5, 10, 50).  Under dot the last value is what four probed partitions miss.
RECALL = {"l2": (0.2600, 0.6090, 0.7810, 1.0000), "dot": (0.5530, 0.8890, 0.9400, 0.9720)}


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_recall_pins(oracle, metric):
    x, q, cent, P = recall_setup()
    part, codes, add, scale = R.build(oracle, x, cent, P, metric)
    truth, _ = oracle.flat_knn(x, q, 10, metric)
    ids, _ = R.search(oracle, codes, add, scale, part, cent, P, q, 10, 4, metric)
    got = [F.recall(ids, truth)]
    for rf in (5, 10, 50):
        ids, _ = F.rq_search_refine(oracle, codes, add, scale, part, cent, P, q, 10, rf, 4, metric, x)
        got.append(F.recall(ids, truth))
    assert [round(v, 4) for v in got] == list(RECALL[metric])


# ---- (b) full coverage equals flat ---------------------------------------------------------------------------------------------------
def finite_flat(oracle, x, q, k, metric, rid):
    ok = np.isfinite(np.asarray(x, np.float64)).all(axis=1)
    return oracle.flat_knn(np.ascontiguousarray(x[ok]), q, k, metric, row_ids=rid[ok])


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_rq_full_coverage_is_flat(oracle, metric):
    n, k, rf, nlist = 600, 10, 60, 5
    x, q = R.clustered(n, 32, 9, seed=21)
    x[17, 3] = np.inf                                            # a row outside the index: not a candidate, not in the flat answer
    cent = np.ascontiguousarray(x[[1, 100, 200, 300, 400]])
    P = R.rotation(32, 2)
    rid = np.random.default_rng(5).permutation(n).astype(np.uint64)
    part, codes, add, scale = R.build(oracle, x, cent, P, metric)
    gi, gd = F.rq_search_refine(oracle, codes, add, scale, part, cent, P, q, k, rf, nlist, metric, F.raw_by_row_id(x, rid), row_ids=rid)
    oi, od = finite_flat(oracle, x, q, k, metric, rid)
    assert (gi == oi).all() and same_bits(gd, od)


@pytest.mark.parametrize("kind", ["f32", "f16"])
@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_sq_full_coverage_is_flat(oracle, metric, kind):
    n, k, rf, nlist = 600, 10, 60, 4
    x, q = S.gaussian(n, 32, 9, seed=22, kind=kind)
    cent = S.centroids_with_gaps(oracle.normalize(x) if metric == "cosine" else x, nlist, seed=3)
    rid = np.random.default_rng(6).permutation(n).astype(np.uint64)
    xs, part = S.prepare_rows(oracle, x, cent, metric)
    b = S.bounds(xs[:64])
    gi, gd = F.sq_search_refine(oracle, S.encode(xs, *b), part, cent, q, k, rf, nlist, metric, *b, F.raw_by_row_id(x, rid), row_ids=rid)
    oi, od = finite_flat(oracle, x, q, k, metric, rid)           # the ORIGINAL rows and query, also under cosine
    assert (gi == oi).all() and same_bits(gd, od)


# ---- (c) refine_factor = 1 -------------------------------------------------------------------------------------------------------------
def test_refine_factor_one_rescored_not_reselected(oracle):
    x, q = R.clustered(900, 32, 20, seed=4)
    cent = np.ascontiguousarray(x[[5, 105, 205, 305, 405, 505]])
    P = R.rotation(32, 9)
    for metric in ("l2", "dot"):
        part, codes, add, scale = R.build(oracle, x, cent, P, metric)
        ui, ud = R.search(oracle, codes, add, scale, part, cent, P, q, 10, 2, metric)
        ri, rd = F.rq_search_refine(oracle, codes, add, scale, part, cent, P, q, 10, 1, 2, metric, x)
        assert (np.sort(ui, axis=1) == np.sort(ri, axis=1)).all()
        assert not same_bits(ud, rd)                             # the estimate is not the distance
        for qi in range(len(q)):                                 # exact distances, in (dist, rowid) order
            ei, ed = oracle.flat_knn(np.ascontiguousarray(x[ri[qi].astype(np.int64)]), q[qi:qi + 1], 10, metric, row_ids=ri[qi])
            assert (ei[0] == ri[qi]).all() and same_bits(ed[0], rd[qi])
    xs, part = S.prepare_rows(oracle, x, cent, "cosine")
    b = S.bounds(xs[:64])
    codes = S.encode(xs, *b)
    ui, _ = S.search(oracle, codes, part, cent, q, 10, 2, "cosine", *b)
    ri, rd = F.sq_search_refine(oracle, codes, part, cent, q, 10, 1, 2, "cosine", *b, x)
    assert (np.sort(ui, axis=1) == np.sort(ri, axis=1)).all()


def test_missing_slots():
    import oracle
    x, q = R.clustered(50, 16, 2, seed=1)
    cand = np.full((2, 8), F.UNSET, np.uint64)
    cand[0, :3] = [7, 3, 9]
    ids, dists = F.refine(oracle, cand, x, q, 5, "l2")
    assert sorted(ids[0, :3].tolist()) == [3, 7, 9] and (ids[0, 3:] == F.UNSET).all() and np.isinf(dists[0, 3:]).all()
    assert (ids[1] == F.UNSET).all() and np.isinf(dists[1]).all()


# ---- ordered partitions at any k -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rq", "sq"])
@pytest.mark.parametrize("order", F.ORDERS)
@pytest.mark.parametrize("k,cap,N", [(129, 1024, 1568), (768, 1024, 1569), (768, 1024, 1599), (768, 4096, 4671)])
def test_ordered_partitions(oracle, kind, order, k, cap, N):
    """N % 32 = 0, 1, 31 (the IVF_RQ remainder branch) past the buffer plus two chunks; the properties of every order are asserted by
    the fixture itself on the keys of the final layout.  The answer of the spec search depends on the order only through ties."""
    assert N > cap + 2 * F.CHUNK and N % 32 in (0, 1, 31)
    f = F.ordered_partition(oracle, kind, order, "l2", k, cap, N)
    assert f["cut_tie"] == (order == "tie_cut") or kind == "sq"          # (integer sums may tie by themselves)
    assert f["cut_tie"] or order != "tie_cut"
    assert len(f["x"]) == N + 40 and len(f["keys"]) == N
    if order == "tie_cut":                                               # what (dist, position) order would keep is not what the heap keeps
        rid = np.arange(len(f["x"]), dtype=np.uint64)
        if kind == "rq":
            part, codes, add, scale = R.build(oracle, f["x"], f["cent"], f["P"], "l2")
            ids, _ = R.search(oracle, codes, add, scale, part, f["cent"], f["P"], f["q"][None], k, 1, "l2")
        else:
            _, part = S.prepare_rows(oracle, f["x"], f["cent"], "l2")
            ids, _ = S.search(oracle, S.encode(f["x"], *f["bounds"]), part, f["cent"], f["q"][None], k, 1, "l2", *f["bounds"])
        by_position = rid[:N][np.lexsort((rid[:N], f["keys"]))[:k]]
        assert set(ids[0].tolist()) != set(by_position.tolist())
