"""Shared by tests/test_multivec_ann_spec.py (CPU), tests/test_multivec_ann_kernels_cpu.py (CPU) and tests/test_zz_gpu_multivec_ann.py
(GPU): the CPU specification of the multivector ANN search -- per-query-vector candidate lists joined by row id and scored with
XTR-style imputation (Scanner::multivec_ann, scanner.rs:3471-3552; MultivectorScoringExec, knn.rs:1132-1329) -- and the fixtures.

A query of nqv vectors has nqv candidate lists; list j holds at most keff pairs (row id, distance) in (distance, row id) order: the
IVF_PQ search of the index over the FLATTENED vectors (row ids repeated per vector) with k = keff = k * overfetch.  A list is passed as
a row of ids [nqv][keff] uint64 / dists [nqv][keff] float32, valid entries first, then id 2^64 - 1 / +inf.  Every operation below is one
f32 rounding:
    min_sim_j = 1 - (last dist of list j, before dedup), 0 for an empty list            (knn.rs:1226-1230)
    sim_j(r)  = 1 - dist of r's FIRST entry in list j                                    (knn.rs:1235-1244)
    missed_j  = ((0 + min_sim_0) + min_sim_1) + ... + min_sim_{j-1}
    s(r)      = sim_{j0}(r) + missed_{j0}, j0 = r's first list; then for j = j0 + 1 .. nqv - 1: s = s + (sim_j(r) if r in list j else min_sim_j)
    distance  = f32(nqv) - s                                                             (knn.rs:1260-1298)
    answer    = the k_out = k * refine_factor smallest by (distance in total_cmp order, row id)
The lists are taken in query-vector order 0 .. nqv - 1 (the reference takes them in stream-arrival order, which is not deterministic
there; this order is one it can produce).  reference_loop is the reference's HashMap loop transcribed literally, for the cross-check."""
import numpy as np

import flat_order_spec as S
import multivec_spec as M

f32 = np.float32
U64_MAX = np.uint64(0xFFFFFFFFFFFFFFFF)
MAX_KEFF = 4096          # LANCE_HIP_MULTIVEC_ANN_MAX_KEFF
MAX_K_OUT = 1024         # LANCE_HIP_MULTIVEC_ANN_MAX_K_OUT
MAX_NQV = 256            # LANCE_HIP_MULTIVEC_MAX_QUERY_VECTORS


# ---- the specification --------------------------------------------------------------------------------------------------------
def reduce_list(ids, dists):
    """one list -> (min_sim, row ids of the first occurrences in list order, their sims)"""
    ids = np.asarray(ids, np.uint64)
    dists = np.asarray(dists, f32)
    n = int((ids != U64_MAX).sum())
    assert (ids[:n] != U64_MAX).all(), "valid entries come first"
    if n == 0:
        return f32(0), np.empty(0, np.uint64), np.empty(0, f32)
    min_sim = f32(1) - dists[n - 1]
    _, first = np.unique(ids[:n], return_index=True)
    first.sort()
    return min_sim, ids[first], (f32(1) - dists[first]).astype(f32)


def scores(ids, dists, order=None):
    """the join over the lists ids / dists [nqv][keff], taken in `order` (default 0 .. nqv - 1) -> (row ids ascending, distances)"""
    nqv = len(ids)
    lists = [reduce_list(ids[j], dists[j]) for j in (range(nqv) if order is None else order)]
    rows = np.unique(np.concatenate([l[1] for l in lists])) if lists else np.empty(0, np.uint64)
    s = np.zeros(rows.size, f32)
    started = np.zeros(rows.size, bool)
    missed = f32(0)
    for min_sim, rid, sim in lists:
        at = np.searchsorted(rows, rid)
        present = np.zeros(rows.size, bool)
        present[at] = True
        val = np.full(rows.size, min_sim, f32)
        val[at] = sim
        first = present & ~started
        s = np.where(first, val + missed, np.where(started, s + val, s)).astype(f32)
        started |= present
        missed = f32(missed + min_sim)
    assert s.dtype == f32 and started.all()
    return rows, (f32(nqv) - s).astype(f32)


def reference_loop(ids, dists, order=None):
    """knn.rs:1218-1298 line by line: `results` / `query_results` as dicts, missed_sim_sum -> (row ids ascending, distances)"""
    nqv = len(ids)
    results = {}
    missed_sim_sum = f32(0)
    for j in (range(nqv) if order is None else order):
        row_ids, ds = np.asarray(ids[j], np.uint64), np.asarray(dists[j], f32)
        n = int((row_ids != U64_MAX).sum())
        min_sim = f32(1) - ds[n - 1] if n else f32(0)
        visited, query_results = set(), {}
        for r, d in zip(row_ids[:n].tolist(), ds[:n]):
            if r in visited:
                continue
            visited.add(r)
            query_results[r] = f32(1) - d
        for r in results:
            results[r] = f32(results[r] + (query_results[r] if r in query_results else min_sim))
        for r, sim in query_results.items():
            if r not in results:
                results[r] = f32(sim + missed_sim_sum)
        missed_sim_sum = f32(missed_sim_sum + min_sim)
    rows = np.array(sorted(results), np.uint64)
    return rows, np.array([f32(nqv) - results[int(r)] for r in rows], f32)


def topk(ids, dists, k_out):
    """the k_out best joined rows by (distance in total order, row id); padded with id 2^64 - 1 / +inf"""
    rows, d = scores(ids, dists)
    return M.topk(d, k_out, rows)


def scores_pairwise(ids, dists):
    """a WRONG order: the same per-list terms of every row added as a tree"""
    nqv = len(ids)
    lists = [reduce_list(ids[j], dists[j]) for j in range(nqv)]
    rows = np.unique(np.concatenate([l[1] for l in lists]))
    terms = np.empty((nqv, rows.size), f32)
    for j, (min_sim, rid, sim) in enumerate(lists):
        terms[j] = min_sim
        terms[j, np.searchsorted(rows, rid)] = sim
    return rows, (f32(nqv) - M.sum_pairwise(terms)).astype(f32)


# ---- synthetic lists ----------------------------------------------------------------------------------------------------------
def pad_lists(lists, keff):
    """[(ids, dists)] of at most keff entries each -> ids [nqv][keff] uint64, dists [nqv][keff] float32 with the library's padding"""
    ids = np.full((len(lists), keff), U64_MAX, np.uint64)
    dists = np.full((len(lists), keff), np.inf, f32)
    for j, (i, d) in enumerate(lists):
        ids[j, :len(i)] = i
        dists[j, :len(d)] = d
    return ids, dists


def random_lists(nqv, keff, n_rows, seed, id_base=0, id_step=1, short=(), empty=(), dup=0.3, scale=1.2):
    """nqv lists over n_rows distinct row ids (id_base + id_step * row): each list draws its entries with repetition (a row may occur
    several times in a list, the share steered by `dup`), inexact distances in about [0, scale] sorted by (distance, row id); the lists
    named in `short` hold about a third of keff entries, those in `empty` none"""
    rng = np.random.default_rng(seed)
    out = []
    for j in range(nqv):
        n = 0 if j in empty else max(1, keff // 3) if j in short else keff
        pool = rng.choice(n_rows, size=max(1, int(n_rows * (1 - dup))), replace=False)
        rows = pool[rng.integers(0, pool.size, n)]
        ids = (np.uint64(id_base) + rows.astype(np.uint64) * np.uint64(id_step)).astype(np.uint64)
        d = (rng.random(n) * scale).astype(f32) * f32(1.0000001) + f32(1e-3) * rng.standard_normal(n).astype(f32)
        o = np.lexsort((ids, S.keys(d)))
        out.append((ids[o], d[o]))
    return pad_lists(out, keff)


def order_fixture():
    """32 lists x 100 candidates over 400 rows, one empty list, row ids above 2^40, small distances (the sum of the sims is near 29, the
    distance near 3: a last-place difference in the sum survives the final subtraction): reversing the list order or summing as a tree
    changes the bits of many rows (asserted in tests/test_multivec_ann_spec.py)"""
    return random_lists(32, 100, 400, seed=11, id_base=(1 << 40) + 7, id_step=3, empty=(9,), dup=0.2, scale=0.12)


# ---- end to end: a multivector column, its flattened IVF_PQ index in the oracle --------------------------------------------------
def unit_rows(n, d, seed, centers=None, spread=0.35):
    """rows around `centers` (or plain gaussian): real-valued, no two equal"""
    rng = np.random.default_rng(seed)
    if centers is None:
        return rng.standard_normal((n, d)).astype(f32)
    return (centers[rng.integers(0, len(centers), n)] + spread * rng.standard_normal((n, d))).astype(f32)


def small_column(kind="f32", n_rows=600, lo=4, hi=12, d=32, seed=5, clustered=False):
    """-> (values [total][d], offsets [n_rows + 1], flat_rid [total] uint64 = the row index repeated per vector)"""
    lens = M.lengths(n_rows, lo, hi, seed)
    off = M.offsets_of(lens)
    total = int(off[-1])
    if clustered:
        rng = np.random.default_rng(seed + 1)
        topics = rng.standard_normal((40, d)).astype(f32)
        row_topic = rng.integers(0, 40, n_rows)
        values = (np.repeat(topics[row_topic], lens, axis=0) + 0.5 * rng.standard_normal((total, d))).astype(f32)
    else:
        values = unit_rows(total, d, seed + 2)
    if kind == "f16":
        values = values.astype(np.float16)
    return values, off, np.repeat(np.arange(n_rows, dtype=np.uint64), lens)


def train_model(oracle, values, nlist, m, seed=3):
    """IVF centroids and a PQ codebook for a cosine index over `values`, trained by the oracle (a few iterations: a model, not a good one)"""
    x = np.ascontiguousarray(values, f32)
    xs = oracle.normalize(x)
    cent, _, _, _ = oracle.kmeans_train(xs, nlist, max_iters=6, seed=seed)
    part, _ = oracle.assign(xs, cent)
    res = oracle.residual(xs, cent, np.where(part == oracle.NONE, 0, part))
    cb, _ = oracle.pq_train(res, m, max_iters=6, seed=seed + 1)
    if values.dtype == np.float16:
        cent, cb = cent.astype(np.float16), cb.astype(np.float16)
    return cent, cb


def candidate_lists(oidx, q, keff, nprobes, prefilter=None):
    """the oracle's search of the flattened index with k = keff, no refine -> ids [nqv][keff], dists [nqv][keff]"""
    return oidx.search(np.ascontiguousarray(q), keff, nprobes, prefilter=prefilter)


def ann_spec(oracle, oidx, values, offsets, q, k, nprobes, overfetch=10, refine_factor=None, prefilter=None):
    """IvfPqMultivectorIndex.nearest for one query: the candidate lists, the join, and with a refine factor the exact multivector
    distance (multivec_spec) of the k * refine_factor joined rows, best k -> (ids [k] uint64, dists [k])"""
    ci, cd = candidate_lists(oidx, q, k * overfetch, nprobes, prefilter)
    if refine_factor is None:
        return topk(ci, cd, k)
    cand, _ = topk(ci, cd, k * refine_factor)
    cand = cand[cand != U64_MAX]
    if cand.size == 0:
        return M.topk(np.empty(0, f32), k, np.empty(0, np.uint64))
    offsets = np.asarray(offsets, np.int64)
    rows = cand.astype(np.int64)
    lens = offsets[rows + 1] - offsets[rows]
    sub = np.concatenate([np.arange(offsets[r], offsets[r + 1]) for r in rows])
    dist = M.distances(oracle, values[sub], M.offsets_of(lens), q, "cosine")
    return M.topk(dist, k, cand)
