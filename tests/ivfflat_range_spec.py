"""Shared by tests/test_ivfflat_range_spec.py (CPU) and the GPU tests of distance ranges and adaptive probing
(tests/test_zz_gpu_ivfflat_range.py, tests/test_zz_gpu_adaptive_probing.py): the CPU specification of an IVF_FLAT search under a
distance range, of adaptive probing above any IVF specification, and the fixtures of those files.

The specification (lance-index flat/index.rs:91-149; lance io/exec/knn.rs:714-860):
    range      inside every probed partition only rows with lower <= d < upper are offered to the partition's k-heap
               (oracle.heap_topk(..., lower=, upper=)); d is the metric's own distance; an open end is f32::MIN / f32::MAX; the
               comparison is OrderedFloat's total order, so a NaN distance is above every bound
    prefilter  unselected rows are skipped ahead of the heap, in storage order (as tests/sq_spec.py:97-101)
    adaptive   every query searches min_np partitions; while a query holds fewer than k rows and partitions are left, it is searched
               again with min(max_np, max(2 n, n + 1)) partitions; late_search's shortcut: when the prefilter selects at most k rows
               (and there is neither a refine factor nor a range) a query that has not found them all gets the rest at +inf, in
               ascending row id order, and stops"""
import numpy as np

f32 = np.float32
UNSET = np.uint64(np.iinfo(np.uint64).max)


def _prepare(oracle, x, centroids, q, nprobes, metric):
    """oracle.ivfflat_search's set-up: -> (rows as scored, queries as scored, partition offsets, storage order, probes [nq][nprobes])"""
    if np.asarray(x).dtype == np.float16:
        x = np.ascontiguousarray(x, np.float16); centroids = np.ascontiguousarray(centroids, np.float16)
        q = np.ascontiguousarray(q, np.float16).reshape(-1, x.shape[1])
    else:
        x = np.ascontiguousarray(x, f32); centroids = np.ascontiguousarray(centroids, f32)
        q = np.ascontiguousarray(q, f32).reshape(-1, x.shape[1])
    coarse = metric
    if metric == "cosine":
        x = oracle.normalize(x); q = oracle.normalize(q); coarse = "l2"
    part, _ = oracle.assign(x, centroids, coarse)
    offs, perm = oracle.partition_layout(part, centroids.shape[0])
    probes, _ = oracle.find_partitions(q, centroids, nprobes, coarse)
    return x, q, offs, perm, probes


def _partition_rows(offs, perm, p, rid, allow):
    rows = perm[int(offs[p]):int(offs[p + 1])]
    if allow is not None and len(rows):
        r = rid[rows]
        ok = r < allow.size
        ok[ok] = allow[r[ok]]
        rows = rows[ok]
    return rows


def search(oracle, x, centroids, q, k, nprobes, metric, lower, upper, row_ids=None, prefilter=None):
    """IVF_FLAT under [lower, upper) (either may be None; both None: no range at all) -> (ids u64 [nq][k], dists f32 [nq][k])"""
    xs, qs, offs, perm, probes = _prepare(oracle, x, centroids, q, nprobes, metric)
    rid = np.arange(xs.shape[0], dtype=np.uint64) if row_ids is None else np.asarray(row_ids, np.uint64)
    allow = None if prefilter is None else np.asarray(prefilter, bool)
    out_i = np.full((qs.shape[0], k), UNSET, np.uint64)
    out_d = np.full((qs.shape[0], k), np.inf, f32)
    for qi in range(qs.shape[0]):
        ci, cd = [], []
        for p in probes[qi]:
            rows = _partition_rows(offs, perm, p, rid, allow)
            if len(rows) == 0:
                continue
            d = oracle.distance_batch(metric, qs[qi], xs[rows])
            hi, hd = oracle.heap_topk(d, rid[rows], k, lower=lower, upper=upper)
            ci.append(hi); cd.append(hd)
        if ci:
            si, sd = oracle.sort_fetch(np.concatenate(ci), np.concatenate(cd), k)
            out_i[qi, :len(si)] = si; out_d[qi, :len(sd)] = sd
    return out_i, out_d


def post_filtered(oracle, x, centroids, q, k, nprobes, metric, lower, upper, row_ids=None, prefilter=None):
    """the WRONG answer: the k nearest first, the range applied to them afterwards"""
    ids, dists = search(oracle, x, centroids, q, k, nprobes, metric, None, None, row_ids=row_ids, prefilter=prefilter)
    lo = f32(np.finfo(f32).min if lower is None else lower)
    hi = f32(np.finfo(f32).max if upper is None else upper)
    out_i = np.full_like(ids, UNSET)
    out_d = np.full_like(dists, np.inf)
    for qi in range(ids.shape[0]):
        ok = (ids[qi] != UNSET) & (dists[qi] >= lo) & (dists[qi] < hi)
        out_i[qi, :ok.sum()] = ids[qi][ok]; out_d[qi, :ok.sum()] = dists[qi][ok]
    return out_i, out_d


def probed_distances(oracle, x, centroids, q, nprobes, metric):
    """per query the distances of every row of its probed partitions (one array per query), in probe then storage order"""
    xs, qs, offs, perm, probes = _prepare(oracle, x, centroids, q, nprobes, metric)
    out = []
    for qi in range(qs.shape[0]):
        rows = np.concatenate([perm[int(offs[p]):int(offs[p + 1])] for p in probes[qi]])
        out.append(oracle.distance_batch(metric, qs[qi], xs[rows]) if len(rows) else np.zeros(0, f32))
    return out


def partition_sizes(oracle, x, centroids, metric):
    xs, _, offs, _, _ = _prepare(oracle, x, centroids, np.asarray(x)[:1], 1, metric)
    return np.diff(offs.astype(np.int64))


def found(ids):
    """rows found per query"""
    return (np.asarray(ids) != UNSET).sum(axis=1)


def adaptive(search_fn, nq, k, min_np, max_np, nlist, selected_ids=None):
    """The doubling loop over any specification.  search_fn(query indices, nprobes) -> (ids u64 [len][k], dists f32 [len][k]) of
    those queries.  max_np None: all partitions.  selected_ids: the row ids a prefilter selects WHEN the shortcut applies (no
    refine factor, no range), else None.  -> (ids, dists, partitions searched per query [nq])"""
    max_np = nlist if max_np is None else max_np
    max_np = max(min(max_np, nlist), min(min_np, nlist))
    min_np = min(min_np, max_np)
    everyone = np.arange(nq)
    ids, dists = (np.array(a) for a in search_fn(everyone, min_np))
    used = np.full(nq, min_np, np.int64)
    if max_np <= min_np:
        return ids, dists, used
    if selected_ids is not None and len(selected_ids) <= k:
        sel = np.sort(np.asarray(selected_ids, np.uint64))
        for qi in range(nq):
            have = ids[qi][ids[qi] != UNSET]
            if len(have) < k and len(have) < len(sel):
                rest = np.setdiff1d(sel, have)
                ids[qi, len(have):len(have) + len(rest)] = rest
                dists[qi, len(have):len(have) + len(rest)] = np.inf
        return ids, dists, used
    npb = min_np
    while npb < max_np:
        starved = np.flatnonzero(found(ids) < k)
        if starved.size == 0:
            break
        npb = min(max_np, max(2 * npb, npb + 1))
        si, sd = search_fn(starved, npb)
        ids[starved] = si; dists[starved] = sd
        used[starved] = npb
    return ids, dists, used


# ---- fixtures -------------------------------------------------------------------------------------------------------------------
NLIST, K, NPROBES = 8, 10, 3
RANGES = [(60.0, 90.0), (40.0, 64.0), (0.0, 1.0), (70.0, 70.0), (None, 60.0), (80.0, None)]      # (70, 70): lower == upper


def base_fixture():
    """3000 x 16 integers in -3 .. 3 and 64 queries drawn the same way; 8 centroids that are rows of x.  Every L2 and dot distance
    is an exact integer, so rows sit exactly on integer bounds and tie in large numbers.  -> (x, q, centroids) f32"""
    rng = np.random.default_rng(1)
    x = rng.integers(-3, 4, (3000, 16)).astype(f32)
    q = rng.integers(-3, 4, (64, 16)).astype(f32)
    cent = np.ascontiguousarray(x[rng.choice(3000, NLIST, replace=False)])
    return x, q, cent


def padded(x, q, cent, d=20):
    """the same rows with zero columns appended: same L2 distances, a dimension no fixed-dimension kernel takes"""
    pad = lambda a: np.ascontiguousarray(np.pad(a, ((0, 0), (0, d - a.shape[1]))))
    return pad(x), pad(q), pad(cent)


def sparse_prefilter(n=3000, count=30, seed=6):
    """a prefilter selecting `count` of n rows"""
    allow = np.zeros(n, bool)
    allow[np.random.default_rng(seed).choice(n, count, replace=False)] = True
    return allow


STARVING_RANGE = (30.0, 45.0)      # L2 on the base fixture: so few rows that many queries never find k of them
NAN_ROW = 7


def nan_fixture():
    """dot: 300 small-integer rows and one FINITE row (NAN_ROW) whose dot product with the query is inf - inf = NaN (the two
    products land in different lane accumulators).  Both centroids are zero where that row is huge, so its assignment is
    ordinary.  -> (x [300][16], q [1][16], centroids [2][16]) f32"""
    rng = np.random.default_rng(4)
    x = rng.integers(-3, 4, (300, 16)).astype(f32)
    x[NAN_ROW] = 0.0
    x[NAN_ROW, :2] = [3e38, -3e38]
    q = rng.integers(-3, 4, (1, 16)).astype(f32)
    q[0, :2] = 2e19
    cent = x[[0, 1]].copy()
    cent[:, :2] = 0.0
    return x, q, np.ascontiguousarray(cent)
