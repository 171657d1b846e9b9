"""Shared by tests/test_knn_combined_spec.py (CPU), tests/test_knn_combined_kernel_cpu.py (CPU) and tests/test_zz_gpu_knn_combined.py (GPU):
the CPU specification of the search over a column whose index is behind its rows -- lance_amd.VectorColumn.nearest and
the stage lance_hip_take_flat_knn --, in numpy on the oracle's pieces, and three wrong variants a fixture must tell it from.

The plan (Scanner::nearest, rust/lance/src/dataset/scanner.rs:2847-3030, 3336-3468; fast_search = false):
    1. use_index = False or no delta     flat_knn over the column with prefilter and range
    2. ANN over every delta              keff = k * (refine_factor or 1); each delta's own search takes the prefilter and, where the index
                                         type answers ranges, the bounds (on the index's distances, inside the partitions);
                                         SortExec(_distance, _rowid).fetch(keff) over the union of the lists
    3. refine_factor                     take + flat_knn over the keff ids: exact distances, the bounds on them, fetch k
    4. fast_search or no unindexed rows  done
    5. knn_combined                      flat_knn(k) over the unindexed fragments (row ids, prefilter, bounds); UnionExec with the list so
                                         far (NO de-duplication); flat_knn over the union: every distance recomputed exactly, the bounds on
                                         those, SortExec(_distance, _rowid).fetch(k)
take_flat_knn is steps 3 and 5's common stage.  Exact distances are oracle.flat_knn's bits; ranges are tests/flat_range_spec.py's (the
total order on f32, an absent bound is not tested)."""
import numpy as np

import flat_order_spec as FO
import flat_range_spec as FR
import ivfflat_range_spec as IR
import rq_spec as RQ
import sq_spec as SQ

f32 = np.float32
UNSET = np.uint64(0xFFFFFFFFFFFFFFFF)


# ---- the stage ---------------------------------------------------------------------------------------------------------------------
def _score(oracle, x, qrow, ids, metric):
    """(ids, exact distances) of the candidate rows `ids` (duplicates kept) in flat_knn's order"""
    if ids.size == 0:
        return ids, np.empty(0, f32)
    if int(ids.max()) >= len(x):
        raise ValueError(f"a candidate row id is >= n_rows = {len(x)}")
    ai, ad = FR.every_row(oracle, x[ids.astype(np.int64)], qrow, metric, row_ids=ids)
    return ai[0], ad[0]


def take_flat_knn(oracle, x, q, ids_a, k, metric, ids_b=None, dists_b=None, lower=None, upper=None, dists_a=None, bounds=True, dedup=False):
    """The model of lance_hip_take_flat_knn: ids_a [nq][ca] / ids_b [nq][cb] uint64 (UNSET = an empty slot); dists_b: list B's distances
    taken as they are (None: scored like list A) -> (ids [nq][k] uint64, distances [nq][k]); missing slots UNSET / +inf.
    The arguments behind `upper` make the WRONG variants: dists_a keeps list A's given distances instead of scoring its rows;
    bounds=False does not test the bounds here; dedup=True drops the later copies of a row id."""
    x = np.asarray(x)
    q = np.asarray(q).astype(x.dtype).reshape(-1, x.shape[1])
    nq = q.shape[0]
    ids_a = np.asarray(ids_a).astype(np.uint64).reshape(nq, -1)
    out_i = np.full((nq, k), UNSET, np.uint64)
    out_d = np.full((nq, k), np.inf, f32)
    for i in range(nq):
        va = ids_a[i] != UNSET
        if dists_a is None:
            ci, cd = _score(oracle, x, q[i], ids_a[i][va], metric)
        else:
            ci, cd = ids_a[i][va], np.asarray(dists_a, f32).reshape(nq, -1)[i][va]
        if ids_b is not None:
            b = np.asarray(ids_b).astype(np.uint64).reshape(nq, -1)[i]
            vb = b != UNSET
            if dists_b is None:
                bi, bd = _score(oracle, x, q[i], b[vb], metric)
            else:
                if b[vb].size and int(b[vb].max()) >= len(x):
                    raise ValueError(f"a candidate row id is >= n_rows = {len(x)}")
                bi, bd = b[vb], np.asarray(dists_b, f32).reshape(nq, -1)[i][vb]
            ci, cd = np.concatenate([ci, bi]), np.concatenate([cd, bd])
        if dedup and ci.size:
            _, first = np.unique(ci, return_index=True)
            first.sort()
            ci, cd = ci[first], cd[first]
        if bounds:
            ok = FR.in_range(cd, lower, upper)
            ci, cd = ci[ok], cd[ok]
        o = np.lexsort((ci, FO.keys(cd)))[:k]
        out_i[i, :o.size] = ci[o]
        out_d[i, :o.size] = cd[o]
    return out_i, out_d


def join(lists, keff):
    """SortExec(_distance, _rowid).fetch(keff) over the union of the deltas' lists"""
    if len(lists) == 1:
        return lists[0]
    ids, dists = np.concatenate([l[0] for l in lists], 1), np.concatenate([l[1] for l in lists], 1)
    nq = ids.shape[0]
    out_i = np.full((nq, keff), UNSET, np.uint64)
    out_d = np.full((nq, keff), np.inf, f32)
    for i in range(nq):
        v = ids[i] != UNSET
        ci, cd = ids[i][v], dists[i][v]
        o = np.lexsort((ci, FO.keys(cd)))[:keff]
        out_i[i, :o.size] = ci[o]
        out_d[i, :o.size] = cd[o]
    return out_i, out_d


# ---- the column ----------------------------------------------------------------------------------------------------------------------
class Delta:
    """one delta index of the specification: the fragments it is recorded to cover and its own search,
    search(q, keff, nprobes, prefilter, lower, upper) -> (ids uint64 [nq][keff], distances)"""

    def __init__(self, kind, fragments, rows, search):
        self.kind, self.fragments, self.rows, self.search = kind, frozenset(fragments), rows, search


class Column:
    def __init__(self, x, metric, fragment_sizes=None, deltas=()):
        self.x, self.metric = np.asarray(x), metric
        sizes = [len(self.x)] if fragment_sizes is None else list(fragment_sizes)
        self.offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self.deltas = list(deltas)

    def rows_of(self, fragments):
        parts = [np.arange(self.offsets[f], self.offsets[f + 1], dtype=np.uint64) for f in sorted(fragments)]
        return np.concatenate(parts) if parts else np.empty(0, np.uint64)

    def tail_runs(self):
        covered = set()
        for dl in self.deltas:
            covered |= dl.fragments
        frags = [f for f in range(self.offsets.size - 1) if f not in covered]
        runs, i = [], 0
        while i < len(frags):
            j = i
            while j + 1 < len(frags) and frags[j + 1] == frags[j] + 1:
                j += 1
            r0, r1 = int(self.offsets[frags[i]]), int(self.offsets[frags[j] + 1])
            if r1 > r0:
                runs.append((r0, r1))
            i = j + 1
        return runs


def _no_range(kind, lower, upper):
    if lower is not None or upper is not None:
        raise NotImplementedError(f"{kind}: distance_range is not supported by this engine")


def pq_delta(oracle, col, fragments, cent, codebook, nbits=8, rows=None):
    rows = col.rows_of(fragments) if rows is None else np.asarray(rows, np.uint64)
    idx = oracle.build_index(col.x[rows.astype(np.int64)], cent, codebook, col.metric, row_ids=rows, nbits=nbits)
    return Delta("IVF_PQ", fragments, rows,
                 lambda q, keff, nprobes, pf, lo, hi: idx.search(q, keff, nprobes, prefilter=pf, lower=lo, upper=hi))


def flat_delta(oracle, col, fragments, cent, rows=None):
    rows = col.rows_of(fragments) if rows is None else np.asarray(rows, np.uint64)
    xs = col.x[rows.astype(np.int64)]
    return Delta("IVF_FLAT", fragments, rows,
                 lambda q, keff, nprobes, pf, lo, hi: IR.search(oracle, xs, cent, q, keff, nprobes, col.metric, lo, hi, row_ids=rows, prefilter=pf))


def sq_delta(oracle, col, fragments, cent, bounds, rows=None):
    rows = col.rows_of(fragments) if rows is None else np.asarray(rows, np.uint64)
    xs, part = SQ.prepare_rows(oracle, col.x[rows.astype(np.int64)], cent, col.metric)
    codes = SQ.encode(xs, *bounds)

    def search(q, keff, nprobes, pf, lo, hi):
        _no_range("IVF_SQ", lo, hi)
        return SQ.search(oracle, codes, part, cent, q, keff, nprobes, col.metric, *bounds, row_ids=rows, prefilter=pf)
    return Delta("IVF_SQ", fragments, rows, search)


def rq_delta(oracle, col, fragments, cent, P, rows=None):
    rows = col.rows_of(fragments) if rows is None else np.asarray(rows, np.uint64)
    part, codes, add, scale = RQ.build(oracle, np.asarray(col.x[rows.astype(np.int64)], f32), cent, P, col.metric)

    def search(q, keff, nprobes, pf, lo, hi):
        _no_range("IVF_RQ", lo, hi)
        return RQ.search(oracle, codes, add, scale, part, cent, P, q, keff, nprobes, col.metric, row_ids=rows, prefilter=pf)
    return Delta("IVF_RQ", fragments, rows, search)


def _selected(rows, prefilter):
    if prefilter is None:
        return rows
    pf = np.asarray(prefilter, bool)
    ok = rows < pf.size
    ok[ok] = pf[rows[ok].astype(np.int64)]
    return rows[ok]


def tail_lists(oracle, col, q, k, prefilter, lower, upper):
    """flat_knn(k) over every contiguous run of unindexed fragments -> (ids [nq][runs * k], distances) or (None, None)"""
    out = []
    for r0, r1 in col.tail_runs():
        rows = _selected(np.arange(r0, r1, dtype=np.uint64), prefilter)
        if rows.size:
            out.append(FR.flat_knn(oracle, col.x[rows.astype(np.int64)], np.asarray(q).astype(col.x.dtype), k, col.metric, lower, upper, row_ids=rows))
    if not out:
        return None, None
    return np.concatenate([o[0] for o in out], 1), np.concatenate([o[1] for o in out], 1)


MUTANTS = ("approx", "bounds_before", "dedup")


def nearest(oracle, col, q, k=10, nprobes=1, refine_factor=None, prefilter=None, distance_range=None, fast_search=False, use_index=True,
            mutant=None):
    """VectorColumn.nearest -> (ids uint64 [nq][k], distances f32 [nq][k]).  mutant (step 5 only): "approx" keeps the ANN list's
    approximate distances in the union; "bounds_before" applies the bounds before the union only; "dedup" de-duplicates the union."""
    assert mutant is None or mutant in MUTANTS
    lo, hi = (None, None) if distance_range is None else distance_range
    x = col.x
    q = np.asarray(q).astype(x.dtype).reshape(-1, x.shape[1])
    if not use_index or not col.deltas:
        rows = _selected(np.arange(len(x), dtype=np.uint64), prefilter)
        return FR.flat_knn(oracle, x[rows.astype(np.int64)], q, k, col.metric, lo, hi, row_ids=rows)
    if refine_factor is not None and refine_factor < 1:
        raise ValueError("Refine factor can not be zero")
    keff = k * (1 if refine_factor is None else refine_factor)
    ids, dists = join([dl.search(q, keff, nprobes, prefilter, lo, hi) for dl in col.deltas], keff)
    if refine_factor is not None:
        ids, dists = take_flat_knn(oracle, x, q, ids, k, col.metric, lower=lo, upper=hi)
    if fast_search or not col.tail_runs():
        return ids, dists
    bi, bd = tail_lists(oracle, col, q, k, prefilter, lo, hi)
    return take_flat_knn(oracle, x, q, ids, k, col.metric, ids_b=bi, dists_b=bd, lower=lo, upper=hi,
                         dists_a=dists if mutant == "approx" else None, bounds=mutant != "bounds_before", dedup=mutant == "dedup")


def same(a, b):
    return bool((np.asarray(a[0]).view(np.uint64) == np.asarray(b[0]).view(np.uint64)).all()
                and (np.asarray(a[1], f32).view(np.uint32) == np.asarray(b[1], f32).view(np.uint32)).all())


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def clustered(n, d, seed, centres=12, spread=0.35):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d)).astype(f32) * f32(2.0)
    return (c[rng.integers(0, centres, n)] + rng.standard_normal((n, d)).astype(f32) * f32(spread)).astype(f32)


def pq_model(oracle, x, metric, nlist, m, nbits=8, seed=1):
    """(centroids, codebook) trained on the CPU oracle from the rows x (normalised for cosine), as create_index trains them"""
    xs = oracle.normalize(x) if metric == "cosine" else x
    km = "l2" if metric == "cosine" else metric
    cent, _, _, _ = oracle.kmeans_train(xs, nlist, max_iters=8, balance_factor=f32(1.0) / f32(len(xs)), seed=seed, metric=km)
    part, _ = oracle.assign(xs, cent, km)
    res = oracle.residual(xs, cent, part) if km == "l2" else xs
    cb, _ = oracle.pq_train(res, m, nbits=nbits, max_iters=6, seed=seed + 1)
    return cent, cb


def mutant_fixture(oracle, metric, n=1400, d=16, k=6, seed=5):
    """A column of three fragments (900, 300, 200 rows) under one IVF_PQ delta RECORDED over fragment 0 but built over fragments 0 and 1
    (a stale fragment bitmap), so the rows of fragment 1 are in the ANN list AND in the tail scan; the queries sit on rows of fragments
    1 and 2.  -> dict(col, q, k, nprobes, ann, range, range_query, range_row): under `range` the ANN row `range_row` of query
    `range_query` is in range by the index's distance and out of range by the exact one -- (None, its exact distance) when a PQ distance
    lies below the exact one (the nearest such row: fewer than k rows are nearer, so a variant that keeps it returns it), else
    (its PQ distance, None)."""
    x = clustered(n, d, seed)
    col = Column(x, metric, [900, 300, 200])
    cent, cb = pq_model(oracle, x[:1200], metric, 6, 4, seed=seed)
    rng = np.random.default_rng(seed + 1)
    qrows = np.concatenate([rng.choice(np.arange(900, 1200), 3, replace=False), rng.choice(np.arange(1200, 1400), 3, replace=False)])
    q = (x[qrows] + rng.standard_normal((6, d)).astype(f32) * f32(0.05)).astype(f32)
    col.deltas = [pq_delta(oracle, col, [0], cent, cb, rows=np.arange(1200, dtype=np.uint64))]
    nprobes = 6
    ai, ad = col.deltas[0].search(q, k, nprobes, None, None, None)
    ei, ed = take_flat_knn(oracle, x, q, ai, k, metric)
    key = lambda v: int(FO.keys(np.asarray([v], f32))[0])
    below, above = [], []          # (exact or PQ key, query, row, PQ distance, exact distance)
    for i in range(len(q)):
        by_id = dict(zip(ei[i].tolist(), ed[i].tolist()))
        for r, a in zip(ai[i].tolist(), ad[i].tolist()):
            if r == int(UNSET):
                continue
            e = by_id[r]
            if key(a) < key(e):
                below.append((key(e), i, r, a, e))
            elif key(a) > key(e):
                above.append((key(a), i, r, a, e))
    out = dict(col=col, q=q, k=k, nprobes=nprobes, ann=(ai, ad), range=None)
    if below:
        _, i, r, a, e = min(below)
        out.update(range=(None, float(e)), range_query=i, range_row=r, range_pq=a, range_exact=e)
    elif above:
        _, i, r, a, e = min(above)
        out.update(range=(float(a), None), range_query=i, range_row=r, range_pq=a, range_exact=e)
    return out
