"""Shared by tests/test_rowid_fixtures.py (CPU) and tests/test_zz_gpu_row_addresses.py (GPU): row ids as a multi-fragment table has them
-- row ADDRESSES, fragment << 32 | offset, at and above 2^32 and unrelated to the storage order -- with the inputs of every case the two
files run, so that the CPU file proves on the oracle what the GPU file then asks of the kernels.

Every result of the library is ordered by (distance, row id) on the FULL 64-bit id (SortExec(dist, rowid).fetch(k), scanner.rs:3440-3468).
A kernel that compares, carries, packs or shuffles only one half of an id, or orders ties by where a row is stored, answers every case
here differently from the oracle: `mutants` restates those three wrong orders as id arrays, tests/test_rowid_fixtures.py shows that the
oracle's own answer changes under each of them for every case, so no case can pass by accident.

The data: every row occurs `COPIES` times (integer-valued, so the copies' distances are equal bit for bit), the copies scattered over
the storage order and -- with row_addresses -- over the fragments.  Groups of three against k = 1 / 10 / 100 / 128 put a tie at the
k-th place, and the integer grid adds ties between different rows around it."""
import functools
import types

import numpy as np

f32 = np.float32
u64 = np.uint64
NONE_ID = np.uint64(0xFFFFFFFFFFFFFFFF)       # "no row": flat_knn's and the searches' padding
FRAGMENTS = (0, 1, 3, 2 ** 31 - 1)            # fragment 0, a fragment >= 2, the largest whose address stays below 2^63
COPIES = 3


# ---- ids ----------------------------------------------------------------------------------------------------------------------
def _offset_pool(m):
    """m ascending offsets, the first half below 2^31, the rest from 2^31 up (the low word's top bit set)"""
    h = m // 2
    return np.concatenate([np.arange(h, dtype=u64) * u64(7) + u64(3), u64(1 << 31) + np.arange(m - h, dtype=u64) * u64(5) + u64(1)])


def row_addresses(n, seed):
    """n distinct addresses fragment << 32 | offset (all below 2^63, none ~0) in a storage order unrelated to them.  Fragment j of
    FRAGMENTS takes a window of the offset pool that starts half a window BELOW fragment j - 1's: windows overlap (a low word occurs in
    two fragments, a high word in many rows), and the higher the fragment the lower its offsets -- the order by low word is roughly
    the reverse of the order by address.  Fragment 0's offsets all lie above 2^31, so every address is >= 2^31."""
    assert n >= 16
    nf = len(FRAGMENTS)
    per = -(-n // nf)
    step = max(1, per // 2)
    pool = _offset_pool(per + (nf - 1) * step)
    ids = []
    for j, frag in enumerate(FRAGMENTS):
        cnt = min(per, n - j * per)
        start = (nf - 1 - j) * step
        ids.append((u64(frag) << u64(32)) | pool[start:start + cnt])
    ids = np.concatenate(ids)
    assert ids.size == n
    return np.ascontiguousarray(ids[np.random.default_rng(seed).permutation(n)])


def small_offset_addresses(n, seed):
    """fragment << 32 | i with the i a permutation of 0 .. n-1: every low word is a valid index into a mask (or a raw column) of n
    entries, but only the fragment-0 rows' ADDRESSES are"""
    rng = np.random.default_rng(seed)
    frag = np.asarray(FRAGMENTS, u64)[rng.integers(0, len(FRAGMENTS), n)]
    return np.ascontiguousarray((frag << u64(32)) | rng.permutation(n).astype(u64))


def ids_indexing_raw(n, seed):
    """a permutation of 0 .. n-1: ids that index a raw column of n rows (lay it out with raw_by_id)"""
    return np.random.default_rng(seed).permutation(n).astype(u64)


def raw_by_id(x, rid):
    """the raw column as refine reads it: raw[rid[i]] = x[i]"""
    out = np.empty_like(x)
    out[np.asarray(rid).astype(np.int64)] = x
    return out


def mask_by_id(selected, rid):
    """a prefilter mask indexed by id that selects row i iff selected[i] (ids must be small: the mask is max(id) + 1 long)"""
    m = np.zeros(int(np.asarray(rid).max()) + 1, bool)
    m[np.asarray(rid).astype(np.int64)] = selected
    return m


def selected_rows(mask, rid):
    """row i is selected iff its id lies inside the mask and the mask holds True there"""
    rid = np.asarray(rid, u64)
    ok = rid < u64(len(mask))
    ok[ok] = np.asarray(mask, bool)[rid[ok].astype(np.int64)]
    return ok


def mutants(rid):
    """three WRONG id orders, as id arrays (the ranks 0 .. n-1 under the wrong key) with the map back to the true ids:
         "low"   ties broken by the low word alone (then storage position: equal low words have no other order)
         "high"  by the high word, then storage position
         "pos"   by storage position
    -> {name: (mutant ids u64 [n], back u64 [n])}, true id of a row = back[mutant id].  Used only to prove that a case can fail."""
    rid = np.asarray(rid, u64)
    pos = np.arange(rid.size)
    out = {}
    for name, keys in (("low", (pos, rid & u64(0xFFFFFFFF))), ("high", (pos, rid >> u64(32))), ("pos", (pos,))):
        order = np.lexsort(keys)
        rank = np.empty(rid.size, np.int64)
        rank[order] = pos
        out[name] = (rank.astype(u64), rid[order])
    return out


def unmap(ids, back):
    """mutant ids in a result -> true ids (padding stays padding)"""
    ids = np.asarray(ids, u64)
    out = np.full(ids.shape, NONE_ID, u64)
    ok = ids != NONE_ID
    out[ok] = back[ids[ok].astype(np.int64)]
    return out


# ---- data ---------------------------------------------------------------------------------------------------------------------
def clustered(n, d, seed, ncl=16, sigma=20.0):
    """integer-valued rows in 0 .. 218 around ncl centres"""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(0, 128, (ncl, d))
    return np.clip(np.rint(centers[rng.integers(0, ncl, n)] + rng.normal(0, sigma, (n, d))), 0, 218).astype(f32)


def copies(base, seed):
    """every row of base COPIES times, scattered over the storage order"""
    x = np.tile(base, (COPIES, 1))
    return np.ascontiguousarray(x[np.random.default_rng(seed).permutation(x.shape[0])])


def queries_near(base, nq, seed):
    """rows of base plus 0 / 1 per element (integer distances, many equal); the first query IS a row"""
    rng = np.random.default_rng(seed)
    q = base[rng.integers(0, base.shape[0], nq)] + rng.integers(0, 2, (nq, base.shape[1])).astype(base.dtype)
    q[0] = base[0]
    return np.ascontiguousarray(q)


def models(oracle, x, nlist, m, metric, seed, nbits=8):
    """centroids and codebook, trained by the oracle on a prefix of the rows"""
    xs = oracle.normalize(x) if metric == "cosine" else x
    km = "l2" if metric == "cosine" else metric
    cent, _, _, _ = oracle.kmeans_train(xs[: nlist * 40], nlist, max_iters=4, seed=seed, metric=km)
    part, _ = oracle.assign(xs, cent, km)
    res = oracle.residual(xs, cent, np.where(part == oracle.NONE, 0, part)) if km == "l2" else xs
    cb, _ = oracle.pq_train(res[: 256 * 12], m, nbits=nbits, max_iters=3, seed=seed + 1)
    return cent, cb


# ---- flat KNN -----------------------------------------------------------------------------------------------------------------
# name: (element type, d, nq, metric, ks) -- 6000 rows each (the streaming kernel starts at 4096 rows, the matrix-core filters run the
# epochs after the first 2048 rows).  The kernel each shape reaches is named in tests/test_zz_gpu_row_addresses.py
FLAT_CASES = {
    "small_1q": ("f32", 100, 1, "l2", (1, 10, 128)),
    "small_2q": ("f32", 100, 2, "dot", (1, 10, 128)),
    "filter_v2": ("f32", 64, 7, "l2", (1, 10)),
    "mfma_batch": ("f32", 32, 130, "l2", (10,)),
    "mfma_wide": ("f32", 256, 130, "l2", (10,)),
    "generic_cosine": ("f32", 20, 9, "cosine", (10,)),
    "large_k": ("f32", 64, 9, "l2", (200,)),
    "f16_dot": ("f16", 64, 5, "dot", (10,)),
    "f16_native": ("f16", 64, 7, "l2", (10,)),
    "int8_native": ("int8", 64, 130, "dot", (10,)),
}


@functools.lru_cache(maxsize=None)
def flat_case(name):
    kind, d, nq, metric, ks = FLAT_CASES[name]
    seed = 1000 + sorted(FLAT_CASES).index(name)
    base = clustered(2000, d, seed)
    if kind == "int8":
        base = base - f32(100)                       # -100 .. 118
    x, q = copies(base, seed + 1), queries_near(base, nq, seed + 2)
    if kind == "f16":
        x, q = (x / f32(256)).astype(np.float16), (q / f32(256)).astype(np.float16)      # integer / 256: exact in binary16
    elif kind == "int8":
        x, q = x.astype(np.int8), q.astype(np.int8)
    return types.SimpleNamespace(name=name, kind=kind, metric=metric, x=x, q=q, ks=ks, rid=row_addresses(x.shape[0], seed + 3))


def flat_answers(oracle, c, rid, nq=None):
    """[(ids, dists)] of the oracle's flat scan, one per k"""
    x = c.x if c.kind == "f16" else c.x.astype(f32)
    q = (c.q if c.kind == "f16" else c.q.astype(f32))[:nq]
    return [oracle.flat_knn(x, q, k, c.metric, row_ids=rid) for k in c.ks]


# ---- IVF_FLAT -----------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def ivfflat_case(ids="addresses"):
    """the fixture of tests/test_zz_gpu_zz_ivfflat_ties.py -- 4000 identical rows, far more than a candidate pool of 2048: those queries
    are replayed through the heap -- on top of rows in three copies.  ids: "addresses" | "small" (small_offset_addresses)"""
    import oracle
    rng = np.random.default_rng(5)
    d = 32
    base = rng.integers(0, 30, (3000, d)).astype(f32)
    x = copies(base, 6)
    n = x.shape[0]
    x[1000:5000] = x[7]
    q = rng.integers(0, 30, (12, d)).astype(f32)
    q[:4] = x[7]
    q[4:8] = x[7] + 1.0
    q[8] = x[5500]
    cent, _, _, _ = oracle.kmeans_train(x[5000:5384], 6, max_iters=5, seed=3)
    part, _ = oracle.assign(x, cent)
    rid = row_addresses(n, 7) if ids == "addresses" else small_offset_addresses(n, 7)
    return types.SimpleNamespace(x=x, q=q, cent=cent, part=part, rid=rid, metric="l2", runs=((10, 6), (100, 3), (5, 1)))


def ivfflat_answers(oracle, c, rid, keep=None):
    """keep: boolean over the rows (a prefilter's selection) -- the reference scans the selected rows of a partition in storage order"""
    x, ids = (c.x, rid) if keep is None else (c.x[keep], np.asarray(rid)[keep])
    return [oracle.ivfflat_search(x, c.cent, c.q, k, nprobes, c.metric, row_ids=ids) for k, nprobes in c.runs]


# ---- IVF_PQ -------------------------------------------------------------------------------------------------------------------
# name: (d, M, nbits, nlist, metric, queries, runs = ((nq, k, nprobes), ...)) -- 6000 rows each.  A 256-CU device answers 512 queries
# and more one workgroup per query (nsplit == 1) and fewer with the probes split over several; nq * nprobes >= 4096 (2048 for the tiled
# shapes) takes the partition-major flow where the shape has one, and nq * nprobes >= 96 * nlist the matrix-core scan
IVFPQ_CASES = {
    "query_major": (64, 8, 8, 16, "l2", 520, ((520, 10, 5), (520, 1, 3), (3, 10, 8), (1, 100, 16))),     # M = 8: no partition-major kernel
    "partition_major": (64, 16, 8, 48, "l2", 640, ((640, 10, 7), (640, 100, 7))),                       # 4480 pairs < 96 x 48
    "mscan": (64, 16, 8, 24, "l2", 700, ((700, 10, 8), (700, 128, 6))),
    "tiled_m48": (48 * 8, 48, 8, 24, "l2", 300, ((300, 10, 7),)),
    "four_bit": (64, 16, 4, 16, "l2", 100, ((100, 10, 16), (100, 10, 3), (3, 10, 4))),
    "dot_flow": (64, 16, 8, 24, "dot", 700, ((700, 10, 8),)),
    "overflow": (128, 16, 8, 16, "l2", 512, ((512, 10, 8),)),
}


@functools.lru_cache(maxsize=None)
def ivfpq_case(name, ids="addresses", kind="f32"):
    """ids: "addresses" | "small" | "raw" (ids_indexing_raw: what refine needs); kind "int8": an Int8 column (the model stays f32),
    "f32_frac": f32 with one fractional element"""
    import oracle
    d, m, nbits, nlist, metric, nq, runs = IVFPQ_CASES[name]
    seed = 2000 + 10 * sorted(IVFPQ_CASES).index(name)
    base = clustered(2000, d, seed)
    if kind == "int8":
        base = base - f32(100)
    x = copies(base, seed + 1)
    n = x.shape[0]
    q = queries_near(base, nq, seed + 2)
    if name == "overflow":       # 400 identical rows in one partition: more ties at the bound than a candidate buffer holds
        rng = np.random.default_rng(seed + 3)
        hot = x[5].copy()
        x[rng.choice(np.arange(100, n), 400, replace=False)] = hot
        q[: nq // 2] = hot + rng.integers(-1, 2, (nq // 2, d)).astype(f32)
        q[0] = hot
    if kind == "f32_frac":       # one fraction: the column is no longer a widened u8 column
        x[n - 1, d - 1] += f32(0.5)
    cent, cb = models(oracle, x, nlist, m, metric, seed + 4, nbits=nbits)
    rid = {"addresses": row_addresses, "small": small_offset_addresses, "raw": ids_indexing_raw}[ids](n, seed + 5)
    return types.SimpleNamespace(name=name, kind=kind, x=x, q=q, cent=cent, cb=cb, metric=metric, nbits=nbits, nlist=nlist, runs=runs, rid=rid)


def ivfpq_oracle_index(oracle, c, rid):
    return oracle.build_index(c.x, c.cent, c.cb, c.metric, row_ids=rid, nbits=c.nbits)


def ivfpq_answers(oracle, c, rid, nq=None, refine=0, raw=None, prefilter=None, runs=None, **range_):
    """[(ids, dists)] per run; nq caps the queries of every run (the CPU file's mutant runs)"""
    oidx = ivfpq_oracle_index(oracle, c, rid)
    out = []
    for rq, k, nprobes in (c.runs if runs is None else runs):
        rq = rq if nq is None else min(rq, nq)
        out.append(oidx.search(c.q[:rq], k, nprobes, refine=refine, raw=raw, prefilter=prefilter, **range_))
    return out


# the other searches over the same ids, read by both test files.  OTHER_SEARCHES: the cases whose first run is also searched filtered, under
# a distance range and as candidate lists; REFINE_RUNS: (nq, k, nprobes) of the refined searches
OTHER_SEARCHES = ("query_major", "partition_major")
CANDIDATES_KEFF = 40                # search_candidates(keff) of an unrefined index
REFINE_RUNS = {"query_major": (520, 10, 5), "partition_major": (640, 10, 7)}
REFINE_FACTORS = (1, 3, 10)
REFINE_CANDIDATES = (64, 30)        # (queries, keff) of search_candidates on an index with a raw column
RANGE_QUANTILES = (0.2, 0.8)


def range_bounds(oidx, c):
    """[lower, upper) of the range search: two quantiles of the finite PQ distances of the first run's queries at k = CANDIDATES_KEFF"""
    nq, _, nprobes = c.runs[0]
    _, ud = oidx.search(c.q[:nq], CANDIDATES_KEFF, nprobes)
    fin = ud[np.isfinite(ud)]
    return float(np.quantile(fin, RANGE_QUANTILES[0])), float(np.quantile(fin, RANGE_QUANTILES[1]))


def ivfpq_tie_census(oracle, c, oidx, nq, k, nprobes):
    """How the k-th place of every query of a run falls -> (decided by id, left to the heap, no tie).  A tie at the k-th place is decided
    by the id order alone unless ONE partition holds more than k of the rows at or below that distance: then that partition's heap has
    dropped some of them by its own (storage) order, and the engine replays the query through its heap emulation.  The first kind is
    what makes the scan and merge kernels' id compare decide a result; counted from the oracle's answer for k + 64."""
    wide = k + 64
    ids, dist = oidx.search(c.q[:nq], wide, nprobes)
    where = np.argsort(oidx.row_ids)
    by_id = by_heap = 0
    for r in range(ids.shape[0]):
        key = dist[r].view(np.uint32)
        if ids[r, k] == NONE_ID or key[k] != key[k - 1]:
            continue
        at_or_below = ids[r][(dist[r] <= dist[r, k - 1]) & (ids[r] != NONE_ID)]
        stored = where[np.searchsorted(oidx.row_ids[where], at_or_below)]
        part = np.searchsorted(oidx.part_offsets, stored, side="right") - 1
        heap = at_or_below.size == wide or np.bincount(part).max() > k
        by_heap += heap
        by_id += not heap
    return by_id, by_heap, ids.shape[0] - by_id - by_heap


def pq_partition_case():
    """one partition for pq_scan_topk: random codes in three copies, so that equal codes give equal sums"""
    rng = np.random.default_rng(6)
    d, m, n_p = 32, 8, 3000
    cb = rng.standard_normal((m, 256, d // m)).astype(f32)
    codes = copies(rng.integers(0, 256, (n_p // COPIES, m), dtype=np.uint8), 7)
    return types.SimpleNamespace(cb=cb, codes=codes, qr=rng.standard_normal(d).astype(f32), rid=row_addresses(n_p, 8), ks=(1, 20, 200))


def pq_partition_answers(oracle, c, rid):
    dist = oracle.pq_scan(oracle.build_lut(c.qr, c.cb), oracle.transpose(c.codes))
    out = []
    for k in c.ks:
        hi, hd = oracle.heap_topk(dist, rid, k)
        out.append(oracle.sort_fetch(hi, hd, k))
    return out


# ---- IVF_SQ -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sq_case(name, ids="addresses"):
    """"gaussian": sq_spec.gaussian rows in three copies (k = 10 cuts a group of copies inside one partition: replayed through the heap;
    k = 9 does not: the fast path answers, the copies inside the list in id order); "ties": sq_spec.tie_fixture (256 distinct
    vectors: every query is replayed through the heap)"""
    import oracle
    import sq_spec as S
    if name == "gaussian":
        base, q = S.gaussian(1000, 32, 33, seed=41)
        x = copies(base, 42)
        metric, nlist = "l2", 8
        cent = S.centroids_with_gaps(x, nlist, seed=43)
        runs = ((10, 3), (9, 3), (1, 1), (128, 8))      # k = 9: the cut falls between two groups of copies -- no partition's heap has to choose
    else:
        x, q, _ = S.tie_fixture()
        metric, nlist = "l2", 4
        cent = S.centroids_with_gaps(x, nlist, seed=3)
        runs = ((10, 3), (1, 1), (128, 4))
    xs, part = S.prepare_rows(oracle, x, cent, metric)
    b = S.bounds(xs[:64]) if name == "gaussian" else S.bounds(xs)
    rid = (row_addresses if ids == "addresses" else small_offset_addresses)(x.shape[0], 44)
    return types.SimpleNamespace(name=name, x=x, xs=xs, q=q, cent=cent, part=part, bounds=b, codes=S.encode(xs, *b), metric=metric,
                                 nlist=nlist, runs=runs, rid=rid)


def sq_answers(oracle, c, rid, nq=None, prefilter=None):
    import sq_spec as S
    return [S.search(oracle, c.codes, c.part, c.cent, c.q[:nq], k, nprobes, c.metric, *c.bounds, row_ids=rid, prefilter=prefilter)
            for k, nprobes in c.runs]


# ---- multivector flat KNN -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def multivec_case():
    """2100 rows (700 distinct rows of 1 .. 4 vectors, three copies each): more than one selection block of 2048 candidates, so the
    selection runs a second round over the blocks' survivors"""
    import multivec_spec as M
    d, nqv, nb = 20, 5, 700
    lens_b = M.lengths(nb, 1, 4, 51)
    values_b, off_b, q = M.column(lens_b, d, nqv, 52)
    order = np.random.default_rng(53).permutation(np.tile(np.arange(nb), COPIES))
    values = np.concatenate([values_b[off_b[r]:off_b[r + 1]] for r in order])
    off = M.offsets_of(lens_b[order])
    return types.SimpleNamespace(values=np.ascontiguousarray(values), off=off, q=q, metric="cosine", ks=(1, 10, 128),
                                 rid=row_addresses(order.size, 54))


def multivec_answers(oracle, c, rid):
    import multivec_spec as M
    dist = M.distances(oracle, c.values, c.off, c.q, c.metric)
    return [M.topk(dist, k, rid) for k in c.ks]


# ---- merge of gathered candidate lists ----------------------------------------------------------------------------------------
def merge_case():
    """what Engine.merge_topk gets from four "shards": per query 4 x 24 candidates, ids drawn from row_addresses (as int64 bit patterns),
    distances on a grid of six values (equal distances across shards), a fifth of the slots empty (id -1, distance +inf), and -- for
    the refine variant -- exact distances on a grid of their own"""
    rng = np.random.default_rng(61)
    nq, c = 9, 96
    pool = row_addresses(400, 62)
    ids = np.stack([pool[rng.permutation(pool.size)[:c]] for _ in range(nq)])
    dists = rng.integers(0, 6, (nq, c)).astype(f32) * f32(0.5)
    exact = rng.integers(0, 4, (nq, c)).astype(f32) * f32(0.25)
    hole = rng.random((nq, c)) < 0.2
    ids[hole] = NONE_ID
    dists[hole] = np.inf
    exact[hole] = np.inf
    return types.SimpleNamespace(ids=ids, dists=dists, exact=exact, k=10, keff=30)


def merge_answers(oracle, c, ids, exact):
    """(dist, rowid) merge of every query's filled slots; exact: the keff best by PQ distance re-ranked by the exact distances"""
    out_i = np.full((c.ids.shape[0], c.k), NONE_ID, u64)
    out_d = np.full((c.ids.shape[0], c.k), np.inf, f32)
    for r in range(c.ids.shape[0]):
        ok = c.ids[r] != NONE_ID
        if exact:
            si, _ = oracle.sort_fetch(ids[r][ok], c.dists[r][ok], c.keff)
            ex = dict(zip(ids[r][ok].tolist(), c.exact[r][ok].tolist()))
            si, sd = oracle.sort_fetch(si, np.array([ex[i] for i in si.tolist()], f32), c.k)
        else:
            si, sd = oracle.sort_fetch(ids[r][ok], c.dists[r][ok], c.k)
        out_i[r, :si.size] = si
        out_d[r, :sd.size] = sd
    return [(out_i, out_d)]
