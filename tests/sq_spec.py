"""Shared by tests/test_sq_spec.py, tests/test_sq_kernels_cpu.py (CPU) and tests/test_zz_gpu_sq.py, tests/test_zz_gpu_sq_scan.py (GPU):
the CPU specification of 8-bit scalar quantisation and of the IVF_SQ search, in numpy, composed with the oracle's existing functions
for the IVF side, the fixtures of these files, and wrong selections (mutants) the fixtures must tell from the specification.

The specification (lance-index sq.rs:43-89, 263-287; sq/storage.rs:398-468; lance-linalg l2.rs:44-49, dot.rs:152-161;
flat/index.rs:82-177), every floating-point operation one rounding in the stated format:
    bounds     start.min(v) .. end.max(v) over every element widened to f64, from f64::MAX .. f64::MIN; min / max skip NaN
    code       start == end: 0.  Else t = (f64(v) - start) * 255.0 / (end - start) in f64, `t as u8`: truncated toward zero,
               saturated to 0 .. 255, NaN -> 0
    sum        L2 and cosine: sum of (|x_i - y_i| as u32)^2 in u32;  dot: sum of x_i * y_i in u32
    dist0      sum as f32 (round to nearest even);  dot: 1.0f - that
    dist       (dist0 * (r * r)) / 65025.0f in f32, r = (end - start) as f32
    partition  oracle.heap_topk over the rows in storage order (FlatIndex::search: push while len < k, else replace the root only
               if root.dist > dist), unselected rows skipped under a prefilter
    query      normalised for cosine, encoded with the index bounds; partitions by oracle.find_partitions (L2 for cosine);
               the partition results merged by oracle.sort_fetch (dist, rowid)"""
import functools

import numpy as np

f32, f64 = np.float32, np.float64
FRESH_BOUNDS = (float(np.finfo(f64).max), float(np.finfo(f64).min))      # ScalarQuantizer::new
NONE = 0xFFFFFFFF


# ---- the quantiser ------------------------------------------------------------------------------------------------------------
def bounds(x, start=FRESH_BOUNDS[0], end=FRESH_BOUNDS[1]):
    v = np.asarray(x).astype(f64).ravel()
    v = v[~np.isnan(v)]
    if v.size:
        start, end = min(f64(start), v.min()), max(f64(end), v.max())
    return float(start), float(end)


def encode(x, start, end):
    x = np.asarray(x)
    if start == end:
        return np.zeros(x.shape, np.uint8)
    with np.errstate(all="ignore"):
        t = (x.astype(f64) - f64(start)) * f64(255.0) / (f64(end) - f64(start))
    codes = np.zeros(x.shape, np.uint8)
    pos = t > 0                                    # NaN compares false: code 0
    codes[pos] = np.minimum(t[pos], 255.0).astype(np.uint8)      # in [0, 255]: the cast truncates
    return codes


def int_sums(codes, qcode, metric):
    """u32 sums of one encoded query against codes [n][d]"""
    x = np.asarray(codes, np.uint8).astype(np.uint32)
    y = np.asarray(qcode, np.uint8).astype(np.uint32)
    if metric == "dot":
        return (x * y).sum(axis=1, dtype=np.uint32)
    diff = np.abs(x.astype(np.int64) - y.astype(np.int64)).astype(np.uint32)
    return (diff * diff).sum(axis=1, dtype=np.uint32)


def scale(sums, metric, start, end):
    d0 = np.asarray(sums, np.uint32).astype(f32)
    if metric == "dot":
        d0 = f32(1.0) - d0
    r = f32(f64(end) - f64(start))
    with np.errstate(all="ignore"):
        return (d0 * f32(r * r)) / f32(65025.0)


def distances(codes, q, metric, start, end):
    """[nq][n] distances of RAW queries (encoded here with the same bounds) against codes [n][d]"""
    qc = encode(np.asarray(q).reshape(-1, np.asarray(codes).shape[1]), start, end)
    return np.stack([scale(int_sums(codes, c, metric), metric, start, end) for c in qc])


# ---- IVF_SQ -------------------------------------------------------------------------------------------------------------------
def prepare_rows(oracle, x, centroids, metric):
    """the transform chain of the build: (rows as stored -- normalised for cosine --, part ids assigned in L2 / under dot; rows
    with a non-finite element have none)"""
    xs = oracle.normalize(x) if metric == "cosine" else x
    part, _ = oracle.assign(xs, centroids, "l2" if metric == "cosine" else metric)
    part[~np.isfinite(np.asarray(xs, f64)).all(axis=1)] = NONE      # KeepFiniteVectors ahead of the partition transform (ivf.rs)
    return xs, part


def search(oracle, codes, part_ids, centroids, q, k, nprobes, metric, start, end, row_ids=None, prefilter=None, select=None):
    """codes [n][d] in input order; part_ids [n] (NONE = dropped); q raw queries in the column's element type.  select: a MUTANT of
    the per-partition selection (int_sum_select, unscaled_select below) in place of the heap -- what a wrong kernel would answer"""
    codes = np.asarray(codes, np.uint8)
    n, d = codes.shape
    nlist = centroids.shape[0]
    rid = np.arange(n, dtype=np.uint64) if row_ids is None else np.asarray(row_ids, np.uint64)
    offs, perm = oracle.partition_layout(part_ids, nlist)
    q = np.asarray(q).reshape(-1, d)
    qs = oracle.normalize(q) if metric == "cosine" else q
    probes, _ = oracle.find_partitions(qs, centroids, nprobes, "l2" if metric == "cosine" else metric)
    qc = encode(qs, start, end)
    allow = None if prefilter is None else np.asarray(prefilter, bool)
    out_i = np.full((q.shape[0], k), np.iinfo(np.uint64).max, np.uint64)
    out_d = np.full((q.shape[0], k), np.inf, f32)
    for qi in range(q.shape[0]):
        ci, cd = [], []
        for p in probes[qi]:
            rows = perm[int(offs[p]):int(offs[p + 1])]
            if allow is not None and len(rows):
                r = rid[rows]
                ok = r < allow.size
                ok[ok] = allow[r[ok]]
                rows = rows[ok]
            if len(rows) == 0:
                continue
            sums = int_sums(codes[rows], qc[qi], metric)
            dist = scale(sums, metric, start, end)
            hi, hd = oracle.heap_topk(dist, rid[rows], k) if select is None else select(oracle, sums, dist, rid[rows], k, metric)
            ci.append(hi); cd.append(hd)
        if ci:
            si, sd = oracle.sort_fetch(np.concatenate(ci), np.concatenate(cd), k)
            out_i[qi, :len(si)] = si; out_d[qi, :len(sd)] = sd
    return out_i, out_d


# ---- wrong selections: what a kernel answers whose key is not the scaled f32 distance --------------------------------------------
def int_sum_select(oracle, sums, dist, rid, k, metric):
    """MUTANT: the k best of a partition by (u32 sum -- dot: descending --, storage position).  Two sums above 2^24 that are one float
    are a tie to the reference (the heap decides) and an order here"""
    key = sums.astype(np.int64) * (-1 if metric == "dot" else 1)
    keep = np.lexsort((np.arange(len(sums)), key))[:k]
    return rid[keep], dist[keep]


def unscaled_select(oracle, sums, dist, rid, k, metric):
    """MUTANT: the heap keyed by f32(sum) (dot: 1 - f32(sum)), before the multiply by r^2 and the divide by 65025: two floats that
    the scaling rounds into one are a tie to the reference and an order here"""
    d0 = sums.astype(f32)
    if metric == "dot":
        d0 = f32(1.0) - d0
    pos, _ = oracle.heap_topk(d0, np.arange(len(sums), dtype=np.uint64), k)
    pos = pos.astype(np.int64)
    return rid[pos], dist[pos]


def sorted_search(oracle, codes, part_ids, centroids, q, k, nprobes, metric, start, end, row_ids=None):
    """the WRONG answer a search gives that ignores the heap: every probed row sorted by (dist, rowid), the first k"""
    codes = np.asarray(codes, np.uint8)
    n, d = codes.shape
    rid = np.arange(n, dtype=np.uint64) if row_ids is None else np.asarray(row_ids, np.uint64)
    offs, perm = oracle.partition_layout(part_ids, centroids.shape[0])
    q = np.asarray(q).reshape(-1, d)
    qs = oracle.normalize(q) if metric == "cosine" else q
    probes, _ = oracle.find_partitions(qs, centroids, nprobes, "l2" if metric == "cosine" else metric)
    qc = encode(qs, start, end)
    out_i = np.full((q.shape[0], k), np.iinfo(np.uint64).max, np.uint64)
    for qi in range(q.shape[0]):
        rows = np.concatenate([perm[int(offs[p]):int(offs[p + 1])] for p in probes[qi]])
        if len(rows):
            dist = scale(int_sums(codes[rows], qc[qi], metric), metric, start, end)
            si, _ = oracle.sort_fetch(rid[rows], dist, k)
            out_i[qi, :len(si)] = si
    return out_i


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
def permuted_ids(n, seed):
    """explicit row ids unrelated to the storage order"""
    return (np.random.default_rng(seed).permutation(n).astype(np.uint64) * np.uint64(3) + np.uint64(7))


def gaussian(n, d, nq, seed, kind="f32"):
    """clustered Gaussian rows (16 centres) and queries near rows; "f16": rounded to binary16 (rows and queries)"""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((16, d)) * 2.0
    x = centres[rng.integers(0, 16, n)] + rng.standard_normal((n, d)) * 0.6
    q = x[rng.integers(0, n, nq)] + rng.standard_normal((nq, d)) * 0.3
    dt = np.float16 if kind == "f16" else f32
    return np.ascontiguousarray(x.astype(dt)), np.ascontiguousarray(q.astype(dt))


def centroids_with_gaps(x, nlist, seed):
    """nlist centroids of x's element type: rows of x, one of them moved far away (an EMPTY partition, when nlist > 1)"""
    rng = np.random.default_rng(seed)
    c = np.array(x[rng.choice(x.shape[0], nlist, replace=False)], dtype=x.dtype)
    if nlist > 1:
        c[nlist - 1] = c[nlist - 1] * 0 + 60.0
    return np.ascontiguousarray(c)


def tie_fixture(n=3000, nq=33, seed=11):
    """d = 4 on a four-value grid: 256 distinct vectors among n rows, so far more rows tie at a partition's k-th distance than fit;
    row ids are permuted, so which tied rows the heap keeps is not what (dist, rowid) would pick"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 4, (n, 4)).astype(f32)
    q = rng.integers(0, 4, (nq, 4)).astype(f32)
    return x, q, permuted_ids(n, seed + 1)


def large_sum_fixture(d=1024):
    """integer-valued rows under bounds 0 .. 255 (code = value) against a zero query: the sums 1023 * 255^2 + {0, 1, 4, 9} lie above
    2^24, where f32 is spaced by 4 -- the first two become one float.  -> (x [4][d] f32, q [1][d] f32, bounds)"""
    x = np.full((4, d), 255.0, f32)
    x[:, -1] = [0.0, 1.0, 2.0, 3.0]
    return x, np.zeros((1, d), f32), (0.0, 255.0)


LARGE_SUM_BOUNDS = (0.0, 441.5)       # r^2 / 65025 = 2.9977: the scaling is no power of two, it merges floats of its own
LARGE_SUM_TAIL = 12                   # varying columns; one more column in front of them tells the two partitions apart
LARGE_SUM_OTHER = 24                  # rows of the second partition
LARGE_SUM_DIMS = ((259, 900), (516, 900), (1024, 900), (1536, 900), (4096, 900), (16384, 300))      # (d, rows of partition 0) the GPU file runs
LARGE_SUM_KS = (1, 10, 128)
LARGE_SUM_WIDE = ((1536, (129, 768)), (16384, (129,)))      # keff whose list the design query's partition cuts with a tie: 300 rows at d = 16384


@functools.lru_cache(maxsize=None)
def large_sum_cached(d, metric, n):
    """one fixture per (d, metric) for every test of a process; nobody writes to it"""
    return large_sum_partition(d, metric, n)


def large_sum_partition(d, metric, n, seed=0):
    """Partition 0 of a two-partition index whose integer sums against the design query lie above 2^24 (from d = 516 on) and differ by
    single units, so that f32 holds several of them in one value -- and the scaling by r^2 / 65025 merges further ones -- while the
    sums themselves are distinct.  Column layout: d - 13 main columns | 1 selector | 12 tail columns.
        rows       main code 255 (saturated: the value lies above the bound); tail codes from 0 .. 5; every tail pattern is stored
                   three times, far apart, so a key is tied wherever a partition's list is cut
        query 0    L2: codes 0 everywhere -- the sum is (d - 13) 255^2 + sum(tail^2).  dot: code 255 on the main columns and 0 / 1 / 2
                   on the tail -- (d - 13) 255^2 + sum(tail * q), in steps of one
        query 1    the same with other tail codes (L2: 0 .. 2); query 2: the codes of a row of partition 1
        partition 1  LARGE_SUM_OTHER rows of the same kind (codes 255 | 1 | tail): their keys fall among partition 0's, so nprobes = 2 merges two
                   lists that interleave.  The selector column (-200 / code 0 in partition 0 and the queries, code 1 in partition 1)
                   and the centroids (equal but for -1000 / +1000 there) assign every row and the design queries under L2 and under dot.
    Values are real numbers inside their code's cell, (code + u) (end - start) / 255 with u in [0.2, 0.8), not the cell's edge.
    -> dict x f32 [n + LARGE_SUM_OTHER][d] (input order = storage order, partition 0 first), codes (intended), q f32 [3][d], qcodes,
       cent f32 [2][d], bounds, rid (permuted row ids), n"""
    start, end = LARGE_SUM_BOUNDS
    tail, m = LARGE_SUM_TAIL, n + LARGE_SUM_OTHER
    main = d - tail - 1
    assert main >= 1 and n % 3 == 0
    rng = np.random.default_rng([seed, d, n, int(metric == "dot")])
    codes = np.full((m, d), 255, np.uint8)
    third = rng.integers(0, 6, (n // 3, tail))
    codes[:n, main + 1:] = np.concatenate([third, third[rng.permutation(n // 3)], third[rng.permutation(n // 3)]])
    codes[n:, main + 1:] = rng.integers(0, 6, (LARGE_SUM_OTHER, tail))
    codes[:n, main] = 0
    codes[n:, main] = 1
    qcodes = np.zeros((3, d), np.uint8)
    if metric == "dot":
        qcodes[:, :main] = 255
        qcodes[:2, main + 1:] = rng.integers(0, 3, (2, tail))
    else:
        qcodes[1, main + 1:] = rng.integers(0, 3, tail)
    qcodes[2] = codes[n + 1]
    qcodes[2, main] = 0
    value = lambda c: ((c.astype(f64) + rng.uniform(0.2, 0.8, c.shape)) * (end - start) / 255.0 + start).astype(f32)
    x, q = value(codes), value(qcodes)
    x[:n, main] = -200.0
    q[:, main] = -200.0
    cent = np.full((2, d), f32(end + 0.5 * (end - start) / 255.0), f32)
    cent[:, main + 1:] = f32(2.5 * (end - start) / 255.0)
    cent[0, main], cent[1, main] = -1000.0, 1000.0
    return {"x": np.ascontiguousarray(x), "codes": codes, "q": np.ascontiguousarray(q), "qcodes": qcodes, "cent": cent,
            "bounds": LARGE_SUM_BOUNDS, "rid": permuted_ids(m, seed + 17), "n": n}


def order_key(a):
    """f32::total_cmp as an unsigned key: what the kernels' lists and heaps compare"""
    b = np.ascontiguousarray(a, f32).view(np.uint32)
    return np.where(b >> 31 != 0, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def large_sum_keys(f, metric, qi=0):
    """(u32 sums, order keys of the scaled distances) of partition 0's rows, in storage order, for query qi of the fixture"""
    sums = int_sums(f["codes"][:f["n"]], f["qcodes"][qi], metric)
    return sums, order_key(scale(sums, metric, *f["bounds"]))


def saturation_fixture(n=257, d=16, seed=5):
    """bounds trained on a SAMPLE (the first 32 rows), so later rows fall below start and above end.  -> (x f32, bounds)"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d)).astype(f32)
    x[100, 3] = -40.0; x[200, 5] = 40.0
    return x, bounds(x[:32])


SPECIALS = [np.nan, np.inf, -np.inf, -0.0, 0.0, 1e-40, -1e-40, 6e-8, -6e-8]      # 1e-40: f32 subnormal; 6e-8: f16 subnormal


def encode_fixture(n, d, kind, seed):
    """values around bounds (-1.5, 2.25) -- both exact in f16 -- with NaN, +-inf, -0.0, subnormals, exactly start, exactly end, and
    values below / above the bounds planted wherever the array has room.  -> (x, bounds)"""
    rng = np.random.default_rng(seed)
    start, end = -1.5, 2.25
    x = (rng.standard_normal((n, d)) * 1.5 + 0.3)
    flat = x.ravel()
    plant = SPECIALS + [start, end, start - 0.5, end + 0.5, start - 1e3, end + 1e3]
    pos = rng.permutation(flat.size)[:len(plant)]
    flat[pos] = plant[:len(pos)]
    return np.ascontiguousarray(x.astype(np.float16 if kind == "f16" else f32)), (start, end)
