"""Shared by tests/test_sq_spec.py (CPU) and tests/test_zz_gpu_sq.py (GPU): the CPU specification of 8-bit scalar quantisation and
of the IVF_SQ search, in numpy, composed with the oracle's existing functions for the IVF side, and the fixtures of both files.

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


def search(oracle, codes, part_ids, centroids, q, k, nprobes, metric, start, end, row_ids=None, prefilter=None):
    """codes [n][d] in input order; part_ids [n] (NONE = dropped); q raw queries in the column's element type"""
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
            dist = scale(int_sums(codes[rows], qc[qi], metric), metric, start, end)
            hi, hd = oracle.heap_topk(dist, rid[rows], k)
            ci.append(hi); cd.append(hd)
        if ci:
            si, sd = oracle.sort_fetch(np.concatenate(ci), np.concatenate(cd), k)
            out_i[qi, :len(si)] = si; out_d[qi, :len(sd)] = sd
    return out_i, out_d


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
