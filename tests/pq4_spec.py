"""Specification and fixtures of the 4-bit IVF_PQ distance computation (tests/test_pq4_spec.py on the CPU, tests/test_zz_gpu_pq4.py on
the GPU).

The reference computes the distances of one (query, partition) pair in `compute_pq_distance_4bit` (pq/distance.rs:147-284):

  flat_num = max(200, min(k_hint, n)), at most n; k_hint = k * refine_factor (flat/index.rs:94)
  rows [0, flat_num)                     exact: the f32 table entries of the row added one by one, sub-vector order
  qmax                                   the largest exact distance of those rows by f32::total_cmp (a positive NaN is the largest)
  qmin                                   fold(INFINITY, f32::min) over the table: NaN entries are ignored
  quantised table                        ((entry - qmin) * (255 / (qmax - qmin))).round() as u8: half away from zero, saturating, NaN -> 0
  rows [flat_num, n - n % 16)            saturating u8 sum of the quantised entries, then q * ((qmax - qmin) / 255) + qmin, two roundings
  rows [max(n - n % 16, flat_num), n)    exact again (only when n % 16 != 0)
  dot                                    minus (M - 1) on every row, last (pq/storage.rs:949-957)

and, under a row-id prefilter, per selected row in `PQDistCalculator::distance` (pq/storage.rs:893-921): the unquantised table, one term per
code byte (entry[2i][low nibble] + entry[2i + 1][high nibble]), the terms folded from -0.0, dot minus (M - 1); k_hint plays no part.

`scan4` and `masked_rows` restate both in numpy, written from that text; `search` puts them into the per-partition heap / range / merge /
refine flow (the heap, the final sort and the table itself are the oracle's own entry points, tested elsewhere).  MUTANTS are single
plausible kernel mistakes of the same model; CAUGHT_BY names, for each, a case below whose answer it changes.

Fixtures are indices built from HAND-ASSIGNED partition ids (DeviceIndex.create groups rows stably, so the order inside a partition is the
input order and the fixture decides which rows are the exact head), seeded, d 16..128, at most about 4300 rows."""
import functools

import numpy as np

import oracle as O

f32 = np.float32
NOID = np.uint64(0xFFFFFFFFFFFFFFFF)
FLAT_NUM = 200

MUTANTS = ("flat_num_200", "k_hint_is_k", "wrapping_add", "tail_quantised", "tail_from_block_end", "round_half_even", "fused_dequantise",
           "qmax_over_all_rows", "nan_poisons_qmin", "bias_before_qmax", "prefilter_fast_scan")


# ---- the model -----------------------------------------------------------------------------------------------------------------------
def order_key(a):
    """f32::total_cmp as an unsigned key"""
    u = np.ascontiguousarray(a, f32).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000))


def entries(lut, codes_t):
    """lut [M][16], codes_t [M/2][n] packed (low nibble = sub-vector 2b, high = 2b + 1) -> the row's table entries [M][n]"""
    m = lut.shape[0]
    e = np.empty((m, codes_t.shape[1]), f32)
    e[0::2] = np.take_along_axis(lut[0::2], (codes_t & 15).astype(np.intp), axis=1)
    e[1::2] = np.take_along_axis(lut[1::2], (codes_t >> 4).astype(np.intp), axis=1)
    return e


def _sum_in_order(e, start):
    s = start
    for j in range(e.shape[0]):
        s = s + e[j]
    return s


def round_half_away(v):
    v = v.astype(np.float64)          # |v| + 0.5 is exact in f64 for every f32 v the conversion does not saturate anyway
    return np.copysign(np.floor(np.abs(v) + 0.5), v)


def saturate_u8(r):
    return np.clip(np.where(np.isnan(r), 0.0, r), 0.0, 255.0).astype(np.uint8)


class Scan:
    """distances of one partition and what the model did on the way"""

    def __init__(self, d, flat_num, tail_start, qmax, qmin, acc):
        self.d, self.flat_num, self.tail_start, self.qmax, self.qmin, self.acc = d, flat_num, tail_start, qmax, qmin, acc

    @property
    def quantised(self):
        """[start, end) of the rows that carry a de-quantised distance"""
        return self.flat_num, max(self.flat_num, len(self.d) - len(self.d) % 16)


def scan4(lut, codes_t, k_hint, metric="l2", mut=None):
    lut = np.ascontiguousarray(lut, f32).reshape(-1, 16)
    m, n = lut.shape[0], codes_t.shape[1]
    dot = metric == "dot"
    bias = f32(m) - f32(1.0)
    with np.errstate(all="ignore"):
        e = entries(lut, codes_t)
        flat_num = min(max(FLAT_NUM, min(k_hint, n)), n)
        if mut == "flat_num_200":
            flat_num = min(FLAT_NUM, n)
        d = np.zeros(n, f32)
        d[:flat_num] = _sum_in_order(e[:, :flat_num], np.zeros(flat_num, f32))
        if mut == "bias_before_qmax" and dot:
            d[:flat_num] = d[:flat_num] - bias
        head = d[:flat_num] if mut != "qmax_over_all_rows" else _sum_in_order(e, np.zeros(n, f32))
        qmax = head[int(np.argmax(order_key(head)))]
        qmin = np.minimum.reduce(lut.reshape(-1), initial=f32(np.inf)) if mut == "nan_poisons_qmin" else np.fmin.reduce(lut.reshape(-1), initial=f32(np.inf))
        qmin = f32(qmin)
        factor = f32(255.0) / (qmax - qmin)
        scaled = (lut - qmin) * factor
        qt = saturate_u8(np.rint(scaled.astype(np.float64)) if mut == "round_half_even" else round_half_away(scaled))
        qe = entries(qt, codes_t).astype(np.uint32)
        acc = np.zeros(n, np.uint32)
        for j in range(m):
            acc = (acc + qe[j]) & 255 if mut == "wrapping_add" else np.minimum(acc + qe[j], 255)
        rem = n % 16
        q_end = n if mut == "tail_quantised" else n - rem
        rng_ = (qmax - qmin) / f32(255.0)
        if q_end > flat_num:
            a = acc[flat_num:q_end].astype(f32)
            if mut == "fused_dequantise":
                d[flat_num:q_end] = (a.astype(np.float64) * np.float64(rng_) + np.float64(qmin)).astype(f32)
            else:
                d[flat_num:q_end] = a * rng_ + qmin
        tail_start = n
        if rem > 0 and mut != "tail_quantised":
            tail_start = n - rem if mut == "tail_from_block_end" else max(n - rem, flat_num)
            # compute_pq_distance_4bit_flat ADDS to what the slots hold: zero for rows past flat_num
            d[tail_start:] = _sum_in_order(e[:, tail_start:], d[tail_start:].copy() if tail_start < flat_num else np.zeros(n - tail_start, f32))
        if dot:
            if mut == "bias_before_qmax":
                d[flat_num:] = d[flat_num:] - bias
            else:
                d = d - bias
        acc = acc.astype(np.uint8)
    return Scan(d, flat_num, tail_start, qmax, qmin, acc)


def masked_rows(lut, codes_t, metric="l2"):
    """PQDistCalculator::distance for every row of the partition (the caller selects)"""
    lut = np.ascontiguousarray(lut, f32).reshape(-1, 16)
    with np.errstate(all="ignore"):
        e = entries(lut, codes_t)
        s = np.full(codes_t.shape[1], -0.0, f32)
        for b in range(lut.shape[0] // 2):
            s = s + (e[2 * b] + e[2 * b + 1])
        if metric == "dot":
            s = s - (f32(lut.shape[0]) - f32(1.0))
    return s


class Index:
    """an IVF_PQ index in the reference's layout (per-partition transposed codes) plus the columns DeviceIndex.create takes"""

    def __init__(self, metric, cent, cb, part, codes, nbits=4):
        self.metric, self.cent, self.cb, self.part, self.codes, self.nbits = metric, cent, cb, part, codes, nbits
        self.f16 = cent.dtype == np.float16
        nlist = cent.shape[0]
        self.offs, self.perm = O.partition_layout(part, nlist)
        cs = codes[self.perm]
        mb = codes.shape[1]
        self.codes_t = np.empty(cs.size, np.uint8)
        for p in range(nlist):
            a, b = int(self.offs[p]), int(self.offs[p + 1])
            self.codes_t[a * mb:b * mb] = np.ascontiguousarray(cs[a:b].T).reshape(-1)
        self.row_ids = self.perm.astype(np.uint64)
        self.mb = mb

    def partition(self, p):
        a, b = int(self.offs[p]), int(self.offs[p + 1])
        return self.codes_t[a * self.mb:b * self.mb].reshape(self.mb, b - a), self.row_ids[a:b]

    def oracle(self):
        return O.IvfPqIndex(self.metric, self.cent, self.cb, self.offs, self.codes_t, self.row_ids, f16=self.f16, nbits=self.nbits)


def search(ix, q, k, nprobes, refine=0, raw=None, prefilter=None, lower=None, upper=None, mut=None, info=None):
    """the reference's search of a 4-bit index with `scan4` / `masked_rows` as the distance computation.
    info: a dict that receives `scans` [(query, partition, Scan)] and `saturated` [set of row ids per query]"""
    assert ix.nbits == 4
    m = ix.cb.shape[0]
    et = np.float16 if ix.f16 else f32
    qs = np.ascontiguousarray(q, et).reshape(-1, ix.cent.shape[1])
    scan_metric = "l2" if ix.metric == "cosine" else ix.metric
    qn = O.normalize(qs) if ix.metric == "cosine" else qs
    nprobes = min(nprobes, ix.cent.shape[0])
    probes, _ = O.find_partitions(qn, ix.cent, nprobes, scan_metric)
    keff = k * (refine if refine else 1)
    has = lower is not None or upper is not None
    lo = f32(np.finfo(f32).min if lower is None else lower)
    hi = f32(np.finfo(f32).max if upper is None else upper)
    out_i = np.full((qs.shape[0], k), NOID, np.uint64)
    out_d = np.full((qs.shape[0], k), np.inf, f32)
    allow = None if prefilter is None else np.ascontiguousarray(prefilter, bool)
    cent32, cb32 = ix.cent.astype(f32), ix.cb.astype(f32)
    for qi in range(qs.shape[0]):
        ci, cd = [], []
        sat = set()
        for p in probes[qi]:
            codes_t, rids = ix.partition(int(p))
            if rids.size == 0:
                continue
            with np.errstate(all="ignore"):
                qr = qn[qi].astype(f32) - cent32[p] if scan_metric == "l2" else qn[qi].astype(f32)
                if ix.f16 and scan_metric == "l2":
                    qr = qr.astype(np.float16).astype(f32)      # arrow `sub` on Float16 (v2.rs:326)
                lut = O.build_lut(qr, cb32, scan_metric, nbits=4)
            if allow is not None:
                sel = (rids < allow.size) & allow[np.minimum(rids, max(allow.size, 1) - 1).astype(np.int64)]
                if mut == "prefilter_fast_scan":
                    d = scan4(lut, codes_t, keff, scan_metric).d[sel]
                else:
                    d = masked_rows(lut, codes_t, scan_metric)[sel]
                rids = rids[sel]
            else:
                s = scan4(lut, codes_t, k if mut == "k_hint_is_k" else keff, scan_metric, mut)
                d = s.d
                if info is not None:
                    info.setdefault("scans", []).append((qi, int(p), s))
                    a, b = s.quantised
                    sat.update(int(r) for r in rids[a:b][s.acc[a:b] == 255])
            hi_, hd_ = O.heap_topk(d, rids, keff, lo if has else None, hi if has else None)
            ci.append(hi_); cd.append(hd_)
        if info is not None:
            info.setdefault("saturated", []).append(sat)
        if not ci:
            continue
        si, sd = O.sort_fetch(np.concatenate(ci), np.concatenate(cd), keff)
        if refine and raw is not None:
            with np.errstate(all="ignore"):
                ex = O.distance_batch(ix.metric, qs[qi], raw[si.astype(np.int64)])
            if has:
                ok = (ex >= lo) & (ex < hi)
                si, ex = si[ok], ex[ok]
            si, sd = O.sort_fetch(si, ex, k)
        si, sd = si[:k], sd[:k]
        out_i[qi, :si.size] = si
        out_d[qi, :sd.size] = sd
    return out_i, out_d


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
GRID_SIZES = (1, 15, 16, 17, 199, 200, 201, 208, 215, 216, 217, 255, 256, 257, 1008, 1005, 0)     # 1005 % 16 = 13; one empty partition
KEFFS = (1, 10, 128, 129, 200, 201, 250, 300, 1000, 5000)                                             # 5000 is above every partition

# name -> (metric, d, M, dtype, sizes, layout, poison)
INDICES = {
    "l2-m32":      ("l2", 64, 32, "f32", GRID_SIZES, "gauss", None),          # d / M = 2; the largest M: the exact kernel's sweep
    "l2-m8":       ("l2", 32, 8, "f32", GRID_SIZES, "gauss", None),           # d / M = 4
    "l2-m2":       ("l2", 32, 2, "f32", (257, 1005, 216, 15), "gauss", None),  # d / M = 16
    "l2-m16":      ("l2", 128, 16, "f32", (257, 1005, 216, 15), "gauss", None),   # d / M = 8
    "cosine-m8":   ("cosine", 64, 8, "f32", (257, 1005, 216, 15, 208), "gauss", None),
    "dot-signs":   ("dot", 32, 16, "f32", GRID_SIZES, "unit", None),           # table entries of both signs
    "dot-low":     ("dot", 32, 8, "f32", (257, 1005, 216, 15), "bytes", None),     # components 0..218: every entry far below zero, qmax < qmin
    "near-head":   ("l2", 32, 8, "f32", (1008, 333, 208), "near_far", None),   # the 200 head rows beside the query, the rest far away: saturation
    "far-head":    ("l2", 32, 8, "f32", (1008, 333, 208), "far_near", None),   # the reverse: qmax large, the near rows spread over many levels
    "zero-cb":     ("l2", 16, 8, "f32", (257, 1005, 216), "gauss", "zero"),    # with the query on a centroid: qmax == qmin, factor inf
    "nan-codeword": ("l2", 16, 8, "f32", (257, 1005, 216), "gauss", "nan"),    # NaN entry met by rows past the head: quantised 0, exact tail NaN
    "nan-in-head": ("l2", 16, 8, "f32", (257, 1005, 216), "gauss", "nan-head"),     # ... and by a head row: qmax NaN
    "inf-codeword": ("l2", 16, 8, "f32", (257, 1005, 216), "gauss", "inf"),    # +inf entry met by rows past the head only (see poison())
    "halves":      ("l2", 16, 8, "f32", (257, 1005, 216), "int", "halves"),    # integer table, qmax - qmin = 510: entries land on exact halves
    "f16":         ("l2", 32, 8, "f16", (257, 1005, 216, 15), "gauss16", None),
}
POISON_SUB, POISON_CODE = 1, 5       # sub-vector 1 = the high nibble of code byte 0


class Fx(dict):
    __getattr__ = dict.__getitem__


def _rows_of(rng, layout, c, n, d):
    g = rng.standard_normal((n, d))
    if layout == "near_far":
        return c + g * np.where(np.arange(n) < FLAT_NUM, 0.5, 6.0)[:, None]
    if layout == "far_near":
        return c + g * np.where(np.arange(n) < FLAT_NUM, 1.6, 1.0)[:, None]
    if layout == "unit":
        return c + g * 0.5
    if layout == "bytes":
        return np.clip(np.rint(c * 20 + 100 + g * 20), 0, 218)
    if layout == "gauss16":
        return c * 0.7 + g * 0.7
    return c + g


def poison(codes, part, nlist, kind):
    """rows whose sub-vector POISON_SUB takes the poisoned codeword: position 205 (quantised), 230 and the last row (the exact tail where
    n % 16 != 0) of every partition above 216 rows; `nan-head` adds position 7.  Nobody else keeps that codeword.
    An inf entry stays out of the head on purpose: qmax = +inf makes range = inf and every quantised distance 0 * inf, a NaN the
    arithmetic GENERATES, whose sign is the host CPU's in the reference (x86: negative) -- nothing to compare."""
    hi = codes[:, 0] >> 4
    codes[:, 0] = np.where(hi == POISON_CODE, (codes[:, 0] & 15) | ((POISON_CODE + 1) << 4), codes[:, 0])
    for p in range(nlist):
        rows = np.flatnonzero(part == p)
        if rows.size <= 216:
            continue
        pos = [205, 230, rows.size - 1] + ([7] if kind == "nan-head" else [])
        codes[rows[pos], 0] = (codes[rows[pos], 0] & 15) | (POISON_CODE << 4)
    return codes


def halves(rng, part, nlist, d, m):
    """codebook and codes by hand (L2, d / M = 2): codeword c of every sub-vector is (c, 0), so a query ON its centroid has the table
    entry c * c.  Row 0 of a partition has the codes 15 15 6 4 2 2 0 0 = 510, every other head row stays below (codes 0..7): qmin 0,
    qmax 510, factor exactly 0.5 -- every odd c quantises from an exact half (0.5, 4.5, 12.5 ..).  Later rows: codes 0..9."""
    assert d == 16 and m == 8
    cb = np.zeros((m, 16, 2), f32)
    cb[:, :, 0] = np.arange(16, dtype=f32)[None, :]
    sub = np.empty((part.size, m), np.uint8)
    for p in range(nlist):
        rows = np.flatnonzero(part == p)
        sub[rows] = rng.integers(0, 10, (rows.size, m))
        sub[rows[:FLAT_NUM]] = rng.integers(0, 8, (min(rows.size, FLAT_NUM), m))
        if rows.size:
            sub[rows[0]] = (15, 15, 6, 4, 2, 2, 0, 0)
    return cb, (sub[:, 0::2] | (sub[:, 1::2] << 4)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def index_fixture(name, nbits=4):
    """-> Fx(ix: Index, x: the column (un-normalised), name, seed).  nbits = 8: an 8-bit index of the same rows and partitions."""
    metric, d, m, dtype, sizes, layout, kind = INDICES[name]
    seed = 1000 + sorted(INDICES).index(name)
    rng = np.random.default_rng(seed)
    nlist, n = len(sizes), int(sum(sizes))
    t = np.float16 if dtype == "f16" else f32
    cent = rng.standard_normal((nlist, d)) * (1.0 if layout in ("unit", "gauss16") else 3.0)
    part = rng.permutation(np.repeat(np.arange(nlist, dtype=np.uint32), sizes))
    x = np.empty((n, d), np.float64)
    for p in range(nlist):
        x[part == p] = _rows_of(rng, layout, cent[p], sizes[p], d)
    if metric == "cosine":
        x += 1.0
    x = x.astype(t)
    if layout == "bytes":
        cent = cent * 20 + 100
    if layout == "int":
        cent = np.rint(cent)
    cent = cent.astype(t)
    xs = O.normalize(x) if metric == "cosine" else x
    if metric == "cosine":
        cent = np.stack([xs[part == p].astype(np.float64).mean(0) if sizes[p] else cent[p] for p in range(nlist)]).astype(t)
    res = O.residual(xs, cent, part) if metric != "dot" else xs
    if kind == "zero":
        cb = np.zeros((m, 1 << nbits, d // m), t)
    else:
        cb = O.pq_train(res, m, nbits=nbits, max_iters=4, seed=seed + 1)[0].astype(t)
    codes = O.pq_encode(res, cb, "l2", nbits=nbits)
    if kind == "halves" and nbits == 4:
        cb, codes = halves(rng, part, nlist, d, m)
    if kind in ("nan", "nan-head", "inf") and nbits == 4:
        cb = cb.copy()
        cb[POISON_SUB, POISON_CODE, :] = np.inf if kind == "inf" else np.nan
        codes = poison(codes.copy(), part, nlist, kind)
    return Fx(name=name, seed=seed, x=x, ix=Index(metric, cent, cb, part, codes, nbits), layout=layout, sizes=sizes)


def queries(fx, nq, seed=0, special=None):
    """nq queries beside the centroids, partitions in turn (the empty one included).
    special: `centroid` -- the centroids themselves; `nan` -- query 1 carries a NaN component"""
    ix = fx.ix
    rng = np.random.default_rng(fx.seed * 7 + seed + nq)
    nlist, d = ix.cent.shape
    p = np.arange(nq) % nlist
    if fx.layout in ("near_far", "far_near"):
        p = np.zeros(nq, np.int64)             # all beside the 1008-row partition, whose head the layout arranges
    c = ix.cent[p].astype(np.float64)
    if special == "centroid":
        return ix.cent[p].copy()
    if fx.layout == "bytes":
        q = np.clip(np.rint(c + rng.standard_normal((nq, d)) * 20), 0, 218)
    elif fx.layout in ("near_far", "far_near"):
        q = c + rng.standard_normal((nq, d)) * 0.05
    elif ix.metric == "cosine":
        q = (c + rng.standard_normal((nq, d)) * 0.05) * 3.0
    else:
        q = c + rng.standard_normal((nq, d)) * (0.5 if fx.layout in ("unit", "gauss16") else 1.0)
    q = q.astype(ix.cent.dtype)
    if special == "nan":
        q[1, 3] = np.nan
    return q


def prefilter(fx, frac, seed=0):
    return np.random.default_rng(fx.seed * 13 + seed).random(fx.x.shape[0]) < frac


# ---- search cases ---------------------------------------------------------------------------------------------------------------------
# bounds: None, or (lower, upper) each one of
#   None           absent
#   ("at", j)      the oracle's own j-th returned distance of query 0 in the same search without a range: a row sits exactly on the bound
#   "inf"          +inf
#   "same"         (upper only) equal to lower: an empty range
# regime: conditions asserted on the model by tests/test_pq4_spec.py
def case(name, index, k, refine=0, nq=6, nprobes=None, frac=None, bounds=None, special=None, regime=()):
    return Fx(name=name, index=index, k=k, refine=refine, nq=nq, nprobes=nprobes, frac=frac, bounds=bounds, special=special, regime=tuple(regime))


CASES = [
    # k * refine across both kernels and both sides of flat_num = 200, on the largest M
    case("m32 k1", "l2-m32", 1),
    case("m32 k10", "l2-m32", 10),
    case("m32 k128", "l2-m32", 128),
    case("m32 k129", "l2-m32", 129),
    case("m32 k200", "l2-m32", 200),
    case("m32 k201", "l2-m32", 201, regime=("flat_num>200",)),
    case("m32 k250", "l2-m32", 250, regime=("flat_num>200", "tail_at_flat_num")),
    case("m32 60x5", "l2-m32", 60, refine=5, regime=("flat_num>200",)),
    case("m32 k1000", "l2-m32", 1000, regime=("flat_num>200", "tail_at_flat_num")),
    case("m32 k5000", "l2-m32", 5000),
    case("m32 10x5 few probes", "l2-m32", 10, refine=5, nprobes=3),
    # shapes
    case("m8 k10", "l2-m8", 10),
    case("m8 k250", "l2-m8", 250, regime=("flat_num>200",)),
    case("m2 k10", "l2-m2", 10),
    case("m2 k300", "l2-m2", 300, regime=("flat_num>200",)),
    case("m16 k10", "l2-m16", 10),
    case("m16 50x5", "l2-m16", 50, refine=5, regime=("flat_num>200",)),
    case("cosine k10", "cosine-m8", 10),
    case("cosine k128", "cosine-m8", 128),
    case("cosine 60x5", "cosine-m8", 60, refine=5, regime=("flat_num>200",)),
    # dot, both table regimes
    case("dot signs k10", "dot-signs", 10, regime=("both_signs",)),
    case("dot signs k250", "dot-signs", 250, regime=("both_signs", "flat_num>200")),
    case("dot signs 30x4", "dot-signs", 30, refine=4, regime=("both_signs",)),
    case("dot low k10", "dot-low", 10, regime=("qmax<qmin",)),
    case("dot low k300", "dot-low", 300, regime=("qmax<qmin", "flat_num>200")),
    # saturation and its reverse
    case("near head k10", "near-head", 10, nq=4),
    case("near head k128 above the head", "near-head", 128, nq=4, bounds=(("at", 120), None), regime=("saturated>=32", "on_lower")),
    case("near head k250", "near-head", 250, nq=4, regime=("flat_num>200",)),
    case("far head k10", "far-head", 10, nq=4, regime=("many_levels",)),
    case("far head k250", "far-head", 250, nq=4, regime=("flat_num>200",)),
    # degenerate tables
    case("exact halves", "halves", 10, nq=3, special="centroid", regime=("halves",)),
    case("zero codebook", "zero-cb", 10, special="centroid", regime=("qmax==qmin",)),
    case("nan codeword", "nan-codeword", 10),
    case("nan codeword k128", "nan-codeword", 128),
    case("nan in head", "nan-in-head", 10, regime=("qmax_nan",)),
    case("inf codeword", "inf-codeword", 10),
    case("nan query", "l2-m8", 10, special="nan"),
    # f16 column: the f16-rounded residual feeds the table
    case("f16 k10", "f16", 10),
    case("f16 k250", "f16", 250, regime=("flat_num>200",)),
    case("f16 20x3", "f16", 20, refine=3),
    # prefilter: the per-row arithmetic, which ignores k_hint
    case("prefilter 0.5 k10", "l2-m32", 10, frac=0.5),
    case("prefilter 0.5 k250", "l2-m32", 250, frac=0.5),
    case("prefilter 0.01 k250", "l2-m32", 250, frac=0.01),
    case("prefilter 0.5 60x5", "l2-m32", 60, refine=5, frac=0.5),
    case("prefilter 0.01 10x5", "l2-m32", 10, refine=5, frac=0.01),
    case("prefilter dot 0.5 k10", "dot-signs", 10, frac=0.5),
    case("prefilter dot 0.01 k250", "dot-signs", 250, frac=0.01),
    # ranges: rows exactly on the bounds
    case("range l2", "l2-m8", 20, bounds=(("at", 3), ("at", 12)), regime=("on_lower", "on_upper")),
    case("range l2 empty", "l2-m8", 20, bounds=(("at", 3), "same")),
    case("range l2 no lower", "l2-m8", 20, bounds=(None, ("at", 12)), regime=("on_upper",)),
    case("range l2 no upper", "l2-m8", 20, bounds=(("at", 3), None), regime=("on_lower",)),
    case("range l2 inf upper", "l2-m8", 20, bounds=(("at", 3), "inf"), regime=("on_lower",)),
    case("range l2 narrow", "l2-m8", 20, bounds=(("at", 3), ("at", 5)), regime=("on_lower", "on_upper", "fewer_than_k")),
    case("range l2 k250", "l2-m8", 250, bounds=(("at", 30), ("at", 200)), regime=("on_lower", "on_upper", "flat_num>200")),
    case("range l2 prefilter", "l2-m8", 20, frac=0.5, bounds=(("at", 3), ("at", 12)), regime=("on_lower", "on_upper")),
    case("range l2 refine", "l2-m8", 10, refine=4, bounds=(("at", 2), ("at", 8)), regime=("on_lower", "on_upper")),
    case("range dot negative", "dot-signs", 20, bounds=(("at", 3), ("at", 12)), regime=("on_lower", "on_upper", "negative_range")),
    case("range dot prefilter", "dot-signs", 20, frac=0.5, bounds=(("at", 3), ("at", 12)), regime=("on_lower", "on_upper")),
    case("range dot refine", "dot-signs", 10, refine=4, bounds=(("at", 2), ("at", 8)), regime=("on_lower", "on_upper")),
    case("range cosine", "cosine-m8", 20, bounds=(("at", 3), ("at", 12)), regime=("on_lower", "on_upper")),
    case("range cosine prefilter", "cosine-m8", 20, frac=0.5, bounds=(("at", 3), ("at", 12)), regime=("on_lower", "on_upper")),
    case("range cosine refine", "cosine-m8", 10, refine=4, bounds=(("at", 2), None), regime=("on_lower",)),      # ADC = L2 of unit rows, about twice the exact cosine distance: an upper bound from the exact scale would cut on the ADC side
]
CASE = {c.name: c for c in CASES}
RANGE_CASES = [c.name for c in CASES if c.bounds is not None and c.index != "near-head"]

# mutant -> the case whose answer it changes (tests/test_pq4_spec.py checks each)
CAUGHT_BY = {
    "flat_num_200": "m32 k250",
    "k_hint_is_k": "m16 50x5",
    "wrapping_add": "near head k10",
    "tail_quantised": "m2 k10",
    "tail_from_block_end": "m32 k1000",
    "round_half_even": "exact halves",
    "fused_dequantise": "m8 k250",
    "qmax_over_all_rows": "m8 k250",
    "nan_poisons_qmin": "nan codeword",
    "bias_before_qmax": "dot signs k250",
    "prefilter_fast_scan": "prefilter 0.5 k10",
}


def case_inputs(c):
    """-> (fixture, queries, nprobes, prefilter mask or None)"""
    fx = index_fixture(c.index)
    q = queries(fx, c.nq, special=c.special)
    nprobes = fx.ix.cent.shape[0] if c.nprobes is None else c.nprobes
    allow = None if c.frac is None else prefilter(fx, c.frac)
    return fx, q, nprobes, allow


def resolve_bounds(c, unranged_d):
    """the case's (lower, upper) as f32 or None, from the distances of the same search without a range"""
    if c.bounds is None:
        return None, None

    def one(b, lower):
        if b is None:
            return None
        if b == "inf":
            return f32(np.inf)
        if b == "same":
            return lower
        return f32(unranged_d[0, b[1]])

    lo = one(c.bounds[0], None)
    return lo, one(c.bounds[1], lo)
