"""Shared by tests/test_flat_range_spec.py (CPU) and tests/test_zz_gpu_flat_range.py (GPU): the CPU specification of the flat scan's
distance range, the wrong models a fixture must tell it from, numpy models of the two-sided surrogate test of the two
matrix-core filters, and the fixtures of both files.

The specification (Scanner::flat_knn, rust/lance/src/dataset/scanner.rs:3336-3412: KNNVectorDistanceExec ->
LanceFilterExec(_distance >= lower AND _distance < upper) -> SortExec(_distance, _rowid).fetch(k)):
    every row    oracle.flat_knn(x, q, k = n): all rows in (distance, row id) order with the exact bits of the un-ranged scan
    keep         lo_key <= key(d) < hi_key on the total-order keys (IEEE 754 totalOrder, f32::total_cmp): -NaN < -inf < .. < -0 < +0
                 < .. < +inf < +NaN.  An ABSENT bound is no test: it is not -FLT_MAX / FLT_MAX
    take k, pad  id 2^64 - 1, distance +inf (flat_knn's padding)
Multivector columns: the same on tests/multivec_spec.py's distances."""
import functools

import numpy as np

import flat_order_spec as S
import magnitude_spec as M
import multivec_spec as MV

f32 = np.float32
UNSET = np.uint64(0xFFFFFFFFFFFFFFFF)
FLT_MAX = float(np.finfo(f32).max)
NEG_NAN_BITS = 0xFFC00000


def key(v):
    return int(S.keys(np.asarray([v], f32))[0])


# ---- the specification ---------------------------------------------------------------------------------------------------------------
def in_range(dist, lower, upper):
    k = S.keys(dist)
    ok = np.ones(k.shape, bool)
    if lower is not None:
        ok &= k >= np.uint32(key(lower))
    if upper is not None:
        ok &= k < np.uint32(key(upper))
    return ok


def in_range_closed_upper(dist, lower, upper):
    """WRONG: d <= upper"""
    k = S.keys(dist)
    ok = np.ones(k.shape, bool)
    if lower is not None:
        ok &= k >= np.uint32(key(lower))
    if upper is not None:
        ok &= k <= np.uint32(key(upper))
    return ok


def in_range_open_lower(dist, lower, upper):
    """WRONG: d > lower"""
    k = S.keys(dist)
    ok = np.ones(k.shape, bool)
    if lower is not None:
        ok &= k > np.uint32(key(lower))
    if upper is not None:
        ok &= k < np.uint32(key(upper))
    return ok


def in_range_ieee(dist, lower, upper):
    """WRONG: the IEEE comparison of the values (a NaN is in no range, -0 == +0) instead of the total order"""
    d = np.asarray(dist, f32)
    ok = np.ones(d.shape, bool)
    with np.errstate(invalid="ignore"):
        if lower is not None:
            ok &= d >= f32(lower)
        if upper is not None:
            ok &= d < f32(upper)
    return ok


def _pad(ids, d, k):
    pad = k - ids.size
    if pad > 0:
        ids = np.concatenate([ids, np.full(pad, UNSET)])
        d = np.concatenate([d, np.full(pad, np.inf, f32)])
    return ids, d


def select(all_ids, all_d, k, lower, upper, keep=in_range):
    """all_ids / all_d [nq][n]: every row in (distance, row id) order -> (ids [nq][k] uint64, distances [nq][k])"""
    nq = all_ids.shape[0]
    ids = np.empty((nq, k), np.uint64)
    d = np.empty((nq, k), f32)
    for i in range(nq):
        ok = keep(all_d[i], lower, upper)
        ids[i], d[i] = _pad(all_ids[i][ok][:k], all_d[i][ok][:k], k)
    return ids, d


def post_filtered(all_ids, all_d, k, lower, upper):
    """WRONG: the in-range part of the un-ranged top k"""
    nq = all_ids.shape[0]
    ids = np.empty((nq, k), np.uint64)
    d = np.empty((nq, k), f32)
    for i in range(nq):
        ti, td = all_ids[i][:k], all_d[i][:k]
        ok = in_range(td, lower, upper)
        ids[i], d[i] = _pad(ti[ok], td[ok], k)
    return ids, d


def every_row(oracle, x, q, metric, row_ids=None):
    """(ids [nq][n], distances [nq][n]): the un-ranged scan's answer with k = n"""
    n = len(x)
    nq = np.asarray(q).reshape(-1, np.asarray(x).shape[1]).shape[0]
    if n == 0:
        return np.empty((nq, 0), np.uint64), np.empty((nq, 0), f32)
    return oracle.flat_knn(x, q, n, metric, row_ids=row_ids)


def flat_knn(oracle, x, q, k, metric, lower, upper, row_ids=None):
    return select(*every_row(oracle, x, q, metric, row_ids), k, lower, upper)


WRONG = {
    "post_filter": post_filtered,
    "closed_upper": lambda ai, ad, k, lo, hi: select(ai, ad, k, lo, hi, keep=in_range_closed_upper),
    "open_lower": lambda ai, ad, k, lo, hi: select(ai, ad, k, lo, hi, keep=in_range_open_lower),
    "ieee": lambda ai, ad, k, lo, hi: select(ai, ad, k, lo, hi, keep=in_range_ieee),
}


def same(a, b):
    return bool((a[0] == b[0]).all() and (a[1].view(np.uint32) == b[1].view(np.uint32)).all())


def differs_per_query(a, b):
    return (a[0] != b[0]).any(axis=1) | (a[1].view(np.uint32) != b[1].view(np.uint32)).any(axis=1)


def multivec_topk(dist, k, lower, upper, rid=None):
    """the multivector spec: MV.distances' [n_rows] -> the k nearest in-range rows, padded"""
    rid = np.arange(dist.size, dtype=np.uint64) if rid is None else np.asarray(rid, np.uint64)
    ok = in_range(dist, lower, upper)
    return MV.topk(dist[ok], k, rid[ok])


# ---- numpy models of the two-sided surrogate tests -------------------------------------------------------------------------------------
E12 = f32(0.000244140625)       # 2^-12
DOT_ULP = f32(4.7683716e-7)     # 2^-22
FW_EW, FW_EWC = f32(0.0084), f32(0.0085)


def _split3_dot(x, q):
    """x.q on the two-term bf16 split of both operands (hi.hi + hi.lo + lo.hi in f32), as magnitude_spec.flat_filter_model forms it"""
    xh, qh = M.bf16_rne(x), M.bf16_rne(q)
    xl, ql = M.bf16_rne(x - xh), M.bf16_rne(q - qh)
    dot = qh @ xh.T
    dot = dot + qh @ xl.T
    return dot + ql @ xh.T


def short_row_model(x, q, T, lower, metric="l2", guard=True):
    """-> (queued [nq][n], lower_rejected [nq][n]) of flat_mfma.hip's LOWER filter against the thresholds T [nq] and the bound `lower`.
    Upper side: magnitude_spec.flat_filter_model (L2) / its dot form.  Lower side: a pair is rejected when
    fma(-mul, x.q, lq - xlo) > 0, i.e. s + E < lower with E = 2^-12 (|x|^2 + |q|^2) (dot: + 2^-22); a bound that is not finite and a
    pair outside the margin's validity (guard) reject nothing."""
    x, q, T = np.asarray(x, f32), np.asarray(q, f32), np.asarray(T, f32)
    with np.errstate(all="ignore"):
        dot = _split3_dot(x, q).astype(np.float64)
        xn = (x * x).sum(axis=1, dtype=f32)
        qn = (q * q).sum(axis=1, dtype=f32)
        if metric == "l2":
            up = M.flat_filter_model(x, q, T, guard)
            xlo = xn + E12 * xn
            lq = f32(lower) - (qn + E12 * qn)
            sl = (2.0 * dot + (lq[:, None] - xlo[None, :]).astype(np.float64)).astype(f32)
        else:
            xk1 = f32(1) + (-E12 * xn)
            tq = T + E12 * qn + DOT_ULP
            s = (-dot + (xk1[None, :] - tq[:, None]).astype(np.float64)).astype(f32)
            up = s <= 0
            xlo = f32(1) + E12 * xn
            lq = f32(lower) - E12 * qn - DOT_ULP
            sl = (dot + (lq[:, None] - xlo[None, :]).astype(np.float64)).astype(f32)
        rej = sl > 0
        if not np.isfinite(f32(lower)):
            rej[:] = False
        if guard:
            E = E12 * (xn[None, :] + qn[:, None])
            free = ~(E > f32(2.0 ** M.GUARD_LOG2)) | ~np.isfinite(E)
            up = up | free
            rej = rej & ~free
    return up & ~rej, rej


def long_row_model(x, q, T, lower, metric="l2"):
    """-> (queued, lower_rejected) of flat_mfma_wide.hip's LOWER filter: ONE bf16 product, margins EW (|x|^2 + |q|^2) (L2, dot) and
    EWC |x| |q| (cosine); the mirrored tests of the file's header."""
    x, q, T = np.asarray(x, f32), np.asarray(q, f32), np.asarray(T, f32)
    lower = f32(lower)
    with np.errstate(all="ignore"):
        dot = (M.bf16_rne(q).astype(np.float64) @ M.bf16_rne(x).astype(np.float64).T).astype(f32)
        xn = (x * x).sum(axis=1, dtype=f32)
        qn = (q * q).sum(axis=1, dtype=f32)
        if metric == "cosine":
            sx, sq = np.sqrt(xn), np.sqrt(qn)
            up = ((f32(1) - FW_EWC - T) * sq)[:, None] * sx[None, :] - dot <= 0
            rej = dot - ((f32(1) + FW_EWC - lower) * sq)[:, None] * sx[None, :] > 0
        elif metric == "dot":
            up = (f32(1) - FW_EW * xn)[None, :] - (T + FW_EW * qn + DOT_ULP)[:, None] - dot <= 0
            rej = dot - (((f32(1) - lower) + FW_EW * qn + DOT_ULP)[:, None] + (FW_EW * xn)[None, :]) > 0
        else:
            up = f32(-2) * dot + ((xn - FW_EW * xn)[None, :] - (T - (qn - FW_EW * qn))[:, None]) <= 0
            rej = f32(2) * dot - (((qn + FW_EW * qn) - lower)[:, None] + (xn + FW_EW * xn)[None, :]) > 0
        if not np.isfinite(lower):
            rej[:] = False
    return up & ~rej, rej


# ---- the epoch schedule of flat_topk_v2 under a lower bound (flat.hip: FLAT_LO_FIRST_ROWS, FLAT_LO_MIN_ROWS) ------------------------------------
POOL_CAP, QUEUE_CAP, LO_FIRST_ROWS, LO_MIN_ROWS = 4096, 2048, 2048, 16384


def sized_schedule(n, k, fill_of):
    """-> (epochs [(r0, r1, "exact" | "mc", fullest queue or None)], fell_back).  The un-ranged schedule (2048 rows, then growing by
    POOL_CAP / 16k, no small tail), with every matrix-core epoch cut to `rows` and `rows` set after it to what fills the queues by half
    (fill_of(r0, r1) = the fullest queue of that epoch); an epoch that would fall under LO_MIN_ROWS sends the rest to the exact filter."""
    growth = max(2, POOL_CAP // (16 * k))
    seen, mc, rows, fell_back, epochs = 0, True, LO_FIRST_ROWS, False, []
    while seen < n:
        want = POOL_CAP // 2 if seen == 0 else seen * (growth - 1)
        r0, r1 = seen, min(n, seen + max(want, 1))
        if n - r1 < (r1 - r0) // 4:
            r1 = n
        sized = mc and seen > 0 and seen >= k
        if sized and r1 - r0 > rows:
            r1 = r0 + rows
        fill = int(fill_of(r0, r1)) if sized else None
        epochs.append((r0, r1, "mc" if sized else "exact", fill))
        seen = r1
        if sized and seen < n:
            nxt = (r1 - r0) * (QUEUE_CAP // 2) // max(fill, 1)
            if nxt < LO_MIN_ROWS:
                mc, fell_back = False, True
            else:
                rows = min(nxt, 1 << 24)
    return epochs, fell_back


def model_fill(x, q, dist, lower, k, model, reject=True, **kw):
    """fill_of for sized_schedule from a filter model: T = each query's k-th in-range distance among the rows seen (dist [nq][row]);
    reject = False: the one-sided filter (what a build without the lower-side reject queues)"""
    def fill_of(r0, r1):
        T = np.full(len(q), np.inf, f32)
        for i in range(len(q)):
            seen = np.sort(dist[i, :r0][in_range(dist[i, :r0], lower, None)])
            if seen.size >= k:
                T[i] = seen[k - 1]
        return model(x[r0:r1], q, T, lower if reject else -np.inf, **kw)[0].sum(axis=1).max()
    return fill_of


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------
def spectrum(d, strong=4.0, count=16):
    """per-dimension scales of the main fixtures: sixteen strong directions, the rest weak -- the decaying spectrum of an embedding.
    The distances then spread widely against the norms, which is what lets a guard-banded surrogate decide most pairs"""
    s = np.ones(d, f32)
    s[:min(count, d // 2)] = strong
    return s


@functools.lru_cache(maxsize=None)
def main_fixture(d, n=20000, nq=130, seed=7, strong=4.0, count=16):
    """the matrix-core shapes of the issue: nq >= 128 queries over 20,000 rows (epochs: 2048 exact, the rest on the matrix cores)"""
    rng = np.random.default_rng(seed + d)
    sc = spectrum(d, strong, count)
    x = rng.standard_normal((n, d), dtype=f32) * sc
    q = rng.standard_normal((nq, d), dtype=f32) * sc
    return x, q


def long_fixture():
    """d = 256 for the long-row filter, whose single bf16 product has a guard band thirty times wider than the bf16x3 one: four
    directions at 32 spread the distances far enough that the band around the median holds ~2 % of the rows.  With sixteen directions
    at 4 it holds 5-8 %, next to the point (one row in sixteen) where flat_topk_v2 hands the column to the exact filter"""
    return main_fixture(256, nq=128, strong=32.0, count=4)


def all_distances(oracle, x, q, metric):
    """(ids, distances in (distance, row id) order, distances by row [nq][n], the median of all of them)"""
    ai, ad = every_row(oracle, x, q, metric)
    dist = np.empty_like(ad)
    np.put_along_axis(dist, ai.astype(np.int64), ad, axis=1)
    return ai, ad, dist, float(np.median(ad))


@functools.lru_cache(maxsize=None)
def tie_fixture(n=6000, d=8, nq=5, seed=3):
    """small integers: exact distances, hundreds of rows tied at every value -- rows exactly on either bound, ties across position k"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (n, d)).astype(f32)
    q = rng.integers(-2, 3, (nq, d)).astype(f32)
    return x, q


def specials(x, seed=11):
    """a copy of x (f32, d >= 8, n >= 64) with, at random positions, rows whose L2 distance is +inf (an element 3e38: the square
    overflows), the positive NaN (a canonical np.nan element), the NEGATIVE NaN (an element with bits 0xFFC00000: handed on with its
    sign, the row sorts first) -- no NaN that arithmetic generates (inf - inf), whose sign belongs to the host CPU.
    -> (x, {"inf": rows, "pos_nan": rows, "neg_nan": rows})"""
    x = np.array(x, f32)
    rng = np.random.default_rng(seed)
    p = rng.permutation(len(x))[:24]
    rows = {"inf": p[:8], "pos_nan": p[8:16], "neg_nan": p[16:]}
    cols = rng.integers(0, x.shape[1], 24)
    x[rows["inf"], cols[:8]] = 3e38
    x[rows["pos_nan"], cols[8:16]] = np.nan
    x.view(np.uint32)[rows["neg_nan"], cols[16:]] = NEG_NAN_BITS
    return x, rows


def zero_sign_fixture(n=5000, d=8, seed=13):
    """L2 rows equal to a query: distance +0.0 exactly.  No metric here produces -0.0 (sums of squares, 1 - s), so the sign of zero
    shows on the BOUNDS: lower = +0.0 keeps the +0.0 rows and upper = +0.0 drops them; (-0.0, +0.0) is a legal range that holds
    only -0.0 (nothing here); (+0.0, -0.0) has its lower bound ABOVE its upper bound in the total order and is refused -- under the
    IEEE comparison both are the empty range lower == upper.  in_range on the literal array [-0.0, +0.0] pins the row side."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, (n, d)).astype(f32)
    q = x[[17, 170, 1700]].copy()
    return x, q


def duplicates_fixture(d=8):
    """the repair loop: 2048 far rows (the first epoch), then 4200 copies of one vector, all nearer than the far rows' k-th and all
    at the SAME distance from each of the three queries (q = dup +- a unit step: L2 distance 1 exactly), and 40 copies of the
    queries themselves (distance 0, below the bound).  With lower = 1 the 4200 ties are in range and overflow a pool of 4096."""
    rng = np.random.default_rng(17)
    far = rng.integers(20, 40, (2048, d)).astype(f32)
    dup = np.zeros((1, d), f32)
    q = np.zeros((3, d), f32)
    q[0, 0], q[1, 1], q[2, 2] = 1.0, -1.0, 1.0
    near = np.repeat(q, 14, axis=0)[:40]
    x = np.concatenate([far, np.repeat(dup, 4200, axis=0), near]).astype(f32)
    return x, q
