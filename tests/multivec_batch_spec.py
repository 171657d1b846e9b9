"""Shared by tests/test_multivec_batch_spec.py (CPU) and tests/test_zz_gpu_multivec_batch.py (GPU): the specification of a BATCH of
multivector queries (lance_hip_flat_multivec_topk_batch, lance_amd/csrc/multivec_batch.hip) and a numpy model of its matrix-core filter.

The specification of a batch is the single query's, per query: multivec_spec.topk(multivec_spec.distances(...)).

The model restates the filter of multivec_batch.hip's header:
    x^      = x / sqrt(sum x^2) in f32; a vector that is not finite, whose norm is not above 2^-50 or whose squared norm is not below
              2^126 is stored as zeros and makes its row (its query) DEGENERATE
    hi, lo  = bf16_rne(x^), bf16_rne(x^ - hi)                     the operand split, held exactly
    sim~    = hi.hi + hi.lo + lo.hi                               in f64 here (the matrix pipe's own rounding is the margin's term (c))
    D~      = 1 - sum_i max_j sim~(i, j)                          maxima and sum in f32, the sum piece by piece as the kernel takes it
    margin  = E(nqv, K) = nqv EP(K) + (nqv + 1)(nqv + 3) 2^-23,   EP(K) = 3.002 * 2^-16 + (9.2 K + 20) 2^-24 + 2^-30,
              K = the power of two >= max(d, 16); EP's terms one by one in `terms`
    t       = the k-th smallest D~ over the non-degenerate rows (+inf when there are fewer)
    survivors = {D~ <= t + 2 E} and the degenerate rows
The mutants of test_multivec_batch_spec.py are this model with one term or rule changed."""
import numpy as np

import multivec_spec as M

S = M.S
f32, f64 = np.float32, np.float64
U = 2.0 ** -24
MV_SEL = 2048            # capacity of a query's survivor list
CHUNK_Q, CHUNK_COLS = 64, 2048
MAX_D = 256              # the largest d the filter serves
TINY, HUGE = 2.0 ** -50, 2.0 ** 126


def kpad(d):
    k = 16
    while k < d:
        k *= 2
    return k


def terms(d, operand=3.002, accumulation=True):
    """EP(K) term by term: (b) the operand split, (c) the matrix pipe's accumulation, (a) + (d) the normalisations and the exact
    side's own f32 arithmetic, (e) underflow"""
    K = kpad(d)
    return {"operands": operand * 2.0 ** -16, "accumulation": 6.2 * K * U if accumulation else 0.0, "f32_sides": (3.0 * K + 20.0) * U,
            "underflow": 2.0 ** -30}


def margin(nqv, d, operand=3.002, accumulation=True, nqv_factor=True):
    ep = sum(terms(d, operand, accumulation).values())
    return (nqv if nqv_factor else 1) * ep + (nqv + 1.0) * (nqv + 3.0) * 2.0 ** -23


def margin_f32(nqv, d):
    """E as the library rounds it: up to f32"""
    return np.nextafter(f32(margin(nqv, d)), f32(np.inf))


def bf16_rne(x):
    u = np.ascontiguousarray(x, f32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(f32)


def split(v):
    """[n][d] -> (x^ f32, hi, lo, ok [n])"""
    x = np.asarray(v).astype(f32)
    with np.errstate(all="ignore"):
        s = (x * x).sum(axis=1, dtype=f32)
        n = np.sqrt(s)
        ok = (n > f32(TINY)) & (s < f32(HUGE))
        xn = np.where(ok[:, None], x / np.where(ok, n, f32(1))[:, None], f32(0)).astype(f32)
    hi = bf16_rne(xn)
    lo = bf16_rne(xn - hi)
    return xn, hi, lo, ok


def kept_products(hi, lo, qh, ql):
    """the three products the kernel keeps, exact in f64 -> [n][nqv]"""
    hi, lo, qh, ql = (a.astype(f64) for a in (hi, lo, qh, ql))
    return hi @ qh.T + hi @ ql.T + lo @ qh.T


def pipe_truncating(hi, lo, qh, ql):
    """a matrix pipe that rounds every partial sum toward zero in f32, the products in the kernel's order: a stand-in for `whatever it
    rounds inside` -> [n][nqv] f32"""
    acc = np.zeros((hi.shape[0], qh.shape[0]), f64)

    def add(a, b):
        nonlocal acc
        t = acc + np.outer(a.astype(f64), b.astype(f64))
        r = t.astype(f32)
        r = np.where(np.abs(r.astype(f64)) > np.abs(t), np.nextafter(r, f32(0)), r)
        acc = r.astype(f64)
    for e in range(hi.shape[1]):
        add(lo[:, e], qh[:, e]); add(hi[:, e], ql[:, e]); add(hi[:, e], qh[:, e])
    return acc.astype(f32)


def surrogate(values, offsets, q, col0=0, pipe=None):
    """-> (D~ [n_rows] f32, degenerate rows [n_rows] bool, the query is degenerate).  col0: the query's first column in its chunk
    (the sum is taken piece by piece, the pieces end at multiples of 32 columns)"""
    offsets = np.asarray(offsets, np.int64)
    _, hi, lo, okx = split(values)
    _, qh, ql, okq = split(q)
    sim = (pipe(hi, lo, qh, ql) if pipe else kept_products(hi, lo, qh, ql)).astype(f32)
    best = np.maximum.reduceat(sim, offsets[:-1], axis=0)            # [rows][nqv]
    s = np.zeros(best.shape[0], f32)
    i = 0
    while i < best.shape[1]:
        e = min(best.shape[1], (col0 + i) // 32 * 32 + 32 - col0)
        p = np.zeros(best.shape[0], f32)
        for c in range(i, e):
            p = p + best[:, c]
        s = s + p
        i = e
    assert s.dtype == f32
    return f32(1) - s, ~np.logical_and.reduceat(okx, offsets[:-1]), not bool(okq.all())


def threshold(dt, degen, k):
    good = np.sort(dt[~degen].astype(f32))
    return f32(np.inf) if good.size < k else good[k - 1]


def survivors(dt, degen, k, e, slack=2.0, degenerate_in_t=False):
    """the rows the filter hands to the exact evaluation -> bool [n_rows]"""
    t = threshold(dt, np.zeros_like(degen) if degenerate_in_t else degen, k)
    with np.errstate(all="ignore"):
        thr = f32(t + f32(slack * e)) if np.isfinite(t) else f32(np.inf)
    return degen | ~(dt > thr)


def superset_count(dist, degen, k, e):
    """rows with D_spec <= t_spec + 4 E, and the degenerate rows: no filter within the margin evaluates more (|D~ - D| <= E)"""
    t = threshold(dist, degen, k)
    with np.errstate(all="ignore"):
        return int((degen | ~(dist.astype(f64) > f64(t) + 4.0 * f64(e))).sum())


def batch_spec(oracle, values, offsets, queries, k, metric="cosine", rid=None):
    """the specification of a batch: per query -> (ids [B][k] uint64, dists [B][k] f32, the distances [B][n_rows])"""
    out = [M.distances(oracle, values, offsets, q, metric) for q in queries]
    tk = [M.topk(d, k, rid) for d in out]
    return np.stack([t[0] for t in tk]), np.stack([t[1] for t in tk]), np.stack(out)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
def queries(nqvs, d, seed, kind="f32"):
    """a batch: one [nqv][d] array per entry of nqvs, in the style of multivec_spec.column"""
    out = []
    for i, n in enumerate(nqvs):
        out.append((S.real_f32 if kind == "f32" else S.real_f16)(1, d, n, seed + 31 * i)[1])
    return out


def adversarial(nqv=8, d=16):
    """A unit vector u whose first d - 1 elements sit just under half an ulp of the kept bits from their bf16 neighbour -- u_i =
    2^-2 + lo, lo = 2^-10 - 2^-17 + 2^-19 (1 - 2^-3): hi = 2^-2 drops lo, and lo itself lies 2^-19 (1 - 2^-3) above ITS bf16
    neighbour -- with a last element that brings the f32 norm to 1; every error has the sign of the (positive) product, so they add.
    The column: row 0 = [u], then rows of ordinary vectors; the query: nqv copies of u (cosine 1 with row 0)."""
    lo = 2.0 ** -10 - 2.0 ** -17 + 2.0 ** -19 * (1 - 2.0 ** -3)
    u = np.full(d, f32(0.25 + lo), f32)
    u[-1] = f32(np.sqrt(1.0 - float((u[:-1].astype(f64) ** 2).sum())))
    rest = S.real_f32(12, d, 1, 99)[0]
    values = np.concatenate([u[None, :], rest]).astype(f32)
    off = np.array([0, 1, 4, 8, 13], np.int64)
    return values, off, np.repeat(u[None, :], nqv, 0).astype(f32)
