"""Shared by tests/test_multivec_spec.py (CPU) and tests/test_zz_gpu_multivec.py (GPU): the CPU specification of the multivector
(late-interaction) distance and its flat KNN, composed from the oracle's existing functions, and the fixtures of both files.

The specification (lance-linalg distance.rs:107-206 multivec_distance / multivec_distance_impl, lance-index flat.rs:129-133), for a
query of nqv vectors q_i and a row of L >= 1 vectors v_j, every operation one f32 rounding:
    sim(i, j)  = 1 - dist(q_i, v_j)       dist = oracle.distance_batch: l2 | 1 - dot | cosine (x = the query vector); Float16 columns take
                                          half::f16's own arms (the oracle's DOT_H / COSINE_H) as every f16 column does
    best_i     = max_j sim(i, j)          by f32::total_cmp: a segmented max on the total-order keys (the positive NaN is the maximum)
    s          = ((0 + best_0) + best_1) + ...   sequentially, in query-vector order (Iterator::sum)
    distance   = 1 - s                    not nqv - s
    top k      = ascending (distance by total_cmp, row id): a stable sort by (key, row id), the flat scan's order.

The fixtures are real-valued in the style of tests/flat_order_spec.py (standard_normal * 3 in f32, * 0.7 in f16: every partial sum
inexact, no two vectors equal), with random row lengths and permuted row ids unrelated to the storage order."""
import numpy as np

import flat_order_spec as S

f32 = np.float32
NAN_BITS = 0x7FC00000          # the canonical positive NaN (np.nan as f32)


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
def lengths(n_rows, lo, hi, seed):
    return np.random.default_rng(seed).integers(lo, hi + 1, n_rows).astype(np.int64)


def offsets_of(lens):
    off = np.zeros(len(lens) + 1, np.int64)
    off[1:] = np.cumsum(lens)
    return off


def column(lens, d, nqv, seed, kind="f32"):
    """(values [sum lens][d], offsets [rows + 1], q [nqv][d]); kind "f32": standard_normal * 3, "f16": * 0.7 rounded to binary16
    (the query of a Float16 column is f16 too)"""
    off = offsets_of(lens)
    values, q = (S.real_f32 if kind == "f32" else S.real_f16)(int(off[-1]), d, nqv, seed)
    return values, off, q


def row_ids(n_rows, seed):
    return np.random.default_rng(seed).permutation(n_rows).astype(np.uint64) * 3 + 5


# ---- the specification --------------------------------------------------------------------------------------------------------
def key_to_f32(keys):
    k = np.ascontiguousarray(keys, np.uint32)
    return np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32).view(f32)


def maxima(oracle, values, offsets, q, metric):
    """best[i][r] = max_j (1 - dist(q_i, v_{r,j})) by total_cmp -> [nqv][n_rows] f32"""
    offsets = np.asarray(offsets, np.int64)
    assert (np.diff(offsets) > 0).all(), "the specification has no value for an empty row (the reference unwraps a None)"
    out = np.empty((len(q), len(offsets) - 1), f32)
    for i, qi in enumerate(q):
        sim = f32(1) - oracle.distance_batch(metric, qi, values)
        assert sim.dtype == f32
        out[i] = key_to_f32(np.maximum.reduceat(S.keys(sim), offsets[:-1]))
    return out


def sum_sequential(best):
    s = np.zeros(best.shape[1], f32)
    for b in best:
        s = s + b
    assert s.dtype == f32
    return s


def sum_pairwise(best):
    """a WRONG order: the same maxima added as a tree (what a cross-lane reduction would do)"""
    p = best
    while p.shape[0] > 1:
        if p.shape[0] % 2:
            p = np.concatenate([p, np.zeros((1, p.shape[1]), f32)])
        p = p[0::2] + p[1::2]
    return p[0]


def distances(oracle, values, offsets, q, metric):
    """multivec_distance of the query to every row -> [n_rows] f32"""
    return f32(1) - sum_sequential(maxima(oracle, values, offsets, q, metric))


def distances_per_pair(oracle, values, offsets, q, metric):
    """the same from the oracle's one-pair functions (l2 / 1 - dot / cosine), pair by pair: small inputs only"""
    offsets = np.asarray(offsets, np.int64)
    out = np.empty(len(offsets) - 1, f32)
    for r in range(len(out)):
        s = f32(0)
        for qi in q:
            best = None
            for v in values[offsets[r]:offsets[r + 1]]:
                dist = f32(oracle.l2(qi, v)) if metric == "l2" else f32(1) - f32(oracle.dot(qi, v)) if metric == "dot" else f32(oracle.cosine(qi, v))
                sim = f32(1) - dist
                if best is None or S.keys(sim) >= S.keys(best):
                    best = sim
            s = f32(s + best)
        out[r] = f32(1) - s
    return out


def topk(dist, k, rid=None):
    """the k smallest by (distance in total order, row id); slots beyond the rows: id 2^64 - 1, distance +inf (flat_knn's padding)"""
    ids, d = S.topk(dist, k, rid)
    pad = k - ids.size
    if pad > 0:
        ids = np.concatenate([ids, np.full(pad, np.uint64(0xFFFFFFFFFFFFFFFF))])
        d = np.concatenate([d, np.full(pad, np.inf, f32)])
    return ids, d
