"""Shared by tests/test_flat_order_spec.py (CPU) and tests/test_zz_gpu_flat_real.py (GPU): the REAL-VALUED fixtures of the flat KNN
tests, a numpy model of the summation order the flat kernels claim, and three wrong orders a kernel could take instead.

The claim (lance-linalg l2.rs:57-91, dot.rs:30-58; oracle/lance_oracle.c orc_l2_f32 / orc_dot_f32), every operation one f32 rounding:
  * the d % 16 tail elements are summed first, in element order, into an accumulator of their own (starting at +0);
  * 16 lane accumulators take the full 16-chunks in order (lane i: elements i, 16 + i, 32 + i, ...);
  * the lanes are folded in lane order, ((0 + a0) + a1) + ... + a15;
  * the value is tail + fold; the dot metric finishes with 1 - value.
The wrong orders:
  * "sequential":     one accumulator over the elements 0 .. d-1 in order;
  * "pairwise":       the 16 lane sums folded as a tree, ((a0 + a1) + (a2 + a3)) + ..., tail + tree;
  * "remainder_last": the tail taken as a last, zero-padded chunk of the lane accumulators (tail element j joins lane j after the
                      full chunks) -- what a kernel does that pads rows to a multiple of 16.  (Adding the finished tail sum to the
                      fold on the other side is no different order: one f32 addition commutes.)
On integer-valued data whose partial sums stay under 2^24 all four give the same bits; on the fixtures here they do not
(tests/test_flat_order_spec.py measures by how much)."""
import numpy as np

f32 = np.float32
ORDERS = ("sequential", "pairwise", "remainder_last")


# ---- fixtures -----------------------------------------------------------------------------------------------------------------
def real_f32(n, d, nq, seed):
    """standard_normal * 3 rows and queries: no two rows equal, every partial sum inexact"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, d), dtype=f32) * f32(3)
    q = rng.standard_normal((nq, d), dtype=f32) * f32(3)
    return x, q


def real_f16(n, d, nq, seed):
    """standard_normal * 0.7 rounded to binary16 (rows and queries: a Float16 column's query key is f16 too)"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((n, d)) * 0.7).astype(np.float16)
    q = (rng.standard_normal((nq, d)) * 0.7).astype(np.float16)
    return x, q


def int8_rows(n, d, nq, seed):
    rng = np.random.default_rng(seed)
    return rng.integers(-128, 128, (n, d)).astype(np.int8), rng.integers(-128, 128, (nq, d)).astype(np.int8)


def sift_like_flat_small(n, d, nq, seed):
    """the integer fixture of tests/test_zz_gpu_flat_small.py (rounded, clipped to 0..218, queries = rows + {0, 1})"""
    rng = np.random.default_rng(seed)
    centers = rng.uniform(0, 128, (32, d))
    x = np.clip(np.rint(centers[rng.integers(0, 32, n)] + rng.normal(0, 24, (n, d))), 0, 218).astype(f32)
    q = x[rng.integers(0, n, nq)] + rng.integers(0, 2, (nq, d)).astype(f32)
    return x, q


def f16_over_256(n, d, nq, seed):
    """the Float16 fixture of today's tests: integer / 256"""
    rng = np.random.default_rng(seed)
    return (rng.integers(0, 219, (n, d)) / 256.0).astype(np.float16), (rng.integers(0, 219, (nq, d)) / 256.0).astype(np.float16)


# ---- the model ----------------------------------------------------------------------------------------------------------------
def _terms(x, q, metric):
    """[n][d] f32: the per-element terms, each rounded once (widening f16 / int8 elements to f32 is exact)"""
    x = np.asarray(x).astype(f32)
    q = np.asarray(q).astype(f32)
    if metric == "dot":
        return x * q[None, :]
    diff = x - q[None, :]
    return diff * diff


def _seq(t, acc):
    for e in range(t.shape[1]):
        acc = acc + t[:, e]
    return acc


def distances(x, q, metric, order="reference"):
    """distances of ONE query to every row of x in the given summation order -> [n] f32"""
    t = _terms(x, q, metric)
    assert t.dtype == f32
    n, d = t.shape
    full = d // 16 * 16
    zero = np.zeros(n, f32)
    if order == "sequential":
        v = _seq(t, zero)
    else:
        lanes = np.zeros((n, 16), f32)
        for c in range(0, full, 16):
            lanes = lanes + t[:, c:c + 16]
        if order == "remainder_last":
            lanes[:, :d - full] = lanes[:, :d - full] + t[:, full:]
            tail = zero
        else:
            tail = _seq(t[:, full:], zero)
        if order == "pairwise":
            p = lanes
            while p.shape[1] > 1:
                p = p[:, 0::2] + p[:, 1::2]
            fold = p[:, 0]
        else:
            fold = _seq(lanes, zero)
        v = tail + fold
    assert v.dtype == f32
    return f32(1) - v if metric == "dot" else v


def keys(dist):
    """f32 -> uint32 in f32::total_cmp order (the reference's SortExec order on _distance)"""
    b = np.ascontiguousarray(dist, f32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def topk(dist, k, row_ids=None):
    """the k smallest by (distance in total order, row id) -> (ids uint64, distances f32)"""
    rid = np.arange(dist.size, dtype=np.uint64) if row_ids is None else np.asarray(row_ids, np.uint64)
    o = np.lexsort((rid, keys(dist)))[:k]
    return rid[o], dist[o]
