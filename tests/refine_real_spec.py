"""Shared by tests/test_refine_real_spec.py (CPU) and tests/test_zz_gpu_refine_real.py (GPU): REAL-VALUED columns for the exact refine
(lance_amd/csrc/search.hip launch_refine: refine_kernel<metric, float | __half | int8_t>, its four-lane cosine path, refine_pair_kernel),
numpy models of the reference's sums, and the sums a subtly wrong kernel would compute instead.

Why: the older refine tests use SIFT-like columns (integers 0 .. 218).  Every partial sum of such a distance is exact in f32, so any
number of lane accumulators and any fold give the same bits (test_refine_real_spec.py::test_integer_columns_cannot_see_the_order), and
f32 integer-valued columns leave for the u8 copy anyway.  On the columns here the order of the additions shows in the bits.

The reference's sums (oracle/lance_oracle.c, one f32 rounding per operation):
  l2 / dot on f32, l2 on f16, l2 / dot on int8   16 lane accumulators over the whole 16-chunks (lane i: elements i, 16 + i, ...), mul then
                                                 add; the d % 16 tail summed first, in element order; lanes folded ((0 + a0) + a1) + ...
  dot on f16                                     the same with 32 lanes
  cosine on f32 / int8 (cosine_fast)             16 FUSED multiply-add accumulators, an 8-wide group for d % 16 >= 8, the scalar tail;
                                                 a_i + a_(i+8), then the tree ((a0 + a4) + (a2 + a6)) + ((a1 + a5) + (a3 + a7));
                                                 d = 8 and 16 (cosine_once): plain products and the tree
  cosine on f16 (cosine_scalar)                  xy and y.y by the 32-lane dot; 1 - xy / (|x| * sqrt(y.y))
model(.., "reference") restates them and equals oracle.flat_knn bit for bit on every fixture of the grid (the CPU test asserts it).

wrong_order(): the same sums with HALF the lane accumulators -- 8 for the 16-lane forms, 16 for the 32-lane f16 forms -- and, for f32
cosine_fast, multiply-then-add in place of the fused multiply-add ("no_fma").  Two notes on "half":
  * a row that is all tail (f32 l2 / dot at d = 8, f16 dot / cosine at d = 16) is summed element by element, and so is one chunk of half as
    many lanes followed by the fold: the same additions in the same order.  For those lengths "half_lanes" folds the tail as a pairwise
    tree, ((t0 + t1) + (t2 + t3)) + ..., the other order a kernel could take there.
  * cosine_once (f32 cosine at d = 8 and 16) has no accumulators: "half_lanes" sums its eight terms in element order in place of the
    tree, and there is no "no_fma" (it multiplies and adds already).
Two more, each the slip one kernel could make: "fold_halves_swapped" -- refine_pair_kernel adding the other lane's accumulators 8 .. 15
before its own 0 .. 7 (f32 l2 / dot, d % 16 == 0) -- and "quad_pairs_swapped" -- the four-lane cosine path doing its xor-1 shuffle before
its xor-2, (a_i + a_(i+4)) + (a_(i+8) + a_(i+12)) for the reference's (a_i + a_(i+8)) + (a_(i+4) + a_(i+12)) (f32 cosine, d >= 256,
d % 16 == 0).  A wrong LANES in a dist_exact_rt instantiation of refine_kernel is "half_lanes" itself.
Share of the candidates (37 queries x up to 100, nprobes = 8) whose distance bits a wrong order changes, measured by
test_refine_real_spec.py::test_wrong_orders_show (every one must be at least a quarter; smallest .. largest over the lengths of an arm):
  f32 l2, pair kernel lengths      half_lanes 0.53 .. 0.72 (d = 144 .. 1536)      f32 l2, one-lane lengths    half_lanes 0.40 (d = 8) .. 0.57
  f32 dot, pair kernel lengths     half_lanes 0.54 .. 0.72                        f32 dot, one-lane lengths   half_lanes 0.41 (d = 8) .. 0.53
  f32 cosine, narrow               half_lanes 0.43 .. 0.65, no_fma 0.27 (d = 40), 0.32 (d = 100, 240, 264)
  f32 cosine, wide                 half_lanes 0.53 .. 0.77, no_fma 0.32 .. 0.34, quad_pairs_swapped 0.34 .. 0.36
  f32 l2 / dot, pair kernel lengths: fold_halves_swapped 0.58 .. 0.66 / 0.59 .. 0.69
  f16 l2                           half_lanes 0.27 (d = 16), 0.50, 0.59
  f16 dot                          half_lanes 0.43 .. 0.74                        f16 cosine                  half_lanes 0.53 .. 0.75
  int8 l2 at d = 1024              half_lanes 0.42
  int8 at d = 16, 40, 128 (l2, dot, cosine): 0 -- a squared difference is at most 255^2, a product at most 128^2, and d <= 128 of them
  stay under 2^24: every partial sum is exact.  These lengths check indexing, tails and widening.
  int8 dot at d = 1024: 0 as well, for any column -- |sum| <= 1024 * 128^2 = 2^24, so every partial sum is an integer f32 holds.  Only l2
  can pass 2^24 at that length (up to 1024 * 255^2), and only between rows far apart: neighbours in a clustered column differ by far
  less than the ~128 per element it takes.  So the queries of that fixture (all but the first three) are moved to the far end of the
  range (_fixture), where the squared differences are ~160^2 and the sums ~2.6e7.
  SIFT-like f32 column: 0.
The f32 cosine columns (d > 16) have elements of unequal weight, without which no_fma stayed under a quarter: see _fixture.

Fixture layout (fixture()): n = 3000 rows around 12 centres (uniform in [1, 4]^d, unit spread), 12 of them outliers around (4, -2, 4, -2, ..);
eight lists: six centroids from the oracle's k-means on the other rows, list SHORT = the outliers' mean (12 rows), list EMPTY = a
centroid no row is assigned to.  37 queries: q[0] next to an outlier (its first probe is SHORT), q[1] aimed at EMPTY, q[2] the query of
the duplicate block, the others next to rows.  The column holds 41 equal rows (BLOCK) whose code ranks 80th in q[2]'s PQ order, so the
block straddles keff = 100; with_duplicates() makes the raw column hold, at those ids, the row of q[2]'s nearest candidate, so the block
and that row tie for the first place and the (distance, row id) order decides the 10 returned."""
import functools
import types

import numpy as np

import oracle

f32 = np.float32
f64 = np.float64
N, NQ, NLIST, SHORT, EMPTY = 3000, 37, 8, 5, 3
NOUT = 12                              # rows of the short list
K, RF, KEFF = 10, 10, 100
NDUP, DUP_RANK = 41, 80
Q_SHORT, Q_EMPTY, Q_DUP = 0, 1, 2
KINDS = ("f32", "f16", "int8")
METRICS = ("l2", "dot", "cosine")
NONE_ID = np.uint64(np.iinfo(np.uint64).max)

# ---- the grid: (kind, metric) -> {d: M}; the smallest shapes that reach each code path (tests/test_zz_gpu_refine_real.py names them) ----
PAIR = {16: 4, 48: 12, 128: 16, 144: 9, 272: 17, 1536: 96}             # refine_pair_kernel
ONE_LANE = {8: 2, 24: 4, 40: 5, 100: 4}                                 # refine_kernel<.., float>
COS_NARROW = {8: 2, 16: 4, 40: 5, 100: 4, 240: 15, 264: 33}
COS_WIDE = {256: 16, 272: 17, 1536: 96}
F16_L2 = {16: 4, 40: 5, 272: 17}
F16_32 = {16: 4, 40: 5, 64: 8, 72: 9, 272: 17}
INT8 = {16: 4, 40: 5, 128: 16}
INT8_LONG = {1024: 64}
ARMS = {
    "f32-l2-pair": ("f32", "l2", PAIR), "f32-dot-pair": ("f32", "dot", PAIR),
    "f32-l2-one": ("f32", "l2", ONE_LANE), "f32-dot-one": ("f32", "dot", ONE_LANE),
    "f32-cosine-narrow": ("f32", "cosine", COS_NARROW), "f32-cosine-wide": ("f32", "cosine", COS_WIDE),
    "f16-l2": ("f16", "l2", F16_L2), "f16-dot": ("f16", "dot", F16_32), "f16-cosine": ("f16", "cosine", F16_32),
    "int8-l2": ("int8", "l2", {**INT8, **INT8_LONG}), "int8-dot": ("int8", "dot", {**INT8, **INT8_LONG}), "int8-cosine": ("int8", "cosine", INT8),
}
GRID = [(arm, kind, metric, d) for arm, (kind, metric, dims) in ARMS.items() for d in dims]


def num_sub_vectors(kind, metric, d):
    for k, m, dims in ARMS.values():
        if (k, m) == (kind, metric) and d in dims:
            return dims[d]
    return {64: 8}[d]


def order_shows(kind, metric, d):
    """whether the order of the additions can leave a trace at all (module docstring: an int8 sum must pass 2^24 for that)"""
    return kind != "int8" or (metric == "l2" and d >= 1024)


# ---- numpy models of the sums ---------------------------------------------------------------------------------------------------------
def keys(dist):
    """f32 -> uint32 in f32::total_cmp order"""
    b = np.ascontiguousarray(dist, f32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def _seq(t):
    acc = np.zeros(t.shape[0], f32)
    for e in range(t.shape[1]):
        acc = acc + t[:, e]
    return acc


def _pairwise(t):
    p = t
    while p.shape[1] > 1:
        if p.shape[1] % 2:
            p = np.concatenate([p, np.zeros((p.shape[0], 1), f32)], axis=1)
        p = p[:, 0::2] + p[:, 1::2]
    return p[:, 0] if p.shape[1] else np.zeros(t.shape[0], f32)


def _tree8(a):
    return ((a[:, 0] + a[:, 4]) + (a[:, 2] + a[:, 6])) + ((a[:, 1] + a[:, 5]) + (a[:, 3] + a[:, 7]))


def lane_sum(t, lanes, tail="seq"):
    """t [n][d] f32 terms -> tail + fold: `lanes` accumulators over the whole chunks, the d % lanes tail first (l2.rs:57-91, dot.rs:30-58)"""
    assert t.dtype == f32
    n, d = t.shape
    full = d // lanes * lanes
    acc = np.zeros((n, lanes), f32)
    for c in range(0, full, lanes):
        acc = acc + t[:, c:c + lanes]
    s = _seq(t[:, full:]) if tail == "seq" else _pairwise(t[:, full:])
    return s + _seq(acc)


def _fma(a, b, c):
    """round_f32(a * b + c) with ONE rounding: the product of two f32 is exact in f64; the f64 sum is rounded to odd (the error term of
    the two-sum says on which side the exact value lies), after which the rounding to f32 is the rounding of the exact value"""
    p = a.astype(f64) * b.astype(f64)
    c = np.broadcast_to(c.astype(f64), p.shape)
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    bits = s.view(np.int64).copy()
    fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((bits & 1) == 0)
    up = (err > 0) == (s > 0)
    bits[fix & up] += 1
    bits[fix & ~up] -= 1
    return bits.view(f64).astype(f32)


def _mul_add(a, b, c):
    return c + a * b


def _cosine_f32(x, y, order):
    """Cosine for f32 (cosine.rs:127-231) of one query x against rows y [n][d], both f32"""
    n, d = y.shape
    with np.errstate(all="ignore"):
        xn = np.sqrt(lane_sum((x * x)[None, :], 16))[0]
        if d in (8, 16):                                    # cosine_once
            xy, yy = y * x[None, :], y * y
            if d == 16:
                xy, yy = xy[:, :8] + xy[:, 8:], yy[:, :8] + yy[:, 8:]
            red = _tree8 if order in ("reference", "no_fma") else _seq
            return f32(1) - red(xy) / xn / np.sqrt(red(yy))
        mac = _mul_add if order == "no_fma" else _fma
        lanes = 8 if order == "half_lanes" else 16
        unrolled, aligned = d // lanes * lanes, d // 8 * 8
        xy16, yn16 = np.zeros((n, lanes), f32), np.zeros((n, lanes), f32)
        for c in range(0, unrolled, lanes):
            xy16 = mac(np.broadcast_to(x[c:c + lanes], (n, lanes)), y[:, c:c + lanes], xy16)
            yn16 = mac(y[:, c:c + lanes], y[:, c:c + lanes], yn16)
        xy8, yn8 = np.zeros((n, 8), f32), np.zeros((n, 8), f32)
        for c in range(unrolled, aligned, 8):
            xy8 = mac(np.broadcast_to(x[c:c + 8], (n, 8)), y[:, c:c + 8], xy8)
            yn8 = mac(y[:, c:c + 8], y[:, c:c + 8], yn8)
        if lanes == 16:
            t16, u16 = xy16[:, :8] + xy16[:, 8:], yn16[:, :8] + yn16[:, 8:]
        else:
            t16, u16 = xy16, yn16
        yt, xt = y[:, aligned:], np.broadcast_to(x[aligned:], (n, d - aligned))
        nrest = np.sqrt(lane_sum(yt * yt, 16))
        red16 = _tree8
        if order == "quad_pairs_swapped":                   # the four-lane path with its two shuffles in the other order
            t16, u16 = xy16, yn16
            red16 = _quads_swapped
        y_norm = red16(u16) + _tree8(yn8) + nrest * nrest
        xy = red16(t16) + _tree8(xy8) + lane_sum(xt * yt, 16)
        return f32(1) - xy / xn / np.sqrt(y_norm)


def _quads_swapped(a):
    """16 accumulators reduced as the four-lane cosine path would with xor-1 before xor-2: u_i = (a_i + a_(i+4)) + (a_(i+8) + a_(i+12)),
    then (u0 + u2) + (u1 + u3); the reference pairs a_i with a_(i+8) first: ((a_i + a_(i+8)) + (a_(i+4) + a_(i+12)))"""
    u = (a[:, 0:4] + a[:, 4:8]) + (a[:, 8:12] + a[:, 12:16])
    return (u[:, 0] + u[:, 2]) + (u[:, 1] + u[:, 3])


def model(metric, kind, q, rows, order="reference"):
    """distances of ONE query to rows [n][d] (any of the three element types; widening is exact) -> [n] f32.
    order: "reference" | "half_lanes" | "no_fma" (f32 / int8 cosine beyond cosine_once only) | "fold_halves_swapped" (16-lane l2 / dot:
    lanes 8 .. 15 folded before lanes 0 .. 7) | "quad_pairs_swapped" (f32 cosine, d % 16 == 0)"""
    assert order in ("reference", "half_lanes", "no_fma", "fold_halves_swapped", "quad_pairs_swapped")
    x = np.asarray(q).astype(f32).reshape(-1)
    y = np.asarray(rows).astype(f32)
    d = y.shape[1]
    if metric == "cosine" and kind != "f16":
        return _cosine_f32(x, y, order)
    assert order not in ("no_fma", "quad_pairs_swapped")
    lanes = 32 if kind == "f16" and metric != "l2" else 16
    tail = "seq"
    if order == "fold_halves_swapped":                      # refine_pair_kernel summing the other lane's eight accumulators first
        assert lanes == 16 and d % 16 == 0 and metric != "cosine"
        t = y - x[None, :] if metric == "l2" else y
        t = t * t if metric == "l2" else t * x[None, :]
        acc = np.zeros((y.shape[0], 16), f32)
        for c in range(0, d, 16):
            acc = acc + t[:, c:c + 16]
        v = f32(0) + _seq(np.concatenate([acc[:, 8:], acc[:, :8]], axis=1))
        return v if metric == "l2" else f32(1) - v
    if order == "half_lanes":
        if d < lanes:
            tail = "pairwise"                               # all tail: half the lanes would be the same additions (module docstring)
        else:
            lanes //= 2
    with np.errstate(all="ignore"):
        if metric == "l2":
            diff = y - x[None, :]
            return lane_sum(diff * diff, lanes, tail)
        if metric == "dot":
            return f32(1) - lane_sum(y * x[None, :], lanes, tail)
        xn = np.sqrt(lane_sum((x * x)[None, :], 32))[0]      # f16 cosine: norm_l2_impl::<f16, f32, 32>; the query is not the operand under test
        y_sq, xy = lane_sum(y * y, lanes, tail), lane_sum(y * x[None, :], lanes, tail)
        return f32(1) - xy / (xn * np.sqrt(y_sq))


def wrong_order(metric, kind, q, rows):
    """{name: [n] f32}: what a subtly wrong kernel would compute (module docstring)"""
    d = np.asarray(rows).shape[1]
    out = {"half_lanes": model(metric, kind, q, rows, "half_lanes")}
    if metric == "cosine" and kind != "f16" and d not in (8, 16):
        out["no_fma"] = model(metric, kind, q, rows, "no_fma")
    if metric == "cosine" and kind == "f32" and d >= 256 and d % 16 == 0:      # refine_wide_rows(d): the four-lane path
        out["quad_pairs_swapped"] = model(metric, kind, q, rows, "quad_pairs_swapped")
    if metric != "cosine" and kind == "f32" and d % 16 == 0:                     # refine_pair_kernel's lengths
        out["fold_halves_swapped"] = model(metric, kind, q, rows, "fold_halves_swapped")
    return out


def refine_with(dist_fn, cand, raw, q, k):
    """the refine of candidate lists cand u64 [nq][keff] (~0 = none) with dist_fn(query, rows) -> (ids [nq][k], dists [nq][k], every
    candidate's distance [nq][keff] (+inf for none))"""
    nq, keff = cand.shape
    out_i = np.full((nq, k), NONE_ID, np.uint64)
    out_d = np.full((nq, k), np.inf, f32)
    every = np.full((nq, keff), np.inf, f32)
    for qi in range(nq):
        ok = cand[qi] != NONE_ID
        c = cand[qi][ok]
        if len(c):
            dist = dist_fn(q[qi], raw[c.astype(np.int64)])
            every[qi, ok] = dist
            o = np.lexsort((c, keys(dist)))[:k]
            out_i[qi, :len(o)] = c[o]; out_d[qi, :len(o)] = dist[o]
    return out_i, out_d, every


def oracle_rows(a):
    """a column or queries as the oracle takes them: f16 stays f16 (it selects f16's own dot / cosine), int8 is widened"""
    a = np.asarray(a)
    return a if a.dtype == np.float16 else a.astype(f32)


def oracle_distances(metric, q, rows):
    """the function flat_knn uses for the rows' element type and the metric, one query"""
    return oracle.distance_batch(metric, np.asarray(q).astype(f32), oracle_rows(rows))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------------
def _to_kind(v, kind):
    """values already on the column's scale -> the column's element type"""
    if kind == "int8":
        return np.ascontiguousarray(np.clip(np.rint(v), -128, 127).astype(np.int8))
    return np.ascontiguousarray(np.asarray(v).astype(np.float16 if kind == "f16" else f32))


NOISE = {"f32": 1.0, "f16": 0.25, "int8": 12.0}            # the unit spread on each column's scale


def _cast(a, kind, rng, label, outliers):
    """unit-spread rows -> the column: f32 as they are, f16 = 0.25 x rounded to binary16, int8 = 12 x rounded with about a fifth of the
    elements +-127 or -128 (the full range).  Which elements: a fifth of every CENTRE's coordinates, the same for all rows around it --
    drawn row by row they would be the larger part of every distance and leave no lists to speak of.  The outliers keep their values."""
    if kind != "int8":
        return _to_kind(a * NOISE[kind], kind)
    u = rng.random((int(label.max()) + 1, a.shape[1]))[label]
    u[outliers] = 1.0
    v = np.clip(np.rint(a * 12.0), -128, 127)
    return _to_kind(np.where(u < 0.08, 127.0, np.where(u < 0.14, -127.0, np.where(u < 0.20, -128.0, v))), kind)


def _train(kind, metric, x, m, regular, outliers, seed):
    """eight centroids and the codebook in the column's model type (f16 for an f16 column, else f32), and the point q[Q_EMPTY] aims at"""
    xo = oracle_rows(x)
    km = "l2" if metric == "cosine" else metric
    xs = oracle.normalize(xo) if metric == "cosine" else xo
    six, _, _, _ = oracle.kmeans_train(np.ascontiguousarray(xs[regular]), NLIST - 2, max_iters=5, seed=seed, metric=km)
    short = xs[outliers].astype(f64).mean(axis=0)
    mean = xs[regular].astype(f64).mean(axis=0)
    if metric == "l2":                                      # far from every row
        empty = np.full_like(mean, -120.0) if kind == "int8" else -8.0 * np.abs(mean)
        aim = np.full_like(mean, -128.0) if kind == "int8" else empty
    elif metric == "dot":                                   # every row has a larger product with its own list's centroid than 0
        empty, aim = np.zeros_like(mean), -mean
    else:                                                   # opposite every (normalised) row
        empty = -mean / np.linalg.norm(mean)
        aim = -xo[regular].astype(f64).mean(axis=0)
    six = six.astype(f64)
    cent = np.ascontiguousarray(np.stack([six[0], six[1], six[2], empty, six[3], short, six[4], six[5]]).astype(np.float16 if kind == "f16" else f32))
    assert (EMPTY, SHORT) == (3, 5)
    part, _ = oracle.assign(xs, cent, km)
    res = oracle.residual(xs, cent, np.where(part == oracle.NONE, 0, part)) if km == "l2" else xs
    cb, _ = oracle.pq_train(np.ascontiguousarray(res), m, max_iters=4, seed=seed + 1)
    return cent, cb, aim


def _sizes(kind, metric, x, cent):
    xo = oracle_rows(x)
    xs = oracle.normalize(xo) if metric == "cosine" else xo
    part, _ = oracle.assign(xs, cent, "l2" if metric == "cosine" else metric)
    return np.bincount(part[part != oracle.NONE], minlength=NLIST), part


def oracle_index(fx, x=None):
    return oracle.build_index(oracle_rows(fx.x if x is None else x), fx.cent, fx.cb, fx.metric)


@functools.lru_cache(maxsize=None)
def fixture(kind, metric, d, n=N, seed=0):
    """-> namespace: x [n][d], q [37][d] (both in the column's element type), cent [8][d], cb [M][256][d / M], and m, block (the ids of
    the 41 equal rows), tie (the id whose row the block takes in with_duplicates), outliers, oidx (the oracle's index of x).
    A draw that misses one of the layout's properties is redrawn with the next seed."""
    for draw in range(8):
        fx = _fixture(kind, metric, d, n, seed + draw)
        if fx is not None:
            return fx
    raise AssertionError(f"no usable draw for {kind} {metric} d={d}")


def _fixture(kind, metric, d, n, seed):
    m = num_sub_vectors(kind, metric, d)
    rng = np.random.default_rng([seed, d, n, KINDS.index(kind), METRICS.index(metric)])
    centres = rng.uniform(1.0, 4.0, (12, d))
    label = rng.integers(0, 12, n)
    a = centres[label] + rng.standard_normal((n, d))
    outliers = np.sort(rng.choice(n, NOUT, replace=False))
    a[outliers] = np.where(np.arange(d) % 2 == 0, 4.0, -2.0)[None, :] + 0.3 * rng.standard_normal((NOUT, d))
    if metric == "cosine" and kind == "f32" and d > 16:     # (d = 8, 16: cosine_once multiplies and adds)
        # Elements of unequal weight: every 16th element x 8, every other 16-chunk x 16 (powers of two: no mantissa changes).  On rows of
        # equal weight the low bits of a product seldom reach the sum -- an accumulator is soon far larger than the next product, and
        # the total far larger than any accumulator -- and multiply-then-add for the fused multiply-add changed 0.11 (d = 40) to 0.27
        # (d = 1536) of the distances: under the quarter asked for.  Here a chunk's products outweigh the sum so far every other step,
        # and one accumulator carries most of the total.
        i = np.arange(d)
        a = a * (np.where(i % 16 == 0, 8.0, 1.0) * 16.0 ** ((i // 16) % 2))[None, :]
    regular = np.setdiff1d(np.arange(n), outliers)
    near =rng.choice(regular, NQ, replace=False)
    near[Q_SHORT] = outliers[3]
    x = _cast(a, kind, rng, label, outliers)
    if kind == "int8":
        assert 0.12 < np.isin(x, (127, -127, -128)).mean() < 0.28
    if kind == "f32":
        assert (x != np.rint(x)).any()                      # the u8 copy cannot be taken
    cent, cb, aim = _train(kind, metric, x, m, regular, outliers, seed + 11)
    q = _to_kind(x[near].astype(f64) + 0.05 * NOISE[kind] * rng.standard_normal((NQ, d)), kind)
    q[Q_EMPTY] = _to_kind(aim, kind)
    if kind == "int8" and metric == "l2" and d >= 1024:
        # the only int8 sums that can pass 2^24: squared differences of ~160 each.  Neighbours do not differ by that much, so these
        # queries sit at the far end of the range from the rows they were drawn next to (the first three keep their places)
        q[3:] = _to_kind(q[3:].astype(f64) - 160.0, kind)
    fx = types.SimpleNamespace(kind=kind, metric=metric, d=d, m=m, n=n, x=x, q=q, cent=cent, cb=cb, outliers=outliers)
    # ---- the duplicate block: the row whose code ranks DUP_RANK-th in q[Q_DUP]'s PQ order, 40 more times under scattered ids
    pre = oracle_index(fx)
    ci, _ = pre.search(oracle_rows(q[Q_DUP:Q_DUP + 1]), 200, NLIST)
    if (ci[0] == NONE_ID).any():
        return None
    r0 = int(ci[0, DUP_RANK])
    free = np.setdiff1d(regular, np.concatenate([ci[0].astype(np.int64), near]))
    dups = np.sort(rng.choice(free, NDUP - 1, replace=False))
    x[dups] = x[r0]
    fx.block = np.sort(np.concatenate([[r0], dups])).astype(np.uint64)
    fx.oidx = oracle_index(fx)
    ex = oracle_distances(metric, q[Q_DUP], x[ci[0, :DUP_RANK].astype(np.int64)])
    fx.tie = int(ci[0, np.argmin(keys(ex))])
    # ---- the layout's properties
    sizes, _ = _sizes(kind, metric, x, cent)
    qq = oracle_rows(q[:2])
    first, _ = oracle.find_partitions(oracle.normalize(qq) if metric == "cosine" else qq, cent, 1, "l2" if metric == "cosine" else metric)
    ok = sizes[EMPTY] == 0 and sizes[SHORT] == NOUT and sizes.sum() == n and (first[:, 0] == [SHORT, EMPTY]).all()
    return fx if ok else None


SPOILS = ("nan", "inf", "subnormal", "negzero", "tiny_row")


def spoils_for(kind, metric):
    """nan / subnormal / -0.0 everywhere; +inf not under cosine: inf / inf is a NaN the DIVISION makes, whose sign is the dividing
    machine's (lance_amd/csrc/exact.cuh cosine_finish) -- the all-zero row's reason; the row of 1e-30 is an f32 row"""
    assert kind in ("f32", "f16")
    return tuple(s for s in SPOILS if not (s == "inf" and metric == "cosine") and not (s == "tiny_row" and kind != "f32"))


def spoiled_raw(x, kind, metric="l2", avoid=(), seed=0):
    """-> (the column handed to set_raw, the changed row numbers, what each got): x except at 40 rows spread over the column"""
    rng = np.random.default_rng([seed, x.shape[1], 77])
    raw = np.array(x)
    free = np.setdiff1d(np.arange(x.shape[0]), np.asarray(avoid, np.int64))
    rows = np.sort(rng.choice(free, 40, replace=False))
    kinds = spoils_for(kind, metric)
    what = [kinds[i % len(kinds)] for i in range(len(rows))]
    for r, w in zip(rows, what):
        e = int(rng.integers(0, x.shape[1]))
        if w == "nan":
            raw[r, e] = np.nan
        elif w == "inf":
            raw[r, e] = np.inf
        elif w == "subnormal":
            raw[r, e] = 1e-40 if kind == "f32" else 6e-8
        elif w == "negzero":
            raw[r, e] = -0.0
        else:
            raw[r, :] = 1e-30
    assert np.isnan(raw.astype(f32)).sum() == what.count("nan") and np.signbit(raw[rows][np.array(what) == "negzero"]).any()
    return raw, rows, what


def spoiled_fixture(kind, metric, d):
    """-> (fx, raw, rows, what, queries): the spoiled column with the duplicate block's rows replaced (with_duplicates), and one query per
    changed row (next to the CLEAN row, which is what the index stores) followed by the duplicate block's query"""
    fx = fixture(kind, metric, d)
    avoid = np.concatenate([fx.block.astype(np.int64), [fx.tie], fx.outliers[:-2]])
    raw, rows, what = spoiled_raw(fx.x, kind, metric, avoid=avoid)
    raw = with_duplicates(fx, raw)
    rng = np.random.default_rng([d, 78])
    clean = fx.x[rows].astype(f64)
    if metric == "dot":          # under dot "next to" is not "first": step along the row's own offset from its list's centroid
        _, part = _sizes(kind, metric, fx.x, fx.cent)
        clean = clean + 4.0 * (clean - fx.cent[part[rows]].astype(f64))
    qs = _to_kind(clean + 0.02 * NOISE[kind] * rng.standard_normal(clean.shape), kind)
    return fx, raw, rows, what, np.ascontiguousarray(np.concatenate([qs, fx.q[Q_DUP:Q_DUP + 1]]))


def with_duplicates(fx, raw):
    """the raw column with the row of fx.tie at the block's 41 ids: the block (the part of it inside the candidate list) and that row tie"""
    raw = np.array(raw)
    raw[fx.block.astype(np.int64)] = raw[fx.tie]
    return raw


def sift_like(n, d, seed):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(0, 128, (32, d))
    return np.clip(np.rint(centers[rng.integers(0, 32, n)] + rng.normal(0, 24, (n, d))), 0, 218).astype(f32)
