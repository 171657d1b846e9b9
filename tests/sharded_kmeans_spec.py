"""Specification of the row-sharded Lloyd trainer (lance_hip_kmeans_shard_* / lance_hip_kmeans_estep_partial / the loop in
lance_amd/csrc/comm.cpp / lance_amd.dist.train_kmeans_sharded), in numpy on top of the CPU oracle's assignment.  No product code
except the split RNG (lance_amd._rng.Rng, the twin of csrc/rng.h).

The contract it writes down:

  * a shard's partials have ONE value: per (cluster, column) the members are added sequentially in row order in f32, the per-cluster
    loss is an f64 chain in row order, the radius an f32 max from 0 (kmeans_accumulate_body / kmeans_stats_body);
  * the ranks' partials are folded in rank order (f32 add, f64 add, f32 max);
  * every rank then runs the same update on the folded numbers (kmeans_shard_update_kernel): centroid = sum * (1 / count), sizes
    from the f32 counts, the FIRST cluster of maximal size by id, `adjusted`, the f32 balance loss with the f64 loss summed in
    cluster order, the empty-cluster split with Rng(seed ^ 0x5BD1E995), the convergence test, bf_used = min(adjusted, bf / n_total)
    and the next bias from the POST-split sizes.

On one rank the row order is the single trainer's, so the result equals oracle.kmeans_train bit for bit; wherever every partial sum
is exact (integer-valued rows, sums below 2^24) it does so for any shard layout.  The one known divergence from the reference: the
reference takes, among the clusters of maximal size, the one whose last member comes first in row order; the reduced buffers carry no
last row, so the sharded trainer takes the smallest id.  The choice only matters through `adjusted`, i.e. when two clusters tie for
largest in an iteration whose `adjusted` is the binding term of the next balance factor (case "tie").
"""
import functools

import numpy as np

from lance_amd._rng import Rng

f32 = np.float32
f64 = np.float64
FLT_MAX = f32(np.finfo(f32).max)
DBL_MAX = float(np.finfo(f64).max)
LAYOUTS = ("w1", "w2", "w3", "w5")


def _oracle():
    import oracle
    oracle.lib()
    return oracle


def estep(x_shard, cent, metric="l2", bias=None):
    """-> (ids u32, dists f32) of the shard's rows: the oracle's assignment, cosine trained as L2 like the library"""
    orc = _oracle()
    x = np.ascontiguousarray(x_shard, f32)
    if x.shape[0] == 0:
        return np.zeros(0, np.uint32), np.zeros(0, f32)
    m = "l2" if metric == "cosine" else metric
    return orc.assign(x, np.ascontiguousarray(cent, f32), m, None if bias is None else np.ascontiguousarray(bias, f32))


def partials(x_shard, cent, metric="l2", bias=None, _dists_out=None):
    """One shard's contribution -> (sums [k,d] f32, counts [k] f32, losses [k] f64, radius [k] f32)"""
    orc = _oracle()
    x = np.ascontiguousarray(x_shard, f32)
    cent = np.ascontiguousarray(cent, f32)
    k, d = cent.shape
    sums = np.zeros((k, d), f32); counts = np.zeros(k, f32); losses = np.zeros(k, f64); radius = np.zeros(k, f32)
    ids, dists = estep(x, cent, metric, bias)
    if _dists_out is not None:
        _dists_out.append(dists[ids != orc.NONE])
    zrow = np.zeros((1, d), f32)
    with np.errstate(invalid="ignore", over="ignore"):
        for c in np.unique(ids):
            if c == orc.NONE:
                continue
            rows = np.flatnonzero(ids == c)                      # ascending: row order
            # the chains start from +0 (0 + -0 = +0); cumsum keeps the order of the adds, np.sum would not
            sums[c] = np.cumsum(np.concatenate([zrow, x[rows]]), axis=0, dtype=f32)[-1]
            counts[c] = f32(rows.size)
            dc = dists[rows]
            losses[c] = np.cumsum(np.concatenate([[0.0], dc.astype(f64)]), dtype=f64)[-1]
            radius[c] = np.fmax.reduce(dc, initial=f32(0))      # f32::max / fmaxf: a NaN operand is dropped
    return sums, counts, losses, radius


def fold(parts):
    """left fold in rank order: f32 add, f64 add, f32 max"""
    s, c, l, r = (a.copy() for a in parts[0])
    with np.errstate(invalid="ignore", over="ignore"):
        for s1, c1, l1, r1 in parts[1:]:
            s = (s + s1).astype(f32); c = (c + c1).astype(f32); l = l + l1; r = np.fmax(r, r1)
    return s, c, l, r


def finalize(sums, counts):
    """centroid = sum * (1 / count); an empty cluster keeps its (zero) sum"""
    cent = sums.copy()
    for c in range(counts.size):
        if counts[c] > 0:
            cent[c] = (sums[c] * (f32(1.0) / f32(counts[c]))).astype(f32)
    return cent


def _split(n_total, sizes, cent, rng, wrong=None):
    k, d = cent.shape
    eps = f32(1.0 / 1024.0)
    up, down = f32(1.0) + eps, f32(1.0) - eps
    if wrong == "one_sided_split":
        down = f32(1.0)
    even = np.arange(d) % 2 == 0
    nsplit = 0
    for i in range(k):
        if sizes[i] != 0:
            continue
        if not (sizes >= 2).any():            # `splittable`: the rejection loop below would never end
            break
        j = 0
        while True:
            p = (f32(sizes[j]) - f32(1.0)) / f32(n_total - k)
            if f32(rng.next_f32()) < p:
                break
            j = (j + 1) % k
        sizes[i] = sizes[j] // 2
        sizes[j] -= sizes[i]
        cj = cent[j].copy()
        cent[i] = np.where(even, cj * up, cj * down).astype(f32)
        cent[j] = np.where(even, cj * down, cj * up).astype(f32)
        nsplit += 1
    return nsplit


def train(shards, k, n_total, max_iters, tol, balance_factor, init, seed, metric="l2", wrong=None):
    """The loop kmeans_shard_update_kernel documents, over any list of row shards.  -> (centroids, loss, iters, trace)
    `wrong` (fixture checks only) makes one deliberate mistake, so that a test can show that a case would notice it:
    "presplit_bias": the next bias from the sizes before the split; "one_sided_split": the (1 - 1/1024) side of a split left out."""
    cent = np.ascontiguousarray(init, f32).copy()
    bf_param = f32(balance_factor) / f32(n_total)
    rng = Rng(seed ^ 0x5BD1E995)
    adjusted = FLT_MAX
    bf_used = FLT_MAX if FLT_MAX < bf_param else bf_param
    bias = np.zeros(k, f32)
    loss, last_loss, iters = DBL_MAX, DBL_MAX, 0
    trace = []
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        for _ in range(max_iters):
            iters += 1
            dd = []
            s, cnt, l, r = fold([partials(sh, cent, metric, bias if bf_param != 0 else None, dd) for sh in shards])
            cent = finalize(s, cnt)
            sizes = cnt.astype(np.uint32).astype(np.int64)
            max_id = int(np.argmax(sizes))                      # first maximal cluster by id
            adjusted = (r[max_id] - f32(l[max_id]) / f32(sizes[max_id])) / f32(n_total)
            size_loss = f32(int((sizes.astype(object) ** 2).sum()))
            balance_loss = f32(bf_used) * (size_loss - f32(int(n_total) * int(n_total)) / f32(k))
            lsum = 0.0
            for v in l:                                          # f64 chain in cluster order
                lsum = lsum + float(v)
            last_loss = lsum + float(balance_loss)
            alld = np.concatenate(dd) if dd else np.zeros(0, f32)
            pos = np.abs(alld[alld != 0])
            rec = {"sizes": sizes.copy(), "empties": int((sizes == 0).sum()), "tied": int((sizes == sizes.max()).sum()),
                   "adjusted_binds": bool(adjusted < bf_param), "min_nonzero_dist": float(pos.min()) if pos.size else float("inf"),
                   "splits": 0}
            if rec["empties"]:
                before = sizes.copy()
                rec["splits"] = _split(int(n_total), sizes, cent, rng, wrong)
            trace.append(rec)
            done = abs(loss - last_loss) < tol * last_loss
            if not done:
                loss = last_loss
            bf_used = adjusted if adjusted < bf_param else bf_param
            bsizes = before if (wrong == "presplit_bias" and rec["empties"]) else sizes
            bias = (f32(bf_used) * bsizes.astype(f32)).astype(f32)       # from the post-split sizes
            if done:
                break
    return cent, last_loss, iters, trace


# ---- fixtures ----------------------------------------------------------------------------------------------------------------
def sift_like(n, d, seed, ncl=32):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(0, 128, (ncl, d))
    x = centers[rng.integers(0, ncl, n)] + rng.normal(0, 24, (n, d))
    return np.clip(np.rint(x), 0, 218).astype(f32)


def blobs(n, d, seed, ncl=8):
    rng = np.random.default_rng(seed)
    centers = rng.standard_normal((ncl, d)) * 4
    return (centers[rng.integers(0, ncl, n)] + rng.standard_normal((n, d))).astype(f32)


def layouts(n):
    """shard cut points: 1 rank; 2 uneven ranks; 3 ranks; 5 ranks, one of them with no row and one with a single row"""
    a, b = n * 2 // 7, n * 5 // 8
    return {"w1": [0, n], "w2": [0, n * 3 // 8 + 1, n], "w3": [0, n // 3 + 1, n * 2 // 3 + 2, n], "w5": [0, a, a, a + 1, b, n]}


def _rows(x, seed, k):
    return x[np.random.default_rng(seed).permutation(x.shape[0])[:k]].copy()


def _case(name, kind, x, init, k, bf, max_iters, seed, metric="l2", tol=1e-4, **props):
    x = np.ascontiguousarray(x, f32)
    return dict(name=name, kind=kind, x=x, init=np.ascontiguousarray(init, f32), k=k, bf=bf, max_iters=max_iters, seed=seed, metric=metric,
                tol=tol, layouts=layouts(x.shape[0]), props=props)


@functools.lru_cache(maxsize=None)
def cases():
    """name -> case.  `props` names what the case is there for; tests/test_sharded_kmeans_spec.py asserts each from the trace."""
    out = {}

    def add(c):
        out[c["name"]] = c

    x = sift_like(3001, 32, 5)
    add(_case("l2_bf0", "exact", x, _rows(x, 1, 16), 16, 0.0, 20, 5, converges_off_8=True, never_binds=True))
    add(_case("l2_bf1", "exact", x, _rows(x, 3, 16), 16, 1.0, 30, 5, converges_9_29=True, never_binds=True))
    # tol = 0: `|loss - last| < 0` never holds, so the run is cut off by max_iters (past the fixed point the iterations repeat)
    add(_case("l2_bf1_runs_out", "exact", x, _rows(x, 1, 16), 16, 1.0, 30, 5, tol=0.0, runs_out=True))
    add(_case("dot_splits", "exact", x, _rows(x, 2, 16), 16, 0.0, 12, 5, metric="dot", split_iterations=2, both_split_sides=True))
    init = _rows(x, 1, 16); init[5] = init[3]; init[9] = init[3]
    # (the two halves of a duplicated centroid part the same rows whether one side or both are perturbed: this case checks the
    # split's RNG draws, sizes and placement, "dot_splits" also its two factors)
    add(_case("l2_dup_init", "exact", x, init, 16, 0.0, 20, 5, split_iterations=1))
    # ... and with a balance factor: the bias that follows a split comes from the sizes AFTER it
    add(_case("l2_dup_init_bf", "exact", x, init, 16, 1e4, 20, 5, split_iterations=1, bias_after_split=True))
    xk = sift_like(3000, 20, 11, ncl=300)
    add(_case("k300", "exact", xk, _rows(xk, 3, 300), 300, 1.0, 10, 7, wide_group=True))
    x1 = sift_like(301, 20, 13)
    add(_case("k1", "exact", x1, x1[7:8].copy(), 1, 1.0, 10, 2))
    add(_case("l2_adjusted_binds", "exact", x, _rows(x, 1, 16), 16, 1e6, 12, 5, binds=True))
    for metric in ("l2", "dot"):
        for bf in (0.0, 1.0):
            xb = blobs(2001, 16, 17)
            add(_case("blobs_%s_bf%d" % (metric, int(bf)), "ordered", xb, _rows(xb, 4, 8), 8, bf, 15, 5, metric=metric))
    # two clusters tie for largest at iteration 5 while `adjusted` binds: 8 iterations where the reference takes 7
    rng = np.random.default_rng(7)
    xt = rng.integers(0, 12, (40, 2)).astype(f32)
    add(_case("tie", "tie", xt, xt[rng.permutation(40)[:4]].copy(), 4, 1e6, 8, 1, tie_binds=True))
    return out


def shards_of(case, layout):
    cuts = case["layouts"][layout]
    return [case["x"][a:b] for a, b in zip(cuts[:-1], cuts[1:])]


@functools.lru_cache(maxsize=None)
def spec_result(name, layout):
    """(centroids, loss, iters, trace) of the specification for one case and shard layout; computed once, treat as read-only"""
    c = cases()[name]
    return train(shards_of(c, layout), c["k"], c["x"].shape[0], c["max_iters"], c["tol"], c["bf"], c["init"], c["seed"], c["metric"])


@functools.lru_cache(maxsize=None)
def oracle_result(name):
    """(centroids, loss, iters) of the single-process reference trainer on the whole case"""
    c = cases()[name]
    n = c["x"].shape[0]
    oc, ol, oit, _ = _oracle().kmeans_train(c["x"], c["k"], max_iters=c["max_iters"], tol=c["tol"], balance_factor=f32(c["bf"]) / f32(n),
                                            init=c["init"], seed=c["seed"], metric=c["metric"])
    return oc, ol, oit


def nan_case():
    """a shard with an all-NaN row, a partly-NaN row and an inf row among ordinary ones -> (x, centroids)"""
    rng = np.random.default_rng(29)
    x = (rng.standard_normal((130, 20)) * 3).astype(f32)
    cent = x[rng.permutation(130)[:33]].copy()
    x[5] = np.nan
    x[70, 3] = np.nan
    x[99, 11] = np.inf
    return x, cent


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.dtype.itemsize in (4, 8), (a.dtype, b.dtype)
    u = np.uint32 if a.dtype.itemsize == 4 else np.uint64
    return a.shape == b.shape and bool((a.view(u) == b.view(u)).all())
