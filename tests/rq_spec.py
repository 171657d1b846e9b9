"""Shared by tests/test_rq_spec.py (CPU), tests/test_rq_kernels_cpu.py (CPU), tests/test_zz_gpu_rq.py and tests/test_zz_gpu_rq_scan.py (GPU): the CPU specification
of the 1-bit RaBitQ quantiser and of the IVF_RQ search, in numpy, composed with the oracle's functions for the IVF side.

The specification (lance-index bq/builder.rs, bq/transform.rs, bq/storage.rs:130-156, 249-369, 409-445; ivf.rs:281-326;
lance/src/index/vector/ivf/v2.rs:316-332; flat/index.rs:82-177).  Every floating-point operation is ONE rounding in f32, left to
right, never contracted.  d % 8 == 0, D = d, P [D][D] f32 is the rotation (part of the model).

    build, row v of partition p (centroid c), dist_v_c = what the partition assignment reports (oracle.assign's second value):
        r        v - c
        rot[j]   dot(P[j], r) in the order of lance_linalg::distance::dot (16 lane accumulators, then the tail; dot.rs:30-58)
        bit j    1 iff the sign bit of rot[j] is clear (+0.0 -> 1, -0.0 -> 0); byte j / 8, bit j % 8
        ip       (sum_j |rot[j]|, sequential from 0.0) / sqrt(f32(d))
        res2     L2: dist_v_c                       dot: sum r_i^2 (sequential)
        add      L2: res2                           dot: dist_v_c + (sum c_i^2, sequential)
        scale    ip == 0: L2 0.0, dot -0.0 (the reference negates `div_checked(..).unwrap_or_default()`, transform.rs:192-198)
                 else L2: (-2 res2) / ip            dot: -(res2 / ip)
    The reference rotates the rows with an ndarray GEMM, whose summation order is the BLAS kernel's: the two orders above are this
    project's definition.  Everything below is the reference's own arithmetic.

    query q against probed partition p (dist_q_c from the coarse quantiser):
        qr = q - c_p;  rq[j] = dot(P[j], qr);  sum_q = f32::sum of rq (sequential from -0.0);  sqrt_d = sqrt(f32(d))
        q_factor = dist_q_c (L2), dist_q_c - 1 (dot)
        table    t[s][0] = 0, t[s][j] = t[s][j - lowbit(j)] + rq[4 s + ctz(j)] for every segment s of 4 dimensions
    rows in storage order, n rows, np = n - n % 32; code byte b uses tables 2b (low nibble) and 2b + 1 (high nibble):
        no prefilter, i <  np   qmin / qmax over the table by total_cmp; equal: every e is 0, else factor = 255 / (qmax - qmin),
                                e = round_half_away((t - qmin) factor) as u8;  s = min(65535, sum of e)  (u16 saturating);
                                dist = f32(s) ((qmax - qmin) / 255) + f32(d / 4) qmin
        no prefilter, i >= np   dist = 0.0; dist += t[2b][lo] + t[2b+1][hi] for every b in order
        under a prefilter       every selected row: the same terms folded by f32::sum (from -0.0); no quantised table
        final                   ((2 dist - sum_q) / sqrt_d) scale[i] + add[i] + q_factor
    partition: oracle.heap_topk over the rows in storage order; partitions merged by oracle.sort_fetch (dist, rowid)."""
import numpy as np

f32, f64 = np.float32, np.float64
NONE = 0xFFFFFFFF
BATCH = 32


# ---- sums in the reference's orders ---------------------------------------------------------------------------------------------
def dot16(a, b):
    """lance_linalg::distance::dot along the last axis (operands broadcast): 16 lane accumulators over the full chunks, summed in
    lane order from 0.0, plus the sequentially summed tail (tail first: `tail + lanes`)"""
    with np.errstate(all="ignore"):
        prod = np.asarray(a, f32) * np.asarray(b, f32)
        d = prod.shape[-1]
        full = d // 16 * 16
        s = np.zeros(prod.shape[:-1], f32)
        for i in range(full, d):
            s = s + prod[..., i]
        lanes = np.zeros(prod.shape[:-1] + (16,), f32)
        for c in range(0, full, 16):
            lanes = lanes + prod[..., c:c + 16]
        tot = np.zeros(prod.shape[:-1], f32)
        for i in range(16):
            tot = tot + lanes[..., i]
        return (s + tot).astype(f32)


def seq_sum(a, start=0.0):
    """sequential f32 sum along the last axis"""
    a = np.asarray(a, f32)
    acc = np.full(a.shape[:-1], start, f32)
    with np.errstate(all="ignore"):
        for i in range(a.shape[-1]):
            acc = acc + a[..., i]
    return acc.astype(f32)


def rotate(P, r, block=256):
    """[n][D] = dot(P[j], r_i), in row blocks (the broadcast product is n D d floats: at most 2^20 of them at a time, which stay in cache --
    at d = 1024 that is a row per step and nearly three times as fast as 64)"""
    r = np.asarray(r, f32).reshape(-1, P.shape[1])
    out = np.empty((r.shape[0], P.shape[0]), f32)
    block = max(1, min(block, (1 << 20) // (P.shape[0] * P.shape[1])))
    for i in range(0, r.shape[0], block):
        out[i:i + block] = dot16(P[None, :, :], r[i:i + block, None, :])
    return out


def rotation(d, seed):
    """the default rotation: Q of the QR decomposition of a seeded Gaussian matrix in f64, cast to f32"""
    g = np.random.default_rng(seed).standard_normal((d, d))
    return np.ascontiguousarray(np.linalg.qr(g)[0].astype(f32))


# ---- build ----------------------------------------------------------------------------------------------------------------------
def encode(x, part_ids, dist_v_c, centroids, P, metric):
    """-> (codes u8 [n][d / 8], add f32 [n], scale f32 [n]); a row without a partition (NONE) gets zeros"""
    x = np.asarray(x, f32); cent = np.asarray(centroids, f32); P = np.asarray(P, f32)
    n, d = x.shape
    assert d % 8 == 0 and P.shape == (d, d)
    part = np.asarray(part_ids).astype(np.uint32)
    has = part != NONE
    codes = np.zeros((n, d // 8), np.uint8); add = np.zeros(n, f32); scale = np.zeros(n, f32)
    if not has.any():
        return codes, add, scale
    with np.errstate(all="ignore"):
        c = cent[part[has]]
        r = (x[has] - c).astype(f32)
        rot = rotate(P, r)
        bits = ~np.signbit(rot)
        codes[has] = np.packbits(bits, axis=1, bitorder="little")
        ip = (seq_sum(np.abs(rot)) / np.sqrt(f32(d))).astype(f32)
        dvc = np.asarray(dist_v_c, f32)[has]
        if metric == "dot":
            res2 = seq_sum(r * r)
            a = (dvc + seq_sum(c * c)).astype(f32)
            sc = -(res2 / ip)
            sc[ip == 0] = f32(-0.0)
        else:
            res2 = dvc
            a = res2
            sc = (f32(-2.0) * res2) / ip
            sc[ip == 0] = f32(0.0)
    add[has] = a; scale[has] = sc.astype(f32)
    return codes, add, scale


# ---- query ----------------------------------------------------------------------------------------------------------------------
def order_key(a):
    b = np.asarray(a, f32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def dist_table(rq):
    """build_dist_table_direct: [d / 4][16]"""
    rq = np.asarray(rq, f32)
    t = np.zeros((rq.size // 4, 16), f32)
    with np.errstate(all="ignore"):
        for j in range(1, 16):
            low = j & -j
            t[:, j] = t[:, j - low] + rq[low.bit_length() - 1::4][:t.shape[0]]
    return t


def quantise_table(t):
    """quantize_dist_table -> (qmin, qmax, e u8 [d / 4][16])"""
    flat = t.ravel()
    keys = order_key(flat)
    qmin, qmax = flat[np.argmin(keys)], flat[np.argmax(keys)]
    if qmin == qmax:
        return qmin, qmax, np.zeros(t.shape, np.uint8)
    with np.errstate(all="ignore"):
        factor = f32(255.0) / f32(qmax - qmin)
        v = ((t - qmin).astype(f32) * factor).astype(f32)
        rounded = np.where(v >= 0, np.floor(v.astype(f64) + 0.5), np.ceil(v.astype(f64) - 0.5))      # half away from zero (exact in f64)
    e = np.where(np.isnan(rounded), 0.0, np.clip(rounded, 0.0, 255.0)).astype(np.uint8)                # Rust's saturating `as u8`
    return qmin, qmax, e


class Query:
    """what dist_calculator prepares for one (query, partition): qr is the residual query, already q - c"""

    def __init__(self, qr, dist_q_c, P, metric):
        qr = np.asarray(qr, f32)
        self.d = qr.size
        self.rq = rotate(np.asarray(P, f32), qr[None])[0]
        self.sum_q = seq_sum(self.rq, -0.0)
        self.sqrt_d = np.sqrt(f32(self.d))
        with np.errstate(all="ignore"):
            self.q_factor = f32(dist_q_c) if metric != "dot" else f32(f32(dist_q_c) - f32(1.0))
        self.table = dist_table(self.rq)
        self.qmin, self.qmax, self.e = quantise_table(self.table)

    def _terms(self, codes):
        codes = np.asarray(codes, np.uint8)
        b = np.arange(codes.shape[1])
        with np.errstate(all="ignore"):
            return (self.table[2 * b, codes & 15] + self.table[2 * b + 1, codes >> 4]).astype(f32)

    def raw_f32(self, codes, start):
        return seq_sum(self._terms(codes), start)

    def raw_packed(self, codes):
        codes = np.asarray(codes, np.uint8)
        b = np.arange(codes.shape[1])
        s = (self.e[2 * b, codes & 15].astype(np.uint32) + self.e[2 * b + 1, codes >> 4].astype(np.uint32)).sum(axis=1, dtype=np.uint32)
        s = np.minimum(s, 65535)           # u16 saturating adds of non-negative terms: the sum saturates
        with np.errstate(all="ignore"):
            rng = f32(f32(self.qmax - self.qmin) / f32(255.0))
            return (s.astype(f32) * rng + f32(f32(self.d // 4) * self.qmin)).astype(f32)

    def finish(self, dist, add, scale):
        with np.errstate(all="ignore"):
            x = ((f32(2.0) * dist - self.sum_q).astype(f32) / self.sqrt_d).astype(f32)
            return ((x * scale).astype(f32) + add + self.q_factor).astype(f32)

    def distance_all(self, codes, add, scale):
        """no prefilter: packed rows through the quantised table, the remainder in f32"""
        n = len(codes)
        np_ = n - n % BATCH
        raw = np.concatenate([self.raw_packed(codes[:np_]), self.raw_f32(codes[np_:], 0.0)]) if n else np.zeros(0, f32)
        return self.finish(raw, np.asarray(add, f32), np.asarray(scale, f32))

    def distance(self, codes, add, scale):
        """DistCalculator::distance of every given row (the prefilter branch)"""
        return self.finish(self.raw_f32(codes, -0.0), np.asarray(add, f32), np.asarray(scale, f32))


def distances(codes, add, scale, qr, dist_q_c, P, metric, quantised):
    """[nq][n]: one partition's rows against nq residual queries"""
    qr = np.asarray(qr, f32).reshape(-1, np.asarray(P).shape[1])
    out = np.empty((qr.shape[0], len(codes)), f32)
    for i in range(qr.shape[0]):
        c = Query(qr[i], np.asarray(dist_q_c, f32)[i], P, metric)
        out[i] = c.distance_all(codes, add, scale) if quantised else c.distance(codes, add, scale)
    return out


# ---- IVF_RQ -----------------------------------------------------------------------------------------------------------------------
def prepare_rows(oracle, x, centroids, metric):
    """-> (part ids, dist_v_c): the partition transform with its distance; rows with a non-finite element have no partition"""
    part, dvc = oracle.assign(x, centroids, metric)
    part[~np.isfinite(np.asarray(x, f64)).all(axis=1)] = NONE
    return part, dvc


def build(oracle, x, centroids, P, metric):
    part, dvc = prepare_rows(oracle, x, centroids, metric)
    codes, add, scale = encode(x, part, dvc, centroids, P, metric)
    return part, codes, add, scale


def search(oracle, codes, add, scale, part_ids, centroids, P, q, k, nprobes, metric, row_ids=None, prefilter=None):
    """codes / add / scale in input order; part_ids [n] (NONE = dropped) -> (ids u64 [nq][k], dists f32 [nq][k])"""
    codes = np.asarray(codes, np.uint8)
    n = codes.shape[0]
    cent = np.asarray(centroids, f32)
    nlist, d = cent.shape
    rid = np.arange(n, dtype=np.uint64) if row_ids is None else np.asarray(row_ids, np.uint64)
    offs, perm = oracle.partition_layout(part_ids, nlist)
    q = np.asarray(q, f32).reshape(-1, d)
    probes, pd = oracle.find_partitions(q, cent, nprobes, metric)
    allow = None if prefilter is None else np.asarray(prefilter, bool)
    out_i = np.full((q.shape[0], k), np.iinfo(np.uint64).max, np.uint64)
    out_d = np.full((q.shape[0], k), np.inf, f32)
    for qi in range(q.shape[0]):
        ci, cd = [], []
        for j, p in enumerate(probes[qi]):
            rows = perm[int(offs[p]):int(offs[p + 1])]
            if len(rows) == 0:
                continue
            calc = Query((q[qi] - cent[p]).astype(f32), pd[qi, j], P, metric)
            if allow is None:
                dist = calc.distance_all(codes[rows], add[rows], scale[rows])
            else:
                r = rid[rows]
                ok = r < allow.size
                ok[ok] = allow[r[ok]]
                rows = rows[ok]
                if len(rows) == 0:
                    continue
                dist = calc.distance(codes[rows], add[rows], scale[rows])
            hi, hd = oracle.heap_topk(dist, rid[rows], k)
            ci.append(hi); cd.append(hd)
        if ci:
            si, sd = oracle.sort_fetch(np.concatenate(ci), np.concatenate(cd), k)
            out_i[qi, :len(si)] = si; out_d[qi, :len(sd)] = sd
    return out_i, out_d


# ---- fixtures -----------------------------------------------------------------------------------------------------------------------
def signed_permutation(d, seed):
    rng = np.random.default_rng(seed)
    P = np.zeros((d, d), f32)
    P[np.arange(d), rng.permutation(d)] = rng.choice([-1.0, 1.0], d)
    return P


def rotations(d, seed=0):
    return {"identity": np.eye(d, dtype=f32), "signed_perm": signed_permutation(d, seed + 1), "qr": rotation(d, seed + 2)}


def permuted_ids(n, seed):
    """explicit row ids unrelated to the storage order"""
    return np.random.default_rng(seed).permutation(n).astype(np.uint64) * np.uint64(3) + np.uint64(7)


def clustered(n, d, nq, seed, centres=8, spread=0.6):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((centres, d)) * 2.0
    x = c[rng.integers(0, centres, n)] + rng.standard_normal((n, d)) * spread
    q = x[rng.integers(0, n, nq)] + rng.standard_normal((nq, d)) * 0.3
    return np.ascontiguousarray(x.astype(f32)), np.ascontiguousarray(q.astype(f32))


def sized_partitions(sizes, d, seed, dup_block=0):
    """rows constructed so that explicit centroids (4 e_p, far apart) receive exactly sizes[p] rows under L2 and under dot (rows of
    partition p: 4 e_p plus small noise; their dot with c_p is ~16, with any other centroid ~0).  dup_block: the first rows of the
    largest partition are one repeated vector.  -> (x f32 [sum sizes][d], centroids f32 [len sizes][d]); rows are shuffled"""
    rng = np.random.default_rng(seed)
    nlist = len(sizes)
    assert nlist <= d
    cent = np.zeros((nlist, d), f32)
    cent[np.arange(nlist), np.arange(nlist)] = 4.0
    rows = []
    for p, s in enumerate(sizes):
        r = cent[p] + rng.standard_normal((s, d)).astype(f32) * f32(0.25)
        if dup_block and s == max(sizes):
            r[:dup_block] = r[0]
        rows.append(r)
    x = np.concatenate(rows).astype(f32)
    return np.ascontiguousarray(x[rng.permutation(len(x))]), cent


# ---- one partition whose storage order is chosen for one query -------------------------------------------------------------------
# The scan kernel (rq.hip: rq_scan_kernel) reads a partition in chunks of CHUNK rows and sorts / truncates its candidates to k once more
# than CHUNK of them have piled up: with every row a candidate the first truncation follows storage position 2 CHUNK - 1, and from
# then on a row enters only with a key <= the k-th key of that truncation.  The orders below put rows where that threshold, and the
# tie it may have cut, decide the answer.
CHUNK = 256
FIRST_CUT = 2 * CHUNK
TIE = 40                               # copies in the tie block of tie_then_closer / tie_then_displaced
ORDERS = {                             # order -> (rows of the partition, the k it is defined for)
    "descending": (832, (2, 10, 128)),
    "ascending": (832, (2, 10, 128)),
    "staircase": (832, (2, 10, 128)),
    "tie_then_closer": (813, (2, 10)),
    "tie_then_displaced": (813, (2, 10)),
    "tie_across_chunk": (813, (2, 10)),
    "tie_wide": (813, (128,)),
    "tie_across_remainder": (813, (2, 10)),
}


def kth_is_tied(keys, k):
    """are more rows at the k-th smallest key than fit into k?  (the heap, not the order by position, then decides which stay)"""
    s = np.sort(np.asarray(keys))
    return len(s) > k and s[k - 1] == s[k]


class _Redraw(Exception):
    pass


def ordered_partition(oracle, order, metric, k, d=64, prefiltered=False, seed=0, small=40):
    """Partition 0 of two (explicit centroids 4 e_0, 4 e_1; partition 1 holds `small` rows, so that nprobes = 2 has something to
    merge): ORDERS[order][0] rows stored in `order` for the design query q, by the keys of the branch the search will use --
    Query.distance_all without a prefilter, Query.distance with an all-selected one.  A row's assignment, code and factors do not
    depend on where it is stored; its distance does only through the packed / remainder split, so the last N % 32 rows (the ones
    farthest by the remainder branch) are fixed first and only the rows before them are ordered.  Every property an order is for
    is asserted here, on the keys recomputed from the final layout.  A draw in which two generated rows share a key, or in which
    the heap of tie_then_closer happens to keep the k first rows by (key, position), is drawn again: the fixture returned has neither.
    -> dict: x [N + small][d] (input order = storage order), cent [2][d], P, q [d], keys u32 [N] (order_key of the design query's
    distance to partition 0's rows in storage order), cut_tie (more rows tie at the k-th key than fit into k), N"""
    for draw in range(16):
        try:
            return _ordered_partition(oracle, order, metric, k, d, prefiltered, seed, small, draw)
        except _Redraw:
            pass
    raise AssertionError("no usable draw")


def _ordered_partition(oracle, order, metric, k, d, prefiltered, seed, small, draw):
    N = ORDERS[order][0]
    assert k in ORDERS[order][1] and 2 <= k and d >= 2
    cent = np.zeros((2, d), f32)
    cent[0, 0] = cent[1, 1] = 4.0
    P = rotation(d, seed + 5)
    rem = N % BATCH
    head_n = N - rem
    rng = np.random.default_rng([seed, k, int(prefiltered), list(ORDERS).index(order), int(metric == "dot"), draw])
    gauss = lambda n: rng.standard_normal((n, d)).astype(f32) * f32(0.25)
    rows, other, q = (cent[0] + gauss(N)).astype(f32), (cent[1] + gauss(small)).astype(f32), (cent[0] + gauss(1)[0] + gauss(1)[0]).astype(f32)
    pr, pd = oracle.find_partitions(q[None], cent, 2, metric)
    assert pr[0, 0] == 0, "the design query's nearest partition is partition 0"
    calc = Query(q - cent[0], pd[0, 0], P, metric)
    part, codes, add, scale = build(oracle, rows, cent, P, metric)
    assert (part == 0).all()
    if prefiltered:
        kh = kt = order_key(calc.distance(codes, add, scale))
    else:
        kh = order_key(calc.finish(calc.raw_packed(codes), add, scale))
        kt = order_key(calc.finish(calc.raw_f32(codes, 0.0), add, scale))
    by_tail = np.argsort(kt, kind="stable")
    tail = by_tail[head_n:]                                # the remainder rows: the farthest by the branch they will take
    asc = by_tail[:head_n][np.argsort(kh[by_tail[:head_n]], kind="stable")]      # the rows before them, nearest first
    if len(np.unique(np.concatenate([kh[asc], kt[tail]]))) != N:
        raise _Redraw("two generated rows share a key")

    def tie_block(j, copies, into_tail=0):
        """the row at rank j becomes `copies` rows (the farthest rows are overwritten; `into_tail` of them in the remainder)"""
        src = asc[j]
        dst = np.concatenate([asc[head_n - (copies - 1 - into_tail):], tail[:into_tail]])
        rows[dst] = rows[src]
        rest = asc[j + 1:head_n - (copies - 1 - into_tail)]
        return np.concatenate([[src], dst[:copies - 1 - into_tail]]), rest[rng.permutation(len(rest))]

    if order == "descending":
        assert rem == 0
        head = asc[::-1]
    elif order == "ascending":
        assert rem == 0
        head = asc
    elif order == "staircase":
        assert rem == 0
        head = np.concatenate([asc[:k - 1], asc[k - 1:][::-1]])
    elif order == "tie_then_closer":
        j = k // 2
        tie, rest = tie_block(j, TIE)
        near = asc[:j]
        head = np.concatenate([rest[:100], tie, rest[100:600 - TIE], near, rest[600 - TIE:]])
    elif order == "tie_then_displaced":
        j = k // 2                                             # nearer rows ahead of the first truncation; k more come after it
        tie, rest = tie_block(j + k, TIE)
        near, early = asc[:k], asc[k:k + j]
        head = np.concatenate([rest[:100], tie, early, rest[100:600 - TIE - j], near, rest[600 - TIE - j:]])
    elif order == "tie_across_chunk":
        tie, rest = tie_block(k // 2, 13)
        rest = np.concatenate([asc[:k // 2], rest])
        rest = rest[rng.permutation(len(rest))]
        head = np.concatenate([rest[:CHUNK - 6], tie, rest[CHUNK - 6:]])
    elif order == "tie_wide":
        tie, rest = tie_block(k // 2, 300)
        rest = np.concatenate([asc[:k // 2], rest])
        rest = rest[rng.permutation(len(rest))]
        head = np.concatenate([rest[:100], tie, rest[100:]])
    elif order == "tie_across_remainder":
        assert rem == 13
        tie, rest = tie_block(k // 2, 14, into_tail=7)
        rest = np.concatenate([asc[:k // 2], rest])
        rest = rest[rng.permutation(len(rest))]
        head = np.concatenate([rest, tie])
    else:
        raise ValueError(order)
    layout = np.concatenate([head, tail]).astype(np.int64)
    assert len(layout) == N and len(np.unique(layout)) == N
    x = np.ascontiguousarray(np.concatenate([rows[layout], other]).astype(f32))

    # ---- the final layout, from scratch -------------------------------------------------------------------------------------------
    part, codes, add, scale = build(oracle, x, cent, P, metric)
    assert (part[:N] == 0).all() and (part[N:] == 1).all()
    dist = calc.distance(codes[:N], add[:N], scale[:N]) if prefiltered else calc.distance_all(codes[:N], add[:N], scale[:N])
    keys = order_key(dist)
    where = np.empty(N, np.int64)
    where[layout] = np.arange(N)                               # storage position of every generated row
    kth = lambda upto: np.sort(keys[:upto])[k - 1]             # what a truncation after `upto` rows leaves as the threshold
    assert N > FIRST_CUT + CHUNK, "the scan passes two chunks after its first truncation"
    if order == "descending":
        assert len(np.unique(keys)) == N
        for p in range(FIRST_CUT, N):
            assert keys[p] < keys[:p].min()                    # every later row enters, at rank 0
    elif order == "ascending":
        assert (keys[FIRST_CUT:] > kth(FIRST_CUT)).all()       # nothing enters after the first truncation
    elif order == "staircase":
        assert len(np.unique(keys)) == N
        for p in range(FIRST_CUT, N):
            s = np.sort(keys[:p])
            assert s[k - 2] < keys[p] < s[k - 1]               # every later row is exactly the new k-th: the threshold falls step by step
    else:
        tk = keys[where[tie[0]]]
        tied = np.nonzero(keys == tk)[0]
    if order in ("tie_then_closer", "tie_then_displaced"):
        assert len(tied) == TIE and (tied == where[tie]).all() and tied.max() < CHUNK
        assert where[near].min() >= FIRST_CUT and (keys[where[near]] < tk).all()
        first = np.sort(keys[:FIRST_CUT])
        assert first[k - 1] == tk and first[k] == tk           # the first truncation cuts the tie
        final = np.sort(keys)
        if order == "tie_then_closer":
            assert (keys < tk).sum() == k // 2 and final[k - 1] == tk and final[k] == tk
            pos = np.arange(N, dtype=np.uint64)
            heap = set(oracle.heap_topk(dist, pos, k)[0].tolist())
            by_position = set(np.lexsort((pos, keys))[:k].tolist())
            assert len(heap) == k
            if heap == by_position:
                raise _Redraw("the heap happens to keep the first copies by position")
        else:
            assert (keys < tk).sum() >= k and final[k - 1] < tk and final[k - 1] != final[k]
    elif order == "tie_across_chunk":
        assert (tied == np.arange(CHUNK - 6, CHUNK + 7)).all() and kth_is_tied(keys, k) and np.sort(keys)[k - 1] == tk
    elif order == "tie_wide":
        assert (tied == np.arange(100, 400)).all() and kth_is_tied(keys, k) and np.sort(keys)[k - 1] == tk
    elif order == "tie_across_remainder":
        copies = np.arange(head_n - 7, head_n + 7)
        assert (x[copies] == x[copies[0]]).all()
        if prefiltered:
            assert (tied == copies).all() and kth_is_tied(keys, k) and np.sort(keys)[k - 1] == tk
        else:
            assert (tied == copies[:7]).all() and len(np.unique(keys[copies[7:]])) == 1      # two branches: two keys
    return {"x": x, "cent": cent, "P": P, "q": q, "keys": keys, "cut_tie": bool(kth_is_tied(keys, k)), "N": N}
