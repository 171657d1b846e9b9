"""Shared by tests/test_rq_spec.py (CPU), tests/test_rq_kernels_cpu.py (CPU) and tests/test_zz_gpu_rq.py (GPU): the CPU specification
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
    """[n][D] = dot(P[j], r_i), in row blocks (the broadcast product is n D d floats)"""
    r = np.asarray(r, f32).reshape(-1, P.shape[1])
    out = np.empty((r.shape[0], P.shape[0]), f32)
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
