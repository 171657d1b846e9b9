"""The IVF-PQ transform (lance_hip_ivfpq_encode, lance_amd/csrc/build.hip:401-497) on the routes behind the single-pass kernel: which
route serves a call, and fixtures that hold the edges a wrong code byte hides behind.  numpy only; imported by
test_encode_routes_spec.py (CPU, with the oracle) and test_zz_gpu_encode_routes.py.

Routes (build.hip:430-496):
  X  xform_fused            one kernel for the whole chain
  T  xform_tail             d > 128: K-tiled coarse assign, then residual + encode per 128-column block
  P  pq_mfma encode         pq_mfma_estep_kernel<SD, ENC> + pq_mfma_fix_kernel (counters: pq_mfma_encode and encode_fused)
  L  lane-per-row encode    encode_fused_kernel                                (counters: lane_encode and encode_fused)
  S  staged                 launch_assign, residual_kernel, pq_encode_launch (+ pack_nibbles_kernel at 4 bits)

Every case carries: the `spoil` rows (NaN row, +inf, -inf, zero row), duplicated centroids (two, three, five of a kind), and in every
sub-quantiser three duplicated codewords spread over the fix kernel's 64-codeword groups and over the blockIdx.z tiles of the exact
kernels.  The codebook is drawn from the residual sub-vectors of the case's own finite rows (the rows themselves under dot), so every
duplicated codeword is at distance 0 from the row it was drawn from: the tie exists by construction and the reference keeps the
lower index.

What the conditions of test_encode_routes_spec.py cannot ask of a case, and why:
  * int8 columns hold no non-finite value and every finite row gets a partition: they have no row without one.
  * n = 1: the single row is finite (it must reach the encoder to test the one valid lane), so there is no row without a partition;
    its sub-vectors are codewords themselves (that is its tie), so rounding the residual to binary16 cannot move it to another code.
  * nlist = 1: there is no second centroid distance to tie with.
"""
import collections
import zlib

import numpy as np

from test_zz_gpu_xform_fused import clustered, dup_centroids, oracle_chain, spoil

f32 = np.float32
NONE = 0xFFFFFFFF

Case = collections.namedtuple("Case", "route kind metric d m nbits n nlist extras")


def tag(c):
    return f"{c.route}:{c.kind}:{c.metric}:d{c.d}:m{c.m}:b{c.nbits}:n{c.n}:k{c.nlist}" + "".join(":" + e for e in c.extras)


# ---- which route serves a call (aligned operands) --------------------------------------------------------------------------------------
def expected_route(kind, metric, d, m, nbits, n, nlist):
    """"X" | "T" | "P" | "L" | "S": a transcription of the gates of lance_hip_ivfpq_encode for operands on the 16-byte grid"""
    sd = d // m
    f16 = kind == "float16"
    lanes32 = f16 and metric == "dot" and d > 16                                   # build.hip:423

    def xform_fused(met, lanes):                                                   # xform_fused.hip:964-978
        if lanes or nbits != 8 or met not in ("l2", "dot"):                        #   :968-969
            return False
        if d % 16 != 0 or d < 16 or d > 128 or sd not in (4, 8, 16):               #   :970-972
            return False
        return n >= 2048 and nlist >= 32                                           #   :973

    def xform_tail():                                                              # xform_fused.hip:1107-1116
        if nbits != 8 or m > 127 or d <= 128 or n < 2048 or sd not in (4, 8, 16):  #   :1110-1112
            return False
        return d % 16 == 0 and (d % 128 == 0 or sd == 16)                          #   :1113

    def mfma_assign_native():                                                      # pairwise.hip:249-253 -> mfma_assign.hip:779-788
        if d > 128:
            return False                                                           #   mfma_assign.hip:772: f16 / int8 rows of this width arrive as f32
        return d % 16 == 0 and d >= 16 and nlist >= 32 and n >= 2048               #   :783-784

    if metric != "cosine" and xform_fused(metric, lanes32):                        # build.hip:430-431
        return "X"
    mfma_enc = metric != "cosine" and nbits == 8 and sd in (4, 8, 16) and n >= 2048 and d % 4 == 0     # build.hip:435, pq_mfma.hip:339-344
    lane = nbits == 8 and ((d == 128 and sd in (4, 8, 16)) or (d == 64 and sd in (4, 8)))               # encode_fused.hip:107-109
    native = metric != "cosine" and (mfma_enc or lane)                             # build.hip:436
    if metric == "cosine":
        if xform_fused("l2", False):                                               # build.hip:468: the f32 unit rows, L2
            return "X"
        f32_view = True                                                            # build.hip:447-467: the normalised copy
    else:
        assign_native = native and (kind == "float32" or mfma_assign_native())     # build.hip:438-442
        f32_view = kind == "float32" or not assign_native                          # build.hip:443-446, :476
    if f32_view and xform_tail():                                                  # build.hip:477
        return "T"
    if native:                                                                     # build.hip:481-483
        return "P" if mfma_enc else "L"
    return "S"


# ---- fixture builders ------------------------------------------------------------------------------------------------------------------
def dup_centroids_small(cent):
    """nlist < 31: two of a kind and three of a kind (the smaller index wins)"""
    cent = cent.copy()
    k = cent.shape[0]
    if k >= 9:
        cent[2] = cent[k - 2]
        cent[1] = cent[7]; cent[5] = cent[7]
    return cent


def dup_any(cent):
    return dup_centroids(cent) if cent.shape[0] >= 31 else dup_centroids_small(cent)


DUPS8 = ((7, 100), (3, 67), (255, 0))       # (copy, source): different 64-codeword groups (a fix-kernel lane owns c = 64 u + lane) and
DUPS4 = ((3, 12), (15, 0))                  # both sides of every blockIdx.z tile boundary of launch_fixed (CT = 128 at SD 64, 64 at 128)


def dup_codewords_spread(cb):
    cb = cb.copy()
    for dst, src in (DUPS8 if cb.shape[1] == 256 else DUPS4):
        cb[:, dst] = cb[:, src]
    return cb


def f16_overflow_rows(x, cent, rows):
    """f16 column under L2: every centroid at -40 in column 0, `rows` at the largest binary16 in column 0.  The f32 distances stay finite
    (the rows keep a partition); the binary16 residual 65504 + 40 rounds to +inf, so sub-quantiser 0 encodes 0 by unwrap_or(0)"""
    x = x.copy(); cent = cent.copy()
    cent[:, 0] = -40.0
    x[list(rows), 0] = 65504.0
    return x, cent


def nonfinite_codebook(cb):
    cb = cb.copy()
    cb[0, 9, 1] = np.inf
    cb[1, 200, 0] = np.nan
    return cb


def seed_of(c):
    return zlib.crc32(tag(c).encode()) & 0x7FFFFFFF


def raw_rows(c, rows, seed):
    sd = c.d // c.m
    if c.kind == "int8":
        return np.clip(clustered(rows, c.d, seed, scale=30.0, noise=14.0) - 40, -128, 127).astype(np.int8)
    if c.kind == "float16":
        return clustered(rows, c.d, seed, scale=1.5, noise=0.6, integer=False).astype(np.float16)
    if "integer" in c.extras:       # short sub-vectors: a wide alphabet still ties; long ones need a narrow alphabet for equal integer sums
        x = clustered(rows, c.d, seed, noise=12.0 if sd <= 16 else 0.8, integer=True).astype(f32)
    else:
        x = clustered(rows, c.d, seed, scale=6.0, noise=2.5, integer=False).astype(f32)
    if c.metric == "dot":           # mixed signs: rows then prefer different centroids under the inner product
        x = (x - np.rint(x.mean(axis=0))).astype(f32)
    return x


def unpack4(codes):
    """[n][m/2] packed -> [n][m]: byte b = (code[2b+1] << 4) | code[2b] (pq.rs:168-172)"""
    out = np.empty((codes.shape[0], codes.shape[1] * 2), np.uint8)
    out[:, 0::2] = codes & 15
    out[:, 1::2] = codes >> 4
    return out


def chain(oracle, x, cent, cb, metric, nbits=8):
    """oracle_chain of test_zz_gpu_xform_fused.py; 4-bit codebooks take the same chain with the packed encoder"""
    if nbits == 8:
        return oracle_chain(oracle, x, cent, cb, metric)
    part, _, loss = oracle_chain(oracle, x, cent, np.repeat(cb, 16, axis=1), metric)      # (ids and loss do not depend on the codebook)
    xs = oracle.normalize(x) if metric == "cosine" else x
    keep = oracle.is_finite(xs)
    xk = np.ascontiguousarray(xs[keep])
    res = oracle.residual(xk, cent, np.where(part[keep] == NONE, 0, part[keep])) if metric != "dot" else xk
    codes = np.zeros((x.shape[0], cb.shape[0] // 2), np.uint8)
    codes[keep] = oracle.pq_encode(res, cb, "l2", nbits=4)
    return part, codes, loss


Prepared = collections.namedtuple("Prepared", "case x cent cb part codes loss stats")
_CACHE = {}


def prepared(oracle, c):
    """the case's operands, the oracle's answer and the reference-side edge counts; cached per process"""
    t = tag(c)
    if t not in _CACHE:
        _CACHE[t] = _prepare(oracle, c)
    return _CACHE[t]


def _partitioned(oracle, c, xs, cent):
    """(rows of xs that are finite and get a partition, their partition ids)"""
    sm = "l2" if c.metric == "cosine" else c.metric
    fin = np.nonzero(oracle.is_finite(xs))[0]
    pk, _ = oracle.assign(np.ascontiguousarray(xs[fin]), cent, sm)
    ok = pk != NONE
    return fin[ok], pk[ok]


def _prepare(oracle, c):
    seed = seed_of(c)
    rng = np.random.default_rng(seed + 1)
    kc = 1 << c.nbits
    sd = c.d // c.m
    pool = raw_rows(c, max(c.n, 400), seed)       # n = 1: the model is drawn from rows that are not in the column
    x = pool[:c.n].copy()
    if c.n >= 101:
        x = spoil(x)
        if c.metric == "cosine":
            x[100] = 1.0          # a zero row has no direction: normalize gives NaN and the row is dropped -- keep one ordinary row too
            x[101] = 0.0
        pool = x
    else:
        pool = np.concatenate([x, pool[c.n:]])
    over = ()
    if "overflow" in c.extras:
        over = (5, 130, c.n - 2)
    ps = oracle.normalize(pool) if c.metric == "cosine" else pool
    fin = np.nonzero(oracle.is_finite(ps))[0]
    fin = fin[~np.isin(fin, over)]
    pick = rng.choice(fin[fin < c.n] if (fin < c.n).sum() >= c.nlist else fin, c.nlist, replace=False)
    cent = np.ascontiguousarray(ps[pick]).astype(f32)
    if c.kind == "int8":
        cent = cent + rng.normal(0, 0.25, cent.shape).astype(f32)
    if c.n < 101 and c.nlist >= 31:
        cent[30] = ps[0].astype(f32) * (f32(2.0) if c.metric == "dot" else f32(1.0))       # the five of a kind are the row's nearest
    if c.kind == "float16" and c.metric == "l2":
        # every fourth column of every centroid at -200, far from the rows: the column adds the same to every centroid's distance (the
        # partitions stay spread), and x - c near 200 has a binary16 spacing of 2^-3 against a noise of 0.6 in the rows, so rounding
        # the residual as half::f16 does (residual.rs:96) moves sub-vectors across codeword boundaries
        cent[:, 1::4] = f32(-200.0)
    cent = dup_any(cent)
    if c.kind == "float16":
        cent = cent.astype(np.float16)
    if over:
        x, cent = f16_overflow_rows(x, cent, over)
        pool = x
        ps = pool
    # the codebook: residual sub-vectors of finite rows with a partition, the overflow rows excepted
    rows, pk = _partitioned(oracle, c, ps, cent)
    sel = ~np.isin(rows, over)
    rows, pk = rows[sel], pk[sel]
    src = np.ascontiguousarray(ps[rows])
    res = oracle.residual(src, cent, pk) if c.metric != "dot" else src
    res = np.asarray(res, f32)
    inside = np.nonzero(rows < c.n)[0]            # rows of the column itself
    cands = inside[: max(kc // 2, inside.size // 2)] if "integer" in c.extras and inside.size >= kc else np.arange(rows.size)
    idx = np.stack([rng.choice(cands, kc, replace=cands.size < kc) for _ in range(c.m)])
    for i in range(c.m):                          # the duplicated codewords come from rows of the column: distance 0 -> a tie
        for j, (_, s) in enumerate(DUPS8 if kc == 256 else DUPS4):
            idx[i, s] = inside[(i * 7 + j * 3) % inside.size]
    cb = np.stack([res[idx[i]][:, i * sd:(i + 1) * sd] for i in range(c.m)]).astype(f32)
    cb = dup_codewords_spread(cb)
    if "nonfinite_cb" in c.extras:
        cb = nonfinite_codebook(cb)
    if c.kind == "float16":
        cb = cb.astype(np.float16)
    part, codes, loss = chain(oracle, x, cent, cb, c.metric, c.nbits)
    stats = edge_stats(oracle, c, x, cent, cb, part, codes, over)
    return Prepared(c, x, cent, cb, part, codes, loss, stats)


def edge_stats(oracle, c, x, cent, cb, part, codes, over):
    """counts taken from the oracle's outputs alone.  A tie of the two smallest distances is found by asking the oracle again with the
    centroids / codewords in reverse order: its argmin keeps the first of equal minima, so the answers differ exactly where the minimum
    is attained twice with equal bits."""
    kc = 1 << c.nbits
    sd = c.d // c.m
    sm = "l2" if c.metric == "cosine" else c.metric
    xs = oracle.normalize(x) if c.metric == "cosine" else x
    keep = oracle.is_finite(xs)
    s = {"rows": c.n, "no_partition": int((part == NONE).sum())}
    ok = np.nonzero(part != NONE)[0]
    xo = np.ascontiguousarray(xs[ok])
    rp, _ = oracle.assign(xo, np.ascontiguousarray(cent[::-1]), sm)
    s["centroid_ties"] = int((part[ok] != (c.nlist - 1 - rp)).sum())
    res = oracle.residual(xo, cent, part[ok]) if c.metric != "dot" else xo          # (f16 columns: rounded to binary16)
    resf = np.asarray(res, f32)
    sub_ok = np.isfinite(resf.reshape(len(ok), c.m, sd)).all(axis=2)
    fwd = codes[ok] if c.nbits == 8 else unpack4(codes[ok])
    rev = oracle.pq_encode(res, np.ascontiguousarray(cb[:, ::-1]), "l2", nbits=c.nbits)
    rev = (kc - 1) - (rev if c.nbits == 8 else unpack4(rev)).astype(np.int64)
    tie = (fwd != rev) & sub_ok
    s["codeword_ties"] = int(tie.sum())
    cbf = np.asarray(cb, f32)
    r, i = np.nonzero(tie)
    same = (cbf[i, fwd[r, i]] == cbf[i, rev[r, i]]).all(axis=1)          # the two ends of the tie are copies of one codeword
    s["codeword_ties_distinct"] = int((~same).sum())
    if over:
        pos = np.nonzero(np.isin(ok, over))[0]
        r16 = resf[pos, 0]
        s["overflow_rows"] = int((np.isinf(r16) & (fwd[pos, 0] == 0)).sum()) if pos.size == len(over) else -1
        exact = oracle.residual(xo[pos].astype(f32), cent.astype(f32), part[ok][pos])
        s["overflow_changed"] = int((oracle.pq_encode(exact, cbf, "l2")[:, 0] != 0).sum())
    if c.kind == "float16" and sm == "l2":
        exact = oracle.residual(xo.astype(f32), cent.astype(f32), part[ok])
        s["rounding_changes"] = int((oracle.pq_encode(exact, cbf, "l2", nbits=c.nbits) != codes[ok]).sum())
    assert keep.sum() >= len(ok)
    return s


# ---- lance_hip_pq_encode alone (the call rebalance.hip makes on the rows of a split partition) -----------------------------------------------
PqCase = collections.namedtuple("PqCase", "metric d m n")
PQ_CASES = [PqCase(metric, d, m, n) for metric in ("l2", "dot") for n in (300, 2100) for d, m in ((64, 8), (128, 2), (96, 8))]

PqPrepared = collections.namedtuple("PqPrepared", "case x cb codes stats")


def pq_prepared(oracle, c):
    t = ("pq",) + tuple(c)
    if t not in _CACHE:
        sd = c.d // c.m
        seed = zlib.crc32(repr(t).encode()) & 0x7FFFFFFF
        rng = np.random.default_rng(seed + 1)
        # a narrow alphabet around each cluster centre: equal integer sums between distinct codewords
        x = clustered(c.n, c.d, seed, noise=2.0 if sd <= 16 else 0.8, integer=True).astype(f32)
        x = (x - np.rint(x.mean(axis=0))).astype(f32)
        idx = rng.choice(c.n // 2, (c.m, 256), replace=True)
        cb = dup_codewords_spread(np.stack([x[idx[i]][:, i * sd:(i + 1) * sd] for i in range(c.m)]).astype(f32))
        codes = oracle.pq_encode(x, cb, c.metric)
        rev = 255 - oracle.pq_encode(x, np.ascontiguousarray(cb[:, ::-1]), c.metric).astype(np.int64)
        r, i = np.nonzero(codes != rev)
        same = (cb[i, codes[r, i]] == cb[i, rev[r, i]]).all(axis=1)
        _CACHE[t] = PqPrepared(c, x, cb, codes, {"codeword_ties": int(r.size), "codeword_ties_distinct": int((~same).sum())})
    return _CACHE[t]


# ---- the case table --------------------------------------------------------------------------------------------------------------------
def _cases():
    out = []

    def add(route, kind, metric, d, m, n, nlist, *extras, nbits=8):
        out.append(Case(route, kind, metric, d, m, nbits, n, nlist, tuple(extras)))

    # route P: a workgroup covers 1024 rows, a wave 32; 2048 is the gate
    for n in (2048, 2177):
        for metric in ("l2", "dot"):
            add("P", "float32", metric, 64, 16, n, 24, "integer")                 # sub-dimension 4
            add("P", "float32", metric, 40, 5, n, 40)                             # sub-dimension 8; d % 16 != 0: the coarse assign is wide.hip's
        for d, m, nlist in ((128, 16, 40), (64, 4, 33)):                          # lanes32: ma_top3_kernel<.., __half>, the encode has no residual
            add("P", "float16", "dot", d, m, n, nlist)
        add("P", "float16", "l2", 128, 8, n, 24, "overflow")                      # sub-dimension 16
        add("P", "float16", "l2", 48, 12, n, 24)
        for metric in ("l2", "dot"):
            add("P", "int8", metric, 40, 10, n, 40)
        add("P", "int8", "l2", 48, 6, n, 24)
    add("P", "float32", "l2", 200, 25, 2177, 64)                                  # T refuses d % 16 == 8; K-tiled matrix-core coarse assign
    add("P", "float32", "l2", 64, 16, 2177, 24, "nonfinite_cb")
    # route L: a workgroup covers 256 rows
    shapes = ((128, 32), (128, 16), (128, 8), (64, 16), (64, 8))
    for n in (1, 255, 257, 2047):
        for metric in ("l2", "dot"):
            for d, m in shapes:
                add("L", "float32", metric, d, m, n, 40)
                if n == 255:
                    add("L", "float32", metric, d, m, n, 1)
            for d, m in ((128, 32), (64, 8)):
                add("L", "int8", metric, d, m, n, 40)
        for d, m in ((128, 16), (64, 8)):
            add("L", "float16", "l2", d, m, n, 40, *(("overflow",) if n == 257 else ()))
        add("L", "float16", "dot", 64, 16, n, 40)                                 # lanes32 changes the coarse assign, not the route, below 2048 rows
    add("L", "float32", "l2", 128, 16, 2047, 40, "integer")
    # route S
    for metric in ("l2", "dot"):
        add("S", "float32", metric, 32, 4, 300, 24)
    for n in (300, 2100):
        add("S", "float32", "l2", 96, 8, n, 24)                                   # sub-dimension 12: wide.hip's argmin with batches = m
        add("S", "float32", "l2", 128, 2, n, 24, "integer")                       # sub-dimension 64: two blockIdx.z tiles + argmin_merge_kernel
    add("S", "float32", "l2", 128, 1, 300, 24, "integer")                         # sub-dimension 128: four tiles
    for n in (2177, 301):
        add("S", "float32", "l2", 64, 16, n, 24, nbits=4)                         # pack_nibbles_kernel, odd row count
    for n in (2100, 300):
        for kind in ("float32", "float16"):
            add("S", kind, "cosine", 64, 8, n, 24)                                # n = 2100: pq_mfma in training mode writes the codes
    add("S", "float32", "cosine", 40, 5, 2100, 40)
    return out


CASES = _cases()


def cases_of(route, kind):
    return [c for c in CASES if c.route == route and c.kind == kind]
