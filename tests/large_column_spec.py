"""Shared by tests/test_large_column_spec.py (CPU) and tests/test_zz_gpu_large_columns.py (GPU): columns whose element offsets need more
than 31 bits and whose byte offsets need more than 32, with an expected answer for EVERY row although the oracle only ever sees a few
thousand rows.  No such column is materialised on the host: it is built on the device, the oracle works on its ingredients.

Two constructions, one column:

  periodic filler   row r of the column is base[r mod P], P = 4099.  P is prime: an offset wrapped at any power of two lands on another
                    base row (2^j mod 4099 != 0), so a kernel that loses a high bit of `row * d` reads a row whose expected output differs.
                    base is real-valued (standard_normal * 3 around a few dozen centres, * 0.7 in f16, integers in int8) and holds the
                    spoilers of the small tests: one NaN row, one all-zero row, two equal rows (no NaN in int8).
  planted windows   NPLANT distinct planted rows overwrite windows of consecutive positions: window 0 at row 0, one window straddling
                    every boundary row the case names, the last window ending at the column's last row.  The planted rows of every
                    window are different rows, so a high row aliased to a low one is visible.

An operation that is independent per row has the expected output  oracle(base)  tiled, with  oracle(planted)  written over the windows
(expected_rows / assemble).  A top-k search has the oracle's answer over the planted rows alone, with their column positions as row
ids (the position table is ascending, hence monotone inside every tie group: the (distance, row id) order survives) -- provided the
conditions of `planted_answer` hold, which it asserts: every filler row is strictly farther than the k-th planted row, no returned
distance is NaN, every query has an answer beyond every boundary, and a quarter of it in the last window.  Planted rows and queries lie
around +SHIFT in every coordinate, the filler around 0: under dot and cosine they have one sign and a large product, the filler has none.

tests/test_large_column_spec.py runs both constructions at a scaled-down n, where the oracle processes the whole materialised column,
and checks the table's arithmetic.  CASES is the table: n, the boundaries crossed (row at which the offset passes the boundary), and the
device memory a case needs (column + outputs + the scratch its route allocates, 25 % arena headroom included)."""
import functools

import numpy as np

import multivec_spec
import oracle as O
import refine_spec
import rq_spec
import sq_spec

f32 = np.float32
P = 4099
GIB = 1 << 30
MEM_LIMIT = 24 * GIB
WIN = 256                        # rows of window 0 and of every boundary window
LAST = 1536                      # rows of the last window: 60 % of the planted rows at two boundary windows
ELEM = {"f32": 4, "f16": 2, "i8": 1, "u8": 1}
NPDT = {"f32": np.float32, "f16": np.float16, "i8": np.int8}
SHIFT = {"f32": 25.0, "f16": 4.0, "i8": 90.0}
NAN_ROW, ZERO_ROW, DUP_ROWS = 17, 100, (200, 3001)
# The column that is SEARCHED under cosine (d = 256) cannot hold an all-zero row: its cosine distance is 0 / 0, a NaN whose sign belongs
# to the machine that made it (negative on the oracle's host: first in the total order, ahead of every planted row), so the conditions
# of planted_answer cannot hold with it.  There the spoiler keeps one element, -1: a row of 255 zeros, farther than every planted row.
COSINE_DIMS = (256,)


def _is_prime(v):
    return v > 1 and all(v % i for i in range(2, int(v ** 0.5) + 1))


assert _is_prime(P)


# ---- the case table -----------------------------------------------------------------------------------------------------------------
class Case(dict):
    """name, kind, d, n, crosses: [(what, boundary value, unit, row)], need: device bytes at the peak, peak_of: what the peak is made of"""
    __getattr__ = dict.__getitem__

    @property
    def boundary_rows(self):
        return sorted({row for _, _, _, row in self.crosses})


def _scratch(b):
    return b + b // 4            # the context's arena keeps 25 % headroom on every block (ctx.cpp)


def _case(name, kind, d, n, crosses, peak_parts):
    col = n * d * ELEM[kind]
    parts = dict(column=col, **peak_parts)
    return Case(name=name, kind=kind, d=d, n=n, crosses=crosses, column_bytes=col, need=sum(parts.values()), peak_of=parts)


def chunk_rows(n, m):
    """the row chunk of the fused transform (xform_fused.hip: launch_xform_fused / launch_xform_tail)"""
    return max(128, min(n, 1 << 24, ((64 << 20) // m) // 128 * 128))


_N128 = (1 << 24) + P
_N256 = (1 << 23) + P
_N8 = (1 << 25) + P
_NCH32 = 2 * chunk_rows(1 << 30, 32) + P
_NCH96 = 2 * chunk_rows(1 << 30, 96) + P

CASES = {c.name: c for c in [
    # the largest peak of the row: ivfpq_encode under cosine (the normalised f32 copy in the arena) or residual + pq_encode (the
    # residual tensor beside the column), each with the part ids / distances / codes and the comparison's working set
    _case("f32-128", "f32", 128, _N128,
          [("bytes", 1 << 32, 4, 1 << 23), ("elements", 1 << 31, 1, 1 << 24), ("bytes", 1 << 33, 4, 1 << 24)],
          dict(second_column=_scratch(_N128 * 128 * 4), outputs=_N128 * (4 + 4 + 32) + _scratch(_N128 * 8), compare=1 * GIB)),
    _case("chunk-m32", "f32", 128, _NCH32, [("chunk", 2 * chunk_rows(1 << 30, 32), 0, 2 * chunk_rows(1 << 30, 32))],
          dict(scratch=_scratch(chunk_rows(_NCH32, 32) * 32 * 4) + _scratch(_NCH32 * 8), outputs=_NCH32 * (4 + 32), compare=1 * GIB)),
    _case("chunk-m96", "f32", 384, _NCH96, [("chunk", 2 * chunk_rows(1 << 30, 96), 0, 2 * chunk_rows(1 << 30, 96))],
          dict(scratch=_scratch(chunk_rows(_NCH96, 96) * 96 * 4) + _scratch(_NCH96 * (8 + 4 * 4)) + 2 * _scratch(_NCH96 * 384 * 2),
               outputs=_NCH96 * (4 + 96), compare=1 * GIB)),
    # assign on the wide route: two bf16 planes of the rows; flat_topk: one bf16 plane (exact size) + the row norms
    _case("f32-256", "f32", 256, _N256,
          [("bytes", 1 << 32, 4, 1 << 22), ("elements", 1 << 31, 1, 1 << 23), ("bytes", 1 << 33, 4, 1 << 23)],
          dict(planes=2 * _scratch(_N256 * 256 * 2), scratch=_scratch(_N256 * 4) * 6, outputs=_N256 * 8, compare=1 * GIB)),
    # assign widens the column to f32 in the arena
    _case("f16-128", "f16", 128, _N128, [("elements", 1 << 31, 1, 1 << 24), ("bytes", 1 << 32, 2, 1 << 24)],
          dict(widened=_scratch(_N128 * 128 * 4), outputs=_N128 * (4 + 4 + 16) + _scratch(_N128 * 8), compare=1 * GIB)),
    # an integer-valued f32 column attached to an IVF_PQ index as its refine source: the lossless u8 copy beside it
    _case("refine-raw", "f32", 128, _N128,
          [("bytes", 1 << 32, 4, 1 << 23), ("elements", 1 << 31, 1, 1 << 24), ("copy", 1 << 31, 1, 1 << 24)],
          dict(u8_copy=_N128 * 128, scratch=1 * GIB)),
    _case("i8-128", "i8", 128, _N8, [("elements", 1 << 31, 1, 1 << 24), ("elements", 1 << 32, 1, 1 << 25)],
          dict(scratch=1 * GIB)),
    # a column of SQ codes (tiled from the codes of the f32 base and planted rows): sq_distance, then an IVF_SQ index over all of it
    _case("sq-codes", "u8", 128, _N8, [("bytes", 1 << 31, 1, 1 << 24), ("bytes", 1 << 32, 1, 1 << 25)],
          dict(index=_N8 * (128 + 4 + 8) + _scratch(_N8 * 4), part_ids=_N8 * 4, distances=_N8 * 4 * 2, compare=1 * GIB)),
]}

FREE_MARGIN = 4 * GIB            # a case skips unless its need + this much is free


# ---- rows ---------------------------------------------------------------------------------------------------------------------------
def _cast(a, kind):
    if kind == "i8":
        return np.clip(np.rint(a), -128, 127).astype(np.int8)
    return np.ascontiguousarray(a.astype(NPDT[kind]))


@functools.lru_cache(maxsize=None)
def base_rows(kind, d, seed=1):
    """the P filler rows, spoilers included"""
    rng = np.random.default_rng(seed * 1000 + d)
    if kind == "i8":
        x = rng.integers(-40, 41, (P, d)).astype(np.float64)
    else:
        s = 0.7 if kind == "f16" else 3.0
        c = rng.standard_normal((40, d)) * s
        x = c[rng.integers(0, 40, P)] + rng.standard_normal((P, d)) * s
    x = _cast(x, kind)
    if kind != "i8":
        x[NAN_ROW] = np.nan
    x[ZERO_ROW] = 0
    if d in COSINE_DIMS:
        x[ZERO_ROW, 0] = -1          # see COSINE_DIMS
    x[DUP_ROWS[1]] = x[DUP_ROWS[0]]
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def planted_rows(kind, d, nwin, seed=2):
    """the distinct planted rows of nwin windows (window 0, the boundary windows, the last window), in column order.  Every window
    has a centre of its own near +SHIFT, so that the neighbours of a row are mostly rows of its own window"""
    rng = np.random.default_rng(seed * 1000 + d + nwin)
    sizes = window_sizes(nwin)
    s = {"f32": 3.0, "f16": 0.7, "i8": 12.0}[kind]
    rows = []
    for w in sizes:
        centre = SHIFT[kind] + rng.standard_normal(d) * s * 0.5
        rows.append(centre + rng.standard_normal((w, d)) * s)
    x = _cast(np.vstack(rows), kind)
    assert len(np.unique(x, axis=0)) == len(x), "planted rows must be distinct"
    x.setflags(write=False)
    return x


def window_sizes(nwin):
    return [WIN] * (nwin - 1) + [LAST]


def window_starts(n, boundary_rows, sizes=None):
    """window 0 at row 0, a window straddling every boundary row (half below, half at and above), the last window ending at row n - 1"""
    sizes = window_sizes(len(boundary_rows) + 2) if sizes is None else sizes
    starts = [0] + [b - w // 2 for b, w in zip(boundary_rows, sizes[1:-1])] + [n - sizes[-1]]
    ends = [s + w for s, w in zip(starts, sizes)]
    assert all(e <= s2 for e, s2 in zip(ends, starts[1:])), "windows overlap: n is too small for these boundaries"
    return starts


class Column:
    """the column of a case (or its scaled-down twin): never materialised as a whole unless `rows(0, n)` is asked for"""

    def __init__(self, kind, d, n, boundary_rows, base=None, planted=None, sizes=None):
        self.kind, self.d, self.n, self.boundary_rows = kind, d, int(n), list(boundary_rows)
        self.sizes = window_sizes(len(self.boundary_rows) + 2) if sizes is None else list(sizes)
        self.starts = window_starts(self.n, self.boundary_rows, self.sizes)
        self.base = base_rows(kind, d) if base is None else base
        self.planted = planted_rows(kind, d, len(self.starts)) if planted is None else planted
        assert self.base.shape == (P, d) and self.planted.shape == (sum(self.sizes), d)
        self.pstart = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)      # planted index of every window's first row
        self.pos = np.concatenate([np.arange(s, s + w, dtype=np.uint64) for s, w in zip(self.starts, self.sizes)])
        assert (np.diff(self.pos.astype(np.int64)) > 0).all()

    @classmethod
    def of_case(cls, case):
        """(a "u8" case is a column of SQ codes: `sq_codes_of` of this f32 column)"""
        return cls(case.kind if case.kind != "u8" else "f32", case.d, case.n, case.boundary_rows)

    def like(self, base, planted, kind):
        """a column of the same shape whose rows are a per-row function of this one's (codes, for instance)"""
        return Column(kind, base.shape[1], self.n, self.boundary_rows, base, planted)

    def windows(self):
        """[(first column row, planted rows of the window)]"""
        return [(s, self.planted[self.pstart[i]:self.pstart[i + 1]]) for i, s in enumerate(self.starts)]

    def rows(self, r0, r1):
        """rows [r0, r1) of the column on the host"""
        out = np.array(self.base[np.arange(r0, r1) % P])
        for s, rows in self.windows():
            a, b = max(r0, s), min(r1, s + len(rows))
            if a < b:
                out[a - r0:b - r0] = rows[a - s:b - s]
        return out

    def device(self, torch, device="cuda"):
        """the column on the device: base.repeat(...)[:n] (a view: no second copy), the windows written over it"""
        t = torch.from_numpy(np.array(self.base)).to(device)
        col = t.repeat(-(-self.n // P), 1)[:self.n]
        for s, rows in self.windows():
            col[s:s + len(rows)] = torch.from_numpy(np.array(rows)).to(device)
        assert col.is_contiguous()
        return col

    def last_window(self):
        return self.starts[-1]


def scaled_down(case, periods=3):
    """the same construction at n = periods * P + 77 rows, the boundaries spread over the column: the oracle can process all of it"""
    col = Column.of_case(case)
    n = periods * P + 77
    nb = len(case.boundary_rows)
    small = Column(col.kind, col.d, n, [WIN + (i + 1) * (n - LAST - WIN) // (nb + 1) // 2 * 2 + 1 for i in range(nb)])
    assert small.planted is col.planted and small.base is col.base
    return small


# ---- per-row operations -------------------------------------------------------------------------------------------------------------
def expected_rows(col, fn):
    """fn: rows [r][d] -> array or tuple of arrays with r leading.  -> (per base row, [(first column row, per planted row)]) per output"""
    def tup(v):
        return v if isinstance(v, tuple) else (v,)
    eb = tup(fn(np.array(col.base)))
    ep = tup(fn(np.array(col.planted)))
    outs = []
    for b, p in zip(eb, ep):
        outs.append((b, [(s, p[col.pstart[i]:col.pstart[i + 1]]) for i, s in enumerate(col.starts)]))
    return outs


def assemble(n, exp_base, overrides):
    """the whole expected output on the host (scaled-down columns only)"""
    out = np.array(exp_base[np.arange(n) % P])
    for s, rows in overrides:
        out[s:s + len(rows)] = rows
    return out


def same_bits(a, b):
    """equal bit for bit, or both NaN (a NaN's sign and payload belong to the machine that made it)"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return (a.view(f"u{a.dtype.itemsize}") == b.view(f"u{b.dtype.itemsize}")) | (np.isnan(a) & np.isnan(b))
    return a == b


# ---- models -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def models(kind, d, nwin, nlist, m, metric):
    """centroids by the oracle's k-means over filler and planted rows (cosine: over the normalised rows), a codebook by its PQ training
    on their residuals (dot: on the rows), in the column's element type (f32 for int8)"""
    rng = np.random.default_rng(d + nlist + m)
    x = np.vstack([base_rows(kind, d), planted_rows(kind, d, nwin)])
    x = x[np.isfinite(x.astype(f32)).all(axis=1)]
    x = x[rng.permutation(len(x))]
    if metric == "cosine":
        x = O.normalize(x)
        x = x[np.isfinite(x.astype(f32)).all(axis=1)]
    sm = "l2" if metric == "cosine" else metric
    xf = x.astype(f32)
    cent = O.kmeans_train(xf[: nlist * 64], nlist, max_iters=6, seed=3, metric=sm)[0]
    cb = None
    if m:
        part, _ = O.assign(xf, cent, sm)
        res = O.residual(xf, cent, np.where(part == O.NONE, 0, part)) if sm == "l2" else xf
        cb = O.pq_train(res[: 256 * 12], m, max_iters=4, seed=4)[0]
    t = np.float16 if kind == "f16" else f32
    return np.ascontiguousarray(cent.astype(t)), None if cb is None else np.ascontiguousarray(cb.astype(t))


def transform_chain(x, cent, cb, metric):
    """the oracle's IvfTransformer chain per row -> (part ids u32 (NONE: dropped), codes u8 [r][m], zero where there is no partition)"""
    f16 = x.dtype == np.float16
    xs = O.normalize(x) if metric == "cosine" else x
    keep = O.is_finite(xs)
    sm = "l2" if metric == "cosine" else metric
    part = np.full(x.shape[0], O.NONE, np.uint32)
    xk = np.ascontiguousarray(xs[keep])
    pk, _ = O.assign(xk, cent.astype(np.float16) if f16 else cent, sm)
    part[keep] = pk
    res = O.residual(xk, cent, np.where(pk == O.NONE, 0, pk)) if sm == "l2" else xk
    codes = np.zeros((x.shape[0], cb.shape[0]), np.uint8)
    codes[keep] = O.pq_encode(res, cb, "l2")
    codes[part == O.NONE] = 0
    return part, codes


# ---- planted windows: top-k ---------------------------------------------------------------------------------------------------------
def queries(col, nq, seed=7):
    """queries next to planted rows of the last window, in the column's element type"""
    rng = np.random.default_rng(seed + nq)
    lo = int(col.pstart[-2])
    pick = lo + rng.permutation(col.sizes[-1])[:nq] if nq <= col.sizes[-1] else lo + rng.integers(0, col.sizes[-1], nq)
    s = {"f32": 0.5, "f16": 0.1, "i8": 2.0}[col.kind]
    return _cast(col.planted[pick].astype(np.float64) + rng.standard_normal((nq, col.d)) * s, col.kind)


def _oracle_rows(x):
    return x if x.dtype == np.float16 else x.astype(f32)


def keys(dist):
    """f32 -> uint32 in f32::total_cmp order"""
    b = np.ascontiguousarray(dist, f32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000))


def planted_answer(col, q, k, metric, check=True):
    """the oracle's top k over the planted rows alone, ids = column positions.  check: the conditions under which this IS the answer
    over the whole column, and under which the answer cannot come from low rows alone"""
    oi, od = O.flat_knn(_oracle_rows(np.array(col.planted)), _oracle_rows(q), k, metric, row_ids=col.pos)
    if check:
        assert not np.isnan(od).any(), "a returned distance is NaN"
        base = _oracle_rows(np.array(col.base))
        last = np.uint64(col.last_window())
        for i in range(q.shape[0]):
            filler = O.distance_batch(metric, _oracle_rows(q[i:i + 1])[0], base)
            assert keys(filler).min() > keys(od[i, k - 1:k])[0], f"query {i}: a filler row is not strictly farther than the k-th planted row"
            for b in col.boundary_rows:
                assert (oi[i] >= np.uint64(b)).any(), f"query {i}: no answer at or beyond row {b}"
            assert (oi[i] >= last).sum() * 4 >= k, f"query {i}: fewer than a quarter of the answers lie in the last window"
    return oi, od


# ---- index lists --------------------------------------------------------------------------------------------------------------------
# An IVF index over the whole column with part ids given by position: the last window is list nlist - 1 (stored last, so both its storage
# and the rows its gather read lie beyond every boundary), every other row r goes to list r mod (nlist - 1).  The queries probe ONE
# list, the last: the expected answer is the sub-index search (heap of k in storage order, then (distance, row id)) over LAST rows.
def list_ids(col, nlist):
    """part id of every row, on the host (scaled-down columns only; the GPU test writes the same formula with torch)"""
    part = (np.arange(col.n) % (nlist - 1)).astype(np.uint32)
    part[col.last_window():] = nlist - 1
    return part


def list_centroids(col, nlist, rows=None):
    """f32: the mean of the last window's rows for the last list, filler rows for the others"""
    last = (col.planted if rows is None else rows)[col.pstart[-2]:].astype(np.float64)
    base = np.asarray(col.base if rows is None else base_rows("f32", col.d)).astype(f32)
    ok = np.isfinite(base).all(axis=1)
    return np.ascontiguousarray(np.vstack([base[ok][:nlist - 1], last.mean(axis=0)[None]]).astype(f32))


def probes_last_list(q, cent, metric):
    ids, _ = O.find_partitions(_oracle_rows(q), cent, 1, "l2" if metric == "cosine" else metric)
    return (ids[:, 0] == cent.shape[0] - 1).all()


def last_list_rows(col):
    """(the rows of the last list in storage order, their row ids)"""
    return np.array(col.planted[col.pstart[-2]:]), col.pos[col.pstart[-2]:]


def flat_list_answer(rows, rid, q, k, metric, allow=None):
    """FlatIndex::search of one list of raw vectors (l2 / dot): a heap of k over the rows in storage order, then SortExec"""
    if allow is not None:
        rows, rid = rows[allow], rid[allow]
    out_i = np.full((q.shape[0], k), np.iinfo(np.uint64).max, np.uint64)
    out_d = np.full((q.shape[0], k), np.inf, f32)
    for i in range(q.shape[0]):
        hi, hd = O.heap_topk(O.distance_batch(metric, _oracle_rows(q[i:i + 1])[0], _oracle_rows(rows)), rid, k)
        si, sd = O.sort_fetch(hi, hd, k)
        out_i[i, :len(si)] = si; out_d[i, :len(sd)] = sd
    return out_i, out_d


# ---- SQ codes -----------------------------------------------------------------------------------------------------------------------
def sq_bounds(col):
    return sq_spec.bounds(np.vstack([col.base, col.planted]))


def sq_codes_of(col):
    """-> (the column of the codes of col's rows, bounds)"""
    b = sq_bounds(col)
    base, planted = sq_spec.encode(col.base, *b), sq_spec.encode(col.planted, *b)
    base.setflags(write=False); planted.setflags(write=False)
    return col.like(base, planted, "u8"), b


def sq_list_answer(codes, rid, cent, q, k, metric, bounds, allow=None):
    """the IVF_SQ search of sq_spec over ONE list holding `codes` (the last list of list_centroids)"""
    nlist = cent.shape[0]
    part = np.full(len(codes), nlist - 1, np.uint32)
    pre = None
    if allow is not None:
        pre = np.zeros(int(rid.max()) + 1, bool)
        pre[rid[allow].astype(np.int64)] = True
    return sq_spec.search(O, codes, part, cent, q, k, 1, metric, bounds[0], bounds[1], row_ids=rid, prefilter=pre)


# ---- the per-row operations of the table: name -> (rows -> outputs), the oracle's side ------------------------------------------------
NLIST = 64
SQ_TEST_BOUNDS = (-9.5, 31.0)          # inside the data's range on both sides: codes saturate at 0 and at 255


def per_row_ops(col):
    """{name: (fn, models)}: fn maps rows [r][d] of col's element type to a tuple of per-row outputs; models: what the GPU call needs"""
    kind, d, nwin = col.kind, col.d, len(col.starts)
    ops = {}
    if kind in ("f32", "f16"):
        for metric in ("l2", "dot"):
            cent, _ = models(kind, d, nwin, NLIST, 0, metric)
            ops[f"assign-{metric}"] = (functools.partial(_assign, cent=cent, metric=metric), dict(cent=cent, metric=metric))
        for m in ((16, 32) if d == 128 else (d // 4,)):
            for metric in ("l2", "dot", "cosine"):
                if kind == "f16" and metric == "dot":
                    continue                     # f16 under dot with d > 16 keeps the 32-lane kernels: not the route of this table
                cent, cb = models(kind, d, nwin, NLIST, m, metric)
                ops[f"ivfpq_encode-m{m}-{metric}"] = (functools.partial(transform_chain, cent=cent, cb=cb, metric=metric),
                                                      dict(cent=cent, cb=cb, metric=metric))
    if kind == "f32":
        ops["normalize"] = (lambda x: (O.normalize(x),), {})
        cent, cb = models(kind, d, nwin, NLIST, 16, "l2")
        ops["residual+pq_encode"] = (functools.partial(_residual_encode, cent=cent, cb=cb), dict(cent=cent, cb=cb))
        ops["sq_encode"] = (lambda x: (sq_spec.encode(x, *SQ_TEST_BOUNDS),), dict(bounds=SQ_TEST_BOUNDS))
        rot = rq_spec.rotation(d, 5)
        for metric in ("l2", "dot"):
            cent, _ = models(kind, d, nwin, NLIST, 0, metric)
            ops[f"rq_encode-{metric}"] = (functools.partial(_rq_encode, cent=cent, rot=rot, metric=metric), dict(cent=cent, rot=rot, metric=metric))
    return ops


def _assign(x, cent, metric):
    ids, dists = O.assign(x, cent, metric)
    return ids, dists


def _residual_encode(x, cent, cb):
    """Engine.assign -> Engine.residual -> Engine.pq_encode, as a caller chains them (no finite filter: a NaN row has no partition and
    a zero residual)"""
    part, _ = O.assign(x, cent, "l2")
    res = O.residual(x, cent, np.where(part == O.NONE, 0, part))
    res[part == O.NONE] = 0
    return part, res, O.pq_encode(res, cb, "l2")


def _rq_encode(x, cent, rot, metric):
    part, dvc = rq_spec.prepare_rows(O, x, cent, metric)
    return (part, dvc) + tuple(rq_spec.encode(x, part, dvc, cent, rot, metric))


# ---- RQ codes: two lists by position (every row but the last window in list 0, the last window in list 1) -----------------------------
def rq_model(col):
    """(centroids f32 [2][d]: the mean of the finite filler rows and the mean of the last window, rotation)"""
    base = np.asarray(col.base, f32)
    base = base[np.isfinite(base).all(axis=1)]
    last = np.asarray(col.planted[col.pstart[-2]:], np.float64)
    cent = np.vstack([base.astype(np.float64).mean(axis=0)[None], last.mean(axis=0)[None]]).astype(f32)
    return np.ascontiguousarray(cent), rq_spec.rotation(col.d, 5)


def rq_encode_rows(rows, lists, cent, rot, metric):
    """rows with their list by position -> (part ids u32 with NONE for non-finite rows, dist_v_c, codes, add, scale)"""
    rows = np.asarray(rows, f32)
    part = np.asarray(lists, np.uint32).copy()
    dvc = np.zeros(len(rows), f32)
    for p_ in range(cent.shape[0]):
        m = part == p_
        if m.any():
            dvc[m] = O.assign(np.ascontiguousarray(rows[m]), np.ascontiguousarray(cent[p_:p_ + 1]), metric)[1]
    part[~np.isfinite(rows).all(axis=1)] = O.NONE
    return (part, dvc) + tuple(rq_spec.encode(rows, part, dvc, cent, rot, metric))


def rq_expected(col, metric):
    """per output (part, dist_v_c, codes, add, scale): (per base row, [(first column row, per planted row)]) -- and the model"""
    cent, rot = rq_model(col)
    eb = rq_encode_rows(col.base, np.zeros(P, np.uint32), cent, rot, metric)
    lists = np.zeros(len(col.planted), np.uint32)
    lists[col.pstart[-2]:] = 1
    ep = rq_encode_rows(col.planted, lists, cent, rot, metric)
    outs = [(b, [(s_, p_[col.pstart[i]:col.pstart[i + 1]]) for i, s_ in enumerate(col.starts)]) for b, p_ in zip(eb, ep)]
    return outs, cent, rot


def rq_lists(col):
    """list of every row by position, on the host (scaled-down columns only)"""
    lists = np.zeros(col.n, np.uint32)
    lists[col.last_window():] = 1
    return lists


def rq_queries(col, cent, nq):
    """(residual queries q - c_1, their dist_q_c under l2) for rq_distance: queries next to the last window against its centroid"""
    q = queries(col, nq).astype(f32)
    qr = (q - cent[1]).astype(f32)
    return q, qr


def rq_distance_expected(col, outs, qr, dqc, rot, metric):
    """rq_distance(quantised) of every row: the packed path, and the f32 path for the last n % 32 rows of the column"""
    (_, _), (_, _), (cb, cov), (ab, aov), (sb, sov) = outs
    qs = [rq_spec.Query(qr[i], dqc[i], rot, metric) for i in range(len(qr))]

    def packed(codes, add, scale):
        return np.ascontiguousarray(np.stack([c.finish(c.raw_packed(codes), add, scale) for c in qs], axis=1))

    eb = packed(cb, ab, sb)
    ov = [(s_, packed(c_, a_, s2)) for (s_, c_), (_, a_), (_, s2) in zip(cov, aov, sov)]
    tail = col.n % rq_spec.BATCH
    if tail:
        s_, c_ = cov[-1]
        a_, s2 = aov[-1][1], sov[-1][1]
        assert s_ + len(c_) == col.n and tail <= len(c_)
        f = np.ascontiguousarray(np.stack([c.finish(c.raw_f32(c_[-tail:], 0.0), a_[-tail:], s2[-tail:]) for c in qs], axis=1))
        ov.append((col.n - tail, f))
    return eb, ov


def rq_list_answer(col, outs, cent, rot, q, k, metric, allow=None):
    """the IVF_RQ search of rq_spec over list 1 alone (the last window's codes, in storage order)"""
    (_, pov), (_, _), (_, cov), (_, aov), (_, sov) = outs
    codes, add, scale, part = cov[-1][1], aov[-1][1], sov[-1][1], pov[-1][1]
    rid = col.pos[col.pstart[-2]:]
    pre = None
    if allow is not None:
        pre = np.zeros(int(rid.max()) + 1, bool)
        pre[rid[allow].astype(np.int64)] = True
    return rq_spec.search(O, codes, add, scale, part, cent, rot, q, k, 1, metric, row_ids=rid, prefilter=pre)


# ---- multivector rows over the column's vectors -------------------------------------------------------------------------------------------
def multivec_offsets(col, seed=9):
    """rows of 1 .. 8 vectors in a pattern that holds exactly P vectors, repeated: the row pattern has the filler's period.
    -> (offsets int64 [rows + 1] ending at col.n, rows per period)"""
    rng = np.random.default_rng(seed)
    lens = []
    while sum(lens) < P:
        lens.append(int(rng.integers(1, 9)))
    lens[-1] -= sum(lens) - P
    pat = np.cumsum([0] + lens).astype(np.int64)                     # [R + 1], pat[-1] == P
    R = len(lens)
    full, tail = divmod(col.n, P)
    off = (np.arange(full, dtype=np.int64)[:, None] * P + pat[None, :-1]).ravel()
    last = full * P + pat[pat < tail]
    off = np.concatenate([off, last, [col.n]]) if tail else np.concatenate([off, [col.n]])
    assert off[0] == 0 and (np.diff(off) > 0).all() and (np.diff(off) <= 8).all()
    return off, R


def multivec_query(col, nqv=4):
    return queries(col, nqv + 60)[60:]


def multivec_expected(col, off, R, q, metric):
    """multivec_distance of every row: (per pattern row [R], [(first row, distances)] for the rows that touch a window).  The rows of the
    last, partial period lie inside the last window"""
    assert col.n % P < LAST
    eb = multivec_spec.distances(O, np.asarray(col.base), off[:R + 1], q, metric)
    ov = []
    for s_, rows in col.windows():
        r0 = int(np.searchsorted(off, s_, "right")) - 1
        r1 = int(np.searchsorted(off, s_ + len(rows) - 1, "right")) - 1
        a, b = int(off[r0]), int(off[r1 + 1])
        ov.append((r0, multivec_spec.distances(O, col.rows(a, b), off[r0:r1 + 2] - a, q, metric)))
    return eb, ov


def multivec_planted_answer(eb, ov, k):
    """top k over the rows that touch a window, ids = row numbers; asserts that every pattern row is strictly farther and that the
    answer reaches the last window"""
    rid = np.concatenate([np.arange(r0, r0 + len(d_), dtype=np.uint64) for r0, d_ in ov])
    dist = np.concatenate([d_ for _, d_ in ov]).astype(f32)
    ids, d_ = multivec_spec.topk(dist, k, rid)
    assert not np.isnan(d_).any()
    assert keys(eb).min() > keys(d_[k - 1:k])[0], "a filler row is not strictly farther than the k-th planted row"
    assert (ids >= np.uint64(ov[-1][0])).sum() * 4 >= k, "fewer than a quarter of the answers lie in the last window"
    return ids, d_


# ---- refine from the raw column: an IVF_PQ index over the planted rows of the HIGH windows ----------------------------------------------
REFINE_SIZES = [256, 1500, 1500, 3000]          # 6,000 rows in the windows past the boundaries
REFINE_NLIST, REFINE_M = 12, 16


@functools.lru_cache(maxsize=None)
def _refine_rows(d):
    rng = np.random.default_rng(77)
    c = rng.uniform(20, 200, (24, d))
    base = np.clip(np.rint(c[rng.integers(0, 24, P)] + rng.normal(0, 24, (P, d))), 0, 255).astype(f32)
    base[ZERO_ROW] = 0
    base[ZERO_ROW + 1] = 255                    # both ends of the byte range
    base[DUP_ROWS[1]] = base[DUP_ROWS[0]]
    cp = rng.uniform(20, 200, (REFINE_NLIST, d))
    npl = sum(REFINE_SIZES)
    planted = np.clip(np.rint(cp[rng.integers(0, REFINE_NLIST, npl)] + rng.normal(0, 24, (npl, d))), 0, 255).astype(f32)
    assert len(np.unique(planted, axis=0)) == npl
    base.setflags(write=False); planted.setflags(write=False)
    return base, planted


def refine_column(case, n=None, boundary_rows=None):
    base, planted = _refine_rows(case.d)
    return Column("f32", case.d, case.n if n is None else n, case.boundary_rows if boundary_rows is None else boundary_rows, base, planted, REFINE_SIZES)


def refine_index_rows(col):
    """(the indexed rows: the planted rows of every window but window 0, their row ids = column positions)"""
    lo = int(col.pstart[1])
    return np.ascontiguousarray(col.planted[lo:]), np.ascontiguousarray(col.pos[lo:])


@functools.lru_cache(maxsize=None)
def refine_models(d, metric):
    x = np.ascontiguousarray(_refine_rows(d)[1][REFINE_SIZES[0]:])
    cent = O.kmeans_train(x[: REFINE_NLIST * 40], REFINE_NLIST, max_iters=4, seed=5, metric=metric)[0]
    part, _ = O.assign(x, cent, metric)
    res = O.residual(x, cent, np.where(part == O.NONE, 0, part)) if metric == "l2" else x
    return cent, O.pq_train(res[: 256 * 12], REFINE_M, max_iters=3, seed=6)[0]


def refine_queries(col, nq, seed=3):
    """next to rows of the last window (fractions added, so that no distance is zero), CHOSEN among four times as many: those whose
    exact neighbours among the indexed rows lie at least half in the last window under both metrics (the planted rows of all windows
    come from the same clusters; refine_answer asserts the floor of a quarter on the answer itself)"""
    rng = np.random.default_rng(seed)
    lo = int(col.pstart[-2])
    cand = (col.planted[lo + rng.permutation(col.sizes[-1])[:4 * nq]] + rng.uniform(0, 1, (4 * nq, col.d))).astype(f32)
    x, _ = refine_index_rows(col)
    first_last = lo - int(col.pstart[1])
    ok = np.ones(len(cand), bool)
    for metric in ("l2", "dot"):
        ids, _ = O.flat_knn(x, cand, 13, metric)
        ok &= (ids >= first_last).sum(axis=1) * 2 >= 13
    assert ok.sum() >= nq, "too few candidate queries have their neighbours in the last window"
    return np.ascontiguousarray(cand[ok][:nq])


def refine_answer(col, q, k, refine, metric, nprobes=REFINE_NLIST):
    """the oracle's refined IVF_PQ search over the indexed rows, ids mapped to column positions (ascending: ties keep their order);
    asserts that every query has an answer beyond every boundary and a quarter of it in the last window"""
    x, pos = refine_index_rows(col)
    cent, cb = refine_models(col.d, metric)
    oi, od = O.build_index(x, cent, cb, metric).search(q, k, nprobes, refine=refine, raw=x)
    assert (oi < len(pos)).all() and not np.isnan(od).any()
    ids = pos[oi.astype(np.int64)]
    for b in col.boundary_rows:
        assert (ids >= np.uint64(b)).any(axis=1).all()
    assert ((ids >= np.uint64(col.last_window())).sum(axis=1) * 4 >= k).all()
    return ids, od


def sq_refine_index(col, metric):
    """the IVF_SQ index over the same 6,000 rows: (codes u8, part ids, centroids, bounds)"""
    x, _ = refine_index_rows(col)
    cent, _ = refine_models(col.d, metric)
    bounds = sq_spec.bounds(x)
    _, part = sq_spec.prepare_rows(O, x, cent, metric)
    return sq_spec.encode(x, *bounds), part, cent, bounds


def sq_refine_answer(col, q, k, refine, metric, nprobes=REFINE_NLIST):
    """refine_spec's IVF_SQ search with a refine_factor over the indexed rows (local ids, the rows themselves as the raw column), ids
    mapped to column positions; the same conditions as refine_answer"""
    x, pos = refine_index_rows(col)
    codes, part, cent, bounds = sq_refine_index(col, metric)
    oi, od = refine_spec.sq_search_refine(O, codes, part, cent, q, k, refine, nprobes, metric, bounds[0], bounds[1], x)
    assert (oi < len(pos)).all() and not np.isnan(od).any()
    ids = pos[oi.astype(np.int64)]
    for b in col.boundary_rows:
        assert (ids >= np.uint64(b)).any(axis=1).all()
    assert ((ids >= np.uint64(col.last_window())).sum(axis=1) * 4 >= k).all()
    return ids, od
