"""Fixtures for the operand-magnitude sweep (tests/test_magnitude_spec.py on the CPU, tests/test_zz_gpu_magnitude.py on the GPU).

About half of the hot path answers in two steps: a low-precision matrix-core surrogate filters or ranks, and only what lies inside an
error margin is recomputed in the reference's arithmetic.  Every margin is RELATIVE to the operands' norms (E = 2^-13 (|x|^2 + max|c|^2)
and its siblings), and a relative bound stops holding where products or sums sit in the f32 denormal range, where a norm overflows, and
where the norms dwarf the distances being compared.  The kernels guard the lower end with `E2 > 2^-100` (mfma_assign.hip, xform_fused.hip,
pq_mfma.hip, flat_mfma.hip, flat_mfma_wide.hip) or with their own conditions (search_ms.hip: ms_prep_kernel's `ok`).  This module builds
data on both sides of every such guard:

  scaled(fx, e)          every float operand times 2^e (a power of two: exact while nothing leaves the normal range); models are trained
                         once at e = 0 and scaled with the data
  offset(fx, r)          2^r added to rows, queries and centroids; the models are recomputed by the oracle on the shifted rows
  exponents_for(...)     the exponents of a route: DERIVED from the route's E2 as its kernel defines it (two integer exponents on each side
                         of the lower guard, two on each side of the point where |x|^2 stops being finite) plus the fixed points
  classify(...)          invariant / partial / subnormal / overflow, computed from the data (see the function)
  flat_filter_model(...) numpy model of flat_mfma.hip's filter, with and without the lower guard

numpy keeps f32 subnormals (no flush-to-zero), as gfx950 does for f32 arithmetic."""
import functools

import numpy as np

import oracle as O

f32 = np.float32
GUARD_LOG2 = -100                                   # every `E2 > 7.888609052210118e-31f` in lance_amd/csrc
FIXED = (-75, -72, -70, -62, -30, 0, 30)
DOT_EXPONENTS = (-30, -12, 0, 10, 20, 40, 56)       # above 2^58 the reference generates inf - inf, whose sign belongs to the host CPU
OFFSETS = (4, 7, 10)
F16_SCALES = (-8, -11, -13, 3)
FLOAT_KEYS = ("x", "q", "cent", "cb")


def pow2(e):
    v = f32(2.0 ** e)
    assert v > 0 and np.isfinite(v)
    return v


class Fx(dict):
    """a fixture: x / q / cent / cb arrays (those the route needs) plus plain settings"""
    __getattr__ = dict.__getitem__

    def but(self, **kw):
        out = Fx(self)
        out.update(kw)
        return out


def scaled(fx, e):
    """every float operand multiplied by np.float32(2.0 ** e), in its own dtype"""
    s = pow2(e)
    out = Fx(fx)
    for key in FLOAT_KEYS:
        if key in fx:
            a = fx[key]
            out[key] = (a * a.dtype.type(s)).astype(a.dtype)
    out["e"] = e
    return out


# ---- models (oracle only) ----------------------------------------------------------------------------------------------------------
def ivf_models(x, nlist, m, seed, km_iters=6, pq_iters=4, metric="l2"):
    """centroids by the oracle's k-means, codebook by its PQ training on the residuals (dot: on the rows)"""
    cent = O.kmeans_train(x[: nlist * 64], nlist, max_iters=km_iters, seed=seed, metric=metric)[0]
    cb = None
    if m:
        part, _ = O.assign(x, cent, metric)
        res = O.residual(x, cent, np.where(part == O.NONE, 0, part)) if metric == "l2" else x
        cb = O.pq_train(res[: 256 * 12], m, max_iters=pq_iters, seed=seed + 1)[0]
    return cent, cb


def remodel(fx):
    """the models of a fixture recomputed on its present rows (offset family)"""
    out = Fx(fx)
    if fx.kind in ("assign", "xform", "ivfpq", "ivfflat", "sqrq"):
        cent, cb = ivf_models(fx.x.astype(f32), fx.cent.shape[0], fx.get("m", 0), fx.seed, metric="l2")
        out["cent"] = cent.astype(fx.cent.dtype)
        if cb is not None:
            out["cb"] = cb.astype(fx.cb.dtype)
    return out


def offset(fx, r):
    """2^r added to rows, queries and centroids; models recomputed by the oracle on the shifted rows (a `coarse` fixture has no rows:
    its centroids are shifted)"""
    s = pow2(r)
    out = Fx(fx)
    for key in ("x", "q", "cent"):
        if key in fx:
            out[key] = (fx[key] + fx[key].dtype.type(s)).astype(fx[key].dtype)
    out["r"] = r
    return remodel(out) if "x" in fx else out


# ---- base fixtures (e = 0) -----------------------------------------------------------------------------------------------------------
def _gauss(rng, n, d, scale=3.0):
    return (rng.standard_normal((n, d)) * scale).astype(f32)


def _clustered(rng, n, d, ncl, spread=1.0, centre_scale=3.0):
    c = rng.standard_normal((ncl, d)) * centre_scale
    return (c[rng.integers(0, ncl, n)] + rng.standard_normal((n, d)) * spread).astype(f32)


@functools.lru_cache(maxsize=None)
def flat_fixture(d, n=6000, nq=130, seed=5):
    rng = np.random.default_rng(seed + d)
    return Fx(kind="flat", x=_gauss(rng, n, d), q=_gauss(rng, nq, d), seed=seed)


@functools.lru_cache(maxsize=None)
def assign_fixture(d, n=6000, k=48, seed=11):
    rng = np.random.default_rng(seed + d)
    x = _clustered(rng, n, d, 60)
    cent, _ = ivf_models(x, k, 0, seed)
    return Fx(kind="assign", x=x, cent=cent, seed=seed)


@functools.lru_cache(maxsize=None)
def coarse_fixture(d, nlist, nq=130, seed=21):
    rng = np.random.default_rng(seed + d + nlist)
    cent = _gauss(rng, nlist, d)
    q = (cent[rng.integers(0, nlist, nq)] + rng.standard_normal((nq, d))).astype(f32)
    return Fx(kind="coarse", cent=cent, q=q, seed=seed)


@functools.lru_cache(maxsize=None)
def xform_fixture(d, m, n=2200, nlist=32, seed=31, metric="l2"):
    """metric: the metric the models are trained under (dot: the codebook on the rows themselves, no residual)"""
    rng = np.random.default_rng(seed + d + m)
    x = _clustered(rng, n, d, 40)
    cent, cb = ivf_models(x, nlist, m, seed, metric=metric)
    return Fx(kind="xform", x=x, cent=cent, cb=cb, m=m, seed=seed, metric=metric)


@functools.lru_cache(maxsize=None)
def ivfpq_fixture(dtype="f32", n=20000, d=64, m=16, nlist=24, nq=700, seed=41, metric="l2"):
    rng = np.random.default_rng(seed)
    c = rng.standard_normal((48, d)) * (2.0 if dtype == "f16" else 3.0)
    spread = 0.7 if dtype == "f16" else 1.0
    t = np.float16 if dtype == "f16" else f32
    x = (c[rng.integers(0, 48, n)] + rng.standard_normal((n, d)) * spread).astype(t)
    q = (c[rng.integers(0, 48, nq)] + rng.standard_normal((nq, d)) * spread).astype(t)
    cent, cb = ivf_models(x.astype(f32), nlist, m, seed, metric=metric)
    return Fx(kind="ivfpq", x=x, q=q, cent=cent.astype(t), cb=cb.astype(t), m=m, seed=seed, metric=metric)


@functools.lru_cache(maxsize=None)
def ivfflat_fixture(n=8000, d=40, nlist=12, nq=32, seed=51):
    rng = np.random.default_rng(seed)
    x = _gauss(rng, n, d)
    cent, _ = ivf_models(x, nlist, 0, seed)
    return Fx(kind="ivfflat", x=x, q=_gauss(rng, nq, d), cent=cent, seed=seed)


@functools.lru_cache(maxsize=None)
def sqrq_fixture(n=3000, d=64, nlist=16, nq=100, seed=61, metric="l2"):
    rng = np.random.default_rng(seed)
    x = _clustered(rng, n + nq, d, 8, spread=0.6, centre_scale=1.0)
    cent, _ = ivf_models(x[:n], nlist, 0, seed, metric=metric)
    return Fx(kind="sqrq", x=np.ascontiguousarray(x[:n]), q=np.ascontiguousarray(x[n:]), cent=cent, seed=seed, metric=metric)


@functools.lru_cache(maxsize=None)
def f16_fixture(s, n=6000, d=64, nq=130, seed=71):
    """binary16 rows standard_normal * 0.7 * 2^s; 2^3: values beyond +-60000 clipped away (none at this spread: the clip states the intent)"""
    rng = np.random.default_rng(seed)
    sc = 0.7 * 2.0 ** s
    x = np.clip(rng.standard_normal((n, d)) * sc, -60000, 60000).astype(np.float16)
    q = np.clip(rng.standard_normal((nq, d)) * sc, -60000, 60000).astype(np.float16)
    return Fx(kind="flat", x=x, q=q, seed=seed, s=s)


def f16_subnormal_share(a):
    u = np.ascontiguousarray(a).view(np.uint16)
    return float((((u & 0x7C00) == 0) & ((u & 0x03FF) != 0)).mean())


# ---- mixed-scale cases ------------------------------------------------------------------------------------------------------------------
FLAT_FIRST_EPOCH = 2048      # the flat scan gives its first epoch of rows to the exact kernel (flat.hip: `seen > 0` gates the filters)


def row_block_start(fx):
    """the first of the 128 scaled rows.  A flat fixture: row 3000, past the first epoch and across two of flat_mfma.hip's 128-row
    workgroups (ordinary rows beside it in both), so that the block meets flat_mfma.hip / flat_mfma_wide.hip and not the exact kernel; the others: row 1000"""
    return 3000 if fx.kind == "flat" else 1000


def mixed_cases(fx):
    """-> {name: fixture}: rows at 2^-52 with queries at 2^0 and the reverse; one row block at 2^58 among unit-scale rows; one centroid at
    2^40 among unit-scale ones (max|c|^2 then inflates every row's margin).  Only the cases whose operands the fixture has.
    A flat fixture gets the block at 2^59 too: at d = 64 the block's |x|^2 is about 2^125.2 at 2^58, BELOW the filters' 2^126 guard
    (the rows are filtered, with everything finite), and 2^127.2 at 2^59 (the rows are `odd`); at d = 128 and 256 the 2^58 block is `odd`
    already and the 2^59 block's |x|^2 is +inf."""
    out = {}
    if "x" in fx and "q" in fx:
        out["rows 2^-52"] = fx.but(x=(fx.x * fx.x.dtype.type(pow2(-52))).astype(fx.x.dtype))
        out["queries 2^-52"] = fx.but(q=(fx.q * fx.q.dtype.type(pow2(-52))).astype(fx.q.dtype))
    if "x" in fx:
        b0 = row_block_start(fx)
        for e in (58, 59) if fx.kind == "flat" else (58,):
            x = fx.x.copy()
            x[b0:b0 + 128] *= pow2(e)
            out[f"row block 2^{e}"] = fx.but(x=x)
    if "cent" in fx:
        c = fx.cent.copy()
        c[5] *= pow2(40)
        out["centroid 2^40"] = fx.but(cent=c)
    return out


# ---- the routes' margins, as the kernel headers define them ---------------------------------------------------------------------------
def n2(a):
    """|row|^2 in float64 (the derivation of an exponent does not depend on the last bit)"""
    a = np.asarray(a, np.float64)
    return (a * a).sum(axis=-1)


def e2_range(route, fx):
    """(smallest, largest) E2 over the fixture's rows at its own scale, float64:
    assign / coarse / xform: 2 * 2^-13 (|x|^2 + max|c|^2)      mfma_assign.hip:249, :1338, xform_fused.hip:772   (x: the row or the query)
    pq:                      2^-12 (|x_m|^2 + max|c|^2)         pq_mfma.hip:167 (per sub-vector)
    flat / flat_wide:        2^-12 (|x|^2 + |q|^2)              flat_mfma.hip, flat_mfma_wide.hip (per pair)"""
    if route in ("assign", "xform", "coarse"):
        rows = n2(fx.q if route == "coarse" else fx.x)
        c = n2(fx.cent).max()
        return 2.0 ** -12 * (rows.min() + c), 2.0 ** -12 * (rows.max() + c)
    if route == "pq":
        m = fx.cb.shape[0]
        sub = n2(np.asarray(fx.x, np.float64).reshape(fx.x.shape[0], m, -1))
        c = n2(fx.cb).max()
        return 2.0 ** -12 * (sub.min() + c), 2.0 ** -12 * (sub.max() + c)
    if route in ("flat", "flat_wide"):
        a, b = n2(fx.x), n2(fx.q)
        return 2.0 ** -12 * (a.min() + b.min()), 2.0 ** -12 * (a.max() + b.max())
    raise KeyError(route)


def largest_norm2(fx):
    return max(float(n2(fx[k]).max()) for k in FLOAT_KEYS if k in fx)


def guard_exponents(route, fx):
    """the integer exponents around the lower guard: E2 scales by 4^e, so with lo / hi the smallest / largest E2 at e = 0
    below = the largest e at which EVERY row has E2 <= 2^-100, above = the smallest e at which every row has E2 > 2^-100;
    -> (below - 1, below, [the exponents between, where the rows are split], above, above + 1)"""
    lo, hi = e2_range(route, fx)
    below = int(np.floor((GUARD_LOG2 - np.log2(hi)) / 2))
    while hi * 4.0 ** (below + 1) <= 2.0 ** GUARD_LOG2:
        below += 1
    while hi * 4.0 ** below > 2.0 ** GUARD_LOG2:
        below -= 1
    above = below + 1
    while not lo * 4.0 ** above > 2.0 ** GUARD_LOG2:
        above += 1
    return tuple(range(below - 1, above + 2))


def overflow_exponents(fx):
    """two exponents on each side of the point where the largest |x|^2 of the fixture stops being finite in f32"""
    big = largest_norm2(fx)
    last = int(np.floor((128 - np.log2(big)) / 2))
    while big * 4.0 ** last >= 2.0 ** 128:
        last -= 1
    while big * 4.0 ** (last + 1) < 2.0 ** 128:
        last += 1
    return tuple(e for e in range(last - 1, last + 3) if e <= 60)      # 2^61 x 3 sigma would leave f32 as an ELEMENT: not this sweep


# search_ms.hip: ms_prep_kernel's `ok` for an L2 pair, in f32 like the kernel; sigma as ms_build makes it.  A HAND COPY of the L2 branch
# of ms_prep_kernel (lance_amd/csrc/search_ms.hip:230-239; MS_SE 30000 and MS_SLACK_CAP 1500 at :63-64), which points back here: it only
# places the sweep (the exponents where `ok` flips), no answer is compared with it -- the fixed points and the top of the range are swept
# whatever it says.  The dot branch (:213-228) has more guards (G * s, zsum, cmax / cmaxp); the dot sweep uses DOT_EXPONENTS as they are.
def ms_sigma(cbmax):
    with np.errstate(over="ignore"):
        return f32(np.ldexp(f32(1.0), 13 - int(np.frexp(f32(cbmax))[1])))


def ms_pair_ok_l2(T, r2, vmax, sigma, d):
    with np.errstate(all="ignore"):
        T, r2, vmax, sigma = f32(T), f32(r2), f32(vmax), f32(sigma)
        s = f32(30000.0) / T
        sqd = f32(np.sqrt(f32(d))) + f32(1.0)
        rn, st = np.sqrt(r2) * f32(1.000001), np.sqrt(T) * f32(1.000001)
        sig2 = sigma * sigma
        e_abs = f32(6.1035156e-5) * sqd * (f32(3.0) * rn + f32(2.0) * st) / sigma + f32(d) * f32(3.7252903e-9) / sig2
        E = f32(1.05) * (f32(1.9921875e-3) * rn * (rn + st) + f32(1.2207031e-4) * (r2 + T)) + e_abs
        eu = E * s * f32(1.1) + f32(3.0)
        lim = (T * f32(1.0000077) + E) - r2
        return bool(T > 0 and T < np.inf and s > 0 and s < np.inf and r2 < np.inf and vmax * sigma < f32(60000.0) and eu <= f32(1500.0)
                    and abs(lim * sig2) < np.inf and r2 * s < f32(1e30))


def mscan_exponents(fx, T0, lo=-90, hi=64):
    """search_ms.hip has no single E2: scan e and take the exponents where the pair predicate flips for a typical pair (T0: the median
    k-th distance at e = 0; |r|^2 and max|r_i| of the median query's residual against its nearest centroid)"""
    q, cent, cb = (np.asarray(fx[k], np.float64) for k in ("q", "cent", "cb"))
    res = q[:64, None, :] - cent[None, :, :]
    near = (res * res).sum(-1).argmin(1)
    r = res[np.arange(res.shape[0]), near]
    r2 = float(np.median((r * r).sum(-1)))
    vmax = float(np.median(np.abs(r).max(-1)))
    cbmax = float(np.abs(cb).max())

    def ok(e):
        if cbmax * 2.0 ** e < 2.0 ** -149 or cbmax * 2.0 ** e >= 2.0 ** 128:
            return False
        with np.errstate(over="ignore"):
            return ms_pair_ok_l2(T0 * 4.0 ** e, r2 * 4.0 ** e, vmax * 2.0 ** e, ms_sigma(cbmax * 2.0 ** e), q.shape[1])

    state = [ok(e) for e in range(lo, hi + 1)]
    flips = [lo + i for i in range(len(state) - 1) if state[i] != state[i + 1]]
    return tuple(sorted({e + k for e in flips for k in (0, 1) if e + k <= 60})), ok


def exponents_for(route, fx, T0=None):
    """the sweep of a route, ascending.  For the shapes of the GPU test this gives about
    {-75, -72, -70, -62, -52..-46, -30, 0, 30, 56..60}."""
    if route == "mscan":
        near = mscan_exponents(fx, T0)[0]
    else:
        near = guard_exponents(route, fx)
    return tuple(sorted(set(FIXED) | set(near) | set(overflow_exponents(fx))))


# ---- labels ----------------------------------------------------------------------------------------------------------------------------
def _min_nonzero(a):
    a = np.abs(np.asarray(a, f32))
    a = a[a > 0]
    return float(a.min()) if a.size else np.inf


def smallest_term(fx, pairs):
    """the smallest nonzero magnitude the reference squares or multiplies: elements of every operand and the f32 differences a - b of
    every (a, b) in `pairs` (all rows of b against all rows of a)"""
    t = min(_min_nonzero(fx[k]) for k in FLOAT_KEYS if k in fx)
    for ka, kb in pairs:
        a, b = np.asarray(fx[ka], f32), np.asarray(fx[kb], f32)
        for row in b:
            t = min(t, _min_nonzero(a - row))
    return t


def classify(e, smallest, largest2, dist_lo):
    """the label of exponent e for a fixture whose smallest squared term is `smallest`^2, largest norm `largest2` (squared) and smallest
    positive answer distance `dist_lo`, all at e = 0 (powers of two scale them exactly: x 2^e, x 4^e):
      overflow   a norm, or a distance bounded by 2 (|x|^2 + |q|^2), may not be finite:        4 largest2 4^e >= 2^128
      invariant  every square the reference forms is NORMAL and every sum finite: scaling by 2^e commutes with every rounding, so ids,
                 codes and probes equal the unscaled ones and distances equal base x 4^e bit for bit
      subnormal  the answer's own distances are below 2^-126
      partial    in between: some squares are subnormal, the distances are not -- nothing is claimed about the oracle there"""
    if 4.0 * largest2 * 4.0 ** e >= 2.0 ** 128:
        return "overflow"
    if (smallest * 2.0 ** e) ** 2 >= 2.0 ** -126:
        return "invariant"
    if dist_lo * 4.0 ** e < 2.0 ** -126:
        return "subnormal"
    return "partial"


def has_subnormals(d):
    u = np.ascontiguousarray(d, f32).view(np.uint32)
    return bool((((u & 0x7F800000) == 0) & ((u & 0x007FFFFF) != 0)).any())


# ---- numpy model of flat_mfma.hip's filter ---------------------------------------------------------------------------------------------
def bf16_rne(a):
    u = np.ascontiguousarray(a, f32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(f32)


def flat_filter_model(x, q, T, guard):
    """-> bool [nq][n]: the pairs flat_mfma.hip's L2 filter hands to the exact evaluation against the thresholds T [nq].
    Both operands split into two bf16 terms (round-to-nearest-even), x.q = hi.hi + hi.lo + lo.hi in f32 (BLAS order, not the matrix
    pipe's), s = fma(-2, x.q, |x|^2 (1 - 2^-12) - (T - |q|^2 (1 - 2^-12))), a pair passes when s <= 0.
    guard: a pair whose 2^-12 (|x|^2 + |q|^2) is not above 2^-100, or not finite, passes whatever s is."""
    x, q, T = np.asarray(x, f32), np.asarray(q, f32), np.asarray(T, f32)
    with np.errstate(all="ignore"):
        xh, qh = bf16_rne(x), bf16_rne(q)
        xl, ql = bf16_rne(x - xh), bf16_rne(q - qh)
        dot = qh @ xh.T
        dot = dot + qh @ xl.T
        dot = dot + ql @ xh.T
        xn = (x * x).sum(axis=1, dtype=f32)
        qn = (q * q).sum(axis=1, dtype=f32)
        c = f32(0.000244140625)
        xk = xn - c * xn
        tq = T - (qn - c * qn)
        s = (np.float64(-2.0) * dot.astype(np.float64) + (xk[None, :] - tq[:, None]).astype(np.float64)).astype(f32)
        ok = s <= 0
        if guard:
            E = c * (xn[None, :] + qn[:, None])
            ok = ok | ~(E > f32(2.0 ** GUARD_LOG2)) | ~np.isfinite(E)
    return ok


def rejected_neighbours(x, q, ids, dists, guard):
    """true neighbours (the oracle's answer ids [nq][k], T = its k-th distance) the model's filter drops"""
    ok = flat_filter_model(x, q, dists[:, -1], guard)
    return int((~np.take_along_axis(ok, ids.astype(np.int64), axis=1)).sum())
