"""Operand magnitude and offset sweep on every surrogate-then-exact route, bit for bit against the oracle (tests/magnitude_spec.py; the
fixtures themselves are checked on the CPU by tests/test_magnitude_spec.py).

Every route that filters or ranks with a low-precision matrix-core surrogate trusts a margin that is RELATIVE to the operands' norms.
The sweep multiplies every operand by 2^e for e on both sides of each route's lower guard (E2 <= 2^-100: about 2^-51 .. 2^-47 here), on
both sides of the point where |x|^2 leaves f32 (2^57 .. 2^60), and at the fixed points 2^-75, -72, -70 (the reference itself computes
in f32 subnormals), -62, -30, 0, 30; it mixes scales inside one call (rows at 2^-52 against unit queries and the reverse, a row block at
2^58, one centroid at 2^40), adds a common offset 2^4 / 2^7 / 2^10 (every pair passes the filters: the queue-overflow, rescan and
recompute paths do the work), and runs binary16 columns down to 2^-13 (half of the elements are binary16 subnormals).  Ids are compared
as unsigned integers, distances as uint32 views, codes as bytes.  Which kernel answers is asserted only at e = 0 and +-30; near and
beyond the guards that is the library's business and only the answer is asserted.  Every case prints its stage counters and
lance_hip_search_stats (pytest -s shows them).  The dot metric runs on every route that takes it, at DOT_EXPONENTS, with models trained
under dot; each dot answer of the oracle is checked for NaN here too (an inf - inf has the host CPU's sign).

Wall time on an MI355X: 22 tests in 13.5 s, most of it imports and engine start-up -- test_ivf_sq_and_rq[rq] 3.2 s (its specification is
numpy), the child process of test_find_partitions 2.7 s, test_ivf_sq_and_rq[sq] 0.9 s, every other test under 0.6 s
(tests/test_zz_gpu_flat_real.py: 22 s on the same machine)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import magnitude_spec as M

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTED = (-30, 0, 30)          # exponents at which the route is asserted: invariant, at least four binades from every guard
STAGES = ("flat_mfma", "flat_mfma_wide", "flat_scan", "ma_sweep", "ma_recheck", "ma_wide_f16", "xf_assign", "xform_fused", "xf_fix", "xf_pqtrain",
          "pq_mfma_estep", "encode_fused", "coarse_fused", "dist_matrix", "coarse_groups", "select_probes", "ivfpq_mscan", "ivfpq_msbound",
          "ivfpq_exact", "ivfpq_scan", "ivfpq_scan_c1", "ivfflat_exact", "ivfflat_scan", "ivfflat_bound", "ivfsq_scan", "ivfsq_exact", "ivfrq_scan",
          "ivfrq_exact", "refine")


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _dev(a):
    import lance_amd.engine as E
    return E.to_device(a)


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


class Stages:
    """the stage counters a block of calls raised"""

    def __init__(self, eng):
        self.eng = eng

    def __enter__(self):
        self.before = {s: self.eng.timing_query("count:" + s)[1] for s in STAGES}
        self.rose = {}
        return self

    def __exit__(self, *a):
        self.eng.synchronize()
        self.rose = {s: int(self.eng.timing_query("count:" + s)[1] - b) for s, b in self.before.items()}
        self.rose = {s: v for s, v in self.rose.items() if v}
        self.rose["replayed_queries"] = self.eng.search_stats()


def report(route, tag, st):
    print(f"[magnitude] {route} {tag}: {st.rose}")


def ids_differ(got, want):
    """-> the first differing query (row) or None"""
    bad = np.nonzero((np.asarray(got) != np.asarray(want)).reshape(len(want), -1).any(axis=1))[0]
    return None if bad.size == 0 else int(bad[0])


def bits_differ(got, want):
    return ids_differ(np.ascontiguousarray(got, f32).view(np.uint32), np.ascontiguousarray(want, f32).view(np.uint32))


class Failures(list):
    """collects every failing case of a sweep, so that one run names all of them"""

    def check(self, tag, *pairs):
        for what, got, want, as_bits in pairs:
            q = (bits_differ if as_bits else ids_differ)(got, want)
            if q is not None:
                self.append((tag, what, "first differing query / row", q))
                return False
        return True

    def done(self):
        assert not self, f"{len(self)} cases differ from the oracle: {self[:12]}"


def variants(fx, route, metric="l2", T0=None):
    """(tag, fixture, assert the route's counter) of a route's whole family"""
    if metric == "dot":
        return [(f"dot e={e}", M.scaled(fx, e), e in COUNTED) for e in M.DOT_EXPONENTS]
    out = [(f"e={e}", M.scaled(fx, e), e in COUNTED) for e in M.exponents_for(route, fx, T0)]
    out += [(name, m, False) for name, m in M.mixed_cases(fx).items()]
    out += [(f"offset 2^{r}", M.offset(fx, r), False) for r in M.OFFSETS]
    return out


# ---- flat KNN: flat_mfma.hip (d <= 128) and flat_mfma_wide.hip (long rows) -----------------------------------------------------------------
def _flat(eng, oracle, fails, route, tag, fx, metric, ks, counter, counted):
    with np.errstate(all="ignore"):
        oi, od = oracle.flat_knn(fx.x, fx.q, max(ks), metric)
    assert metric != "dot" or not np.isnan(od).any(), (tag, "the oracle's dot answer holds a NaN")
    xd, qd = _dev(fx.x), _dev(fx.q)
    for k in ks:
        with Stages(eng) as st:
            gi, gd = eng.flat_topk(xd, qd, k, metric)
        report(route, f"{tag} {metric} k={k}", st)
        fails.check((tag, metric, k), ("ids", _np(gi).view(np.uint64), oi[:, :k], False), ("distances", _np(gd), od[:, :k], True))
        if counted:
            assert st.rose.get(counter, 0) >= 1, f"{counter} did not serve {tag} k={k}: {st.rose}"
    return st


@pytest.mark.parametrize("d", [64, 128])
def test_flat_filter(eng, oracle, d):
    """flat_mfma.hip: n 6000 (first epoch 2048 rows on the exact kernel, the rest on the filter), nq 130 (two full query tiles and a
    ragged one), k 10 and 100.  The offset family fills the per-query queues (FM_SQ_CAP) and the pools: the exact rescan answers.
    The row blocks at 2^58 and 2^59 are rows 3000 .. 3127: the filter meets them, beside ordinary rows and against ordinary queries
    (d = 64: filtered at 2^58, |x|^2 past the 2^126 guard at 2^59; d = 128: past the guard at 2^58, |x|^2 = +inf at 2^59)."""
    fx = M.flat_fixture(d)
    fails = Failures()
    for tag, v, counted in variants(fx, "flat"):
        _flat(eng, oracle, fails, "flat", tag, v, "l2", (10, 100), "flat_mfma", counted)
    for tag, v, counted in variants(fx, "flat", "dot"):
        _flat(eng, oracle, fails, "flat", tag, v, "dot", (10,), "flat_mfma", counted)
    fails.done()


def test_flat_filter_f16_columns(eng, oracle):
    """binary16 rows and queries at 2^-8, 2^-11, 2^-13 (half of the elements binary16 subnormals) and 2^3"""
    fails = Failures()
    for s in M.F16_SCALES:
        _flat(eng, oracle, fails, "flat f16", f"2^{s}", M.f16_fixture(s), "l2", (10, 100), "flat_mfma", True)
    fails.done()


def test_flat_filter_long_rows(eng, oracle):
    """flat_mfma_wide.hip, d = 256: one bf16 product, margin 0.0084 (|x|^2 + |q|^2); cosine at the bottom, at the guard and in the middle"""
    fx = M.flat_fixture(256)
    fails = Failures()
    for tag, v, counted in variants(fx, "flat_wide"):
        _flat(eng, oracle, fails, "flat_wide", tag, v, "l2", (10,), "flat_mfma_wide", counted)
    for tag, v, counted in variants(fx, "flat_wide", "dot"):
        _flat(eng, oracle, fails, "flat_wide", tag, v, "dot", (10,), "flat_mfma_wide", counted)
    for e in (-75, -49, 0, 30):
        _flat(eng, oracle, fails, "flat_wide", f"e={e}", M.scaled(fx, e), "cosine", (10,), "flat_mfma_wide", e in COUNTED)
    fails.done()


# ---- assign: mfma_assign.hip / the transform kernel's first half ----------------------------------------------------------------------------
def _assign(eng, oracle, fails, route, tag, fx, metric, counter, counted):
    with np.errstate(all="ignore"):
        oi, od = oracle.assign(fx.x, fx.cent, metric)
    with Stages(eng) as st:
        gi, gd = eng.assign(fx.x, fx.cent, metric)
    report(route, f"{tag} {metric}", st)
    ok = oi != oracle.NONE
    fails.check((tag, metric), ("partition ids", _np(gi).view(np.uint32), oi, False), ("distances", _np(gd)[ok], od[ok], True))
    if counted and counter:
        assert st.rose.get(counter, 0) >= 1, f"{counter} did not serve {tag}: {st.rose}"
    return st


@pytest.mark.parametrize("d", [64, 128])
def test_assign(eng, oracle, d):
    """n 6000, k 48.  One centroid at 2^40 inflates every row's margin (all rows undecided); the offset family leaves every centroid inside
    the margin: the exact re-check (ma_recheck) decides, which is asserted"""
    fx = M.assign_fixture(d)
    fails = Failures()
    for tag, v, counted in variants(fx, "assign"):
        st = _assign(eng, oracle, fails, "assign", tag, v, "l2", "ma_sweep", counted)
        if tag.startswith("offset") or counted:
            assert st.rose.get("ma_recheck", 0) >= 1, (tag, st.rose)
    for tag, v, counted in variants(fx, "assign", "dot"):
        _assign(eng, oracle, fails, "assign", tag, v, "dot", "ma_sweep", counted)
    fails.done()


def test_kmeans_training_across_scales(eng, oracle):
    """six iterations of k-means on the scaled rows: centroids, loss and iteration count are the oracle's at that scale"""
    fx = M.assign_fixture(64)
    near = M.guard_exponents("assign", fx)
    for e in (near[0], near[-1], -30, 0, 30):
        s = M.scaled(fx, e)
        with Stages(eng) as st:
            cent, loss, iters = eng.kmeans_train(s.x, 48, max_iters=6, seed=3)
        report("kmeans_train", f"e={e}", st)
        oc, ol, oit, _ = oracle.kmeans_train(s.x, 48, max_iters=6, seed=3)
        assert iters == oit and loss == ol, (e, iters, oit, loss, ol)
        assert bits_differ(_np(cent), oc) is None, e
        if e in COUNTED:
            assert st.rose.get("ma_sweep", 0) >= 1, st.rose


@pytest.mark.parametrize("dtype", ["f32", "f16"])
def test_assign_long_rows(eng, oracle, dtype):
    """d = 256, k 64 (the K-tiled sweep takes 64 centroids and more):   f32: the whole family; f16 rows at 2^0, 2^-8, 2^-11, 2^-13
    (binary16 subnormals) and 2^3.  No counter is asserted on this route: the K-tiled f32 sweep (ma_launch_wide) has no stage name, and
    `ma_wide_f16`, the single-f16-product sweep, is reachable only through the cosine transform's binary16 plane (mfma_assign.hip:831),
    never through `assign` -- test_cosine_long_rows_take_the_f16_product_at_every_scale below asserts it."""
    fx = M.assign_fixture(256, n=3000, k=64)
    fails = Failures()
    if dtype == "f32":
        for tag, v, _ in variants(fx, "assign"):
            _assign(eng, oracle, fails, "assign_wide", tag, v, "l2", None, False)
    else:
        for s in (0,) + M.F16_SCALES:
            v = M.scaled(fx.but(x=(fx.x * f32(0.25)).astype(np.float16), cent=(fx.cent * f32(0.25)).astype(np.float16)), s)
            _assign(eng, oracle, fails, "assign_wide f16", f"2^{s}", v, "l2", None, False)
    fails.done()


def test_cosine_long_rows_take_the_f16_product_at_every_scale(eng, oracle):
    """the one way to `ma_wide_f16`: a cosine transform of long rows (d = 256, 64 lists, M 16).  The normalise kernel leaves unit rows
    and their binary16 plane whatever the scale of the column: the unit rows, hence ids, codes and loss, are the same bit for bit at
    2^-30, 2^0 and 2^30 (asserted on the oracle), and the single-f16-product sweep serves every one of them (all three are invariant
    exponents, far from every guard)."""
    from test_zz_gpu_xform_fused import run_case
    fx = M.assign_fixture(256, n=3000, k=64)
    unit = oracle.normalize(fx.x)
    cent, _ = M.ivf_models(unit, 64, 0, seed=13)      # centroids of unit vectors: inside the unit ball, as the f16 plane's scale needs
    part, _ = oracle.assign(unit, cent, "l2")
    res = oracle.residual(unit, cent, part)
    rng = np.random.default_rng(13)
    cb = np.stack([res[rng.choice(res.shape[0], 256, replace=False)][:, i * 16:(i + 1) * 16] for i in range(16)]).astype(f32)
    for e in COUNTED:
        x = M.scaled(fx, e).x
        assert bits_differ(oracle.normalize(x), unit) is None, ("normalisation kept a scale", e)
        with Stages(eng) as st:
            run_case(eng, oracle, x, cent, cb, "cosine", stage="xform_tail")
        report("cosine transform, long rows", f"e={e}", st)
        assert st.rose.get("ma_wide_f16", 0) >= 1, (e, st.rose)


# ---- the fused transform (xform_fused.hip, pq_mfma.hip) ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m", [(32, 4), (128, 16)])
def test_transform(eng, oracle, d, m):
    """ivfpq_encode (run_case of test_zz_gpu_xform_fused.py: partition ids, codes, the f64 loss, and the fused kernel served the call),
    pq_encode on the residuals, and four iterations of pq_train, on the scaled models"""
    from test_zz_gpu_xform_fused import run_case
    fx = M.xform_fixture(d, m)
    fails = Failures()
    near = M.guard_exponents("pq", fx)
    for tag, v, counted in variants(fx, "xform") + [(f"pq e={e}", M.scaled(fx, e), False) for e in near]:
        with Stages(eng) as st:
            try:
                with np.errstate(all="ignore"):
                    run_case(eng, oracle, v.x, v.cent, v.cb, "l2")
            except AssertionError as err:
                fails.append((tag, "ivfpq_encode", str(err)[:200]))
        report("xform", tag, st)
        with np.errstate(all="ignore"):
            part, _ = oracle.assign(v.x, v.cent)
            res = oracle.residual(v.x, v.cent, np.where(part == oracle.NONE, 0, part))
            ocodes = oracle.pq_encode(res, v.cb)
        with Stages(eng) as st:
            codes = eng.pq_encode(res, v.cb)
        report("pq_encode", tag, st)
        fails.check((tag, "pq_encode"), ("codes", _np(codes), ocodes, False))
        if counted:
            assert st.rose.get("pq_mfma_estep", 0) >= 1, (tag, st.rose)      # (pq_mfma.hip serves pq_encode under this name)
        if tag in ("e=0", "e=-30", "e=30", f"e={near[0]}", f"pq e={near[0]}", f"pq e={near[-1]}"):
            with Stages(eng) as st:
                cb, iters = eng.pq_train(res, m, max_iters=4, seed=9)
            report("pq_train", tag, st)
            ocb, oit = oracle.pq_train(res, m, max_iters=4, seed=9)
            assert (_np(iters) == oit.astype(np.uint32)).all(), (tag, _np(iters), oit)
            fails.check((tag, "pq_train"), ("codebook", _np(cb).reshape(len(ocb), -1), ocb.reshape(len(ocb), -1), True))
            if counted:
                assert st.rose.get("pq_mfma_estep", 0) + st.rose.get("xf_pqtrain", 0) >= 1, (tag, st.rose)
    # dot: models trained under dot; the transform assigns by the largest product and encodes the ROWS (no residual), pq_encode picks the
    # codeword of the largest product per sub-vector.  run_case asserts that the fused kernel served each call.
    fxd = M.xform_fixture(d, m, metric="dot")
    for tag, v, _ in variants(fxd, "xform", "dot"):
        with Stages(eng) as st:
            try:
                with np.errstate(all="ignore"):
                    run_case(eng, oracle, v.x, v.cent, v.cb, "dot")
            except AssertionError as err:
                fails.append((tag, "ivfpq_encode", str(err)[:200]))
        report("xform", tag, st)
        with np.errstate(all="ignore"):
            ocodes = oracle.pq_encode(v.x, v.cb, "dot")
        with Stages(eng) as st:
            codes = eng.pq_encode(v.x, v.cb, "dot")
        report("pq_encode", tag, st)
        fails.check((tag, "pq_encode"), ("codes", _np(codes), ocodes, False))
    fails.done()


# ---- find_partitions on the matrix cores: a child process with LANCE_HIP_MFMA_COARSE=1 (read once per process) ---------------------------------
COARSE_SHAPES = ((64, 100, "coarse_fused"), (128, 960, "coarse_fused"), (64, 961, "dist_matrix"), (64, 1024, "coarse_groups"))


def _coarse_cases():
    """runs inside the child"""
    sys.path.insert(0, ROOT)
    import oracle
    from lance_amd.engine import Engine
    eng = Engine()
    fails = Failures()
    n_cases = 0

    def one(tag, fx, metric, counter, counted):
        nonlocal n_cases
        for nprobes in (1, 10, 64):
            with np.errstate(all="ignore"):
                oi, od = oracle.find_partitions(fx.q, fx.cent, nprobes, metric)
            with Stages(eng) as st:
                gi, gd = eng.find_partitions(fx.q, fx.cent, nprobes, metric)
            report("find_partitions", f"{fx.cent.shape} {tag} {metric} nprobes={nprobes}", st)
            fails.check((fx.cent.shape, tag, metric, nprobes), ("probes", _np(gi).view(np.uint32), oi, False), ("distances", _np(gd), od, True))
            if counted:
                assert st.rose.get(counter, 0) >= 1, f"{counter} did not serve {tag}: {st.rose}"
            n_cases += 1

    for d, nlist, counter in COARSE_SHAPES:
        fx = M.coarse_fixture(d, nlist)
        for tag, v, counted in variants(fx, "coarse"):
            one(tag, v, "l2", counter, counted)
        for tag, v, counted in variants(fx, "coarse", "dot"):
            one(tag, v, "dot", counter, counted)
        # cosine: rows and queries are normalised, then L2 -- the normalisation erases a power-of-two scale exactly
        base = fx.but(q=oracle.normalize(fx.q), cent=oracle.normalize(fx.cent))
        for e in (-30, 0, 30):
            s = M.scaled(fx, e)
            v = fx.but(q=oracle.normalize(s.q), cent=oracle.normalize(s.cent))
            assert bits_differ(v.q, base.q) is None and bits_differ(v.cent, base.cent) is None, ("normalisation kept a scale", e)
            one(f"cosine e={e}", v, "l2", counter, True)
    eng.close()
    fails.done()
    print(f"magnitude coarse cases ok: {n_cases}")


def test_find_partitions():
    """fused (100 and 960 lists), two-kernel (961) and per-group (1024) coarse routes; nq 130, nprobes 1 / 10 / 64"""
    env = dict(os.environ, LANCE_HIP_MFMA_COARSE="1")
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_zz_gpu_magnitude as t; t._coarse_cases()"
                        % (ROOT, os.path.join(ROOT, "tests"))], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    print(r.stdout[-20000:])
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "magnitude coarse cases ok" in r.stdout


# ---- IVF_PQ search: the ADC scan and bound pass on the matrix cores (search_ms.hip) ---------------------------------------------------------------
def _ivfpq(eng, oracle, fails, tag, fx, metric, counted, rescan=False):
    """rescan: assert that the exact rescan's stage (`ivfpq_exact`, search.hip) ran in each search.  Like every stage counter it counts
    launches: the rescan is launched on every search and its workgroups return at once for queries that carry no flag, so the count
    shows that the repair path is wired behind the matrix-core scan, not how many queries it answered.  That number is
    lance_hip_search_stats (`replayed_queries` in the printed line), printed and not asserted: see test_ivfpq_scan_f32."""
    from lance_amd.engine import DeviceIndex
    raw32 = fx.x.astype(f32)
    with np.errstate(all="ignore"):
        oidx = oracle.build_index(fx.x, fx.cent, fx.cb, metric)
    gpart, gcodes, _ = eng.ivfpq_encode(fx.x, fx.cent, fx.cb, metric)
    kept = oidx.part_ids != oracle.NONE          # (a row without a partition -- its distances overflowed -- has no specified code)
    if not fails.check((tag, metric, "encode"), ("partition ids", _np(gpart).view(np.uint32), oidx.part_ids, False),
                       ("codes", _np(gcodes)[kept], oidx.codes_rowmajor[kept], False)):
        return None
    gidx = DeviceIndex.create(eng, metric, fx.cent, fx.cb, gpart, gcodes, None, raw=fx.x)
    try:
        for rf in (0, 4):
            with Stages(eng) as st:
                gi, gd = gidx.search(fx.q, 10, 8, rf)
            report("ivfpq", f"{tag} {metric} refine={rf}", st)
            with np.errstate(all="ignore"):
                oi, od = oidx.search(fx.q, 10, 8, refine=rf, raw=raw32 if rf else None)
            assert metric != "dot" or not np.isnan(od).any(), (tag, rf, "the oracle's dot answer holds a NaN")
            fails.check((tag, metric, rf), ("ids", _np(gi).view(np.uint64), oi, False), ("distances", _np(gd), od, True))
            if counted:
                assert st.rose.get("ivfpq_mscan", 0) >= 1 and st.rose.get("ivfpq_msbound", 0) >= 1, (tag, rf, st.rose)
            if rescan:
                assert st.rose.get("ivfpq_exact", 0) >= 1, (tag, rf, st.rose)
    finally:
        gidx.close()


def _t0(oracle, fx):
    idx = oracle.build_index(fx.x, fx.cent, fx.cb)
    return float(np.median(idx.search(fx.q, 10, 8)[1][:, -1]))


@pytest.mark.parametrize("part", ["low", "middle", "high", "mixed and offset", "dot"])
def test_ivfpq_scan_f32(eng, oracle, part):
    """n 20000, d 64, M 16, 24 lists, 700 queries x 8 probes (the gate nq * nprobes >= 96 * nlist), refine 0 and 4.  The sweep is
    search_ms.hip's own: the exponents where its pair predicate flips (tests/magnitude_spec.py: mscan_exponents), the fixed points and the
    top of the range.  dot: an index whose centroids and codebook were trained under dot (no residual: the codebook spans the rows),
    at DOT_EXPONENTS -- search_ms.hip's dot branch has guards of its own (G * s < 1e30, the centred codebook plane, cmax / cmaxp).
    The offset family asserts that the exact rescan's stage ran (`ivfpq_exact`).  It replays no query at 2^4, 2^7 or 2^10 (printed:
    replayed_queries 0): under L2 the scan works on the residuals q - c, in which a common offset cancels -- the centroids are retrained
    on the shifted rows -- so T and |r|^2 keep their unit scale.  What the offset loads in this chain is the coarse step and the encode
    (every centroid inside the margin: test_assign, test_transform, test_find_partitions).  The scan's own repair does the work in the
    mixed case `rows 2^-52` (634 of 700 queries replayed) and below search_ms.hip's guards in the sweep."""
    if part == "dot":
        fx = M.ivfpq_fixture("f32", metric="dot")
        fails = Failures()
        for tag, v, counted in variants(fx, "mscan", "dot"):
            _ivfpq(eng, oracle, fails, tag, v, "dot", counted)
        fails.done()
        return
    fx = M.ivfpq_fixture("f32")
    fam = variants(fx, "mscan", T0=_t0(oracle, fx))
    sweep = [v for v in fam if v[0].startswith("e=")]
    third = (len(sweep) + 2) // 3
    chosen = {"low": sweep[:third], "middle": sweep[third:2 * third], "high": sweep[2 * third:], "mixed and offset": [v for v in fam if not v[0].startswith("e=")]}[part]
    fails = Failures()
    for tag, v, counted in chosen:
        _ivfpq(eng, oracle, fails, tag, v, "l2", counted, rescan=tag.startswith("offset"))
    if part == "middle":
        base = None
        cent, cb = M.ivf_models(oracle.normalize(fx.x), 24, 16, seed=43)      # the models of a cosine index live on the unit sphere: not scaled
        for e in (-30, 0, 30):      # cosine: the normalisation erases the scale -- the answer is the same at every exponent
            s = M.scaled(fx, e).but(cent=cent, cb=cb)
            with np.errstate(all="ignore"):
                ans = oracle.build_index(s.x, s.cent, s.cb, "cosine").search(s.q, 10, 8)
            base = base or ans
            assert ids_differ(ans[0], base[0]) is None and bits_differ(ans[1], base[1]) is None, ("cosine kept a scale", e)
            _ivfpq(eng, oracle, fails, f"e={e}", s, "cosine", False)
    fails.done()


def test_ivfpq_scan_f16_columns(eng, oracle):
    fx = M.ivfpq_fixture("f16")
    fails = Failures()
    for s in (0,) + M.F16_SCALES:
        _ivfpq(eng, oracle, fails, f"f16 2^{s}", M.scaled(fx, s), "l2", s == 0)
    fails.done()


# ---- IVF_FLAT: the exact scan ------------------------------------------------------------------------------------------------------------------
def test_ivf_flat(eng, oracle):
    from lance_amd.engine import DeviceFlatIndex
    fx = M.ivfflat_fixture()
    fails = Failures()
    for metric in ("l2", "dot"):
        for tag, v, _ in variants(fx, "assign", metric):
            with np.errstate(all="ignore"):
                oi, od = oracle.ivfflat_search(v.x, v.cent, v.q, 10, 4, metric)
            assert metric != "dot" or not np.isnan(od).any(), (tag, "the oracle's dot answer holds a NaN")
            part, _ = eng.assign(v.x, v.cent, metric)
            g = DeviceFlatIndex.create(eng, metric, v.cent, v.x, part)
            try:
                with Stages(eng) as st:
                    gi, gd = g.search(v.q, 10, 4)
                report("ivf_flat", f"{tag} {metric}", st)
                fails.check((tag, metric), ("ids", _np(gi).view(np.uint64), oi, False), ("distances", _np(gd), od, True))
            finally:
                g.close()
    fails.done()


# ---- IVF_SQ and IVF_RQ: the bounds and factors scale with the data ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["sq", "rq"])
def test_ivf_sq_and_rq(eng, oracle, kind):
    """n 3000, d 64, 16 lists; refine_factor 0 (the quantised distances, against sq_spec.search / rq_spec.search) and 4 (exact distances
    of the candidates, tests/refine_spec.py).  r * r / 65025 and the RaBitQ factors under- and overflow in their own order of operations.
    L2: the whole family; dot (both kinds take it): centroids trained under dot, at DOT_EXPONENTS."""
    import refine_spec as F
    import rq_spec as R
    import sq_spec as S
    from lance_amd.engine import DeviceRqIndex, DeviceSqIndex
    fails = Failures()
    for metric in ("l2", "dot"):
        fx = M.sqrq_fixture(metric=metric)
        rid = np.arange(fx.x.shape[0], dtype=np.uint64)
        for tag, v, _ in variants(fx, "assign", metric):
            with np.errstate(all="ignore"):
                if kind == "sq":
                    xs, part = S.prepare_rows(oracle, v.x, v.cent, metric)
                    b = S.bounds(xs[:64])
                    codes = S.encode(xs, *b)
                    gcodes = eng.sq_encode(xs, b)
                    if not fails.check((tag, "sq_encode"), ("codes", _np(gcodes), codes, False)):
                        continue
                    ix = DeviceSqIndex.create(eng, metric, v.cent, gcodes, part, b, row_ids=rid)
                    spec = lambda keff: S.search(oracle, codes, part, v.cent, v.q, keff, 4, metric, *b, row_ids=rid)
                else:
                    P = R.rotation(64, 7)
                    part, codes, add, scale = R.build(oracle, v.x, v.cent, P, metric)
                    gc, ga, gs = eng.rq_encode(v.x, part.view(np.int32), oracle.assign(v.x, v.cent, metric)[1], v.cent, P, metric)
                    if not fails.check((tag, "rq_encode"), ("codes", _np(gc), codes, False), ("add", _np(ga), add, True), ("scale", _np(gs), scale, True)):
                        continue
                    ix = DeviceRqIndex.create(eng, metric, v.cent, P, gc, ga, gs, part.view(np.int32), row_ids=rid)
                    spec = lambda keff: R.search(oracle, codes, add, scale, part, v.cent, P, v.q, keff, 4, metric, row_ids=rid)
                try:
                    ix.set_raw(v.x)
                    for rf in (0, 4):
                        with Stages(eng) as st:
                            gi, gd = ix.search(v.q, 10, 4, refine_factor=rf)
                        report("ivf_" + kind, f"{tag} refine={rf}", st)
                        oi, od = spec(10) if rf == 0 else F.refine(oracle, spec(40)[0], v.x, v.q, 10, metric)
                        assert metric != "dot" or not np.isnan(od).any(), (tag, rf, "the specification's dot answer holds a NaN")
                        fails.check((tag, rf), ("ids", _np(gi).view(np.uint64), oi, False), ("distances", _np(gd), od, True))
                finally:
                    ix.close()
    fails.done()
