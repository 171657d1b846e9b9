"""The numpy model of the batched multivector filter (tests/multivec_batch_spec.py; lance_amd/csrc/multivec_batch.hip) held to its margin,
the mutants of the margin and of the survivor rule each caught by a named fixture, the survivor sets bounded, the host-side
validation of the batch entry points, and the ABI.  No GPU: tests/test_zz_gpu_multivec_batch.py holds the kernels to the same
specification bit for bit.

Measured (this file's prints): the adversarial fixture's operand error is 2.69e-5 per pair = 0.588 of the operand term
3.002 * 2^-16 and 1.76 times what one operand's roundoff alone would allow; with nqv = 8 its |D~ - D| = 2.14e-4 is 0.47 of E."""
import os
import re

import numpy as np
import pytest

import multivec_batch_spec as B
import multivec_spec as M

f32, f64 = np.float32, np.float64
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ragged(rows, lo, hi, d, nqv, seed, kind):
    return M.column(M.lengths(rows, lo, hi, seed), d, nqv, seed, kind)


# name -> (values, offsets, q): what the margin is held to
def _fixtures():
    fx = {"adversarial": B.adversarial(8, 16), "adversarial_nqv1": B.adversarial(1, 16)}
    for kind in ("f32", "f16"):
        for d, nqv in ((8, 5), (20, 33), (128, 32), (136, 7), (256, 64)):
            fx[f"{kind}_d{d}_nqv{nqv}"] = _ragged(120, 1, 40, d, nqv, 1000 + d, kind)
    v, off, q = _ragged(120, 1, 12, 20, 6, 5, "f32")
    fx["scaled_down"] = (v * f32(2.0 ** -40), off, q)
    fx["scaled_up"] = (v * f32(2.0 ** 40), off, q * f32(2.0 ** 40))
    v, off, q = _ragged(60, 1, 8, 128, 256, 6, "f32")
    fx["nqv256"] = (v, off, q)
    return fx


FIXTURES = _fixtures()


def _errors(oracle, name, pipe=None, col0=0):
    values, off, q = FIXTURES[name]
    dist = M.distances(oracle, values, off, q, "cosine")
    dt, degen, qdegen = B.surrogate(values, off, q, col0=col0, pipe=pipe)
    assert not degen.any() and not qdegen, name
    return np.abs(dt.astype(f64) - dist.astype(f64)), q.shape[0], values.shape[1]


# ---- margin -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_margin_holds(oracle, name):
    """|D~_model - D_spec| <= E on every fixture: the f64 pipe, a pipe that truncates every partial sum, and a query that does not
    start at a column block (the sum's pieces move)"""
    for pipe, col0 in ((None, 0), (B.pipe_truncating, 0), (None, 21)):
        if pipe and FIXTURES[name][0].shape[1] > 32:
            continue                                      # (the truncating pipe walks the elements one by one: small d only)
        err, nqv, d = _errors(oracle, name, pipe, col0)
        e = B.margin(nqv, d)
        print(name, "pipe" if pipe else "f64", col0, "max |D~ - D| =", err.max(), "E =", e, "ratio", err.max() / e)
        assert (err <= e).all(), (name, err.max(), e)


def test_adversarial_fixture_reaches_its_fraction(oracle):
    """the elements sit just under half an ulp of the kept bits from their neighbours, errors aligned: the operand error of the pair
    (u, u) is more than HALF the operand term, and |D~ - D| of row 0 more than 0.4 of E at nqv = 8"""
    values, off, q = FIXTURES["adversarial"]
    xn, hi, lo, _ = B.split(values)
    qn, qh, ql, _ = B.split(q)
    err = (xn.astype(f64) @ qn.astype(f64).T - B.kept_products(hi, lo, qh, ql))[0, 0]
    t = B.terms(16)
    print("operand error", err, "of", t["operands"], "=", err / t["operands"])
    assert 0.5 * t["operands"] < err <= t["operands"]
    tot, nqv, d = _errors(oracle, "adversarial")
    assert tot[0] > 0.4 * B.margin(nqv, d)


def test_each_source_within_its_term(oracle):
    """the terms of EP one by one, on the fixtures a truncating pipe can walk: (b) the split against the f64 product of the f32
    normalised operands, (c) the pipe against the exact sum of the kept products, (a) + (d) the f32 normalised product against the
    similarity the exact arithmetic returns"""
    for name in ("adversarial", "f32_d8_nqv5", "f16_d20_nqv33", "scaled_down"):
        values, off, q = FIXTURES[name]
        d = values.shape[1]
        t = B.terms(d)
        xn, hi, lo, _ = B.split(values)
        qn, qh, ql, _ = B.split(q)
        full = xn.astype(f64) @ qn.astype(f64).T
        kept = B.kept_products(hi, lo, qh, ql)
        assert np.abs(full - kept).max() <= t["operands"], name
        acc = np.abs(B.pipe_truncating(hi, lo, qh, ql).astype(f64) - kept).max()
        assert 0 < acc <= t["accumulation"], (name, acc)
        kind = "cosine"
        sim = np.stack([f32(1) - oracle.distance_batch(kind, qi, values) for qi in q], 1)
        assert np.abs(full - sim.astype(f64)).max() <= t["f32_sides"] + t["underflow"], name


# ---- mutants ------------------------------------------------------------------------------------------------------------------
def test_mutant_one_operands_roundoff_only(oracle):
    """operand term 1.001 * 2^-16 (one residual instead of two and the dropped lo lo): fixture `adversarial`, the pair (u, u)"""
    values, off, q = FIXTURES["adversarial"]
    xn, hi, lo, _ = B.split(values)
    qn, qh, ql, _ = B.split(q)
    err = (xn.astype(f64) @ qn.astype(f64).T - B.kept_products(hi, lo, qh, ql))[0, 0]
    assert err > B.terms(16, operand=1.001)["operands"]
    assert err <= B.terms(16)["operands"]


def test_mutant_nqv_factor_dropped(oracle):
    """E = EP + the sums' term: fixture `adversarial`, eight query vectors whose errors add"""
    err, nqv, d = _errors(oracle, "adversarial")
    assert err[0] > B.margin(nqv, d, nqv_factor=False)
    assert err[0] <= B.margin(nqv, d)


def test_mutant_no_accumulation_term(oracle):
    """term (c) = 0: fixture `f32_d8_nqv5` under the truncating pipe -- the pipe's own error is not zero, and nothing else in EP is
    there to pay for it (each source is held to its own term, test_each_source_within_its_term)"""
    values, off, q = FIXTURES["f32_d8_nqv5"]
    _, hi, lo, _ = B.split(values)
    _, qh, ql, _ = B.split(q)
    acc = np.abs(B.pipe_truncating(hi, lo, qh, ql).astype(f64) - B.kept_products(hi, lo, qh, ql)).max()
    assert acc > B.terms(8, accumulation=False)["accumulation"]
    assert acc <= B.terms(8)["accumulation"]


def _attained(k=3):
    """Fixture `attained`: surrogates that reach the margin.  Rows 0 .. k-1 are the true top k with D = 0.1, 0.2, .. ; row k-1's
    surrogate errs up by E, the others' down by E; ten more rows lie far away.  -> (D, D~, E)"""
    e = f32(0.01)
    d = np.concatenate([f32(0.1) * np.arange(1, k + 1, dtype=f32), np.full(10, f32(5))]).astype(f32)
    d[k - 1] = d[k - 2] + f32(0.001)                   # the k-th row nearly ties with the one before it
    dt = d.copy()
    dt[:k - 1] -= f32(0.9999) * e
    dt[k - 1] += f32(0.9999) * e
    dt[k:] -= f32(0.9999) * e
    return d, dt, e


def test_mutant_threshold_t_plus_e():
    """survivors = {D~ <= t + E}: fixture `attained`.  The true k-th row's surrogate errs up by E; a row just behind it in truth
    (D_k + E / 2) errs down by E and becomes the k-th smallest surrogate, so t = D_k - E / 2 and the k-th row sits 1.5 E above t:
    inside t + 2 E, outside t + E"""
    k = 3
    d, dt, e = _attained(k)
    d = np.append(d, d[k - 1] + f32(0.5) * e).astype(f32)
    dt = np.append(dt, d[-1] - f32(0.9999) * e).astype(f32)
    assert (np.abs(dt.astype(f64) - d) <= e).all()
    degen = np.zeros(d.size, bool)
    top = set(np.argsort(d, kind="stable")[:k].tolist())
    assert top == {0, 1, 2}
    good = B.survivors(dt, degen, k, e)
    assert top <= set(np.nonzero(good)[0].tolist())
    bad = B.survivors(dt, degen, k, e, slack=1.0)
    assert not top <= set(np.nonzero(bad)[0].tolist())


def test_mutant_degenerate_rows_counted_in_t(oracle):
    """Fixture `degenerate_near`: k rows that hold the query's own vectors AND one NaN vector.  Their surrogate (the NaN vector stored as
    zeros) is the smallest of the column, their true distance is NaN and sorts last.  Counted in t they make the threshold so small
    that the true top k is dropped."""
    k = 3
    lens = M.lengths(40, 2, 6, 17)
    lens[[5, 11, 23]] = 6
    values, off, q = M.column(lens, 20, 4, 17, "f32")
    for r in (5, 11, 23):
        values[off[r]:off[r] + 4] = q
        values[off[r] + 4, 3] = np.nan
    dist = M.distances(oracle, values, off, q, "cosine")
    dt, degen, _ = B.surrogate(values, off, q)
    assert degen[[5, 11, 23]].all() and degen.sum() == 3 and np.isnan(dist[[5, 11, 23]]).all()
    e = B.margin(4, 20)
    top = set(np.argsort(S_keys(dist), kind="stable")[:k].tolist())
    good = B.survivors(dt, degen, k, e)
    assert top <= set(np.nonzero(good)[0].tolist()) and good[[5, 11, 23]].all()
    bad = B.survivors(dt, degen, k, e, degenerate_in_t=True)
    assert not top <= set(np.nonzero(bad)[0].tolist())


def S_keys(d):
    return M.S.keys(d)


# ---- survivors ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f16"])
def test_survivor_superset(oracle, kind):
    """2000 rows of 1..40 vectors, d = 128, nqv = 32, k = 10: the model's survivors hold the specification's top k, lie inside
    {D_spec <= t_spec + 4 E} (which follows from |D~ - D| <= E), and that set is under a tenth of the rows"""
    values, off, q = _ragged(2000, 1, 40, 128, 32, 21, kind)
    dist = M.distances(oracle, values, off, q, "cosine")
    dt, degen, _ = B.surrogate(values, off, q)
    e = B.margin(32, 128)
    surv = B.survivors(dt, degen, 10, e)
    t_spec = B.threshold(dist, degen, 10)
    inside = ~(dist.astype(f64) > f64(t_spec) + 4 * e)
    print(kind, "survivors", int(surv.sum()), "superset", int(inside.sum()), "of", dist.size)
    assert (surv <= inside).all()
    assert set(np.argsort(S_keys(dist), kind="stable")[:10].tolist()) <= set(np.nonzero(surv)[0].tolist())
    assert 10 <= surv.sum() <= B.superset_count(dist, degen, 10, e) < dist.size // 10


def test_degenerate_rows_and_queries_are_found():
    values, off, q = _ragged(30, 1, 5, 20, 4, 3, "f32")
    values = values.copy()
    values[off[2]] = 0                      # a zero vector
    values[off[7] + 0, 1] = np.nan
    values[off[9], 5] = np.inf
    values[off[12]] *= f32(2.0 ** -60)      # norm under 2^-50
    values[off[14]] = f32(2.0 ** 63)        # squared norm at 2^126 and above
    dt, degen, qdegen = B.surrogate(values, off, q)
    assert np.nonzero(degen)[0].tolist() == [2, 7, 9, 12, 14] and not qdegen and np.isfinite(dt).all()
    q2 = q.copy()
    q2[1] = 0
    assert B.surrogate(values, off, q2)[2]


def test_margin_formula_matches_the_kernels_header():
    """the constants of E in multivec_batch.hip's header and in mvb_margin are this module's"""
    src = open(os.path.join(ROOT, "lance_amd", "csrc", "multivec_batch.hip")).read()
    assert "EP(K) = 3.002 * 2^-16 + (9.2 K + 20) u + 2^-30" in src and "E(nqv, K) = nqv EP(K) + (nqv + 1)(nqv + 3) 2^-23" in src
    assert "3.002 * std::ldexp(1.0, -16) + (9.2 * kpad + 20.0) * u + std::ldexp(1.0, -30)" in src
    assert "nqv * ep + (nqv + 1.0) * (nqv + 3.0) * std::ldexp(1.0, -23)" in src
    assert abs(B.margin(32, 128) - (32 * (3.002 * 2 ** -16 + (9.2 * 128 + 20) * 2 ** -24 + 2 ** -30) + 33 * 35 * 2 ** -23)) < 1e-18
    assert B.kpad(1) == 16 and B.kpad(17) == 32 and B.kpad(136) == 256 and B.kpad(256) == 256
    assert re.search(r"MVB_MAX_D = %d;" % B.MAX_D, src) and re.search(r"MVB_CHUNK_Q = %d;" % B.CHUNK_Q, src)
    assert re.search(r"MVB_CHUNK_COLS = %d;" % B.CHUNK_COLS, src)


# ---- host validation: every refusal is a ValueError before any device call ----------------------------------------------------
def _good():
    values, off, _ = M.column(np.array([2, 1, 3]), 8, 4, 5, "f32")
    return values, off, B.queries([4, 1, 3], 8, 9)


def _knn(match, values, off, qs, **kw):
    import lance_amd
    with pytest.raises(ValueError, match=match):
        lance_amd.multivector_flat_knn(values, off, qs, **{"k": 2, **kw})


def test_validation_of_a_batch():
    values, off, qs = _good()
    _knn("no query", values, off, [])
    _knn(r"\[nqv\]\[d\]", values, off, [qs[0], qs[1][0]])
    _knn(r"d = 8", values, off, [qs[0], qs[1][:, :7]])
    _knn("no vector", values, off, [qs[0], qs[1][:0]])
    _knn("above the limit", values, off, [qs[0], np.zeros((257, 8), f32)])
    _knn("decrease", values, np.array([0, 4, 3, 6]), qs)
    _knn("row 1 is empty", values, np.array([0, 2, 2, 6]), qs)
    _knn("k=", values, off, qs, k=1025)
    _knn("k=", values, off, qs, k=0)
    _knn("not supported", values, off, qs, metric="manhattan")
    _knn("prefilter", values, off, qs, prefilter=np.ones(4, bool))
    _knn("row_ids", values, off, qs, row_ids=np.arange(4, dtype=np.uint64))
    _knn("unsupported multivector element type int8", values.astype(np.int8), off, [q.astype(np.int8) for q in qs])


def test_validation_of_the_engine_call():
    """Engine.multivec_topk_batch checks (q, q_offsets) before it touches the device: called unbound, with no engine at all"""
    from lance_amd.engine import Engine
    values, off, qs = _good()
    q = np.concatenate(qs)
    qo = np.array([0, 4, 5, 8])

    def call(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            Engine.multivec_topk_batch(None, *a, **kw)
    call("starting at 0", values, off, q, qo + 1, 2)
    call("query 1 holds no vector", values, off, q, np.array([0, 4, 4, 8]), 2)
    call("above the limit", values, off, np.zeros((300, 8), f32), np.array([0, 300]), 2)
    call(r"q must be \[8\]\[d\]", values, off, q[:7], qo, 2)
    call(r"q must be \[64\]\[d\]", values, off, q.reshape(-1), np.array([0, 64]), 2)
    call("d = 8", values, off, q[:, :7], qo, 2)
    call("k=", values, off, q, qo, 2000)
    call("row_ids", values, off, q, qo, 2, row_ids=np.arange(5))
    call("end at len", values, off[:-1], q, qo, 2)
    call("1..65535", values, off, np.zeros((65536, 8), f32), np.arange(65537), 2)


def test_arrow_queries_give_the_batch_arguments():
    """an Arrow List<FixedSizeList> array of queries goes through arrow_io.multivector_from_arrow as a column does"""
    pa = pytest.importorskip("pyarrow")
    from lance_amd import arrow_io
    from lance_amd.engine import check_query_offsets
    _, _, qs = _good()
    flat = np.concatenate(qs)
    fsl = pa.FixedSizeListArray.from_arrays(pa.array(flat.reshape(-1)), 8)
    arr = pa.ListArray.from_arrays(pa.array(np.array([0, 4, 5, 8], np.int32)), fsl)
    q, qo = arrow_io.multivector_from_arrow(arr)
    assert (np.asarray(q) == flat).all() and check_query_offsets(qo).tolist() == [0, 4, 5, 8]


# ---- ABI ----------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_everywhere():
    from lance_amd import _lib
    name = "lance_hip_flat_multivec_topk_batch"
    hdr = open(os.path.join(ROOT, "include", "lance_hip.h")).read()
    rs = open(os.path.join(ROOT, "integration", "rust", "lance-linalg", "src", "hip.rs")).read()
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert name in _lib.SYMBOLS and re.search(r"\bint %s\(" % name, hdr) and ("pub fn %s(" % name) in rs and name in doc
    m = re.search(r"int %s\((.*?)\);" % name, hdr, re.S)
    assert len(m.group(1).split(",")) == 19       # ctx .. survivors, as _lib.py binds them
