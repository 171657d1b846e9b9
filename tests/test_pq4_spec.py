"""The numpy model of the 4-bit IVF_PQ distance computation (tests/pq4_spec.py) against the oracle, its mutants, and the regimes the
fixtures are meant to reach.  CPU only; tests/test_zz_gpu_pq4.py runs the same cases on the GPU against the oracle."""
import functools

import numpy as np
import pytest

import pq4_spec as S

f32 = np.float32


def same(a, b):
    ai, ad = a
    bi, bd = b
    return bool((ai == bi).all() and (np.ascontiguousarray(ad, f32).view(np.uint32) == np.ascontiguousarray(bd, f32).view(np.uint32)).all())


@functools.lru_cache(maxsize=None)
def run(name, mut=None, want_info=False):
    """(the model's answer, the oracle's answer, info, (lower, upper)) of a case; bounds come from the oracle's search without a range"""
    c = S.CASE[name]
    fx, q, nprobes, allow = S.case_inputs(c)
    oidx = fx.ix.oracle()
    raw = fx.x if c.refine else None
    raw32 = None if raw is None else raw.astype(f32)
    with np.errstate(all="ignore"):
        lo = hi = None
        if c.bounds is not None:
            _, ud = oidx.search(q, c.k, nprobes, refine=c.refine, raw=raw32, prefilter=allow)
            lo, hi = S.resolve_bounds(c, ud)
        info = {} if want_info else None
        got = S.search(fx.ix, q, c.k, nprobes, refine=c.refine, raw=raw, prefilter=allow, lower=lo, upper=hi, mut=mut, info=info)
        want = oidx.search(q, c.k, nprobes, refine=c.refine, raw=raw32, prefilter=allow, lower=lo, upper=hi)
    return got, want, info, (lo, hi)


@pytest.mark.parametrize("name", [c.name for c in S.CASES])
def test_model_equals_oracle_search(oracle, name):
    got, want, _, _ = run(name)
    assert (got[0] == want[0]).all(), name
    assert same(got, want), name


@pytest.mark.parametrize("index", sorted(S.INDICES))
def test_model_equals_oracle_scan(oracle, index):
    """scan4 == oracle.pq_scan4 on every partition of every index, at every k_hint of the grid, row by row"""
    fx = S.index_fixture(index)
    ix = fx.ix
    scan_metric = "l2" if ix.metric == "cosine" else ix.metric
    q = S.queries(fx, 2, seed=5)
    qn = oracle.normalize(q) if ix.metric == "cosine" else q
    for p in range(ix.cent.shape[0]):
        codes_t, rids = ix.partition(p)
        if rids.size == 0:
            continue
        with np.errstate(all="ignore"):
            qr = qn[p % 2].astype(f32) - ix.cent[p].astype(f32) if scan_metric == "l2" else qn[p % 2].astype(f32)
            lut = oracle.build_lut(qr, ix.cb.astype(f32), scan_metric, nbits=4)
            for kh in S.KEFFS:
                want = oracle.pq_scan4(lut, codes_t, kh, scan_metric)
                got = S.scan4(lut, codes_t, kh, scan_metric).d
                assert (got.view(np.uint32) == want.view(np.uint32)).all(), (index, p, rids.size, kh)


@pytest.mark.parametrize("mut", S.MUTANTS)
def test_every_mutant_is_caught_by_its_case(oracle, mut):
    assert set(S.CAUGHT_BY) == set(S.MUTANTS)
    name = S.CAUGHT_BY[mut]
    got, want, _, _ = run(name, mut)
    assert not same(got, want), f"the mutant {mut} answers the case {name!r} like the reference"
    assert same(run(name)[0], want)


def _scans(name):
    return [s for _, _, s in run(name, None, True)[2]["scans"]]


@pytest.mark.parametrize("name", [c.name for c in S.CASES if c.regime])
def test_cases_reach_their_regime(oracle, name):
    c = S.CASE[name]
    got, want, info, (lo, hi) = run(name, None, True)
    assert same(got, want)
    ids, d = want
    found = ids != S.NOID
    for r in c.regime:
        if r == "flat_num>200":
            assert any(s.flat_num > 200 and s.flat_num < len(s.d) for s in _scans(name)) or c.frac is not None, r
            if c.frac is not None:      # under a prefilter the k_hint is ignored: the same case at k_hint = k * refine above 200
                assert c.k * max(c.refine, 1) > 200
        elif r == "tail_at_flat_num":
            assert any(len(s.d) - len(s.d) % 16 < s.flat_num < len(s.d) and s.tail_start == s.flat_num for s in _scans(name)), r
        elif r == "qmax<qmin":
            assert all(s.qmax < s.qmin for s in _scans(name) if len(s.d) > 216), r
            assert all((s.acc[slice(*s.quantised)] == 0).all() for s in _scans(name)), r
        elif r == "qmax==qmin":
            assert any(s.qmax == s.qmin and s.quantised[1] > s.quantised[0] for s in _scans(name)), r
        elif r == "qmax_nan":
            assert any(np.isnan(s.qmax) for s in _scans(name)), r
        elif r == "both_signs":
            fx, q, _, _ = S.case_inputs(c)
            lut = oracle.build_lut(q[0].astype(f32), fx.ix.cb.astype(f32), "dot", nbits=4)
            assert (lut < 0).any() and (lut > 0).any(), r
            assert all(s.qmax > s.qmin for s in _scans(name) if s.quantised[1] > s.quantised[0]), r
        elif r == "halves":
            assert sum(s.qmin == 0 and s.qmax == 510 and s.quantised[1] > s.quantised[0] for s in _scans(name)) >= 3, r
        elif r == "many_levels":
            s = max(_scans(name), key=lambda s: len(s.d))
            a, b = s.quantised
            assert len(np.unique(s.acc[a:b])) >= 32 and (s.acc[a:b] < 255).mean() > 0.9, (r, len(np.unique(s.acc[a:b])))
        elif r == "saturated>=32":
            n = sum(len(set(int(i) for i in ids[qi][found[qi]]) & info["saturated"][qi]) for qi in range(ids.shape[0]))
            assert n >= 32, (r, n)
        elif r == "on_lower":
            assert lo is not None and (d[found] == lo).any(), r
        elif r == "on_upper":
            assert hi is not None and not (d[found] >= hi).any(), r
            un = run_unranged(name)
            assert (un == hi).any(), r
        elif r == "fewer_than_k":
            assert (~found).any() and np.isinf(d[~found]).all(), r
        elif r == "negative_range":
            assert lo < 0 and hi < 0, (r, lo, hi)
        else:
            raise KeyError(r)


@functools.lru_cache(maxsize=None)
def run_unranged(name):
    c = S.CASE[name]
    fx, q, nprobes, allow = S.case_inputs(c)
    raw32 = fx.x.astype(f32) if c.refine else None
    with np.errstate(all="ignore"):
        return fx.ix.oracle().search(q, c.k, nprobes, refine=c.refine, raw=raw32, prefilter=allow)[1]


def test_fixture_grid_is_what_the_issue_lists():
    assert {1, 15, 16, 17, 199, 200, 201, 208, 215, 216, 217, 255, 256, 257, 1008, 0} <= set(S.GRID_SIZES) and 1005 % 16 == 13
    assert {1, 10, 128, 129, 200, 201, 250, 300, 1000} <= set(S.KEFFS) and max(S.KEFFS) > max(S.GRID_SIZES)
    shapes = {(m, d // m) for _, d, m, *_ in S.INDICES.values()}
    assert {m for m, _ in shapes} == {2, 8, 16, 32} and {sd for _, sd in shapes} == {2, 4, 8, 16}
    for name in S.INDICES:
        fx = S.index_fixture(name)
        assert tuple(np.bincount(fx.ix.part, minlength=len(fx.sizes))) == tuple(fx.sizes) and fx.x.shape[0] <= 4300
