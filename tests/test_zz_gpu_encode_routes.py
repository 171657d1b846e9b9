"""GPU parity of the IVF-PQ transform on the routes behind the single-pass kernel (tests/encode_routes_spec.py; its table is checked on the
CPU by tests/test_encode_routes_spec.py): the matrix-core encoder (pq_mfma.hip: pq_mfma_estep_kernel<SD, ENC> + pq_mfma_fix_kernel), the
lane-per-row encoder (encode_fused.hip) and the staged chain (launch_assign, residual_kernel, pq_encode_launch, pack_nibbles_kernel),
against the oracle's chain bit for bit: partition ids including NONE, the codes of every row with a partition, the f64 loss with ==.

Every case asserts the route by the stage counters: pq_mfma_encode / lane_encode name the two encoders that share encode_fused.  One
test covers a route and an element type and loops over its shapes; every mismatch of the loop is collected and reported together with
its case tag, the first ten rows and got / want there.  pytest -s prints every case's counters.  Sorted last: newest device code last.

Wall time on an MI355X: 10 tests (117 transform cases, 12 pq_encode cases) in 3.1 s, 1.6 s of it the engine's start-up; the oracle's
share is under 2 s for the whole table."""
import numpy as np
import pytest

import encode_routes_spec as S

pytestmark = pytest.mark.gpu
ROUTE_STAGES = ("pq_mfma_encode", "lane_encode", "encode_fused", "xform_fused", "xform_tail")
STAGES = ROUTE_STAGES + ("pq_mfma_estep", "ma_sweep", "xf_assign", "ma_recheck", "ma_wide_f16", "assign")
WANT = {"P": {"pq_mfma_encode": 1, "encode_fused": 1, "lane_encode": 0, "xform_fused": 0, "xform_tail": 0},
        "L": {"pq_mfma_encode": 0, "encode_fused": 1, "lane_encode": 1, "xform_fused": 0, "xform_tail": 0},
        "S": {"pq_mfma_encode": 0, "encode_fused": 0, "lane_encode": 0, "xform_fused": 0, "xform_tail": 0}}


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


@pytest.fixture(scope="module")
def eng():
    import lance_amd
    return lance_amd.default_engine()


def counted(eng, fn):
    before = {s: eng.timing_query("count:" + s)[1] for s in STAGES}
    out = fn()
    eng.synchronize()
    return out, {s: int(eng.timing_query("count:" + s)[1] - b) for s, b in before.items()}


class Failures(list):
    """collects every failing case of a loop, so that one run names all broken routes"""

    def rows(self, tag, what, got, want, rows_ok=None):
        got, want = np.asarray(got), np.asarray(want)
        diff = (got != want).reshape(len(want), -1).any(axis=1)
        if rows_ok is not None:
            diff &= rows_ok
        bad = np.nonzero(diff)[0][:10]
        if bad.size:
            self.append((tag, what, "rows", bad.tolist(), "got", got[bad].tolist(), "want", want[bad].tolist()))

    def value(self, tag, what, got, want):
        if got != want:
            self.append((tag, what, "got", got, "want", want))

    def done(self):
        assert not self, f"{len(self)} mismatches: " + "\n".join(repr(f) for f in self[:24])


@pytest.mark.parametrize("kind", ["float32", "float16", "int8"])
@pytest.mark.parametrize("route", ["P", "L", "S"])
def test_ivfpq_encode_route(eng, oracle, route, kind):
    cases = S.cases_of(route, kind)
    if not cases:
        assert (route, kind) == ("S", "int8")      # the staged route's cases are f32 / f16
        return
    fails = Failures()
    for c in cases:
        t = S.tag(c)
        p = S.prepared(oracle, c)
        (part, codes, loss), ran = counted(eng, lambda: eng.ivfpq_encode(p.x, p.cent, p.cb, c.metric))
        print(f"[encode routes] {t}: {ran}")
        part = _np(part).view(np.uint32); codes = _np(codes)
        fails.rows(t, "partition ids", part, p.part)
        fails.rows(t, "codes", codes, p.codes, rows_ok=p.part != S.NONE)
        fails.value(t, "loss", loss, p.loss)
        for stage, want in WANT[route].items():
            fails.value(t, "count:" + stage, ran[stage], want)
        if route == "S" and c.metric == "cosine" and c.n >= 2048:       # the PQ step is pq_mfma in training mode, writing codes
            fails.value(t, "count:pq_mfma_estep >= 1", ran["pq_mfma_estep"] >= 1, True)
        if route == "P" and kind == "float16" and c.metric == "dot":     # ma_top3_kernel<.., __half>, 32-lane exact re-check
            fails.value(t, "count:ma_sweep >= 1", ran["ma_sweep"] >= 1, True)
            fails.value(t, "count:xf_assign", ran["xf_assign"], 0)
        if c.nlist < 32:
            fails.value(t, "count:ma_sweep", ran["ma_sweep"], 0)
            fails.value(t, "count:xf_assign", ran["xf_assign"], 0)
    fails.done()


def test_pq_encode_alone(eng, oracle):
    """lance_hip_pq_encode, as rebalance.hip calls it on the rows of a split partition: sub-dimension 8 (pq_mfma at 2100 rows, the exact
    kernels at 300), 64 (two blockIdx.z tiles and argmin_merge_kernel) and 12 (wide.hip), integer rows with ties between distinct
    codewords and the spread duplicates"""
    fails = Failures()
    for c in S.PQ_CASES:
        p = S.pq_prepared(oracle, c)
        codes, ran = counted(eng, lambda: eng.pq_encode(p.x, p.cb, c.metric))
        print(f"[encode routes] pq_encode {tuple(c)}: {ran}")
        fails.rows("pq_encode " + repr(tuple(c)), "codes", _np(codes), p.codes)
        for stage in ROUTE_STAGES:
            fails.value("pq_encode " + repr(tuple(c)), "count:" + stage, ran[stage], 0)
    fails.done()
