"""The case table of encode_routes_spec.py, checked against the CPU oracle alone: every case lands on the route it is listed under, and
really holds the edges it is there for (a row without a partition, bit-equal smallest distances on both the centroid and the
codeword side, binary16 residuals that overflow or round to another code).  Run with -s for the per-case counts."""
import collections

import numpy as np
import pytest

import encode_routes_spec as S

ROUTES = ("P", "L", "S")
KINDS = ("float32", "float16", "int8")


def test_route_coverage():
    count = collections.Counter()
    for c in S.CASES:
        got = S.expected_route(c.kind, c.metric, c.d, c.m, c.nbits, c.n, c.nlist)
        assert got == c.route, (S.tag(c), "is served by", got)
        assert got not in ("X", "T")
        count[got] += 1
    print("cases per route:", dict(count))
    assert count["P"] >= 12 and count["L"] >= 20 and count["S"] >= 12
    assert len({S.tag(c) for c in S.CASES}) == len(S.CASES)


def test_routes_the_table_must_not_reach():
    """the gates on shapes other files own: the transcription says X / T there"""
    assert S.expected_route("float32", "l2", 128, 16, 8, 2048, 32) == "X"
    assert S.expected_route("float16", "dot", 16, 4, 8, 2400, 40) == "X"          # d = 16: lanes32 does not apply
    assert S.expected_route("float32", "cosine", 64, 8, 8, 2100, 32) == "X"
    assert S.expected_route("float32", "dot", 192, 12, 8, 2100, 40) == "T"
    assert S.expected_route("float16", "l2", 256, 16, 8, 2300, 48) == "T"         # the coarse assign widens the rows: an f32 view exists
    assert S.expected_route("float32", "l2", 256, 64, 8, 2300, 64) == "T"
    assert S.expected_route("float32", "l2", 192, 48, 8, 2300, 64) == "P"         # last block under 128 columns at sub-dimension 4


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("route", ROUTES)
def test_the_table_holds_the_edges(oracle, route, kind):
    cases = S.cases_of(route, kind)
    if not cases:
        assert (route, kind) == ("S", "int8")      # the staged route's cases are f32 / f16
        return
    for c in cases:
        p = S.prepared(oracle, c)
        s = p.stats
        print(S.tag(c), s)
        t = S.tag(c)
        if c.kind != "int8" and c.n > 1:
            assert s["no_partition"] >= 1, t
        assert s["codeword_ties"] >= 1, t
        if c.nlist > 1:
            assert s["centroid_ties"] >= 1, t
        if "integer" in c.extras:
            assert s["codeword_ties"] >= 20 and s["codeword_ties_distinct"] >= 1, t
        if "overflow" in c.extras:
            assert s["overflow_rows"] == 3, t
            assert s["overflow_changed"] >= 1, t
        if c.kind == "float16" and c.metric == "l2" and c.n > 1:      # (n = 1: the row's own sub-vectors are codewords)
            assert s["rounding_changes"] >= 1, t
        assert p.part.shape == (c.n,) and p.codes.shape == (c.n, c.m if c.nbits == 8 else c.m // 2)
        assert np.isfinite(p.loss)


def test_pq_encode_cases_hold_ties(oracle):
    for c in S.PQ_CASES:
        p = S.pq_prepared(oracle, c)
        print("pq_encode", tuple(c), p.stats)
        assert p.stats["codeword_ties"] >= 20 and p.stats["codeword_ties_distinct"] >= 1, tuple(c)


class _Operand:
    """an operand on the 16-byte grid, as far as the gates of test_zz_gpu_unaligned.py look"""

    def __init__(self, es):
        self.es = es

    def data_ptr(self):
        return 4096

    def element_size(self):
        return self.es


@pytest.mark.parametrize("kind", KINDS)
def test_transcription_agrees_with_the_alignment_tests_gates(kind):
    """two independent transcriptions of the same gates: this file's expected_route and the predicates of test_zz_gpu_unaligned.py
    (its four shapes, L2, nlist = 32, aligned operands)"""
    import test_zz_gpu_unaligned as U
    es = {"float32": 4, "float16": 2, "int8": 1}[kind]
    op = {"x": _Operand(es), "cent": _Operand(4), "cb": _Operand(4), "codes": _Operand(1)}
    for d, m, n in ((128, 16, 2048), (64, 16, 2048), (64, 8, 300), (128, 16, 300)):
        if n >= 2048:       # test_ivfpq_encode: xform_fused == xform_ok, else encode_fused == pq_mfma_ok or lane_encode_ok
            want = "X" if U.xform_ok(op, m) else ("P" if U.pq_mfma_ok(op) else ("L" if U.lane_encode_ok(op, m) else "S"))
        else:
            want = "L" if U.lane_encode_ok(op, m) else "S"
        assert S.expected_route(kind, "l2", d, m, 8, n, 32) == want, (kind, d, m, n)
