"""PQ codebook training and k-means training on every route the E-step can take (tests/train_routes_spec.py; the cases themselves are
checked on the CPU by tests/test_train_routes_spec.py).  Every case is compared with the CPU oracle bit for bit: the codebook / the
centroids as unsigned words (u32, u16 for binary16 models), every entry of `iters`, and for k-means the f64 loss.  There is no
tolerance.  Every failing case of a sweep is collected before the test asserts.

The route is asserted from the stage counters (timing_query("count:<stage>")):

  xf_pqtrain  `xf_pqtrain` and `pq_mfma_estep` rise (launch_pq_mfma opens its stage before it hands over, pq_mfma.hip:306-310)
  pq_mfma     `pq_mfma_estep` rises, `xf_pqtrain` does not
  xf_assign   `xf_assign` and `ma_sweep` rise
  mfma        `ma_sweep` rises, `xf_assign` does not
  mfma_wide   the K-tiled sweep (ma_launch_wide) has no stage of its own: none of the four rises while `assign` does, as below
  fixed/wide  none of the four rises while `assign` does; no counter tells the fixed kernel from the wide one

and a counter that rises does so once per enqueued iteration (= `assign`), at least max(iters) times: no iteration of the call took
another route.  Each case prints its counters (pytest -s shows them)."""
import numpy as np
import pytest

import train_routes_spec as T

pytestmark = pytest.mark.gpu
f32 = np.float32
ROUTE_STAGES = ("xf_pqtrain", "pq_mfma_estep", "xf_assign", "ma_sweep")
RISES = {"xf_pqtrain": {"xf_pqtrain", "pq_mfma_estep"}, "pq_mfma": {"pq_mfma_estep"}, "xf_assign": {"xf_assign", "ma_sweep"}, "mfma": {"ma_sweep"},
         "mfma_wide": set(), "fixed": set(), "wide": set()}


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def _np(t):
    return t.detach().cpu().numpy() if hasattr(t, "detach") else np.asarray(t)


class Stages:
    """the stage counters a call raised (counters = False: the stand-in engine of the dry run has none)"""

    def __init__(self, eng, counters=True):
        self.eng, self.on, self.rose = eng, counters, {}

    def _read(self):
        return {s: int(self.eng.timing_query("count:" + s)[1]) for s in ROUTE_STAGES + ("assign",)}

    def __enter__(self):
        if self.on:
            self.before = self._read()
        return self

    def __exit__(self, *a):
        if self.on and a[0] is None:
            self.eng.synchronize()
            self.rose = {s: v - self.before[s] for s, v in self._read().items()}


class Failures(list):
    """collects every failing case of a sweep, so that one run names all of them"""

    def words(self, tag, what, got, want):
        got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
        if got.dtype != want.dtype or got.shape != want.shape:
            self.append((tag, what, "dtype / shape", str(got.dtype), got.shape, str(want.dtype), want.shape))
            return
        g, w = T.model_bits(got).reshape(got.shape[0], -1), T.model_bits(want).reshape(want.shape[0], -1)
        bad = np.nonzero((g != w).any(axis=1))[0]
        if bad.size:
            self.append((tag, what, f"{bad.size} of {g.shape[0]} blocks differ, first", int(bad[0])))

    def equal(self, tag, what, got, want):
        if got != want:
            self.append((tag, what, got, want))

    def route(self, tag, route, rose, iters):
        ran = rose["assign"]
        want = {s: (ran if s in RISES[route] else 0) for s in ROUTE_STAGES}
        if ran < int(max(iters)) or {s: rose[s] for s in ROUTE_STAGES} != want:
            self.append((tag, f"route {route}", rose))

    def done(self):
        assert not self, f"{len(self)} findings differ from the oracle: {self[:12]}"


def pq_body(eng, oracle, cases, counters=True):
    fails = Failures()
    for c in cases:
        x = T.pq_input(c.name)
        ocb, oit = T.pq_oracle(oracle, c.name)
        with Stages(eng, counters) as st:
            cb, iters = eng.pq_train(x, c.m, nbits=c.nbits, max_iters=c.max_iters, sample_rate=c.sample_rate, seed=c.seed)
        iters = [int(v) for v in _np(iters)]
        print(f"[train routes] pq {c.name} {c.route} {T.pq_layout(c.d, c.m)} iters {iters}: {st.rose}")
        cb = _np(cb)
        fails.words(c.name, "codebook", cb.reshape(c.m, -1), ocb.reshape(c.m, -1))       # (a block = a sub-quantiser)
        fails.equal(c.name, "iters", iters, [int(v) for v in oit])
        if counters:
            fails.route(c.name, c.route, st.rose, iters)
    fails.done()


def km_body(eng, oracle, cases, counters=True):
    fails = Failures()
    for c in cases:
        x, init = T.km_input(c.name)
        oc, ol, oit = T.km_oracle(oracle, c.name)
        with Stages(eng, counters) as st:
            cent, loss, iters = eng.kmeans_train(x, c.k, max_iters=c.max_iters, tol=1e-4, balance_factor=c.bf, init=init, seed=c.seed, metric=c.metric)
        print(f"[train routes] kmeans {c.name} {c.route} iters {iters} loss {loss!r}: {st.rose}")
        fails.words(c.name, "centroids", _np(cent), oc)                                    # (a block = a centroid)
        fails.equal(c.name, "iters", int(iters), int(oit))
        fails.equal(c.name, "loss bits", int(np.float64(loss).view(np.uint64)), int(np.float64(ol).view(np.uint64)))
        if counters:
            fails.route(c.name, c.route, st.rose, [iters])
    fails.done()


@pytest.mark.parametrize("route", ["wide", "fixed", "pq_mfma", "xf_pqtrain"])
def test_pq_train_width_sweep(eng, oracle, route):
    """8 bits, f32, n = 3000: sd 1, 2, 3, 6 (row-major, off the 16-byte grid but for sd 1 x 16), 12, 20 on the batched wide kernel; sd 32,
    64, 96, 128 on the batched fixed kernel (k-split from sd 64 on); sd 4, 8, 16 on pq_mfma and, where batches * sd fills whole
    128-column groups, on xf_pqtrain (d = 256: two groups)"""
    cases = [c for c in T.pq_group("width") if c.route == route]
    assert len(cases) == {"wide": 6, "fixed": 4, "pq_mfma": 3, "xf_pqtrain": 3}[route]
    pq_body(eng, oracle, cases)


def test_pq_train_below_and_at_the_matrix_core_gate(eng, oracle):
    """sd 4, 8, 16 at n = 600 and 2047 (the fixed kernel, workgroups of 64) and at n = 2048, the first n pq_mfma takes"""
    pq_body(eng, oracle, T.pq_group("gate"))


def test_pq_train_4_bits(eng, oracle):
    pq_body(eng, oracle, T.pq_group("4bit"))


def test_pq_train_one_sub_quantiser(eng, oracle):
    """m = 1: the row-major matrix with batches = 1, so the single-problem routes serve a codebook: pq_mfma (d = 16), xf_assign (64),
    wide (20), the K-tiled sweep (256)"""
    pq_body(eng, oracle, T.pq_group("m1"))


def test_pq_train_f16_and_int8_rows(eng, oracle):
    """float16 residuals: f16 M-step, the codebook compared as 16-bit words; int8 rows: f32 model"""
    pq_body(eng, oracle, T.pq_group("types"))


def test_pq_train_mixed_convergence_inside_a_group(eng, oracle):
    pq_body(eng, oracle, T.pq_group("mixed"))


def test_pq_train_empty_clusters_every_iteration(eng, oracle):
    """36 distinct sub-vectors against 256 codewords: split_clusters runs in every iteration, in every sub-quantiser and in exactly one"""
    pq_body(eng, oracle, T.pq_group("split"))


def test_pq_train_sample_cap_and_iteration_budget(eng, oracle):
    """sample_rate 64 at 4 bits: the answer is the oracle's on the first 1024 rows; max_iters 1, 7, 8, 9 around the block of 8"""
    pq_body(eng, oracle, T.pq_group("cap") + T.pq_group("budget"))


def test_kmeans_train_with_a_binding_balance_factor(eng, oracle):
    """balance_factor 1e6 on real-valued rows: the bias decides assignments on xf_assign, the K-tiled sweep, the wide and the fixed kernel
    (with and without a k-split), the 32-lane order (wide two-pass and ma_top3_kernel) and int8 rows"""
    km_body(eng, oracle, [c for c in T.KM_CASES.values() if c.bf == T.BF])


def test_kmeans_train_k512_cap(eng, oracle):
    """k = 4, n = 3000: the first 2048 rows are used; the answer is the oracle's on that prefix with the balance factor over 3000"""
    km_body(eng, oracle, [T.KM_CASES["cap:k512"]])
