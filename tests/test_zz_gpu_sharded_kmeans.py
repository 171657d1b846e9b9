"""The row-sharded Lloyd trainer on the GPU, held to tests/sharded_kmeans_spec.py bit for bit (u32 views of f32, u64 views of f64;
no tolerance anywhere in this file):

  1. one shard's partials: lance_hip_kmeans_estep_partial, lance_hip_kmeans_shard_estep (f32) and _estep_x (f16 / int8), and
     lance_hip_kmeans_finalize;
  2. W ranks emulated on one engine: one shard_estep per shard into its own buffers, a rank-order fold with torch, shard_update on the
     folded buffers, shard_end every 8 iterations -- for every case and shard layout of the specification;
  3. the library's own loop (lance_amd/csrc/comm.cpp), without a communicator and through a callback communicator at world size 1,
     f32 / f16 / int8 shards;
  4. lance_amd.dist.train_kmeans_sharded on the real engine, device loop and host loop;
  5. the calls' refusals.

The contract (see the specification's header): per-shard partials are summed in row order and folded in rank order, so the result
is bit-identical to the single-GPU trainer and to the reference on one rank and, for any layout, wherever the sums are exact; the
one known divergence from the reference is the choice among clusters that tie for largest while `adjusted` binds (case "tie": the
kernels must equal the specification there, tests/test_sharded_kmeans_spec.py shows that the specification differs from the oracle).

A zero-row shard (n == 0, x == NULL) is a supported input: the wrappers pass None for it.  The E-step is skipped for it
(launch_assign is not called), stable_group sizes its grids from max(n, 1) rows (one block that reads no key, since every read is
guarded by r < n), and the statistics / accumulate / count kernels have grids of cdiv(k, 4), cdiv(k * d, 256) and cdiv(k, 256) blocks
whose member loops are empty (starts[c] == starts[c + 1]), so x is never dereferenced.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import sharded_kmeans_spec as S
from sharded_kmeans_spec import same_bits

pytestmark = pytest.mark.gpu
f32 = np.float32
CASES = S.cases()
NAMES = list(CASES)
EXACT = [n for n in NAMES if CASES[n]["kind"] == "exact"]


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


@pytest.fixture(scope="module")
def side(engine):
    """an engine bound to a torch side stream: its kernels and the torch ops issued while that stream is current are ordered"""
    from lance_amd.engine import Engine
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        e = Engine(use_torch_stream=True)
    yield e, stream
    torch.cuda.synchronize()
    e.close()


def _np(t):
    return t.detach().cpu().numpy()


def _result_equal(got, want):
    return same_bits(np.asarray(got[0], f32), want[0]) and np.float64(got[1]).view(np.uint64) == np.float64(want[1]).view(np.uint64) and got[2] == want[2]


def _bf_scaled(c):
    return float(f32(c["bf"]) / f32(c["x"].shape[0]))


# ---- 1. partials -----------------------------------------------------------------------------------------------------------------
def _check_partials(got_buf, got_losses, got_radius, want, k, d, what):
    buf = _np(got_buf)
    assert same_bits(buf[: k * d].reshape(k, d), want[0]), what
    assert same_bits(buf[k * d:], want[1]), what
    assert same_bits(_np(got_losses), want[2]), what
    assert same_bits(_np(got_radius), want[3]), what


def _shard_estep(e, x_dev, cent_dev, metric, bias_dev):
    """lance_hip_kmeans_shard_estep on a fresh (active) state -> (buf, losses, radius)"""
    k, d = cent_dev.shape
    st = e.kmeans_shard_begin(k, d, 1.0 if bias_dev is not None else 0.0, 0)
    if bias_dev is not None:
        st["bias"].copy_(bias_dev)
    for t in (st["buf"], st["losses"], st["radius"]):
        t.fill_(-3.0)                                       # (a kernel that does not write shows)
    e.kmeans_shard_estep(st, x_dev, cent_dev, metric)
    return st["buf"], st["losses"], st["radius"]


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
@pytest.mark.parametrize("d,k", [(2, 4), (20, 33), (32, 256), (20, 300), (128, 64)])
def test_partials_of_one_shard(eng, side, d, k, metric):
    """real-valued rows; shards of 0, 1, 63, 65 and 2049 rows; with and without a bias"""
    se, stream = side
    rng = np.random.default_rng(1000 * d + k)
    xall = (rng.standard_normal((2049, d)) * 3).astype(f32)
    cent = (rng.standard_normal((k, d)) * 3).astype(f32)
    bias = rng.uniform(0, 4, k).astype(f32)
    for n in (0, 1, 63, 65, 2049):
        x = xall[:n]
        for b in (None, bias):
            want = S.partials(x, cent, metric, b)
            assert int(want[1].sum()) == n
            got = eng.kmeans_estep_partial(x, cent, metric, b)
            _check_partials(*got, want, k, d, ("estep_partial", n, b is not None))
            with torch.cuda.stream(stream):
                xd, cd = torch.from_numpy(x).cuda(), torch.from_numpy(cent).cuda()
                bd = None if b is None else torch.from_numpy(b).cuda()
                got = _shard_estep(se, xd, cd, metric, bd)
                _check_partials(*got, want, k, d, ("shard_estep", n, b is not None))


@pytest.mark.parametrize("metric", ["l2", "dot", "cosine"])
def test_partials_with_nan_and_inf_rows(eng, side, metric):
    se, stream = side
    x, cent = S.nan_case()
    k, d = cent.shape
    want = S.partials(x, cent, metric, None)
    assert 0 < int(want[1].sum()) < x.shape[0]             # some row belongs to no cluster and is skipped
    _check_partials(*eng.kmeans_estep_partial(x, cent, metric, None), want, k, d, "estep_partial")
    with torch.cuda.stream(stream):
        got = _shard_estep(se, torch.from_numpy(x).cuda(), torch.from_numpy(cent).cuda(), metric, None)
        _check_partials(*got, want, k, d, "shard_estep")


@pytest.mark.parametrize("dtype", ["float16", "int8"])
def test_shard_estep_x_equals_the_f32_call_on_the_widened_rows(side, dtype):
    from lance_amd import _lib
    from lance_amd._lib import METRICS, check
    se, stream = side
    rng = np.random.default_rng(77)
    k, d = 33, 20
    if dtype == "int8":
        x = rng.integers(-127, 128, (2049, d)).astype(np.int8)
        code = _lib.I8
    else:
        x = (rng.standard_normal((2049, d)) * 3).astype(np.float16)
        code = _lib.F16
    wide = x.astype(f32)
    cent = wide[rng.permutation(2049)[:k]].copy() + f32(0.25)
    bias = rng.uniform(0, 4, k).astype(f32)
    for n in (0, 65, 2049):
        for metric in ("l2", "dot"):
            want = S.partials(wide[:n], cent, metric, bias)
            with torch.cuda.stream(stream):
                cd, bd = torch.from_numpy(cent).cuda(), torch.from_numpy(bias).cuda()
                ref = [t.clone() for t in _shard_estep(se, torch.from_numpy(wide[:n]).cuda(), cd, metric, bd)]
                xd = torch.from_numpy(x[:n]).cuda()
                st = se.kmeans_shard_begin(k, d, 1.0, 0)
                st["bias"].copy_(bd)
                check(se.lib.lance_hip_kmeans_shard_estep_x(se.h, code, METRICS[metric], C.c_void_p(xd.data_ptr()) if n else None, n, d,
                                                            C.c_void_p(cd.data_ptr()), k, C.c_void_p(st["bias"].data_ptr()),
                                                            C.c_void_p(st["state"].data_ptr()), C.c_void_p(st["buf"].data_ptr()),
                                                            C.c_void_p(st["losses"].data_ptr()), C.c_void_p(st["radius"].data_ptr())))
                for a, b in zip((st["buf"], st["losses"], st["radius"]), ref):
                    assert same_bits(_np(a), _np(b)), (dtype, n, metric)
                _check_partials(st["buf"], st["losses"], st["radius"], want, k, d, (dtype, n, metric))


def test_finalize_of_a_folded_buffer(eng):
    """sum * (1 / count) on the fold of three shards' partials; clusters without a member stay 0"""
    rng = np.random.default_rng(5)
    for d, k, n in ((20, 33, 40), (32, 256, 700), (20, 300, 2049), (2, 4, 65)):
        x = (rng.standard_normal((n, d)) * 3).astype(f32)
        cent = (rng.standard_normal((k, d)) * 3).astype(f32)
        cuts = [0, n // 3, n // 3, n]
        parts = [eng.kmeans_estep_partial(x[a:b], cent, "l2", None) for a, b in zip(cuts[:-1], cuts[1:])]
        buf = parts[0][0].clone()
        for p in parts[1:]:
            buf += p[0]
        s, cnt, _, _ = S.fold([S.partials(x[a:b], cent, "l2", None) for a, b in zip(cuts[:-1], cuts[1:])])
        assert same_bits(_np(buf), np.concatenate([s.ravel(), cnt]))
        want = S.finalize(s, cnt)
        got = _np(eng.kmeans_finalize(buf, k, d))
        assert same_bits(got, want)
        if (d, k) == (20, 33):
            assert (cnt == 0).any()
        assert not got[cnt == 0].any()


# ---- 2. W ranks emulated in one process ------------------------------------------------------------------------------------------------
class _Ranks:
    """the sharded loop of lance_amd/dist.py with the all-reduce replaced by a rank-order fold, everything on one stream"""

    def __init__(self, e, case, layout):
        c = self.c = case
        self.e = e
        self.n = c["x"].shape[0]
        self.k, self.d = c["init"].shape
        self.shards = [torch.from_numpy(np.ascontiguousarray(s)).cuda() for s in S.shards_of(c, layout)]
        self.cent = torch.from_numpy(c["init"]).cuda().clone()
        self.st = e.kmeans_shard_begin(self.k, self.d, _bf_scaled(c), c["seed"])
        self.per = [{key: torch.zeros_like(self.st[key]) for key in ("buf", "losses", "radius")} for _ in self.shards]

    def iteration(self, it):
        st = self.st
        for sh, p in zip(self.shards, self.per):
            self.e.kmeans_shard_estep(dict(st, **p), sh, self.cent, self.c["metric"])
        st["buf"].copy_(self.per[0]["buf"]); st["losses"].copy_(self.per[0]["losses"]); st["radius"].copy_(self.per[0]["radius"])
        for p in self.per[1:]:
            st["buf"] += p["buf"]
            st["losses"] += p["losses"]
            torch.fmax(st["radius"], p["radius"], out=st["radius"])
        self.e.kmeans_shard_update(st, self.cent, self.n, self.c["tol"], it)

    def run(self):
        loss, iters, mi = 0.0, 0, self.c["max_iters"]
        for it in range(1, mi + 1):
            self.iteration(it)
            if it % 8 == 0 or it == mi:
                loss, iters, active = self.e.kmeans_shard_end(self.st)
                if not active:
                    break
        return _np(self.cent), loss, iters

    def snapshot(self):
        return [_np(self.cent).copy(), _np(self.st["bias"]).copy()] + [_np(p[key]).copy() for p in self.per for key in ("buf", "losses", "radius")]


@pytest.fixture(scope="module")
def emulated(side):
    e, stream = side
    cache = {}

    def get(name, layout):
        if (name, layout) not in cache:
            with torch.cuda.stream(stream):
                cache[(name, layout)] = _Ranks(e, CASES[name], layout).run()
        return cache[(name, layout)]
    return get


@pytest.mark.parametrize("layout", S.LAYOUTS)
@pytest.mark.parametrize("name", NAMES)
def test_emulated_ranks_equal_the_spec(emulated, name, layout):
    got, want = emulated(name, layout), S.spec_result(name, layout)
    assert got[2] == want[2], (got[2], want[2])
    assert _result_equal(got, want)


@pytest.mark.parametrize("name", EXACT)
def test_exact_cases_equal_the_reference_the_single_gpu_trainer_and_every_layout(eng, emulated, name):
    c = CASES[name]
    ref = emulated(name, "w1")
    for layout in S.LAYOUTS[1:]:
        assert _result_equal(emulated(name, layout), ref), layout
    assert _result_equal(ref, S.oracle_result(name))
    cent, loss, iters = eng.kmeans_train(c["x"], c["k"], max_iters=c["max_iters"], tol=c["tol"], balance_factor=c["bf"], init=c["init"],
                                         seed=c["seed"], metric=c["metric"], hierarchical_k=1)
    assert _result_equal((_np(cent), loss, iters), ref)


@pytest.mark.parametrize("layout", S.LAYOUTS)
def test_iterations_enqueued_past_convergence_change_nothing(side, layout):
    """l2_bf0 converges at an iteration that is no multiple of 8: the host only learns of it at the next check, and what it enqueued
    in between must leave the centroids, the bias, the iteration count and every rank's buffers as they were"""
    e, stream = side
    name = "l2_bf0"
    want = S.spec_result(name, layout)
    conv = want[2]
    assert conv % 8 != 0 and conv < CASES[name]["max_iters"]
    with torch.cuda.stream(stream):
        r = _Ranks(e, CASES[name], layout)
        for it in range(1, conv + 1):
            r.iteration(it)
        before = r.snapshot()
        loss, iters, active = e.kmeans_shard_end(r.st)
        assert not active and iters == conv
        assert _result_equal((before[0], loss, iters), want)
        for it in range(conv + 1, (conv + 7) // 8 * 8 + 1):
            for sh, p in zip(r.shards, r.per):          # an E-step alone on the inactive state ...
                e.kmeans_shard_estep(dict(r.st, **p), sh, r.cent, "l2")
            for a, b in zip(r.snapshot(), before):
                assert same_bits(a, b), it
            r.iteration(it)                              # ... and the whole iteration
            for a, b in zip(r.snapshot(), before):
                assert same_bits(a, b), it
        loss2, iters2, active2 = e.kmeans_shard_end(r.st)
        assert (loss2, iters2, active2) == (loss, iters, False)


# ---- 3. the library loop (comm.cpp) ----------------------------------------------------------------------------------------------------
def _train_sharded(eng, comm, c, x=None):
    return eng.kmeans_train_sharded(comm, c["x"] if x is None else x, c["init"], c["x"].shape[0], max_iters=c["max_iters"], tol=c["tol"],
                                    balance_factor=c["bf"], seed=c["seed"], metric=c["metric"])


@pytest.mark.parametrize("name", NAMES)
def test_library_loop_equals_the_spec_on_one_rank(eng, name):
    c, want = CASES[name], S.spec_result(name, "w1")
    cent, loss, iters = _train_sharded(eng, None, c)
    assert _result_equal((_np(cent), loss, iters), want)
    calls = []
    comm = eng.comm_from_callback(lambda buf, count, dtype, op, stream: calls.append((count, dtype, op)) or 0, 1, 0)
    try:
        cent, loss, iters = _train_sharded(eng, comm, c)
    finally:
        eng.comm_destroy(comm)
    assert _result_equal((_np(cent), loss, iters), want)
    # a status word, then [sums | counts], losses and radii per ENQUEUED iteration (the host looks at the state every 8 iterations)
    enq = min(c["max_iters"], (iters + 7) // 8 * 8)
    assert len(calls) == 1 + 3 * enq, (len(calls), iters)
    k, d = c["init"].shape
    assert calls[0] == (1, 0, 1) and calls[1:4] == [(k * d + k, 0, 0), (k, 1, 0), (k, 0, 1)]


def _narrow_case(dtype):
    """dot_splits / l2_bf1 style problems on an int8 or float16 column; -> (case on the widened rows, the column)"""
    x = S.sift_like(3001, 32, 5)
    if dtype == "int8":
        col = np.clip(x - f32(100), -127, 127).astype(np.int8)
    else:
        col = (x / f32(4)).astype(np.float16)              # multiples of 1/4 below 64: exact in binary16
    wide = col.astype(f32)
    init = wide[np.random.default_rng(3).permutation(3001)[:16]].copy()
    return S._case("narrow_" + dtype, "exact", wide, init, 16, 1.0, 30, 5), col


@pytest.mark.parametrize("dtype", ["float16", "int8"])
def test_library_loop_on_f16_and_int8_shards(eng, dtype):
    c, col = _narrow_case(dtype)
    n = col.shape[0]
    want = S.train([c["x"]], c["k"], n, c["max_iters"], c["tol"], c["bf"], c["init"], c["seed"], c["metric"])
    assert all(it["tied"] == 1 for it in want[3]) and want[2] % 8 != 0
    cent, loss, iters = _train_sharded(eng, None, c, x=col)
    assert cent.dtype == torch.float32
    assert _result_equal((_np(cent), loss, iters), want)
    if dtype == "int8":                                    # an Int8 column has an f32 model on one GPU too
        c1, l1, i1 = eng.kmeans_train(col, c["k"], max_iters=c["max_iters"], tol=c["tol"], balance_factor=c["bf"], init=c["init"], seed=c["seed"])
        assert _result_equal((_np(c1), l1, i1), want)


# ---- 4. lance_amd.dist.train_kmeans_sharded on the real engine, no process group -----------------------------------------------------------
@pytest.mark.parametrize("loop", ["device", "host"])
@pytest.mark.parametrize("name", NAMES)
def test_dist_loops_equal_the_spec_on_one_rank(eng, name, loop):
    from lance_amd.dist import train_kmeans_sharded
    c, want = CASES[name], S.spec_result(name, "w1")
    x = torch.from_numpy(c["x"])
    cent, loss, iters = train_kmeans_sharded(eng, x.cuda() if loop == "device" else x, c["k"], x.shape[0], max_iters=c["max_iters"], tol=c["tol"],
                                             balance_factor=c["bf"], init=c["init"], seed=c["seed"], metric=c["metric"])
    torch.cuda.synchronize()
    assert _result_equal((_np(cent), loss, iters), want)
    if c["kind"] == "exact":
        assert _result_equal((_np(cent), loss, iters), S.oracle_result(name))


@pytest.mark.parametrize("loop", ["device", "host"])
@pytest.mark.parametrize("name", ["l2_bf1", "blobs_l2_bf1"])
def test_dist_loops_draw_their_own_initial_rows(eng, oracle, name, loop):
    """init=None: kmeans_init_indices(n, k, seed) of the rank's rows, as the reference's kmeans_random_init"""
    from lance_amd.dist import train_kmeans_sharded
    c = CASES[name]
    x, n, seed = c["x"], c["x"].shape[0], 11
    init = x[oracle.kmeans_init_indices(n, c["k"], seed).astype(np.int64)].copy()
    want = S.train([x], c["k"], n, 12, c["tol"], c["bf"], init, seed, c["metric"])
    xt = torch.from_numpy(x)
    cent, loss, iters = train_kmeans_sharded(eng, xt.cuda() if loop == "device" else xt, c["k"], n, max_iters=12, tol=c["tol"], balance_factor=c["bf"],
                                             init=None, seed=seed, metric=c["metric"])
    torch.cuda.synchronize()
    assert _result_equal((_np(cent), loss, iters), want)
    assert all(it["tied"] == 1 for it in want[3])
    oc, ol, oit, _ = oracle.kmeans_train(x, c["k"], max_iters=12, tol=c["tol"], balance_factor=f32(c["bf"]) / f32(n), init=None, seed=seed, metric=c["metric"])
    assert _result_equal((_np(cent), loss, iters), (oc, ol, oit))       # one rank: the row order is the single trainer's


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched(side):
    from lance_amd import _lib
    e, stream = side
    d = 4
    with torch.cuda.stream(stream):
        x = torch.ones((8, d), device="cuda")

        def outputs(k):
            return (torch.full((k * d + k,), 7.0, device="cuda"), torch.full((k,), 7.0, dtype=torch.float64, device="cuda"),
                    torch.full((k,), 7.0, device="cuda"))

        def p(t):
            return C.c_void_p(t.data_ptr())

        def untouched(ts):
            return all(bool((t == 7.0).all()) for t in ts)

        k = 4097
        cent = torch.zeros((k, d), device="cuda")
        buf, losses, radius = outputs(k)
        torch.cuda.synchronize()
        rc = e.lib.lance_hip_kmeans_estep_partial(e.h, _lib.F32, _lib.L2, p(x), 8, d, p(cent), k, None, p(buf), p(losses), p(radius), None)
        assert rc == _lib.EINVAL and untouched((buf, losses, radius))
        st = e.kmeans_shard_begin(k, d, 0.0, 0)
        rc = e.lib.lance_hip_kmeans_shard_estep(e.h, _lib.L2, p(x), 8, d, p(cent), k, None, p(st["state"]), p(buf), p(losses), p(radius))
        e.synchronize()
        assert rc == _lib.EINVAL and untouched((buf, losses, radius))
        k = 4
        cent = torch.zeros((k, d), device="cuda")
        buf, losses, radius = outputs(k)
        out = torch.full((k, d), 7.0, device="cuda")
        torch.cuda.synchronize()
        for code in (_lib.F16, _lib.I8, 9):
            rc = e.lib.lance_hip_kmeans_estep_partial(e.h, code, _lib.L2, p(x), 8, d, p(cent), k, None, p(buf), p(losses), p(radius), None)
            assert rc == _lib.EINVAL and untouched((buf, losses, radius)), code
            rc = e.lib.lance_hip_kmeans_finalize(e.h, code, p(buf), k, d, p(out))
            assert rc == _lib.EINVAL and untouched((out,)), code
