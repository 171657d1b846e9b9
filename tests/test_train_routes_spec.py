"""The cases of tests/train_routes_spec.py, checked on the CPU: the oracle alone establishes what every case is named for -- the route its
shape takes, the layout, the convergence pattern, the empty clusters, the caps, the binding balance factor -- so that a case cannot
silently stop testing its edge.  tests/test_zz_gpu_train_routes.py holds the kernels to the oracle on the same cases, bit for bit."""
import numpy as np
import pytest

import sharded_kmeans_spec as S
import train_routes_spec as T

f32 = np.float32
PQ, KM = T.PQ_CASES, T.KM_CASES


def same_words(a, b):
    a, b = T.model_bits(a), T.model_bits(b)
    return a.dtype == b.dtype and a.shape == b.shape and bool((a == b).all())


def f64_bits(v):
    return int(np.float64(v).view(np.uint64))


# ---- routes ------------------------------------------------------------------------------------------------------------------------------
def test_every_case_takes_the_route_its_table_names():
    for c in PQ.values():
        assert T.pq_route(c) == c.route, c.name
        assert c.max_iters <= 12 or c.group == "mixed", c.name
    for c in KM.values():
        assert T.km_route(c) == c.route, c.name
    assert {c.route for c in PQ.values()} | {c.route for c in KM.values()} == set(T.ROUTES)
    # both layouts, each on more than one route; every 8-bit width of the issue's sweep
    by_layout = {lay: {c.route for c in PQ.values() if T.pq_layout(c.d, c.m) == lay} for lay in ("sliced", "row-major")}
    assert by_layout["sliced"] >= {"xf_pqtrain", "pq_mfma", "fixed", "wide"} and by_layout["row-major"] >= {"wide", "pq_mfma", "xf_assign", "mfma_wide"}
    assert {c.d // c.m for c in T.pq_group("width")} == {1, 2, 3, 6, 12, 20, 32, 64, 96, 128, 4, 8, 16}
    assert {c.d // c.m for c in T.pq_group("4bit")} == {3, 4, 12, 16, 32}
    assert sorted(c.max_iters for c in T.pq_group("budget")) == [1, 7, 8, 9]


def test_the_layout_gate():
    assert T.pq_layout(64, 8) == "sliced" and T.pq_layout(48, 4) == "sliced"
    assert T.pq_layout(64, 1) == "row-major" and T.pq_layout(48, 8) == "row-major" and T.pq_layout(16, 16) == "row-major"
    for c in PQ.values():       # row-major with a width off the 4-element grid: the operands are unaligned, only the wide kernel reads them
        if (c.d // c.m) % 4:
            assert T.pq_layout(c.d, c.m) == "row-major" and c.route == "wide", c.name


def test_the_gates_one_clause_at_a_time():
    r = T.expected_route
    assert r("float32", "l2", 8, 256, 2048, 16, False, True) == "xf_pqtrain"
    assert r("float32", "l2", 8, 256, 2048, 15, False, True) == "pq_mfma"               # 120 columns: no whole group
    assert r("float32", "l2", 8, 256, 2047, 16, False, True) == "fixed"
    assert r("float32", "l2", 8, 16, 3000, 16, False, True) == "fixed"                  # 4 bits
    assert r("float32", "l2", 8, 256, 3000, 16, True, True) == "fixed"                  # pq_mfma carries no bias
    assert r("float32", "dot", 8, 256, 3000, 16, False, True) == "fixed"
    assert r("float32", "l2", 12, 256, 3000, 4, False, True) == "wide"
    assert r("float32", "l2", 64, 48, 4096, 1, True, False) == "xf_assign"
    assert r("float32", "l2", 64, 31, 4096, 1, True, False) == "fixed"
    assert r("float32", "l2", 64, 48, 2047, 1, True, False) == "fixed"
    assert r("float32", "l2", 64, 256, 3000, 2, False, True) == "fixed"                 # batches > 1: no single-problem matrix-core route
    assert r("float16", "dot", 64, 48, 4096, 1, True, False) == "mfma"                  # the 32-lane order: xf_assign refuses it
    assert r("float16", "dot", 16, 48, 4096, 1, True, False) == "xf_assign"             # up to 16 elements both orders coincide
    assert r("float16", "dot", 64, 24, 4096, 1, True, False) == "wide"                  # ... and the fixed kernel has no 32-lane form
    assert r("float16", "l2", 64, 48, 4096, 1, True, False) == "xf_assign"
    assert r("float32", "l2", 256, 64, 3000, 1, True, False) == "mfma_wide"
    assert r("float32", "l2", 256, 63, 3000, 1, True, False) == "wide"
    assert r("float32", "l2", 144, 64, 3000, 1, True, False) == "mfma_wide"
    assert r("float32", "l2", 20, 40, 3000, 1, True, False) == "wide"


def test_the_launch_shapes_the_cases_are_named_for():
    """workgroups of 64 below the gate; a k-split of the fixed kernel at sd 64 / 96 / 128 and in k-means; a k-split of the wide kernel"""
    for c in T.pq_group("gate"):
        if c.n < 2048:
            assert T.fixed_launch(c.d // c.m, 256, c.n, c.m) == (64, 1), c.name       # one centroid tile at sd <= 32: nothing to split
    split = {c.d // c.m: T.fixed_launch(c.d // c.m, 256, c.n, c.m) for c in T.pq_group("width") if c.route == "fixed"}
    assert split[32] == (64, 1) and split[64] == (64, 2) and split[96][1] > 1 and split[128][1] > 1, split
    assert [T.wide_ksplit(256, 3000, c.m) for c in T.pq_group("width") if c.route == "wide"] == [1, 1, 1, 1, 2, 3]
    assert T.wide_ksplit(256, 3000, 1) == 4                                             # m1, d = 20
    km = {c.name: T.fixed_launch(c.d, c.k, c.n, 1) for c in KM.values() if c.route == "fixed"}
    assert km["float32:l2:n1500:d64:k48"] == (64, 1) and km["float32:l2:n1500:d64:k160"] == (64, 2) and km["float32:l2:n1500:d128:k100"] == (64, 2), km
    assert T.wide_ksplit(160, 1500, 1) == 3 and T.wide_ksplit(40, 3000, 1) == 1


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------
def _integer(x):
    xf = np.asarray(x, f32)
    return xf == np.rint(xf)


@pytest.mark.parametrize("name", list(PQ))
def test_pq_input_is_real_valued(name):
    """no PQ input is integer-valued except the split blocks (f32 sums of integers are exact in any order: such rows hide a wrong order).
    int8 rows are integers by type; they are eighths of the same blobs, spread over more than a hundred levels."""
    c = PQ[name]
    x = T.pq_input(name)
    sd = c.d // c.m
    assert x.shape == (c.n, c.d) and x.dtype == {"float32": f32, "float16": np.float16, "int8": np.int8}[c.kind]
    if c.kind == "int8":
        assert np.unique(x).size > 100 and (np.abs(x.astype(np.int32)) < 127).mean() > 0.99
        return
    whole = _integer(x)
    block = np.zeros(c.d, bool)
    if c.data.startswith("pairs"):
        which = c.data.split(":")[1]
        if which == "all":
            block[:] = True
        else:
            block[int(which) * sd:(int(which) + 1) * sd] = True
        assert whole[:, block].all()
        subs = x[:, block].reshape(c.n, -1, sd)
        for j in range(subs.shape[1]):
            assert np.unique(subs[:, j], axis=0).shape[0] == 36, (name, j)
    # a real-valued element lands on an integer once per integer's worth of spacings: 2^-7 between 8 and 16 in binary16, 2^-20 in f32
    assert block.all() or whole[:, ~block].mean() <= (0.01 if c.kind == "float16" else 1e-4), name


@pytest.mark.parametrize("name", list(KM))
def test_kmeans_input_is_real_valued_and_init_is_rows_of_x(name):
    c = KM[name]
    x, init = T.km_input(name)
    assert x.shape == (c.n, c.d) and init.shape == (c.k, c.d)
    if c.kind != "int8":
        assert _integer(x).mean() <= (0.01 if c.kind == "float16" else 1e-4)
    xs = np.asarray(x[:T.km_rows_used(c)], f32)
    rows = {r.tobytes() for r in xs}
    assert all(np.asarray(r, f32).tobytes() in rows for r in init), name
    assert np.unique(np.asarray(init, f32), axis=0).shape[0] == c.k - int(c.dup_init)


# ---- what the cases are named for --------------------------------------------------------------------------------------------------------
def test_mixed_convergence_inside_one_group(oracle):
    """some sub-quantiser of a 128-column group stops at iteration <= 8 (before the host's first read of the flags, kmeans.hip:400) and
    another of the SAME group later than 8: the workgroup column of that group runs on with part of its flags cleared"""
    c = PQ["mixed:d256:m16"]
    _, iters = T.pq_oracle(oracle, c.name)
    per_group = 128 // (c.d // c.m)
    groups = np.asarray(iters).reshape(-1, per_group)
    assert groups.shape == (2, 8)
    assert any((g <= 8).any() and (g > 8).any() for g in groups), iters
    assert iters.max() < c.max_iters        # every sub-quantiser converges by itself: none is cut off by the budget


def empties_per_iteration(oracle, name):
    """[m][T]: clusters without a row in the E-step of iteration t + 1, T = the iterations every sub-quantiser runs.  From the oracle alone:
    the codebook after t iterations (the initial rows for t = 0; splits applied) is the oracle's answer at max_iters = t, and the E-step of
    the next iteration is its assignment of the sub-quantiser's rows to that codebook."""
    c = PQ[name]
    sd, k = c.d // c.m, 1 << c.nbits
    x = T.pq_oracle_rows(name)
    _, iters = T.pq_oracle(oracle, name)
    steps = int(min(iters))
    out = np.zeros((c.m, steps), np.int64)
    for t in range(steps):
        if t:
            cb, it = oracle.pq_train(x, c.m, nbits=c.nbits, max_iters=t, sample_rate=c.sample_rate, seed=c.seed)
            assert (it == t).all()
        for j in range(c.m):
            sub = np.ascontiguousarray(x[:, j * sd:(j + 1) * sd])
            cent = cb[j] if t else sub[oracle.kmeans_init_indices(sub.shape[0], k, c.seed + j).astype(np.int64)]
            ids, _ = oracle.assign(sub, cent, "l2")
            out[j, t] = k - np.unique(ids[ids != oracle.NONE]).size
    return out


@pytest.mark.parametrize("name", [c.name for c in T.pq_group("split")])
def test_split_cases_lose_clusters_in_iteration_after_iteration(oracle, name):
    c = PQ[name]
    which = c.data.split(":")[1]
    ocb, oit = T.pq_oracle(oracle, name)
    empties = empties_per_iteration(oracle, name)
    assert empties.shape[1] >= 4
    for j in range(c.m):
        if which == "all" or int(which) == j:
            assert (empties[j] >= 256 - 36).all(), (name, j, empties[j])     # 36 distinct rows: at most 36 clusters hold one, in EVERY iteration
        else:
            assert not empties[j].any(), (name, j, empties[j])
    if which != "all":      # the neighbours are the blobs' own codebooks: the same columns without the block train to the same bits
        plain = oracle.pq_train(T.blobs(c.n, c.d, c.seed), c.m, nbits=c.nbits, max_iters=c.max_iters, seed=c.seed)[0]
        assert all(same_words(plain[j], ocb[j]) == (j != int(which)) for j in range(c.m))


def test_the_sample_cap_is_observable(oracle):
    c = PQ["cap:sample_rate"]
    assert T.pq_rows_used(c) == 1024 < c.n
    x = T.pq_input(c.name)
    prefix, pit = T.pq_oracle(oracle, c.name)
    capped, cit = oracle.pq_train(x, c.m, nbits=c.nbits, max_iters=c.max_iters, sample_rate=c.sample_rate, seed=c.seed)
    assert same_words(prefix, capped) and (pit == cit).all()                 # the reference caps by itself ...
    whole, _ = oracle.pq_train(x, c.m, nbits=c.nbits, max_iters=c.max_iters, seed=c.seed)
    assert all(not same_words(prefix[j], whole[j]) for j in range(c.m))      # ... and every sub-quantiser would differ without the cap
    assert all(T.pq_rows_used(o) == o.n for o in PQ.values() if o is not c)


def test_the_k512_cap_is_observable(oracle):
    import oracle_engine
    c = KM["cap:k512"]
    assert T.km_rows_used(c) == 2048 < c.n
    x, init = T.km_input(c.name)
    pc, pl, pit = T.km_oracle(oracle, c.name)
    wc, wl, _, _ = oracle.kmeans_train(x, c.k, max_iters=c.max_iters, tol=1e-4, balance_factor=f32(c.bf) / f32(c.n), init=init, seed=c.seed)
    assert not same_words(pc, wc) and f64_bits(pl) != f64_bits(wl)
    # the balance factor is divided by 3000, not by 2048: the other choice is a different run
    oc, ol, _, _ = oracle.kmeans_train(x[:2048], c.k, max_iters=c.max_iters, tol=1e-4, balance_factor=f32(c.bf) / f32(2048), init=init, seed=c.seed)
    assert f64_bits(ol) != f64_bits(pl)
    ec, el, eit = oracle_engine.OracleEngine().kmeans_train(x, c.k, max_iters=c.max_iters, balance_factor=c.bf, init=init, seed=c.seed)
    assert same_words(ec.numpy(), pc) and f64_bits(el) == f64_bits(pl) and eit == pit
    assert all(T.km_rows_used(o) == o.n for o in KM.values() if o is not c)


@pytest.mark.parametrize("name", [c.name for c in KM.values() if c.conditions])
def test_binding_bias_cases(oracle, name):
    """the adjusted balance factor binds in every iteration, the trainer splits at least once, and the bias decides assignments: the
    centroids differ from the run without a balance factor.  float16 and int8 cases are held to the last only (the numpy specification
    of the trainer models the f32 M-step)."""
    c = KM[name]
    assert c.bf == T.BF
    oc, ol, oit = T.km_oracle(oracle, name)
    assert np.isfinite(np.asarray(oc, f32)).all() and np.isfinite(ol)
    if "differs_from_bf0" in c.conditions:
        zc, _, _ = T.km_oracle(oracle, name, bf=0.0)
        assert not same_words(oc, zc)
    if "binds" in c.conditions or "splits" in c.conditions:
        assert c.kind == "float32"
        x, init = T.km_oracle_rows(name)
        sc, sl, sit, trace = S.train([x], c.k, c.n, c.max_iters, 1e-4, c.bf, init, c.seed, c.metric)
        assert same_words(sc, oc) and f64_bits(sl) == f64_bits(ol) and sit == oit          # the trace is the oracle's own run
        assert len(trace) == oit >= 4
        if "binds" in c.conditions:
            assert all(t["adjusted_binds"] for t in trace)
        if "splits" in c.conditions:
            assert sum(t["splits"] for t in trace) >= 1


def test_which_cases_carry_which_conditions():
    first = [c for c in KM.values() if c.kind == "float32" and c.name != "cap:k512"]
    assert len(first) == 10 and all(c.conditions == T.BINDS for c in first)
    assert {(c.n, c.d, c.k, c.metric) for c in first} >= {(4096, 64, 48, "l2"), (4096, 64, 48, "dot"), (4096, 128, 256, "l2"), (3000, 256, 64, "l2"),
                                                          (3000, 20, 40, "l2"), (4096, 32, 16, "l2"), (1500, 64, 48, "l2")}
    assert {(c.kind, c.metric, c.n, c.d, c.k) for c in KM.values() if c.kind != "float32"} >= {("float16", "dot", 6000, 32, 24), ("int8", "l2", 6000, 32, 24)}
