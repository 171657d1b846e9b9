"""The fixtures of tests/sharded_kmeans_spec.py, checked on the CPU: every property a case is named for is asserted from the
specification's trace (a case must not silently stop exercising it), the specification is compared with the single-process reference
trainer (oracle.kmeans_train), and the product's Python loop (lance_amd.dist.train_kmeans_sharded, host path) with the
specification, bit for bit.  tests/test_zz_gpu_sharded_kmeans.py holds the kernels to the same specification."""
import numpy as np
import pytest
import torch

import sharded_kmeans_spec as S
from sharded_kmeans_spec import same_bits

f32 = np.float32
CASES = S.cases()
EXACT = [n for n, c in CASES.items() if c["kind"] == "exact"]
ORDERED = [n for n, c in CASES.items() if c["kind"] == "ordered"]


def _equal(a, b):
    return same_bits(a[0], b[0]) and np.float64(a[1]).view(np.uint64) == np.float64(b[1]).view(np.uint64) and a[2] == b[2]


def test_the_case_list_is_the_one_the_gpu_tests_expect():
    assert len(EXACT) == 9 and len(ORDERED) == 4 and CASES["tie"]["kind"] == "tie"
    assert {(CASES[n]["metric"], CASES[n]["bf"]) for n in ORDERED} == {("l2", 0.0), ("l2", 1.0), ("dot", 0.0), ("dot", 1.0)}
    for c in CASES.values():
        n = c["x"].shape[0]
        assert n <= 3001 and c["x"].shape[1] <= 128 and n <= c["k"] * 512          # (the single-GPU trainer samples above k * 512 rows)
        cuts = c["layouts"]
        assert [len(cuts[l]) - 1 for l in S.LAYOUTS] == [1, 2, 3, 5]
        for l in S.LAYOUTS:
            assert cuts[l][0] == 0 and cuts[l][-1] == n and (np.diff(cuts[l]) >= 0).all()
        assert np.diff(cuts["w2"])[0] != np.diff(cuts["w2"])[1]                      # two uneven ranks
        assert sorted(np.diff(cuts["w5"]))[:2] == [0, 1]                             # a rank without rows, a rank with one


def test_partials_of_no_rows_are_zero():
    c = CASES["l2_bf0"]
    s, cnt, l, r = S.partials(c["x"][:0], c["init"], "l2", None)
    assert s.shape == (16, 32) and not s.any() and not cnt.any() and not l.any() and not r.any()
    assert l.dtype == np.float64 and s.dtype == cnt.dtype == r.dtype == f32


def test_partials_keep_row_order_and_skip_unassigned_rows():
    """against the plain per-row loop of the reference's M-step, on real-valued rows and on the NaN shard"""
    import oracle
    xb, cb = CASES["blobs_l2_bf0"]["x"][:700], CASES["blobs_l2_bf0"]["init"]
    xn, cn = S.nan_case()
    for x, cent, metric in ((xb, cb, "l2"), (xb, cb, "dot"), (xn, cn, "l2"), (xn, cn, "dot"), (xn, cn, "cosine")):
        ids, dists = S.estep(x, cent, metric)
        k, d = cent.shape
        sums = np.zeros((k, d), f32); counts = np.zeros(k, f32); losses = np.zeros(k, np.float64); radius = np.zeros(k, f32)
        with np.errstate(invalid="ignore", over="ignore"):
            for r in range(x.shape[0]):
                i = ids[r]
                if i == oracle.NONE:
                    continue
                sums[i] = sums[i] + x[r]; counts[i] += 1; losses[i] += np.float64(dists[r]); radius[i] = np.fmax(radius[i], dists[r])
        got = S.partials(x, cent, metric)
        for a, b in zip(got, (sums, counts, losses, radius)):
            assert same_bits(a, b), metric
    ids, _ = S.estep(xn, cn, "l2")
    assert ids[5] == oracle.NONE                                                     # the all-NaN row belongs to no cluster
    assert int(S.partials(xn, cn, "l2")[1].sum()) == int((ids != oracle.NONE).sum()) < xn.shape[0]


@pytest.mark.parametrize("name", EXACT)
def test_exact_case_is_layout_independent_and_equals_the_reference(name):
    c = CASES[name]
    x = c["x"]
    assert (x == np.rint(x)).all() and (c["init"] == np.rint(c["init"])).all()      # integer-valued
    ref = S.spec_result(name, "w1")
    for it in ref[3]:
        assert int(it["sizes"].max()) * float(np.abs(x).max()) < 2 ** 24             # every partial sum is exact
        assert it["tied"] == 1                                                       # no tie for largest: the reference's choice
    for lay in S.LAYOUTS[1:]:
        assert _equal(S.spec_result(name, lay), ref), lay
    assert _equal(ref, S.oracle_result(name))


@pytest.mark.parametrize("name", EXACT)
def test_exact_case_still_exercises_what_it_is_named_for(name):
    c, (_, _, iters, trace) = CASES[name], S.spec_result(name, "w1")
    p = c["props"]
    assert len(trace) == iters
    if p.get("converges_off_8"):
        assert iters % 8 != 0 and iters < c["max_iters"]
    if p.get("converges_9_29"):
        assert c["max_iters"] == 30 and 9 <= iters <= 29
    if p.get("runs_out"):
        assert c["max_iters"] == 30 and iters == 30
    if p.get("split_iterations"):
        assert sum(1 for it in trace if it["splits"] > 0) >= p["split_iterations"]
        assert all(it["splits"] == it["empties"] for it in trace)
    args = (S.shards_of(c, "w1"), c["k"], c["x"].shape[0], c["max_iters"], c["tol"], c["bf"], c["init"], c["seed"], c["metric"])
    if p.get("both_split_sides"):          # the case would notice a split that leaves out its (1 - 1/1024) side
        assert not _equal(S.train(*args, wrong="one_sided_split"), S.spec_result(name, "w1"))
    if p.get("bias_after_split"):          # ... and a bias taken from the sizes before the split
        assert c["bf"] != 0 and trace[0]["splits"] > 0 and len(trace) > 1
        assert not _equal(S.train(*args, wrong="presplit_bias"), S.spec_result(name, "w1"))
    if p.get("wide_group"):
        assert c["k"] > 256 and c["x"].shape[1] == 20 and c["x"].shape[0] >= c["k"] and not any(it["empties"] for it in trace)
    if p.get("never_binds"):
        assert c["bf"] >= 0 and not any(it["adjusted_binds"] for it in trace)
    if p.get("binds"):
        assert any(it["adjusted_binds"] for it in trace)
    if name == "k1":
        assert c["k"] == 1
    if c["metric"] == "dot":
        assert name == "dot_splits"
    assert all(np.isfinite(it["min_nonzero_dist"]) for it in trace)


def test_the_named_properties_are_all_present():
    props = set()
    for n in EXACT:
        props |= set(CASES[n]["props"])
    assert props >= {"converges_off_8", "converges_9_29", "runs_out", "split_iterations", "wide_group", "never_binds", "binds", "bias_after_split", "both_split_sides"}
    assert "k1" in EXACT and "l2_dup_init" in EXACT
    init = CASES["l2_dup_init"]["init"]
    assert (init[5] == init[3]).all() and (init[9] == init[3]).all()


@pytest.mark.parametrize("name", ORDERED)
def test_ordered_case_on_one_rank_equals_the_reference(name):
    """real-valued rows: the sums depend on the shard layout (each layout has its own defined value), one rank keeps the row order"""
    c = CASES[name]
    assert (c["x"] != np.rint(c["x"])).any()
    ref = S.spec_result(name, "w1")
    assert _equal(ref, S.oracle_result(name))
    assert all(it["tied"] == 1 for it in ref[3])
    for lay in S.LAYOUTS[1:]:
        got = S.spec_result(name, lay)
        assert np.isfinite(got[0]).all() and abs(got[1] - ref[1]) <= 1e-3 * abs(ref[1])      # (sanity only: the layouts may differ)


def test_tie_case_pins_the_known_divergence_from_the_reference():
    """PINS A KNOWN DIVERGENCE -- flip this test when it is fixed.  Two clusters tie for largest before the last iteration while
    `adjusted` is the binding term: the sharded trainer takes the first maximal cluster by id, the reference the one whose last
    member comes first in row order (the reduced buffers carry no last row).  The specification is the sharded trainer's contract,
    so it agrees with itself over the layouts and DIFFERS from oracle.kmeans_train."""
    ref = S.spec_result("tie", "w1")
    trace = ref[3]
    tied = [i for i, it in enumerate(trace[:-1]) if it["tied"] >= 2]
    assert tied and all(trace[i]["adjusted_binds"] for i in tied)
    for lay in S.LAYOUTS[1:]:
        assert _equal(S.spec_result("tie", lay), ref), lay
    oc, ol, oit = S.oracle_result("tie")
    assert not _equal(ref, (oc, ol, oit))
    assert (ref[2], oit) == (8, 7)


@pytest.mark.parametrize("name", list(CASES))
def test_dist_host_loop_equals_the_spec_on_one_rank(name):
    """lance_amd.dist.train_kmeans_sharded, host loop, no process group, on the oracle-backed stand-in engine"""
    from test_dist_gloo import OracleEngine
    from lance_amd.dist import train_kmeans_sharded
    c = CASES[name]
    cent, loss, iters = train_kmeans_sharded(OracleEngine(), torch.from_numpy(c["x"]), c["k"], c["x"].shape[0], max_iters=c["max_iters"], tol=c["tol"],
                                             balance_factor=c["bf"], init=c["init"], seed=c["seed"], metric=c["metric"])
    assert _equal((cent.numpy(), loss, iters), S.spec_result(name, "w1"))
