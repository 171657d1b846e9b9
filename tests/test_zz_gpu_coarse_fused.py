"""find_partitions below the per-group route's first list count: sweep and select in one kernel (mfma_assign.hip: coarse_fused_kernel).

The kernel keeps the bf16x3 surrogates of 32 queries in LDS, takes every centroid within the surrogate's error margin of an upper bound
of the nprobes-th smallest, recomputes those exactly in the reference's order and ranks them: partition ids AND distances must equal
`oracle.find_partitions` bit for bit (ids as uint32, distances as their bit patterns).

The matrix-core coarse quantiser switches itself on by problem size (nq * nlist * d >= 2^27); LANCE_HIP_MFMA_COARSE=1 (read once per
process) forces it for every shape it takes, so every group of cases below runs in a fresh child process with the switch on.  The
counter `count:coarse_fused` says that the fused kernel served a call, `count:coarse_fused_prep` that the call built the centroid
constants itself (the plain ABI call always does; an index search only before the index holds them)."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GATE = 960           # the largest list count the fused kernel takes: what 32 rows of surrogates leave room for in a CU's 160 KB of LDS at d = 128
                     # (mfma_assign.hip: CF_MAX_LISTS); 961 .. 1023 lists stay on the two-kernel route, the per-group route starts at 1024


def _setup():
    sys.path.insert(0, ROOT)
    import oracle
    from lance_amd.engine import Engine
    oracle.lib()
    return oracle, Engine()


def _fused(eng):
    return eng.timing_query("count:coarse_fused")[1]


def _eq(eng, oracle, q, cent, nprobes, metric, tag, ref=None):
    """one call; -> how often the fused kernel served it.  ref: the oracle's answer for a superset of the rows (queries are independent)"""
    before = _fused(eng)
    ids, d = eng.find_partitions(q, cent, nprobes, metric)
    served = _fused(eng) - before
    oi, od = ref if ref is not None else oracle.find_partitions(q, cent, nprobes, metric)
    oi, od = oi[:len(q)], od[:len(q)]
    ids = ids.cpu().numpy().view(np.uint32); d = d.cpu().numpy()
    assert np.array_equal(ids, oi), (tag, np.argwhere(ids != oi)[:5])
    assert np.array_equal(d.view(np.uint32), od.view(np.uint32)), tag
    return served


def _data(oracle, rng, d, nlist, nq, metric):
    cent = (rng.standard_normal((nlist, d)) * 3).astype(f32)
    q = (cent[rng.integers(0, nlist, nq)] + rng.standard_normal((nq, d)).astype(f32)).astype(f32)
    if metric == "cosine":     # the index path normalises rows and queries, then L2
        cent = oracle.normalize(cent); q = oracle.normalize(q)
    return q, cent


def _grid(dims, lists, rows, expect):
    """Child: the cross product of the shapes, L2 / dot / cosine; every call must raise the counter by `expect`."""
    oracle, eng = _setup()
    rng = np.random.default_rng(4711)
    n = 0
    for d in dims:
        for nlist in lists:
            for metric in ("l2", "dot", "cosine"):
                q, cent = _data(oracle, rng, d, nlist, max(rows), metric)
                km = "l2" if metric == "cosine" else metric
                probes = [p for p in (1, 10, 50, 64) if p <= nlist] + ([nlist] if nlist in (32, 33) else [])
                for nprobes in probes:
                    ref = oracle.find_partitions(q, cent, nprobes, km)
                    for nq in rows:
                        served = _eq(eng, oracle, q[:nq], cent, nprobes, km, (d, nlist, nq, metric, nprobes), ref)
                        assert served == expect, ("count:coarse_fused", served, d, nlist, nq, metric, nprobes)
                        n += 1
    prep = eng.timing_query("count:coarse_fused_prep")[1]
    assert prep == n * expect, (prep, n)      # the plain ABI call has no index: it prepares the centroids itself
    eng.close()
    print(f"coarse fused grid ok: {n} calls")


def _edges(nlist, groups_expected):
    """Child: a list count the fused kernel must leave to another route (groups_expected: calls the per-group route serves)"""
    oracle, eng = _setup()
    rng = np.random.default_rng(99)
    for d in (64, 128):
        for metric in ("l2", "dot"):
            q, cent = _data(oracle, rng, d, nlist, 200, metric)
            for nprobes in (1, 10, 64):
                assert _eq(eng, oracle, q, cent, nprobes, metric, (d, nlist, metric, nprobes)) == 0
    groups = eng.timing_query("count:coarse_groups")[1]
    assert groups == groups_expected, groups
    eng.close()
    print("coarse fused edges ok")


def _ties(expect):
    """Child: ties and non-finite values at d 64, 512 lists, integer-valued centroids"""
    oracle, eng = _setup()
    rng = np.random.default_rng(2025)
    d, nlist = 64, 512
    cent = np.rint(rng.uniform(0, 40, (nlist, d))).astype(f32)
    cent[7] = cent[300]                            # two identical centroids: the first index wins
    cent[100:260] = cent[100]                      # 160 identical centroids > 128 candidates
    q = np.rint(rng.uniform(0, 40, (130, d))).astype(f32)
    q[3] = cent[100]                               # distance 0 to the whole block: the exact path inside the kernel
    q[4] = cent[7]
    q[5, 2] = np.nan
    q[6] = np.inf
    q[8] = 1e30                                    # squares overflow: inf distances
    # dot takes only the finite variants (inf x 0 and 1 - NaN carry a platform-dependent NaN sign: tests/test_zz_gpu_coarse_mfma.py)
    qd = q.copy(); qd[6] = q[7]; qd[5] = q[9]
    for nprobes in (1, 10, 50, 64):
        assert _eq(eng, oracle, q, cent, nprobes, "l2", ("ties", nprobes)) == expect
        assert _eq(eng, oracle, qd, cent, nprobes, "dot", ("ties-dot", nprobes)) == expect
    # one +inf centroid component: every surrogate row carries a NaN (inf - inf in the bf16 split) -> every row takes the exact path
    cent2 = cent.copy(); cent2[11, 0] = np.inf
    assert _eq(eng, oracle, q, cent2, 10, "l2", "inf-centroid") == expect
    eng.close()
    print("coarse fused ties ok")


STAGES = ("select_probes", "dist_matrix", "coarse_fused", "coarse_fused_prep", "coarse_groups", "graph_capture", "graph_replay")


def _three_calls(eng, oracle, gidx, oidx, q, tag):
    """plain, captured, replayed through the same buffers -> the counter deltas of each; every answer equals the oracle's"""
    import torch
    nq, k, nprobes = len(q), 10, 4
    oi, od = oidx.search(q, k, nprobes)
    dev = torch.device("cuda")
    qd = torch.from_numpy(q).to(dev)
    out = (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
    count = lambda: {s: eng.timing_query("count:" + s)[1] for s in STAGES}
    deltas = []
    for call in range(3):
        out[0].fill_(-7); out[1].fill_(float("nan"))
        torch.cuda.synchronize()
        before = count()
        gidx.search(qd, k, nprobes, 0, out=out, engine=eng)
        eng.synchronize()
        after = count()
        deltas.append({s: int(after[s] - before[s]) for s in STAGES})
        assert (out[0].cpu().numpy().view(np.uint64) == oi).all(), (tag, call, "ids differ from the oracle")
        assert (out[1].cpu().numpy().view(np.uint32) == od.view(np.uint32)).all(), (tag, call, "distances differ from the oracle")
    for call, dl in enumerate(deltas):
        assert dl["coarse_fused"] == 1 and dl["select_probes"] == 1 and dl["dist_matrix"] == 0 and dl["coarse_groups"] == 0, (tag, call, dl)
    assert deltas[1]["graph_capture"] == 1 and deltas[2]["graph_replay"] == 1, (tag, deltas)
    return deltas


def _index():
    """Child: the index path, whose centroid constants are built once per index"""
    oracle, eng = _setup()
    from lance_amd.engine import DeviceIndex, Engine
    from tests import search_routes_spec as spec
    eng2 = Engine()
    for name in ("l2_128_64lists", "dot_128_64lists"):
        metric = spec.INDEXES[name][0]
        gidx, oidx, raw, q = spec.build(eng, oracle, name)
        # the first search of an index builds the constants itself (outside the batch's chain): no call prepares them per batch
        dl = _three_calls(eng, oracle, gidx, oidx, q, (name, "first index"))
        assert [x["coarse_fused_prep"] for x in dl] == [0, 0, 0], dl
        # the same index from a second context: the constants are there
        dl = _three_calls(eng2, oracle, gidx, oidx, q[:777], (name, "second context"))
        assert [x["coarse_fused_prep"] for x in dl] == [0, 0, 0], dl
        part, codes, _ = eng.ivfpq_encode(raw, gidx.centroids, gidx.codebook, metric)
        for prewarm in (False, True):
            other = DeviceIndex.create(eng, metric, gidx.centroids, gidx.codebook, part, codes, None, raw=raw)
            if prewarm:
                other.prewarm()
            first, second = (eng2, eng) if prewarm else (eng, eng2)
            dl = _three_calls(first, oracle, other, oidx, q[:1000], (name, "second index", prewarm))
            assert [x["coarse_fused_prep"] for x in dl] == [0, 0, 0], dl
            dl = _three_calls(second, oracle, other, oidx, q[:333], (name, "second index, other context", prewarm))
            assert [x["coarse_fused_prep"] for x in dl] == [0, 0, 0], dl
            other.close()
    eng2.close()
    eng.close()
    print("coarse fused index ok")


def _child(call, **env):
    e = dict(os.environ, LANCE_HIP_MFMA_COARSE="1")
    for k in ("LANCE_HIP_NO_COARSE_FUSED", "LANCE_HIP_COARSE_GROUPS", "LANCE_HIP_COARSE_GROUPS_MA"):
        e.pop(k, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import tests.test_zz_gpu_coarse_fused as t; t.%s" % (ROOT, call)],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_shape_grid_equals_the_oracle_and_takes_the_fused_kernel():
    out = _child("_grid((16, 64, 96, 128), (32, 33, 100, 256, 512, %d), (1, 31, 32, 33, 300), 1)" % GATE)
    assert "coarse fused grid ok" in out


def test_first_list_count_above_the_gate_stays_on_the_two_kernel_route():
    assert "coarse fused edges ok" in _child("_edges(%d, 0)" % (GATE + 1))


def test_1024_lists_go_to_the_per_group_route():
    assert "coarse fused edges ok" in _child("_edges(1024, 12)")


def test_per_group_route_from_256_lists_keeps_256_lists():
    assert "coarse fused edges ok" in _child("_edges(256, 12)", LANCE_HIP_COARSE_GROUPS="256")


def test_ties_and_non_finite_values():
    assert "coarse fused ties ok" in _child("_ties(1)")


def test_switched_off_the_two_kernel_route_answers_the_same():
    out = _child("_grid((16, 128), (33, 256, %d), (1, 33, 300), 0)" % GATE, LANCE_HIP_NO_COARSE_FUSED="1")
    assert "coarse fused grid ok" in out
    assert "coarse fused ties ok" in _child("_ties(0)", LANCE_HIP_NO_COARSE_FUSED="1")


def test_index_search_with_cached_constants_plain_captured_replayed():
    assert "coarse fused index ok" in _child("_index()")
