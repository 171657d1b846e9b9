"""The grid of tiny IVF-PQ searches behind tests/golden/search_routes.json: one case per route of the search plan
(lance_amd/csrc/search_plan.h) at the smallest shape that still crosses the route's gate, and the A/B switches that move a case to
another route.  scripts/record_search_routes.py runs the grid and writes, per case, the deltas of every `count:<stage>` counter for
three calls with the same buffers (plain, captured, replayed); tests/test_zz_gpu_search_routes.py runs it again and compares.  Every
call's ids and distances are compared with the CPU oracle, bit for bit.

The switches are read once per process, so a case that sets one runs in a child: `python tests/search_routes_spec.py NAME ...` prints
one JSON line {name: [counter deltas per call]} (the environment is the caller's).
"""
import json
import os
import re
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "search_routes.json")
f32 = np.float32

STAGES = ("select_probes", "coarse_groups", "pm_group", "ivfpq_scan", "ivfpq_scan_c0", "ivfpq_scan_c1", "ivfpq_scan_cb", "ivfpq_msbound",
          "ivfpq_mscan", "q_residual", "q_pt_tables", "q_pt_table_only", "ivfpq_merge", "ivfpq_exact", "refine", "refine_u8",
          "graph_capture", "graph_replay")


def scan_max_keff():
    """SCAN_MAX_KEFF of lance_amd/csrc/search_common.cuh: the largest k * refine the scan kernels' heaps hold"""
    with open(os.path.join(ROOT, "lance_amd", "csrc", "search_common.cuh")) as f:
        return int(re.search(r"constexpr int SCAN_MAX_KEFF = (\d+);", f.read()).group(1))


# index name -> (metric, column type, d, M, nbits, nlist, rows, codebook)
INDEXES = {
    "l2_128": ("l2", "float32", 128, 16, 8, 8, 4000, "trained"),
    "l2_128_64lists": ("l2", "float32", 128, 16, 8, 64, 4000, "trained"),
    "l2_192": ("l2", "float32", 192, 48, 8, 8, 4000, "trained"),
    "f16_192": ("l2", "float16", 192, 48, 8, 8, 4000, "trained"),
    "l2_64_4bit": ("l2", "float32", 64, 16, 4, 8, 4000, "trained"),
    "dot_128": ("dot", "float32", 128, 16, 8, 8, 4000, "trained"),
    "dot_128_64lists": ("dot", "float32", 128, 16, 8, 64, 4000, "trained"),
    "l2_128_zero_codebook": ("l2", "float32", 128, 16, 8, 8, 4000, "zero"),
}

_K = scan_max_keff()
# case name -> (index, nq, k, nprobes, refine factor, kind); kind "range" = a distance-range query
CASES = {
    "mscan_pm": ("l2_128", 1024, 10, 4, 2, "knn"),                       # 4096 pairs >= 96 * 8 lists, >= 4096
    "small_batch": ("l2_128", 64, 10, 4, 0, "knn"),                      # 256 pairs: query major
    "integer_scan": ("l2_128_64lists", 1024, 10, 4, 0, "knn"),           # 4096 pairs < 96 * 64 lists
    "tiled_pt": ("l2_192", 512, 10, 4, 0, "knn"),                        # M = 48: 2048 pairs
    "tiled_below_gate": ("l2_192", 511, 10, 4, 0, "knn"),                # 2044 pairs
    "tiled_f16": ("f16_192", 512, 10, 4, 0, "knn"),
    "four_bit": ("l2_64_4bit", 1024, 10, 4, 0, "knn"),
    "exact_only": ("l2_128", 64, (_K + 3) // 3, 4, 3, "knn"),            # k * refine just above SCAN_MAX_KEFF
    "at_keff_cap": ("l2_128", 1024, _K, 4, 0, "knn"),
    "range_query": ("l2_128", 1024, 10, 4, 0, "range"),
    "dot_mscan": ("dot_128", 1024, 10, 4, 2, "knn"),
    "dot_pair_scan": ("dot_128_64lists", 1024, 10, 4, 0, "knn"),         # 4096 pairs < 96 * 64 lists
    "dot_small_batch": ("dot_128", 64, 10, 4, 0, "knn"),
    "zero_codebook": ("l2_128_zero_codebook", 1024, 10, 4, 0, "knn"),
}
# group name -> (environment, cases): one child process per group
SWITCHED = {
    "no_mscan": ({"LANCE_HIP_NO_MSCAN": "1"}, ("mscan_pm", "dot_mscan")),
    "no_msbound": ({"LANCE_HIP_NO_MSBOUND": "1"}, ("mscan_pm", "dot_mscan")),
    "no_qscan": ({"LANCE_HIP_NO_QSCAN": "1"}, ("mscan_pm", "tiled_pt")),
    "pm_nobound": ({"LANCE_HIP_PM_NOBOUND": "1"}, ("mscan_pm", "tiled_pt")),
    "exact_bound": ({"LANCE_HIP_EXACT_BOUND": "1"}, ("mscan_pm", "tiled_pt")),
    "qpt0": ({"LANCE_HIP_QPT": "0"}, ("tiled_pt",)),
    "qpt1": ({"LANCE_HIP_QPT": "1"}, ("tiled_pt",)),
    "no_pm": ({"LANCE_HIP_NO_PM": "1"}, ("mscan_pm",)),
    "no_dot_flow": ({"LANCE_HIP_NO_DOT_FLOW": "1"}, ("dot_mscan",)),
}
SWITCH_NAMES = sorted({k for env, _ in SWITCHED.values() for k in env} |
                      {"LANCE_HIP_MSCAN_MINQ", "LANCE_HIP_BOUND_LISTS", "LANCE_HIP_DOT_BOUND_LISTS", "LANCE_HIP_DOT_FLOW_SKEW"})


def _rows(n, d, seed, dot):
    rng = np.random.default_rng(seed)
    centers = rng.uniform(0, 128, (24, d))
    x = np.clip(np.rint(centers[rng.integers(0, 24, n)] + rng.normal(0, 20, (n, d))), 0, 218).astype(f32)
    return x - f32(64.0) if dot else x


_built = {}


def build(eng, oracle, name):
    """-> (device index, oracle index, rows as f32, queries in the column's type); cached per process"""
    if name in _built:
        return _built[name]
    from lance_amd.engine import DeviceIndex
    metric, dtype, d, m, nbits, nlist, n, cbk = INDEXES[name]
    x = _rows(n, d, 7 + d + m + nlist, metric == "dot")
    q = _rows(1024, d, 8 + d + m + nlist, metric == "dot")
    if dtype == "float16":
        x, q = (x * f32(0.05)).astype(np.float16), (q * f32(0.05)).astype(np.float16)
    cent, _, _, _ = oracle.kmeans_train(x[:2048].astype(f32), nlist, max_iters=4, seed=1, metric=metric)
    cent = cent.astype(x.dtype)
    part, _ = oracle.assign(x, cent, metric)
    res = oracle.residual(x, cent, np.where(part == oracle.NONE, 0, part)) if metric == "l2" else x
    cb, _ = oracle.pq_train(res[:3072], m, nbits=nbits, max_iters=3, seed=2)
    if cbk == "zero":
        cb = np.zeros_like(cb)
    oidx = oracle.build_index(x, cent, cb, metric, nbits=nbits)
    gpart, gcodes, _ = eng.ivfpq_encode(x, cent, cb, metric)
    gidx = DeviceIndex.create(eng, metric, cent, cb, gpart, gcodes, None, raw=x)
    _built[name] = (gidx, oidx, x.astype(f32), q)
    return _built[name]


def run_case(eng, oracle, name):
    """Three calls through the same device buffers -> the counter deltas of each; asserts every answer equals the oracle's."""
    import torch
    index, nq, k, nprobes, rf, kind = CASES[name]
    gidx, oidx, raw, q = build(eng, oracle, index)
    q = q[:nq]
    if kind == "range":
        _, ud = oidx.search(q, 4 * k, nprobes)
        fin = ud[np.isfinite(ud)]
        lo, hi = float(np.quantile(fin, 0.2)), float(np.quantile(fin, 0.7))
        oi, od = oidx.search(q, k, nprobes, lower=lo, upper=hi)
    else:
        oi, od = oidx.search(q, k, nprobes, refine=rf, raw=raw if rf else None)
    dev = torch.device("cuda")
    qd = torch.from_numpy(q).to(dev)
    out = (torch.empty((nq, k), dtype=torch.int64, device=dev), torch.empty((nq, k), dtype=torch.float32, device=dev))
    count = lambda: {s: eng.timing_query("count:" + s)[1] for s in STAGES}
    deltas = []
    for call in range(3):
        out[0].fill_(-7); out[1].fill_(float("nan"))
        torch.cuda.synchronize()
        before = count()
        if kind == "range":
            gidx.search_range(qd, k, nprobes, lower=lo, upper=hi, out=out)
        else:
            gidx.search(qd, k, nprobes, rf, out=out)
        eng.synchronize()
        after = count()
        deltas.append({s: int(after[s] - before[s]) for s in STAGES if after[s] != before[s]})
        bad = np.nonzero((out[0].cpu().numpy().view(np.uint64) != oi).any(axis=1))[0]
        assert bad.size == 0, f"{name} call {call}: ids differ from the oracle for {bad.size} of {nq} queries (first {bad[:5]})"
        assert (out[1].cpu().numpy().view(np.uint32) == od.view(np.uint32)).all(), f"{name} call {call}: distances differ from the oracle"
    return deltas


def run_in_child(env, names, timeout=600):
    """-> {name: deltas} from a fresh process with `env` added (and every other route switch removed)"""
    e = {k: v for k, v in os.environ.items() if k not in SWITCH_NAMES}
    e.update(env)
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + list(names), cwd=ROOT, env=e, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def golden():
    with open(GOLDEN) as f:
        return json.load(f)


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import oracle as orc
    from lance_amd.engine import Engine
    orc.lib()
    e = Engine()
    print(json.dumps({nm: run_case(e, orc, nm) for nm in sys.argv[1:]}))
    e.close()
