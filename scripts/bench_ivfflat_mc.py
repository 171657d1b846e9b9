"""The matrix-core main pass of IVF_FLAT (lance_amd/csrc/flat_ivf_mc.hip) against the query-major kernel it replaces, on the shapes of
DESIGN.md 4f.1: 200,000 x 768 and 100,000 x 1536 f32 rows (real-valued: 1024 normal centres plus normal noise), IVF256, 10,000
queries, k = 10, nprobes = 10, L2 and cosine -> profiles/ivfflat_mc.json.  Not part of bench.py.  Needs an MI355X.

The route is chosen by switches that are read once per process, so each route runs in a child process of this script: "mc" with
LANCE_HIP_FLAT_MC_G=0 (the route at any batch size, for the sweep), "query_major" with LANCE_HIP_NO_FLAT_MC=1 (the parent's route).
Every child builds the same indices from the same seeds and records per (shape, metric)
  * ms per search call of the whole batch: HIP events around every call, one warm-up call, the median of three;
  * the library's stage timers (ivfflat_bound, ivfflat_scan, ivfflat_mc, ivfflat_mc_eval, ivfflat_exact) and the rows the filter queued
    per query (count:ivfflat_mc_queued) over one more call with the timers on;
  * the same time for batches of G * nlist / nprobes queries, G = 16, 32, 64 pairs per partition;
  * the ids and distances of the whole batch, compared between the routes by the parent: they must be equal.

--bound compares the BOUND pass instead (the bound pass) -> profiles/ivfflat_mc_bound.json: "mc_bound" with
LANCE_HIP_FLAT_MC_BOUND_G=0 (the matrix-core bound pass at any batch size) against "query_major_bound" with LANCE_HIP_NO_FLAT_MC_BOUND=1
(the parent's route: query-major bound pass, matrix-core main pass); same shapes, same protocol, same sweep, and per point whether the
new route's slowest call beat the other's fastest."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = {"mc": {"LANCE_HIP_FLAT_MC_G": "0"}, "query_major": {"LANCE_HIP_NO_FLAT_MC": "1"}}      # (new, old)
BOUND_ROUTES = {"mc_bound": {"LANCE_HIP_FLAT_MC_BOUND_G": "0"}, "query_major_bound": {"LANCE_HIP_NO_FLAT_MC_BOUND": "1"}}
TIMERS = ("ivfflat_bound", "ivfflat_mc_bound", "ivfflat_scan", "ivfflat_mc", "ivfflat_mc_eval", "ivfflat_exact")
SHAPES = ((200_000, 768), (100_000, 1536))
METRICS = ("l2", "cosine")
SWEEP = (16, 32, 64)


def child(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_ivfflat_mc.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    from lance_amd.engine import Engine

    eng = Engine(use_torch_stream=True)
    dev = torch.device("cuda", torch.cuda.current_device())

    def data(n, d, seed, centres):
        g = torch.Generator(device=dev).manual_seed(seed)
        pick = torch.randint(0, centres.shape[0], (n,), generator=g, device=dev)
        return (centres[pick] + 0.7 * torch.randn((n, d), generator=g, device=dev)).contiguous()

    def timed(ix, qb):
        run = lambda: ix.search_device(qb, a.k, a.nprobes)
        run()
        ms = []
        for _ in range(3):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        eng.timing(True)
        for t in TIMERS:
            eng.timing_query(t)
        queued0 = eng.timing_query("count:ivfflat_mc_queued")[1]
        run()
        stages = {t: (lambda r: {"ms": r[0], "launches": r[1]})(eng.timing_query(t)) for t in TIMERS}
        queued = eng.timing_query("count:ivfflat_mc_queued")[1] - queued0
        eng.timing(False)
        return {"queries": int(qb.shape[0]), "ms": {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))},
                "stages": stages, "queued_rows_per_query": queued / qb.shape[0], "replayed_queries": int(eng.search_stats())}

    rec, answers = {"device": torch.cuda.get_device_name(0)}, {}
    for n, d in SHAPES:
        centres = torch.randn((1024, d), generator=torch.Generator(device=dev).manual_seed(d), device=dev)
        x, q = data(n, d, 1, centres), data(a.queries, d, 2, centres)
        for metric in METRICS:
            name = f"{n}x{d}_{metric}"
            ix = lance_amd.create_index(x, "IVF_FLAT", metric=metric, num_partitions=a.nlist, max_iters=10, engine=eng)
            rec[name] = {"main": timed(ix, q), "sweep": {str(g): timed(ix, q[:-(-g * a.nlist // a.nprobes)].contiguous()) for g in SWEEP}}
            print(name, rec[name]["main"]["ms"], file=sys.stderr, flush=True)
            ids, dists = ix.search_device(q, a.k, a.nprobes)
            answers[name + "_ids"], answers[name + "_dists"] = ids.cpu().numpy(), dists.cpu().numpy()
            del ix
        del x, q
    np.savez(a.child_out + ".npz", **answers)
    with open(a.child_out, "w") as fh:
        json.dump(rec, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobes", type=int, default=10)
    ap.add_argument("--bound", action="store_true", help="compare the bound pass's routes instead of the main pass's")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child-out", default=None)
    a = ap.parse_args()
    if a.child_out:
        return child(a)

    routes = BOUND_ROUTES if a.bound else ROUTES
    new, old = routes
    a.out = a.out or os.path.join(ROOT, "profiles", "ivfflat_mc_bound.json" if a.bound else "ivfflat_mc.json")
    tmp = tempfile.mkdtemp()
    runs, answers = {}, {}
    for name, env in routes.items():
        path = os.path.join(tmp, f"{name}.json")
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-out", path] + sys.argv[1:], env=dict(os.environ, **env), timeout=1100)
        if r.returncode != 0:
            raise SystemExit(f"the {name} child failed with status {r.returncode}")      # nothing more is started on the device
        runs[name] = json.load(open(path))
        answers[name] = np.load(path + ".npz")
    cases = [k for k in runs[new] if k != "device"]
    rec = {"workload": {"shapes": SHAPES, "metrics": METRICS, "nlist": a.nlist, "queries": a.queries, "k": a.k, "nprobes": a.nprobes, "dtype": "float32"},
           "device": runs[new]["device"], "runs": runs,
           "same_ids": {c: bool((answers[new][c + "_ids"] == answers[old][c + "_ids"]).all()) for c in cases},
           "same_distance_bits": {c: bool((answers[new][c + "_dists"].view(np.uint32) == answers[old][c + "_dists"].view(np.uint32)).all())
                                  for c in cases}}
    rec["ms_per_batch"] = {c: {name: runs[name][c]["main"]["ms"] for name in routes} for c in cases}
    rec["sweep_ms_per_batch"] = {c: {str(g): {name: runs[name][c]["sweep"][str(g)]["ms"] for name in routes} for g in SWEEP} for c in cases}
    rec["queued_rows_per_query"] = {c: {name: runs[name][c]["main"]["queued_rows_per_query"] for name in routes} for c in cases}
    # the acceptance rule of DESIGN.md 4f.1: the new route's slowest call against the other route's fastest
    wins = lambda r: r[new]["max"] < r[old]["min"]
    rec["new_slowest_beats_old_fastest"] = {c: dict({"main": wins(rec["ms_per_batch"][c])}, **{g: wins(r) for g, r in rec["sweep_ms_per_batch"][c].items()})
                                            for c in cases}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k != "runs"}))
    print(json.dumps({name: {c: runs[name][c]["main"]["stages"] for c in cases} for name in routes}))


if __name__ == "__main__":
    main()
