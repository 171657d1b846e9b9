"""The partition-major IVF_RQ scan (lance_amd/csrc/rq_pm.cuh) against the pair-major one on the shape of DESIGN.md 4d: 1M x 128 f32
clustered rows (lance_amd.testing.sift_like), IVF256, L2, 10,000 queries, k = 10, nprobes = 10 -> profiles/rq_grouped_probe.json.
Not part of bench.py.  Needs an MI355X.

The route is chosen by switches that are read once per process, so each route runs in child processes of this script, ALTERNATING
(grouped, pair-major, grouped, pair-major, ...; --rounds of each): every child builds the same index from the same seeds and records
  * ms per search call of the whole batch: HIP events on the context's stream around every call, after warm-up, median / min / max;
  * the library's per-kernel timers (HIP events around each launch) over 5 more calls, per call;
  * the same two for refine_factor 5 and 10 (keff 50 and 100) on the same batch;
  * the bytes the scan requests, counted from the probes of this very batch: pair-major reads a partition's rows (d / 8 code bytes + two
    f32 factors) once per pair, grouped once per block of 32 pairs of the partition;
  * recall@10 against the exhaustive scan on a 1000-query slice, and the ids and distances of the whole batch (compared between the
    routes by the parent: they must be equal);
  * the G sweep: batches of G * nlist / nprobes queries for G = 4 .. 128 mean pairs per partition, same timing.
The grouped children run with LANCE_HIP_RQ_GROUPED_G=0 (grouped at any batch size), the others with LANCE_HIP_NO_RQ_GROUPED=1.
--routes pair_major alone measures a build without the route (the parent commit's pair-major scan, for the build-flag comparison)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROUTES = {"grouped": {"LANCE_HIP_RQ_GROUPED_G": "0"}, "pair_major": {"LANCE_HIP_NO_RQ_GROUPED": "1"}}
TIMERS = ("ivfrq_pm_group", "ivfrq_pm_scan", "ivfrq_scan", "ivfrq_merge", "ivfrq_exact")
SWEEP = (4, 8, 16, 32, 64, 128)
REFINE = (5, 10)


def child(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rq_grouped_probe.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    from lance_amd.engine import Engine
    from lance_amd.testing import sift_like

    eng = Engine(use_torch_stream=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = sift_like(a.rows, a.d, seed=1, device=dev)
    q = sift_like(a.queries, a.d, seed=2, device=dev)
    rq = lance_amd.create_index(x, "IVF_RQ", metric="l2", num_partitions=a.nlist, engine=eng)

    def timed(qb, rf=0):
        run = lambda: rq.search_device(qb, a.k, a.nprobes, refine_factor=rf)
        for _ in range(a.warmup):
            run()
        ms = []
        for _ in range(a.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms.append(e0.elapsed_time(e1))
        eng.timing(True)
        for t in TIMERS:
            eng.timing_query(t)
        for _ in range(5):
            run()
        kernels = {t: (lambda r: {"ms": r[0] / 5, "launches": r[1] / 5})(eng.timing_query(t)) for t in TIMERS}
        eng.timing(False)
        return {"queries": int(qb.shape[0]), "ms": {"median": float(np.median(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}, "kernels": kernels}

    rec = {"device": torch.cuda.get_device_name(0), "main": timed(q)}
    ids, dists = rq.search_device(q, a.k, a.nprobes)
    rec["main"]["replayed_queries"] = int(eng.search_stats())
    np.savez(a.child_out + ".npz", ids=ids.cpu().numpy(), dists=dists.cpu().numpy())
    rec["refine"] = {str(rf): timed(q, rf) for rf in REFINE}
    rec["sweep"] = {str(g): timed(q[:-(-g * a.nlist // a.nprobes)].contiguous()) for g in SWEEP}

    probes = eng.find_partitions(q, torch.from_numpy(rq.centroids).to(dev), a.nprobes, "l2")[0].cpu().numpy().astype(np.int64)
    sizes = np.bincount(rq.part_ids.cpu().numpy().astype(np.int64).clip(min=-1) + 1, minlength=a.nlist + 1)[1:]
    pairs = np.bincount(probes.ravel(), minlength=a.nlist)
    bpr = a.d // 8 + 8
    rec["scan_bytes"] = {"unique": int(sizes.sum()) * bpr, "pair_major": int((sizes * pairs).sum()) * bpr, "grouped": int((sizes * -(-pairs // 32)).sum()) * bpr,
                         "work_items": int((-(-pairs // 32)).sum()), "pairs": int(pairs.sum()), "row_pair_cells": int((sizes * pairs).sum())}
    nr = min(1000, a.queries)
    truth = eng.flat_topk(x, q[:nr].contiguous(), a.k, "l2")[0].cpu().numpy()
    got = ids[:nr].cpu().numpy()
    rec["recall_at_k"] = float(np.mean([len(set(g) & set(t)) / a.k for g, t in zip(got, truth)]))
    with open(a.child_out, "w") as fh:
        json.dump(rec, fh)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobes", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--routes", default="grouped,pair_major")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rq_grouped_probe.json"))
    ap.add_argument("--child-out", default=None)
    a = ap.parse_args()
    if a.child_out:
        return child(a)

    tmp = tempfile.mkdtemp()
    routes = {name: ROUTES[name] for name in a.routes.split(",")}
    runs = {name: [] for name in routes}
    answers = {}
    for rnd in range(a.rounds):
        for name, env in routes.items():
            path = os.path.join(tmp, f"{name}{rnd}.json")
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child-out", path] + sys.argv[1:], env=dict(os.environ, **env), timeout=900)
            if r.returncode != 0:
                raise SystemExit(f"the {name} child failed with status {r.returncode}")      # nothing more is started on the device
            runs[name].append(json.load(open(path)))
            z = np.load(path + ".npz")
            answers.setdefault(name, (z["ids"], z["dists"]))
    rec = {"shape": {"rows": a.rows, "d": a.d, "nlist": a.nlist, "metric": "l2", "queries": a.queries, "k": a.k, "nprobes": a.nprobes, "dtype": "float32"},
           "device": next(iter(runs.values()))[0]["device"], "warmup": a.warmup, "reps": a.reps, "rounds": a.rounds, "runs": runs}
    span = lambda name, pick: {"min": min(pick(r)["ms"]["min"] for r in runs[name]), "max": max(pick(r)["ms"]["max"] for r in runs[name]),
                               "median_of_medians": float(np.median([pick(r)["ms"]["median"] for r in runs[name]]))}
    rec["main_ms_per_batch"] = {name: span(name, lambda r: r["main"]) for name in routes}
    rec["refine_ms_per_batch"] = {str(rf): {name: span(name, lambda r: r["refine"][str(rf)]) for name in routes} for rf in REFINE}
    rec["sweep_ms_per_batch"] = {str(g): {name: span(name, lambda r: r["sweep"][str(g)]) for name in routes} for g in SWEEP}
    if len(routes) == 2:
        gi, gd = answers["grouped"]
        pi, pd = answers["pair_major"]
        rec["same_ids"] = bool((gi == pi).all())
        rec["same_distance_bits"] = bool((gd.view(np.uint32) == pd.view(np.uint32)).all())
        rec["grouped_wins_from_G"] = next((g for g in SWEEP if all(rec["sweep_ms_per_batch"][str(h)]["grouped"]["max"] < rec["sweep_ms_per_batch"][str(h)]["pair_major"]["min"]
                                                                   for h in SWEEP if h >= g)), None)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps({k: v for k, v in rec.items() if k != "runs"}))
    print(json.dumps({name: [r["main"]["kernels"] for r in rs] for name, rs in runs.items()}))
    print(json.dumps({name: [{rf: r["refine"][rf]["kernels"] for rf in r["refine"]} for r in rs] for name, rs in runs.items()}))
    print(json.dumps({name: rs[0]["scan_bytes"] | {"recall": rs[0]["recall_at_k"], "replayed": rs[0]["main"]["replayed_queries"]} for name, rs in runs.items()}))


if __name__ == "__main__":
    main()
