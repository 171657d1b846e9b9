"""One measured run of the combined search on the C2 shape: 1M x 128 f32 clustered rows (lance_amd.testing.sift_like),
IVF256 / PQ16, L2, 10,000 queries, k = 10, nprobes = 10, refine_factor = 10 -> profiles/knn_combined.json.  Not part of bench.py.
Needs an MI355X.

The parent process never touches the GPU: it starts `--processes` fresh children one after the other (each builds the index and measures
everything; HIP events around whole `nearest` calls, 3 warm-up + 15 timed batches, the configurations ALTERNATING batch by batch) and
joins their records.
  (a) VectorColumn.nearest with one delta and no unindexed row, against index.nearest, in the same processes.  Passes when the column's
      worst median is no more than the spread (max - min) of index.nearest's own medians above index.nearest's best median.
  (b) the same rows with 0.1 %, 1 % and 10 % of them moved to an unindexed tail (the index holds the rest, same model): the batch time,
      and next to it the ANN over the delta (its own search for k * refine_factor rows), the flat scan of the tail and the two
      take_flat_knn calls (the library's timer) measured on their own, and what `index.append` of that tail costs (wall clock, device
      drained).  A record, not a threshold."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
TAILS = (0.001, 0.01, 0.1)


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def timed_alternating(torch, runs, warmup, reps):
    for _ in range(warmup):
        for run in runs.values():
            run()
    ms = {name: [] for name in runs}
    for _ in range(reps):
        for name, run in runs.items():           # alternating: all see the same neighbours on a shared host
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return ms


def child(a):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("knn_combined_probe.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    from lance_amd.engine import Engine
    from lance_amd.testing import sift_like

    eng = Engine(use_torch_stream=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = sift_like(a.rows, a.d, seed=1, device=dev)
    q = sift_like(a.queries, a.d, seed=2, device=dev)
    kw = dict(k=a.k, nprobes=a.nprobes, refine_factor=a.refine)
    index = lance_amd.create_index(x, "IVF_PQ", metric="l2", num_partitions=a.nlist, num_sub_vectors=a.m, engine=eng)
    model = dict(index_type="IVF_PQ", metric="l2", num_partitions=a.nlist, num_sub_vectors=a.m, ivf_centroids=index.centroids,
                 pq_codebook=index.codebook)
    whole = lance_amd.VectorColumn(x, engine=eng).with_index(index, [0])
    rec = {"device": torch.cuda.get_device_name(0)}
    ms = timed_alternating(torch, {"index": lambda: index.nearest(q, **kw), "column": lambda: whole.nearest(q, **kw)}, a.warmup, a.reps)
    rec["a"] = {name: stats(v) for name, v in ms.items()}
    gi, gd = index.nearest(q, **kw)
    ci, cd = whole.nearest(q, **kw)
    rec["a"]["same_answer"] = bool((gi == ci).all() and (gd.view(np.uint32) == cd.view(np.uint32)).all())

    rec["b"] = {}
    for share in TAILS:
        t = int(round(a.rows * share))
        col = lance_amd.VectorColumn(x, [a.rows - t, t], engine=eng).create_delta([0], **model)
        delta = col.deltas[0]
        keff = a.k * a.refine
        parts = {"batch": lambda: col.nearest(q, **kw),
                 "ann": lambda: col._ann(delta, "IVF_PQ", q, keff, a.nprobes, None, {}),
                 "tail_scan": lambda: col._tail_lists(eng, q, a.k, "l2", None, {})}
        row = {name: stats(v) for name, v in timed_alternating(torch, parts, a.warmup, a.reps).items()}
        eng.timing(True)
        eng.timing_query("take_flat_knn")                     # a query resets the timer
        for _ in range(3):
            col.nearest(q, **kw)
        row["take_flat_knn_ms_per_batch"] = eng.timing_query("take_flat_knn")[0] / 3
        eng.timing(False)
        tail = x[a.rows - t:]
        rid = torch.arange(a.rows - t, a.rows, dtype=torch.int64, device=dev)
        wall = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            grown = delta.append(tail, row_ids=rid, raw=x)
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1e3)
            grown._ix.close()
        row["index_append_ms"] = stats(wall)
        row["tail_rows"] = t
        rec["b"]["%g%%" % (share * 100)] = row
        delta._ix.close()
    print("__RECORD__" + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--queries", type=int, default=10_000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobes", type=int, default=10)
    ap.add_argument("--refine", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "knn_combined.json"))
    a = ap.parse_args()
    if a.child:
        return child(a)
    args = [v for v in sys.argv[1:] if v != "--child"]
    runs = []
    for _ in range(a.processes):                                  # fresh processes, one after the other
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, capture_output=True, text=True, timeout=900)
        lines = [l for l in r.stdout.splitlines() if l.startswith("__RECORD__")]
        if r.returncode != 0 or not lines:
            raise SystemExit("a measuring process failed:\n" + r.stdout[-2000:] + r.stderr[-4000:])
        runs.append(json.loads(lines[-1][len("__RECORD__"):]))
        print("process %d of %d: %s" % (len(runs), a.processes, json.dumps(runs[-1]["a"])), flush=True)
    rec = {"shape": {"rows": a.rows, "d": a.d, "nlist": a.nlist, "pq_sub_vectors": a.m, "metric": "l2", "queries": a.queries, "k": a.k,
                     "nprobes": a.nprobes, "refine_factor": a.refine, "dtype": "float32"},
           "device": runs[0]["device"], "warmup": a.warmup, "reps": a.reps, "processes": runs}
    med_i = [r["a"]["index"]["median"] for r in runs]
    med_c = [r["a"]["column"]["median"] for r in runs]
    spread = max(med_i) - min(med_i)
    rec["a_summary"] = {"index_medians_ms": med_i, "column_medians_ms": med_c, "index_spread_ms": spread,
                        "column_over_index_ms": max(med_c) - min(med_i),
                        "within_spread": bool(max(med_c) - min(med_i) <= spread), "same_answer": all(r["a"]["same_answer"] for r in runs)}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec["a_summary"]))
    print(json.dumps({k: {p: v[p]["median"] if isinstance(v[p], dict) else v[p] for p in v} for k, v in runs[0]["b"].items()}))


if __name__ == "__main__":
    main()
