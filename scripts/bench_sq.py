"""IVF_SQ against IVF_FLAT on the same rows and centroids: 1M x 128 f32 rows (lance_amd.testing.sift_like), IVF256, L2, k = 10,
nprobes = 10, batches of 1 and 10,000 queries -> profiles/sq_scan.json.  Not part of bench.py.  Needs an MI355X.

What is recorded:
  * build seconds per stage of both indices (create_index's own stage clocks);
  * ms per search call of each index and batch size: HIP events on the context's stream (the engine shares torch's stream here)
    around every call, 5 warm-up + 30 timed calls, median and mean; and the library's per-kernel timers over 5 more calls;
  * the share of IVF_SQ queries replayed through the heap;
  * recall@10 of both indices against the exhaustive scan (flat_knn) on a 1000-query slice;
  * the CPU specification (tests/sq_spec.py): every code byte and partition id of the build, and ids + distance bits of a
    100-query slice of the search.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SQ_TIMERS = ("dist_matrix", "select_probes", "ma_sweep", "ma_recheck", "ivfsq_encode_q", "ivfsq_scan", "ivfsq_merge", "ivfsq_exact")
FLAT_TIMERS = ("dist_matrix", "select_probes", "ma_sweep", "ma_recheck", "ivfflat_bound", "ivfflat_scan", "ivfflat_exact")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobes", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 10_000])
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--spec-queries", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sq_scan.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_sq.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    import oracle
    import sq_spec as S
    from lance_amd.engine import Engine
    from lance_amd.testing import sift_like

    eng = Engine(use_torch_stream=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = sift_like(a.rows, a.d, seed=1, device=dev)
    nq_max = max(max(a.batches), a.recall_queries, a.spec_queries)
    q = sift_like(nq_max, a.d, seed=2, device=dev)
    rec = {"shape": {"rows": a.rows, "d": a.d, "nlist": a.nlist, "metric": "l2", "k": a.k, "nprobes": a.nprobes, "dtype": "float32"},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "build_seconds": {}, "search": {}}

    sq = lance_amd.create_index(x, "IVF_SQ", metric="l2", num_partitions=a.nlist, engine=eng)
    rec["build_seconds"]["ivf_sq"] = dict(sq.stats.seconds)
    rec["bounds"] = list(sq.bounds)
    flat = lance_amd.create_index(x, "IVF_FLAT", metric="l2", num_partitions=a.nlist, ivf_centroids=sq.centroids, engine=eng)
    rec["build_seconds"]["ivf_flat"] = dict(flat.stats.seconds)
    rec["bytes_per_row"] = {"ivf_sq": a.d + 4, "ivf_flat": 4 * a.d}

    def timed(index, qb, timers):
        run = lambda: index.search_device(qb, a.k, a.nprobes)
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
        out = {"ms_median": float(np.median(ms)), "ms_mean": float(np.mean(ms)), "ms_min": float(np.min(ms))}
        eng.timing(True)
        for t in timers:
            eng.timing_query(t)
        for _ in range(5):
            run()
        out["kernel_ms_per_call"] = {t: eng.timing_query(t)[0] / 5 for t in timers}
        eng.timing(False)
        return out

    for nq in a.batches:
        qb = q[:nq].contiguous()
        r = {"ivf_sq": timed(sq, qb, SQ_TIMERS), "ivf_flat": timed(flat, qb, FLAT_TIMERS)}
        sq.search_device(qb, a.k, a.nprobes)
        r["ivf_sq"]["replayed_share"] = eng.search_stats() / nq
        r["flat_over_sq"] = r["ivf_flat"]["ms_median"] / r["ivf_sq"]["ms_median"]
        rec["search"][str(nq)] = r
        print(nq, json.dumps(r), flush=True)

    # recall@10 against the exhaustive scan
    qr = q[:a.recall_queries].contiguous()
    truth = eng.flat_topk(x, qr, a.k, "l2")[0].cpu().numpy()
    for name, index in (("ivf_sq", sq), ("ivf_flat", flat)):
        got = index.search_device(qr, a.k, a.nprobes)[0].cpu().numpy()
        rec.setdefault("recall_at_k", {})[name] = float(np.mean([len(set(g) & set(t)) / a.k for g, t in zip(got, truth)]))

    # the CPU specification: the build's codes and partition ids, then a slice of the search
    t0 = time.perf_counter()
    xh = x.cpu().numpy()
    cent = sq.centroids
    start, end = sq.bounds
    codes = np.concatenate([S.encode(xh[i:i + 65536], start, end) for i in range(0, a.rows, 65536)])
    _, part = S.prepare_rows(oracle, xh, cent, "l2")
    qs = q[:a.spec_queries].cpu().numpy()
    oi, od = S.search(oracle, codes, part, cent, qs, a.k, a.nprobes, "l2", start, end)
    gi, gd = sq.nearest(qs, a.k, a.nprobes)
    rec["spec"] = {"queries": a.spec_queries,
                   "codes_equal": bool((sq._codes.cpu().numpy() == codes).all()),
                   "part_ids_equal": bool((sq.part_ids.cpu().numpy().view(np.uint32) == part).all()),
                   "ids_equal": bool((gi == oi).all()),
                   "distance_bits_equal": bool((gd.view(np.uint32) == od.view(np.uint32)).all()),
                   "cpu_seconds": time.perf_counter() - t0}
    rec["spec"]["equal"] = all(rec["spec"][key] for key in ("codes_equal", "part_ids_equal", "ids_equal", "distance_bits_equal"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
