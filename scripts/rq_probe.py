"""One measured run of IVF_RQ, with IVF_SQ on the same rows, centroids and parameters as context: 1M x 128 f32 clustered rows
(lance_amd.testing.sift_like), IVF256, L2, 10,000 queries, k = 10, nprobes = 10 -> profiles/rq_probe.json.  Not part of bench.py.
Needs an MI355X.

What is recorded:
  * build seconds per stage (create_index's own stage clocks): train_ivf / transform (partition assignment) / encode /
    build_partitions for IVF_RQ, and IVF_SQ's stages;
  * ms per search call of the whole batch: HIP events on the context's stream around every call, after warm-up, the two indices
    ALTERNATING call by call, median / min / max over the repetitions;
  * the library's per-kernel timers (HIP events around each launch) over 5 more calls, per call;
  * the scan kernel's traffic, counted from the probes of this very batch: every (query, partition) pair reads the partition's code
    bytes and factors once (d / 8 + 8 bytes per row; IVF_SQ: d + 4) -- bytes over the scan kernel's time, against the 6.29 TB/s a
    float4 copy reaches on this device.  Pairs that probe the same partition re-read it, mostly from L2 / Infinity Cache, so this
    is a rate of REQUESTED bytes, not of HBM traffic; `unique_bytes` is what HBM must deliver at least once;
  * recall@10 of both indices against the exhaustive scan on a 1000-query slice (IVF_RQ without re-ranking).
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RQ_TIMERS = ("ivfrq_scan", "ivfrq_merge", "ivfrq_exact")
SQ_TIMERS = ("ivfsq_encode_q", "ivfsq_scan", "ivfsq_merge", "ivfsq_exact")
COPY_TBS = 6.29          # measured float4 copy on an MI355X (8.0 TB/s by specification)


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
    ap.add_argument("--recall-queries", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rq_probe.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("rq_probe.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    from lance_amd.engine import Engine
    from lance_amd.testing import sift_like

    eng = Engine(use_torch_stream=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = sift_like(a.rows, a.d, seed=1, device=dev)
    q = sift_like(max(a.queries, a.recall_queries), a.d, seed=2, device=dev)
    rec = {"shape": {"rows": a.rows, "d": a.d, "nlist": a.nlist, "metric": "l2", "queries": a.queries, "k": a.k, "nprobes": a.nprobes,
                     "dtype": "float32"},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps}

    rq = lance_amd.create_index(x, "IVF_RQ", metric="l2", num_partitions=a.nlist, engine=eng)
    sq = lance_amd.create_index(x, "IVF_SQ", metric="l2", num_partitions=a.nlist, ivf_centroids=rq.centroids, engine=eng)
    rec["build_seconds"] = {"ivf_rq": dict(rq.stats.seconds), "ivf_sq": dict(sq.stats.seconds)}
    rec["bytes_per_row"] = {"ivf_rq": a.d // 8 + 8, "ivf_sq": a.d + 4}

    qb = q[:a.queries].contiguous()
    runs = {"ivf_rq": lambda: rq.search_device(qb, a.k, a.nprobes), "ivf_sq": lambda: sq.search_device(qb, a.k, a.nprobes)}
    for _ in range(a.warmup):
        for run in runs.values():
            run()
    ms = {name: [] for name in runs}
    for _ in range(a.reps):
        for name, run in runs.items():           # alternating: both see the same neighbours on a shared host
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            run()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    rec["search_ms_per_batch"] = {name: {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))} for name, v in ms.items()}
    rec["rq_over_sq"] = rec["search_ms_per_batch"]["ivf_rq"]["median"] / rec["search_ms_per_batch"]["ivf_sq"]["median"]

    rec["kernel_ms_per_call"] = {}
    for name, timers in (("ivf_rq", RQ_TIMERS), ("ivf_sq", SQ_TIMERS)):
        eng.timing(True)
        for t in timers:
            eng.timing_query(t)
        for _ in range(5):
            runs[name]()
        rec["kernel_ms_per_call"][name] = {t: eng.timing_query(t)[0] / 5 for t in timers}
        eng.timing(False)
    runs["ivf_rq"]()
    rec["replayed_share"] = {"ivf_rq": eng.search_stats() / a.queries}
    runs["ivf_sq"]()
    rec["replayed_share"]["ivf_sq"] = eng.search_stats() / a.queries

    # the scan's traffic, from the probes of this batch
    probes = eng.find_partitions(qb, torch.from_numpy(rq.centroids).to(dev), a.nprobes, "l2")[0].cpu().numpy().astype(np.int64)
    sizes = np.bincount(rq.part_ids.cpu().numpy().astype(np.int64).clip(min=-1) + 1, minlength=a.nlist + 1)[1:]
    pair_rows = int(sizes[probes].sum())
    rec["scan"] = {"pairs": int(probes.size), "rows_scanned": pair_rows, "partitions_touched": int(np.unique(probes).size)}
    for name, timer in (("ivf_rq", "ivfrq_scan"), ("ivf_sq", "ivfsq_scan")):
        bpr = rec["bytes_per_row"][name]
        t = rec["kernel_ms_per_call"][name][timer] * 1e-3
        rec["scan"][name] = {"kernel_ms": t * 1e3, "requested_bytes": pair_rows * bpr, "unique_bytes": int(sizes.sum()) * bpr,
                             "requested_tb_per_s": pair_rows * bpr / t / 1e12, "share_of_copy_bandwidth": pair_rows * bpr / t / 1e12 / COPY_TBS,
                             "rows_per_s": pair_rows / t}
    rec["scan"]["note"] = ("one workgroup per (query, partition) pair: a partition's codes are read once per pair, not once per group of "
                           "queries; re-reads of a partition by other pairs are served by L2 / Infinity Cache")

    qr = q[:a.recall_queries].contiguous()
    truth = eng.flat_topk(x, qr, a.k, "l2")[0].cpu().numpy()
    rec["recall_at_k"] = {}
    for name, index in (("ivf_rq", rq), ("ivf_sq", sq)):
        got = index.search_device(qr, a.k, a.nprobes)[0].cpu().numpy()
        rec["recall_at_k"][name] = float(np.mean([len(set(g) & set(t)) / a.k for g, t in zip(got, truth)]))

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
