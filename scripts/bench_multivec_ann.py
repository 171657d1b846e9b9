"""Multivector ANN search (IvfPqMultivectorIndex.nearest) on the column of scripts/bench_multivec.py's shape: 100,000 rows of 32..96
vectors, d = 128, float32, cosine; IVF_PQ over its ~6.4 M flattened vectors; 32-vector queries, k = 10, overfetch 10
-> profiles/multivec_ann.json.  Not part of bench.py.  Needs an MI355X: there is no CPU fallback.

The rows are clustered (every row draws its vectors around one of `--topics` directions) so that recall means something; a query is
32 vectors of a row plus noise.  Reported for nprobes in {1, 10, 50} and batches of 1 and 64 queries:
  * ms per nearest() call without a refine factor: the host clock around the synchronous call (warm-up + reps), per call and per query;
  * the library's stage timers (HIP events on the context's stream; timing on, a separate loop -- timing forces the search's
    un-captured path): the IVF_PQ search of all query vectors, the sort of the lists, the scoring, the selection; and for
    refine_factor = 5 the exact scan + selection of the re-rank and the host clock of the whole call;
  * multivector_flat_knn on the same column in the same run: the yardstick (context, not a threshold);
  * recall@10 against that exact answer over `--recall-queries` queries at refine_factor None / 5."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = (("search", "multivec_ann_search"), ("sort", "multivec_ann_sort"), ("score", "multivec_ann_score"), ("select", "multivec_ann_select"),
          ("rerank_scan", "multivec_scan"), ("rerank_select", "multivec_select"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--min-len", type=int, default=32)
    ap.add_argument("--max-len", type=int, default=96)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--topics", type=int, default=2000)
    ap.add_argument("--nqv", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--overfetch", type=int, default=10)
    ap.add_argument("--partitions", type=int, default=2048)
    ap.add_argument("--sub-vectors", type=int, default=16)
    ap.add_argument("--max-iters", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--recall-queries", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multivec_ann.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multivec_ann.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd

    eng = lance_amd.default_engine()
    dev = torch.device("cuda", torch.cuda.current_device())
    lens = np.random.default_rng(1).integers(a.min_len, a.max_len + 1, a.rows).astype(np.int64)
    off = np.zeros(a.rows + 1, np.int64)
    off[1:] = np.cumsum(lens)
    total = int(off[-1])
    g = torch.Generator(device=dev)
    g.manual_seed(2)
    topics = torch.randn((a.topics, a.d), generator=g, device=dev)
    row_topic = torch.randint(0, a.topics, (a.rows,), generator=g, device=dev)
    values = topics[torch.repeat_interleave(row_topic, torch.from_numpy(lens).to(dev))]
    values += 0.6 * torch.randn((total, a.d), generator=g, device=dev)
    nq = max(64, a.recall_queries)
    qrows = torch.randint(0, a.rows, (nq,), generator=g, device=dev).cpu().numpy()
    offd = torch.from_numpy(off).to(dev)
    queries = [(values[int(off[r]):int(off[r]) + a.nqv] + 0.3 * torch.randn((a.nqv, a.d), generator=g, device=dev)).contiguous() for r in qrows]
    torch.cuda.synchronize()

    t0 = time.perf_counter()
    idx = lance_amd.create_multivector_index(values, offd, num_partitions=a.partitions, num_sub_vectors=a.sub_vectors, max_iters=a.max_iters)
    torch.cuda.synchronize()
    build_s = time.perf_counter() - t0
    record = {"shape": {"rows": a.rows, "row_lengths": [a.min_len, a.max_len], "total_vectors": total, "d": a.d, "topics": a.topics, "nqv": a.nqv,
                        "k": a.k, "overfetch": a.overfetch, "partitions": a.partitions, "sub_vectors": a.sub_vectors},
              "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "index_build_s": build_s, "runs": []}

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        w0 = time.perf_counter()
        for _ in range(a.reps):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - w0) / a.reps * 1e3

    def stages(fn):
        eng.timing(True)
        fn()
        for _, name in STAGES:
            eng.timing_query(name)                     # drain
        for _ in range(a.reps):
            fn()
        out = {label: eng.timing_query(name)[0] / a.reps for label, name in STAGES}
        eng.timing(False)
        return out

    # the yardstick: the exact flat scan, one query per call
    flat_ms = timed(lambda: lance_amd.multivector_flat_knn(values, off, queries[0], a.k, "cosine"))
    record["flat_knn_ms_per_query"] = flat_ms
    print("flat", flat_ms, flush=True)

    for nprobes in (1, 10, 50):
        for batch in (1, 64):
            q = queries[0] if batch == 1 else queries[:64]
            run = {"nprobes": nprobes, "batch": batch}
            run["call_ms_host_clock"] = timed(lambda: idx.nearest(q, k=a.k, nprobes=nprobes, overfetch=a.overfetch))
            run["ms_per_query"] = run["call_ms_host_clock"] / batch
            run["stage_ms_hip_events"] = stages(lambda: idx.nearest(q, k=a.k, nprobes=nprobes, overfetch=a.overfetch))
            run["rf5_call_ms_host_clock"] = timed(lambda: idx.nearest(q, k=a.k, nprobes=nprobes, overfetch=a.overfetch, refine_factor=5))
            run["rf5_stage_ms_hip_events"] = stages(lambda: idx.nearest(q, k=a.k, nprobes=nprobes, overfetch=a.overfetch, refine_factor=5))
            run["speedup_over_flat_per_query"] = flat_ms / run["ms_per_query"]
            record["runs"].append(run)
            print(json.dumps(run), flush=True)

    # recall@10 against the exact answer
    exact = [lance_amd.multivector_flat_knn(values, off, q, a.k, "cosine")[0].cpu().numpy() for q in queries[:a.recall_queries]]
    record["recall_at_k"] = {}
    for nprobes in (1, 10, 50):
        for rf in (None, 5):
            ids, _ = idx.nearest(queries[:a.recall_queries], k=a.k, nprobes=nprobes, overfetch=a.overfetch, refine_factor=rf)
            hit = sum(np.intersect1d(ids[i].view(np.int64), exact[i]).size for i in range(a.recall_queries))
            record["recall_at_k"][f"nprobes={nprobes},refine_factor={rf}"] = hit / (a.recall_queries * a.k)
    print(json.dumps(record["recall_at_k"]), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"out": a.out}))


if __name__ == "__main__":
    main()
