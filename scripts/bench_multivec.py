"""Multivector (late-interaction) flat KNN: one 32-vector query against 100,000 rows of 32..96 vectors, d = 128, cosine, k = 10,
on float32 and float16 columns -> profiles/multivec_flat.json.  Not part of bench.py.  Needs an MI355X: there is no CPU fallback.

What is reported, per column type:
  * ms per lance_hip_flat_multivec_topk call: HIP events on the context's stream around the scan and around the selection
    (the library's own timers), and the host clock around the whole synchronous call; warm-up and repetition counts;
  * pair evaluations per second (total vectors x query vectors over the scan's time);
  * the share of the 157.3 TFLOP/s f32 vector peak, counting a non-fused sub / mul / add per element and pair (3 * d per pair);
  * the bytes the scan must read (the column once, the offsets) over its time, against 8 TB/s of HBM;
  * the CPU leg: the specification of tests/multivec_spec.py (the oracle's distance_batch per query vector, a segmented max, the
    sequential sum) timed on the host's cores, and whether the GPU's ids equal its ids.
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

PEAK_F32_FLOPS = 157.3e12
PEAK_HBM_BYTES = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--min-len", type=int, default=32)
    ap.add_argument("--max-len", type=int, default=96)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nqv", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metric", default="cosine")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multivec_flat.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multivec.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    import multivec_spec as M
    import oracle
    from lance_amd.engine import to_device

    eng = lance_amd.default_engine()
    lens = M.lengths(a.rows, a.min_len, a.max_len, 1)
    off = M.offsets_of(lens)
    total = int(off[-1])
    rng = np.random.default_rng(2)
    base = rng.standard_normal((total, a.d), dtype=np.float32)
    qbase = rng.standard_normal((a.nqv, a.d), dtype=np.float32)
    record = {"shape": {"rows": a.rows, "row_lengths": [a.min_len, a.max_len], "total_vectors": total, "d": a.d, "nqv": a.nqv, "k": a.k,
                        "metric": a.metric},
              "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "cpu_threads": oracle.num_threads(), "runs": {}}
    for kind in ("f32", "f16"):
        values = base * np.float32(3) if kind == "f32" else (base * np.float32(0.7)).astype(np.float16)
        q = qbase * np.float32(3) if kind == "f32" else (qbase * np.float32(0.7)).astype(np.float16)
        vd, qd = to_device(values), to_device(q)
        for _ in range(a.warmup):
            ids, dists = eng.multivec_topk(vd, off, qd, a.k, a.metric)
        eng.timing(True)
        s0, n0 = eng.timing_query("multivec_scan")
        t0, _ = eng.timing_query("multivec_select")
        w0 = time.perf_counter()
        for _ in range(a.reps):
            ids, dists = eng.multivec_topk(vd, off, qd, a.k, a.metric)
        wall_ms = (time.perf_counter() - w0) / a.reps * 1e3
        s1, n1 = eng.timing_query("multivec_scan")
        t1, _ = eng.timing_query("multivec_select")
        eng.timing(False)
        assert n1 - n0 == a.reps
        scan_ms, select_ms = (s1 - s0) / a.reps, (t1 - t0) / a.reps
        gi, gd = ids.cpu().numpy().view(np.uint64), dists.cpu().numpy()
        del vd
        torch.cuda.empty_cache()
        c0 = time.perf_counter()
        oi, od = M.topk(M.distances(oracle, values, off, q, a.metric), a.k)
        cpu_ms = (time.perf_counter() - c0) * 1e3
        pairs = total * a.nqv
        esz = 4 if kind == "f32" else 2
        nbytes = total * a.d * esz + off.nbytes
        t_flop, t_byte = pairs * a.d * 3 / PEAK_F32_FLOPS, nbytes / PEAK_HBM_BYTES
        run = {"scan_ms_hip_events": scan_ms, "select_ms_hip_events": select_ms, "call_ms_host_clock": wall_ms,
               "pair_evaluations": pairs, "pair_evaluations_per_s": pairs / (scan_ms * 1e-3),
               "flop_per_pair": a.d * 3, "tflops": pairs * a.d * 3 / (scan_ms * 1e-3) / 1e12,
               "fraction_of_f32_vector_peak": t_flop / (scan_ms * 1e-3),
               "bytes_read": nbytes, "read_tb_per_s": nbytes / (scan_ms * 1e-3) / 1e12, "fraction_of_hbm_peak": t_byte / (scan_ms * 1e-3),
               "bound": "f32 vector rate" if t_flop > t_byte else "HBM",
               "cpu_ms": cpu_ms, "speedup_over_cpu": cpu_ms / wall_ms,
               "ids_equal": bool((gi == oi).all()), "distance_bits_equal": bool((gd.view(np.uint32) == od.view(np.uint32)).all())}
        record["runs"][kind] = run
        print(kind, json.dumps(run), flush=True)
    record["ids_equal"] = all(r["ids_equal"] for r in record["runs"].values())
    record["gpu_faster_than_cpu"] = all(r["call_ms_host_clock"] < r["cpu_ms"] for r in record["runs"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"out": a.out, "ids_equal": record["ids_equal"], "gpu_faster_than_cpu": record["gpu_faster_than_cpu"]}))


if __name__ == "__main__":
    main()
