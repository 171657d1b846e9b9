"""Batched multivector flat KNN (lance_hip_flat_multivec_topk_batch, lance_amd/csrc/multivec_batch.hip) at bench_multivec.py's shape:
B = 1, 8 and 64 queries of 32 vectors against 100,000 rows of 32..96 vectors, d = 128, cosine, k = 10, on float32 and float16 columns
-> profiles/multivec_flat_batch.json.  Not part of bench.py.  Needs an MI355X: there is no CPU fallback.

Per column type and B, in `rounds` rounds that ALTERNATE the two in the same run:
  * the batch call: ms per query by the host clock around the synchronous call, and the library's HIP-event stage times
    (multivec_mc_planes: the column's bf16 planes, once per call; multivec_mc_filter: query planes, the matrix-core surrogate, the
    threshold and the survivor lists; multivec_mc_eval: the exact arithmetic on the survivors; multivec_mc_select);
  * a loop of B single-query calls (lance_hip_flat_multivec_topk, the code from before the batch route): ms per query, host clock;
  * the spread of both over the rounds (min .. max), survivors per query, whether ids and distance bits are equal between the two;
  * the surrogate's share of the 2.5 PFLOP/s dense bf16 peak (three products per pair, K = 128 per product) and the bytes the call
    must move (the column read once, the planes written once and read once per column group) against 8 TB/s, and which of the two
    bounds is the larger."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_BF16_FLOPS = 2.5e15
PEAK_HBM_BYTES = 8.0e12
STAGES = ("multivec_mc_planes", "multivec_mc_filter", "multivec_mc_eval", "multivec_mc_select")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000)
    ap.add_argument("--min-len", type=int, default=32)
    ap.add_argument("--max-len", type=int, default=96)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nqv", type=int, default=32)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", default="1,8,64")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multivec_flat_batch.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_multivec_batch.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    import multivec_batch_spec as BS
    import multivec_spec as M
    from lance_amd.engine import to_device

    eng = lance_amd.default_engine()
    lens = M.lengths(a.rows, a.min_len, a.max_len, 1)
    off = M.offsets_of(lens)
    total = int(off[-1])
    rng = np.random.default_rng(2)
    base = rng.standard_normal((total, a.d), dtype=np.float32)
    batches = [int(b) for b in a.batches.split(",")]
    qbase = rng.standard_normal((max(batches) * a.nqv, a.d), dtype=np.float32)
    kpad = BS.kpad(a.d)
    record = {"shape": {"rows": a.rows, "row_lengths": [a.min_len, a.max_len], "total_vectors": total, "d": a.d, "nqv": a.nqv, "k": a.k,
                        "metric": "cosine"},
              "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "rounds": a.rounds, "margin_E": BS.margin(a.nqv, a.d), "runs": {}}
    for kind in ("f32", "f16"):
        values = base * np.float32(3) if kind == "f32" else (base * np.float32(0.7)).astype(np.float16)
        qall = qbase * np.float32(3) if kind == "f32" else (qbase * np.float32(0.7)).astype(np.float16)
        vd = to_device(values)
        esz = 4 if kind == "f32" else 2
        for nb in batches:
            qd = to_device(qall[:nb * a.nqv])
            qoff = np.arange(nb + 1, dtype=np.int64) * a.nqv

            def batch():
                return eng.multivec_topk_batch(vd, off, qd, qoff, a.k, "cosine", return_survivors=True)

            def loop():
                out = [eng.multivec_topk(vd, off, qd[b * a.nqv:(b + 1) * a.nqv], a.k, "cosine") for b in range(nb)]
                eng.synchronize()
                return out
            for _ in range(a.warmup):
                batch(); loop()
            bt, lt = [], []
            stage = {s: 0.0 for s in STAGES}
            for _ in range(a.rounds):
                eng.timing(True)
                s0 = {s: eng.timing_query(s)[0] for s in STAGES}
                w = time.perf_counter()
                ids, dists, surv = batch()
                eng.synchronize()
                bt.append((time.perf_counter() - w) * 1e3 / nb)
                for s in STAGES:
                    stage[s] += (eng.timing_query(s)[0] - s0[s]) / a.rounds
                eng.timing(False)
                w = time.perf_counter()
                single = loop()
                lt.append((time.perf_counter() - w) * 1e3 / nb)
            gi, gd = ids.cpu().numpy(), dists.cpu().numpy().view(np.uint32)
            same = all((single[b][0].cpu().numpy() == gi[b]).all() and (single[b][1].cpu().numpy().view(np.uint32) == gd[b]).all() for b in range(nb))
            cols = nb * a.nqv
            groups = -(-(-(-cols // 32)) // 4)
            flops = total * cols * kpad * 2 * 3
            nbytes = total * a.d * esz + total * kpad * 4 * (1 + groups)
            filt_s = stage["multivec_mc_filter"] * 1e-3
            run = {"batch_ms_per_query": float(np.median(bt)), "batch_ms_per_query_min_max": [min(bt), max(bt)],
                   "loop_ms_per_query": float(np.median(lt)), "loop_ms_per_query_min_max": [min(lt), max(lt)],
                   "batch_faster": bool(max(bt) < min(lt)), "speedup_median": float(np.median(lt) / np.median(bt)),
                   "stage_ms_per_call_hip_events": stage, "survivors_per_query": [int(surv.min()), float(surv.mean()), int(surv.max())],
                   "ids_and_bits_equal_to_single_calls": bool(same),
                   "surrogate_flop": flops, "fraction_of_bf16_peak": flops / PEAK_BF16_FLOPS / filt_s,
                   "bytes_moved": nbytes, "fraction_of_hbm_peak": nbytes / PEAK_HBM_BYTES / ((stage["multivec_mc_planes"] + stage["multivec_mc_filter"]) * 1e-3),
                   "bound": "bf16 matrix rate" if flops / PEAK_BF16_FLOPS > nbytes / PEAK_HBM_BYTES else "HBM"}
            record["runs"][f"{kind}_B{nb}"] = run
            print(kind, nb, json.dumps(run), flush=True)
        del vd
        torch.cuda.empty_cache()
    record["all_equal"] = all(r["ids_and_bits_equal_to_single_calls"] for r in record["runs"].values())
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(record, fh, indent=1)
        fh.write("\n")
    print(json.dumps({"out": a.out, "all_equal": record["all_equal"]}))


if __name__ == "__main__":
    main()
