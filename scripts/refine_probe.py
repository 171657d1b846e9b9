"""One measured run of IVF_RQ and IVF_SQ searches with and without re-ranking, on scripts/rq_probe.py's shape and protocol: 1M x 128 f32
clustered rows (lance_amd.testing.sift_like), IVF256, L2, 10,000 queries, k = 10, nprobes = 10 -> profiles/refine_probe.json.  Not part
of bench.py.  Needs an MI355X.

What is recorded, for both index types and refine_factor in {none, 1, 5, 10, 50} (keff = 10, 50 and 100 run the scan / merge / replay of
pair_cand.cuh at the capacity of keff <= 128, 500 at the wide one):
  * ms per search call of the whole batch: HIP events on the context's stream around every call, 3 warm-up + 15 timed calls, the
    configurations ALTERNATING call by call, median / min / max;
  * the library's per-kernel timers over 3 more calls, per call, grouped into scan / merge / replay / refine (IVF_SQ: + the query encode);
  * the share of queries replayed through the heap;
  * recall@10 against the exhaustive scan on a 1000-query slice;
  * the candidate buffer's capacity and LDS bytes of the wide scan at this d.
The column is integer-valued (SIFT-like), so the refine reads the index's lossless u8 copy (refine_u8_kernel).

--parent-lib PATH: a liblance_hip.so built from the parent commit.  The unrefined search and refine_factor 5, 10 (keff <= 128) and 50 (above)
of both index types are then measured through both libraries in this process, each called through ctypes alone (the same rows, codes,
centroids, raw column and stream, outputs allocated once; their batches alternating), with each library's per-kernel timers, and their
answers (ids, distance bits) and replay counts are compared.  A keff <= 128 row passes when the new median is at most 3 % above the
parent's (instruction-identical kernels measured 3.0 % apart under this protocol).  --parent-first creates the parent's
context and index handles before this build's -- the control for allocation order -- and only adds that comparison to the record.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

GROUPS = {
    "ivf_rq": {"scan": ("ivfrq_scan", "ivfrq_wide_scan"), "merge": ("ivfrq_merge", "ivfrq_wide_merge"), "replay": ("ivfrq_exact", "ivfrq_wide_exact"),
               "refine": ("refine",)},
    "ivf_sq": {"encode_q": ("ivfsq_encode_q",), "scan": ("ivfsq_scan", "ivfsq_wide_scan"), "merge": ("ivfsq_merge", "ivfsq_wide_merge"),
               "replay": ("ivfsq_exact", "ivfsq_wide_exact"), "refine": ("refine",)},
}
FACTORS = (0, 1, 5, 10, 50)


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


def wide_cap(fixed):
    cap = 1024
    while fixed + cap * 16 <= 65536:
        cap *= 2
    return cap


PARENT_FACTORS = (0, 5, 10, 50)
MARGIN = 1.03


def bare_runs(torch, lib, eng, rq, sq, x, qb, k, nprobes):
    """the searches of one build of the library, called through ctypes alone (no Python wrapper between the events): its own context on
    the torch stream, its own index handles made from the same device arrays, outputs allocated once.
    -> ({"ivf_rq/rf0": run, ...}, (ids, dists), replays(), kernel_ms(run, timer names), what must stay alive)"""
    vp, u64, u32, i32 = C.c_void_p, C.c_uint64, C.c_uint32, C.c_int
    lib.lance_hip_last_error.restype = C.c_char_p
    lib.lance_hip_ctx_create.argtypes = [i32, vp, C.POINTER(vp)]
    lib.lance_hip_ivfrq_create.argtypes = [vp, i32, u32, vp, u32, vp, vp, vp, vp, vp, vp, u64, C.POINTER(vp)]
    lib.lance_hip_ivfsq_create.argtypes = [vp, i32, i32, u32, vp, u32, vp, vp, vp, u64, C.POINTER(C.c_double), C.POINTER(vp)]
    lib.lance_hip_index_set_raw.argtypes = [vp, vp, u64]
    lib.lance_hip_search_stats.argtypes = [vp, C.POINTER(u32)]
    lib.lance_hip_timing_enable.argtypes = [vp, i32]
    lib.lance_hip_timing_query.argtypes = [vp, C.c_char_p, C.POINTER(C.c_double), C.POINTER(u64)]
    for fn in (lib.lance_hip_ivfrq_search, lib.lance_hip_ivfsq_search):
        fn.argtypes = [vp, vp, vp, u32, u32, u32, vp, vp]
    for fn in (lib.lance_hip_ivfrq_search_refine, lib.lance_hip_ivfsq_search_refine):
        fn.argtypes = [vp, vp, vp, u32, u32, u32, u32, vp, u64, vp, vp]

    def ok(rc):
        if rc != 0:
            raise RuntimeError("bare library call: " + lib.lance_hip_last_error().decode())
    p = lambda t: C.c_void_p(t.data_ptr())
    ctx = vp()
    ok(lib.lance_hip_ctx_create(eng.device, vp(torch.cuda.current_stream(eng.device).cuda_stream), C.byref(ctx)))
    n, d = x.shape
    cent, rot = rq._ix.centroids, rq._ix.rotation
    part, dvc = eng.assign(x, cent, "l2")
    codes, add, scale = eng.rq_encode(x, part, dvc, cent, rot, "l2")
    torch.cuda.synchronize()
    hrq, hsq = vp(), vp()
    ok(lib.lance_hip_ivfrq_create(ctx, 0, d, p(cent), cent.shape[0], p(rot), p(codes), p(add), p(scale), p(part), None, n, C.byref(hrq)))
    b = (C.c_double * 2)(*sq.bounds)
    ok(lib.lance_hip_ivfsq_create(ctx, 0, 0, d, p(sq._ix.centroids), cent.shape[0], p(sq._codes), p(sq.part_ids), None, n, b, C.byref(hsq)))
    ok(lib.lance_hip_index_set_raw(hrq, p(x), n))
    ok(lib.lance_hip_index_set_raw(hsq, p(x), n))
    nq = qb.shape[0]
    ids = torch.empty((nq, k), dtype=torch.int64, device=qb.device)
    dists = torch.empty((nq, k), dtype=torch.float32, device=qb.device)
    torch.cuda.synchronize()
    runs = {}
    for name, h, plain, refined in (("ivf_rq", hrq, lib.lance_hip_ivfrq_search, lib.lance_hip_ivfrq_search_refine),
                                    ("ivf_sq", hsq, lib.lance_hip_ivfsq_search, lib.lance_hip_ivfsq_search_refine)):
        runs[name + "/rf0"] = lambda h=h, plain=plain: ok(plain(ctx, h, p(qb), nq, k, nprobes, p(ids), p(dists)))
        for rf in PARENT_FACTORS[1:]:
            runs["%s/rf%d" % (name, rf)] = lambda h=h, refined=refined, rf=rf: ok(refined(ctx, h, p(qb), nq, k, nprobes, rf, None, 0, p(ids), p(dists)))

    def replays():
        cnt = u32(0)
        ok(lib.lance_hip_search_stats(ctx, C.byref(cnt)))
        return cnt.value

    def kernel_ms(run, groups, calls=3):
        def query(t):
            ms, cnt = C.c_double(0), u64(0)
            ok(lib.lance_hip_timing_query(ctx, t.encode(), C.byref(ms), C.byref(cnt)))      # a query resets the timer
            return ms.value
        ok(lib.lance_hip_timing_enable(ctx, 1))
        for ts in groups.values():
            for t in ts:
                query(t)
        for _ in range(calls):
            run()
        out = {g: sum(query(t) for t in ts) / calls for g, ts in groups.items()}
        ok(lib.lance_hip_timing_enable(ctx, 0))
        return out
    keep = (lib, ctx, hrq, hsq, codes, add, scale, part, ids, dists)
    return runs, (ids, dists), replays, kernel_ms, keep


def compare_with_parent(torch, a, eng, rq, sq, x, qb):
    """both builds through the same bare ctypes calls: a second handle of THIS build (another path to the same file would be the same
    handle; the copy is removed again) and the parent's"""
    import shutil
    import tempfile
    from lance_amd import _lib
    tmp = tempfile.mkdtemp()
    mine = shutil.copy(_lib.LIB_PATH, os.path.join(tmp, "liblance_hip_new.so"))
    made = {}
    for who in (("parent", "new") if a.parent_first else ("new", "parent")):
        made[who] = bare_runs(torch, C.CDLL(mine if who == "new" else a.parent_lib), eng, rq, sq, x, qb, a.k, a.nprobes)
    both = {"%s/%s" % (who, name): made[who][0][name] for name in made["new"][0] for who in made}
    ms = timed_alternating(torch, both, a.warmup, a.reps)
    out = {"protocol": "both builds called through ctypes with preallocated outputs, batches alternating; contexts and handles of the %s build "
                       "created first" % ("parent" if a.parent_first else "new"), "margin": MARGIN}
    for name in made["new"][0]:
        row = {}
        for who, (runs, (ids, dists), replays, kernel_ms, _) in made.items():
            runs[name]()
            torch.cuda.synchronize()
            row[who] = dict(stats(ms["%s/%s" % (who, name)]), replays=replays(), answer=(ids.clone(), dists.clone()),
                            kernel_ms_per_call=kernel_ms(runs[name], GROUPS[name.split("/")[0]]))
        (ni, nd), (oi, od) = row["new"].pop("answer"), row["parent"].pop("answer")
        row["same_answer"] = bool((ni == oi).all() and (nd.view(torch.int32) == od.view(torch.int32)).all())
        row["same_replays"] = row["new"]["replays"] == row["parent"]["replays"]
        row["new_over_parent"] = row["new"]["median"] / row["parent"]["median"]
        row["within_margin"] = row["new_over_parent"] <= MARGIN
        out[name] = row
    made.clear()
    shutil.rmtree(tmp, ignore_errors=True)
    return out


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
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-first", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_probe.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("refine_probe.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    from lance_amd.engine import Engine
    from lance_amd.testing import sift_like

    eng = Engine(use_torch_stream=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = sift_like(a.rows, a.d, seed=1, device=dev)
    q = sift_like(max(a.queries, a.recall_queries), a.d, seed=2, device=dev)
    rec = {"shape": {"rows": a.rows, "d": a.d, "nlist": a.nlist, "metric": "l2", "queries": a.queries, "k": a.k, "nprobes": a.nprobes,
                     "dtype": "float32"},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps, "refine_factors": list(FACTORS)}
    rq = lance_amd.create_index(x, "IVF_RQ", metric="l2", num_partitions=a.nlist, engine=eng)
    sq = lance_amd.create_index(x, "IVF_SQ", metric="l2", num_partitions=a.nlist, ivf_centroids=rq.centroids, engine=eng)
    index = {"ivf_rq": rq, "ivf_sq": sq}
    ld = (a.d + 15) // 16 * 16
    rec["wide_scan"] = {"ivf_rq": {"capacity": wide_cap(20 * a.d + 40), "lds_bytes": 20 * a.d + 40 + 8 * wide_cap(20 * a.d + 40)},
                        "ivf_sq": {"capacity": wide_cap(ld + 16), "lds_bytes": ld + 16 + 8 * wide_cap(ld + 16)}}

    qb = q[:a.queries].contiguous()
    if a.parent_first:
        assert a.parent_lib, "--parent-first needs --parent-lib"
        with open(a.out) as fh:                      # the record of the run without --parent-first: only the comparison is added
            rec = json.load(fh)
    else:
        runs = {"%s/rf%d" % (name, rf): (lambda ix=ix, rf=rf: ix.search_device(qb, a.k, a.nprobes, refine_factor=rf))
                for name, ix in index.items() for rf in FACTORS}
        ms = timed_alternating(torch, runs, a.warmup, a.reps)
        rec["search_ms_per_batch"] = {name: stats(v) for name, v in ms.items()}

        rec["kernel_ms_per_call"], rec["replayed_share"] = {}, {}
        for name, run in runs.items():
            groups = GROUPS[name.split("/")[0]]
            eng.timing(True)
            for ts in groups.values():
                for t in ts:
                    eng.timing_query(t)                  # a query resets the timer
            for _ in range(3):
                run()
            rec["kernel_ms_per_call"][name] = {g: sum(eng.timing_query(t)[0] for t in ts) / 3 for g, ts in groups.items()}
            eng.timing(False)
            run()
            rec["replayed_share"][name] = eng.search_stats() / a.queries

        qr = q[:a.recall_queries].contiguous()
        truth = eng.flat_topk(x, qr, a.k, "l2")[0].cpu().numpy()
        rec["recall_at_k"] = {}
        for name, ix in index.items():
            for rf in FACTORS:
                got = ix.search_device(qr, a.k, a.nprobes, refine_factor=rf)[0].cpu().numpy()
                rec["recall_at_k"]["%s/rf%d" % (name, rf)] = float(np.mean([len(set(g) & set(t)) / a.k for g, t in zip(got, truth)]))

    if a.parent_lib:
        rec.setdefault("vs_parent", {})["parent_first" if a.parent_first else "new_first"] = compare_with_parent(torch, a, eng, rq, sq, x, qb)

    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
