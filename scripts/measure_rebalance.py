"""The decision of a partition split / join at the C2 shape: 1M x 128 f32 rows (lance_amd.testing.sift_like), IVF256, PQ16, L2, with
`--append` rows appended near one centroid so that its partition passes 4 * 8192 rows -> profiles/rebalance.json.  Not part of bench.py.
Needs an MI355X.  A record, not a gate.

What is recorded, each as the median / min / max of `--reps` calls after `--warmup`, a pair of HIP events around the library call (the
call ends in a synchronise of the context's stream and reads one flag word back, so the interval is the whole call as the host sees it):
  * lance_hip_index_split            the over-full partition split with trained centroids: a new handle (through DeviceIndex.split)
  * lance_hip_index_join             the smallest partition joined into its neighbours: a new handle (through DeviceIndex.join)
  * lance_hip_reassign_rows, split   the decision alone: every visited row's destination (visit order made on the host, outside the clock)
  * lance_hip_reassign_rows, join
and next to them the decision kernel's own time (the library's per-kernel timers), the visited rows, and -- as context, in the same
session -- the only route the library offers to a rebalanced index today: create_index over all rows (training included).
The visit order (ascending row id per partition) and the candidate list are made on the host, outside the clock.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--append", type=int, default=40_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rebalance.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_rebalance.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    from lance_amd import _lib, vector
    from lance_amd.engine import Engine, to_device
    from lance_amd.testing import sift_like

    eng = Engine(use_torch_stream=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = sift_like(a.rows, a.d, seed=1, device=dev)
    base = lance_amd.create_index(x, "IVF_PQ", metric="l2", num_partitions=a.nlist, num_sub_vectors=a.m, max_iters=10, keep_raw=False, engine=eng)
    cent = base._ix.centroids
    sizes0 = np.diff(base.export_rows()[0].astype(np.int64))
    big = int(np.argmax(sizes0))
    # drifted data: rows around one centroid, spread like that partition's own rows
    gen = torch.Generator(device=dev).manual_seed(5)
    own = x[base.part_ids == big]
    spread = (own - cent[big]).std(dim=0)
    new = cent[big] + torch.randn((a.append, a.d), generator=gen, device=dev) * spread
    raw = torch.cat([x, new]).contiguous()
    grown = base.append(new)
    offs, _, ids = grown.export_rows()
    sizes = np.diff(offs.astype(np.int64))
    target = vector.target_partition_size("IVF_PQ")
    part = vector.should_split(sizes, target)
    if part is None:
        raise SystemExit(f"no partition passed {4 * target} rows (largest {sizes.max()}): raise --append")
    small = int(np.argmin(sizes))

    cent_h = cent.cpu().numpy()

    def candidates(p):
        dist = ((cent_h - cent_h[p]) ** 2).sum(axis=1)          # the order only: the library's distances decide nothing here
        order = np.lexsort((np.arange(a.nlist), dist))
        return [int(c) for c in order[:65] if c != p][:64]

    def visit(p, cands):
        pos, seg = [], [0]
        for q in [p] + cands:
            s, e = int(offs[q]), int(offs[q + 1])
            pos.append(s + np.argsort(ids[s:e], kind="stable"))
            seg.append(seg[-1] + e - s)
        return np.concatenate(pos), np.asarray(seg, np.uint32)

    cands = candidates(part)
    pos, seg = visit(part, cands)
    rows_p = raw[to_device(ids[pos[:seg[1]]].astype(np.int64))]
    c12, _, _ = eng.kmeans_train(rows_p, 2, max_iters=50, seed=0)
    split_args = (to_device(ids[pos]), to_device(seg), cent[[part] + cands].contiguous(), to_device(np.asarray(cands, np.uint32)), c12)
    jc = candidates(small)
    jpos, jseg = visit(small, [])
    jseg = np.concatenate([jseg, np.full(len(jc), jseg[-1], np.uint32)])
    join_args = (to_device(ids[jpos]), to_device(jseg), cent[[small] + jc].contiguous(),
                 to_device(np.asarray([c - (c > small) for c in jc], np.uint32)), None)

    def call(args, p1, p2):
        rid, sg, sc, cd, c2 = args
        dest = torch.empty(rid.numel(), dtype=torch.int32, device=dev)
        ptr = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        fn = lambda: _lib.check(eng.lib.lance_hip_reassign_rows(eng.h, _lib.L2, _lib.REASSIGN_JOIN if c2 is None else _lib.REASSIGN_SPLIT,
                                                                 ptr(raw), raw.shape[0], a.d, ptr(rid), rid.numel(), ptr(sg), ptr(sc), ptr(cd),
                                                                 cd.numel(), ptr(c2), p1, p2, ptr(dest)))
        return fn, dest

    def timed(fn):
        ms = []
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}

    rec = {"shape": {"rows": a.rows, "appended": a.append, "d": a.d, "nlist": a.nlist, "m": a.m, "metric": "l2", "dtype": "float32",
                     "target_partition_size": target},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps}
    for name, args, p1, p2 in (("split", split_args, part, a.nlist), ("join", join_args, _lib.NONE, _lib.NONE)):
        fn, dest = call(args, p1, p2)
        rec[name] = timed(fn)
        eng.timing(True)
        eng.timing_query("rebalance_reassign")
        for _ in range(5):
            fn()
        eng.synchronize()
        ms, launches = eng.timing_query("rebalance_reassign")
        eng.timing(False)
        d_h = dest.cpu().numpy().view(np.uint32)
        n_vis = int(args[0].numel())
        rec[name].update({"kernel_ms": ms / 5, "kernel_launches": int(launches // 5), "visited_rows": n_vis, "candidates": int(args[3].numel()),
                          "rows_that_move": int((d_h != _lib.NONE).sum()), "visited_rows_per_s": n_vis / (ms / 5 * 1e-3) if ms else None})
    fn, dest = call(split_args, part, a.nlist)
    fn()
    d_h = dest.cpu().numpy().view(np.uint32)
    rec["split"].update({"partition": int(part), "partition_rows": int(sizes[part]), "to_c1": int((d_h == part).sum()),
                         "to_c2": int((d_h == a.nlist).sum()), "rows_of_p_to_a_candidate": int(np.isin(d_h[:seg[1]], cands).sum())})
    rec["join"].update({"partition": small, "partition_rows": int(sizes[small])})
    # the whole calls: a new handle each time (closed outside the clock)
    def timed_handles(fn):
        ms = []
        for i in range(a.warmup + a.reps):
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = fn()
            e1.record()
            e1.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
            out.close()
        return {"median_ms": float(np.median(ms)), "min_ms": float(np.min(ms)), "max_ms": float(np.max(ms))}

    gix = grown._ix
    rec["index_split"] = timed_handles(lambda: gix.split(part, c12, raw))
    rec["index_join"] = timed_handles(lambda: gix.join(small, raw))
    after = gix.split(part, c12, raw)
    sizes_after = np.diff(after.export_rows()[0].astype(np.int64))
    rec["index_split"].update({"rows": int(sizes_after.sum()), "nlist_after": int(sizes_after.size), "largest_partition_before": int(sizes.max()),
                               "largest_partition_after": int(sizes_after.max()), "rows_of_part_after": int(sizes_after[part]),
                               "rows_of_new_partition": int(sizes_after[-1])})
    after.close()
    after = gix.join(small, raw)
    sizes_after = np.diff(after.export_rows()[0].astype(np.int64))
    rec["index_join"].update({"rows": int(sizes_after.sum()), "nlist_after": int(sizes_after.size), "smallest_partition_before": int(sizes.min()),
                              "smallest_partition_after": int(sizes_after.min())})
    after.close()
    # context: the route that exists today to an index whose partitions fit the data again
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    again = lance_amd.create_index(raw, "IVF_PQ", metric="l2", num_partitions=a.nlist + 1, num_sub_vectors=a.m, max_iters=10, keep_raw=False,
                                   engine=eng)
    torch.cuda.synchronize()
    rec["create_index_over_all_rows_ms"] = (time.perf_counter() - t0) * 1e3
    rec["create_index_largest_partition"] = int(np.diff(again.export_rows()[0].astype(np.int64)).max())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
