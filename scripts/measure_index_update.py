"""Index maintenance at the C2 shape: 1M x 128 f32 rows (lance_amd.testing.sift_like), IVF256, PQ16, L2 -> profiles/index_update_c2.json.
Appends 100,000 rows and remaps 10 % of the ids (half of them deleted).  Not part of bench.py.  Needs an MI355X.

What is recorded, each as the median (and mean, min) of `--reps` calls after `--warmup`: a pair of HIP events around the library call.
Every one of these calls ends in a synchronise of the context's stream, so the interval is the whole call as the host sees it --
allocations, launches, copies of the offsets and the waits included:
  * merge([base, delta])           lance_hip_index_merge
  * remap                          lance_hip_index_remap
  * create over the concatenation  lance_hip_index_create over the concatenated (part ids, codes) columns of base and delta -- the only
                                   device route before these calls existed, open only to a caller that still holds the columns (the
                                   concatenation itself is made once, outside the clock)
and for merge / remap the copy kernels' own time (the library's per-kernel timers) next to the bytes they move and the device-copy
bandwidth this GPU reaches (lance_hip_ubench 3, read + written).  The merged index is compared with the re-created one row for row before anything
is timed.
"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--append", type=int, default=100_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=256)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_update_c2.json"))
    a = ap.parse_args()

    import torch
    if not torch.cuda.is_available():
        raise SystemExit("measure_index_update.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    from lance_amd import _lib
    from lance_amd.engine import DeviceIndex, Engine, to_device
    from lance_amd.testing import sift_like

    eng = Engine(use_torch_stream=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = sift_like(a.rows + a.append, a.d, seed=1, device=dev)
    base = lance_amd.create_index(x[:a.rows], "IVF_PQ", metric="l2", num_partitions=a.nlist, num_sub_vectors=a.m, max_iters=10,
                                  keep_raw=False, engine=eng)
    ix = base._ix
    part_new, codes_new, _ = eng.ivfpq_encode(x[a.rows:], ix.centroids, ix.codebook, "l2", want_loss=False)
    rid_new = torch.arange(a.rows, a.rows + a.append, dtype=torch.int64, device=dev)
    delta = DeviceIndex.create(eng, "l2", ix.centroids, ix.codebook, part_new, codes_new, rid_new)
    part_all, codes_all = torch.cat([base.part_ids, part_new]), torch.cat([base.codes, codes_new])

    rng = np.random.default_rng(7)
    old = np.sort(rng.choice(a.rows, a.rows // 10, replace=False)).astype(np.uint64)
    new = np.where(rng.random(old.size) < 0.5, np.uint64(_lib.ROW_DELETED), old + np.uint64(1 << 32)).astype(np.uint64)
    old_t, new_t = to_device(old), to_device(new)

    def timed(fn):
        """median / mean / min ms of fn() between two events; fn returns what it built, closed outside the clock"""
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
        return {"median_ms": float(np.median(ms)), "mean_ms": float(np.mean(ms)), "min_ms": float(np.min(ms))}

    def raw_merge():
        arr = (C.c_void_p * 2)(ix.h.value, delta.h.value)
        h = C.c_void_p()
        _lib.check(eng.lib.lance_hip_index_merge(eng.h, arr, 2, C.byref(h)))
        return DeviceIndex(eng, h, "l2", ix.centroids, ix.codebook)

    def raw_remap():
        h = C.c_void_p()
        _lib.check(eng.lib.lance_hip_index_remap(eng.h, ix.h, C.c_void_p(old_t.data_ptr()), C.c_void_p(new_t.data_ptr()), old_t.numel(), C.byref(h)))
        return DeviceIndex(eng, h, "l2", ix.centroids, ix.codebook)

    def raw_create():
        h = C.c_void_p()
        _lib.check(eng.lib.lance_hip_index_create(eng.h, _lib.F32, _lib.L2, a.d, C.c_void_p(ix.centroids.data_ptr()), a.nlist,
                                                  C.c_void_p(ix.codebook.data_ptr()), a.m, 8, C.c_void_p(part_all.data_ptr()),
                                                  C.c_void_p(codes_all.data_ptr()), None, part_all.numel(), C.byref(h)))
        return DeviceIndex(eng, h, "l2", ix.centroids, ix.codebook)

    merged, again = raw_merge(), raw_create()
    same = all(np.array_equal(p, q) for p, q in zip(merged.export_rows(), again.export_rows()))
    n_merged = merged.info()["n"]
    merged.close(); again.close()
    survivors = raw_remap()
    n_remapped = survivors.info()["n"]
    survivors.close()

    rec = {"shape": {"rows": a.rows, "appended": a.append, "d": a.d, "nlist": a.nlist, "m": a.m, "nbits": 8, "metric": "l2", "dtype": "float32",
                     "remapped_ids": int(old.size), "deleted": int((new == np.uint64(_lib.ROW_DELETED)).sum())},
           "device": torch.cuda.get_device_name(0), "warmup": a.warmup, "reps": a.reps,
           "merge_equals_create_over_concatenation": bool(same), "rows_after_merge": int(n_merged), "rows_after_remap": int(n_remapped)}
    rec["merge"] = timed(raw_merge)
    rec["remap"] = timed(raw_remap)
    rec["create_over_concatenation"] = timed(raw_create)

    # the copy kernels alone, and what they move (read + written): codes and row ids
    row_bytes = a.m + 8
    eng.timing(True)
    for name, fn, rows in (("merge", raw_merge, n_merged), ("remap", raw_remap, n_remapped)):
        eng.timing_query("index_update_copy")
        reps = 5
        for _ in range(reps):
            fn().close()
        eng.synchronize()
        ms, launches = eng.timing_query("index_update_copy")
        moved = 2 * rows * row_bytes
        rec[name]["copy_kernels_ms"] = ms / reps
        rec[name]["copy_kernel_launches"] = launches // reps
        rec[name]["bytes_moved"] = int(moved)
        rec[name]["copy_GBps"] = moved / (ms / reps * 1e-3) / 1e9 if ms else None
    eng.timing(False)
    rec["device_copy_GBps_ubench"] = eng.ubench("copy") / 1e9
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(rec, fh, indent=1)
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
