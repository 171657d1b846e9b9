"""Does the distance range cost the un-ranged IVF_FLAT search anything?  Two built trees -- this one and a checkout of the parent
commit with its liblance_hip.so built (--parent-tree) -- measured ALTERNATING in fresh child processes on the same device, and the ranged search's
time for context -> profiles/ivfflat_range.json.  Not part of bench.py.  Needs an MI355X.

Shapes: C2 (1M x 128 f32 clustered rows, lance_amd.testing.sift_like, IVF256, L2, 10,000 queries, k = 10, nprobes = 10: the
partition-major kernels at D = 128) and a small fixed-dimension one (200,000 x 32, IVF64, 4096 queries: D = 32).

Method, per child: lance_amd is imported from the tree under test and the index built with it (the same seeds: the same centroids
in both); HIP events on the context's stream around every search call of the whole batch, after warm-up; median / min / max over the
repetitions.  The parent is repeated --repeats times (at least three): the spread of its own medians is the noise floor, and the
un-ranged median of this tree may exceed the parent's by no more than that spread.  The ranged search is timed at
(None, median of the returned distances), in this tree only (the parent has no such entry point); no threshold applies to it.
A child that fails ends the run: nothing more is started on the device."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {
    "c2": {"rows": 1_000_000, "d": 128, "nlist": 256, "queries": 10_000, "k": 10, "nprobes": 10},
    "small_d32": {"rows": 200_000, "d": 32, "nlist": 64, "queries": 4096, "k": 10, "nprobes": 8},
}


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def child(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ivfflat_range_probe.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    from lance_amd.engine import Engine
    from lance_amd.testing import sift_like

    eng = Engine(use_torch_stream=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    has_range = hasattr(eng.lib, "lance_hip_ivfflat_search_range")
    rec = {"tree": os.path.dirname(os.path.dirname(os.path.abspath(lance_amd.__file__))), "has_range": has_range, "device": torch.cuda.get_device_name(0), "shapes": {}}
    for name, s in SHAPES.items():
        x = sift_like(s["rows"], s["d"], seed=1, device=dev)
        qb = sift_like(s["queries"], s["d"], seed=2, device=dev).contiguous()
        ix = lance_amd.create_index(x, "IVF_FLAT", metric="l2", num_partitions=s["nlist"], max_iters=10, engine=eng)
        runs = {"unranged": lambda: ix._ix.search(qb, s["k"], s["nprobes"])}
        out = {}
        if has_range:
            dists = runs["unranged"]()[1]
            upper = float(dists[torch.isfinite(dists)].median())
            runs["ranged"] = lambda: ix._ix.search(qb, s["k"], s["nprobes"], upper=upper)
            out["ranged_upper"] = upper
            out["ranged_rows_found_share"] = float((runs["ranged"]()[0] != -1).float().mean())
        for _ in range(a.warmup):
            for run in runs.values():
                run()
        ms = {n: [] for n in runs}
        for _ in range(a.reps):
            for n, run in runs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                ms[n].append(e0.elapsed_time(e1))
        out["search_ms_per_batch"] = {n: stats(v) for n, v in ms.items()}
        runs["unranged"]()
        out["replayed_share"] = eng.search_stats() / s["queries"] if has_range else None      # (the parent's IVF_FLAT search keeps no count)
        rec["shapes"][name] = out
        del ix, x, qb
    print("PROBE " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its liblance_hip.so built")
    ap.add_argument("--repeats", type=int, default=3, help="child processes per library, alternating")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--one", action="store_true", help="measure one tree (--tree, default: this one) and print the record")
    ap.add_argument("--tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ivfflat_range.json"))
    a = ap.parse_args()
    if a.one:
        return child(a)
    if not a.parent_tree or not os.path.exists(os.path.join(a.parent_tree, "lance_amd", "liblance_hip.so")):
        raise SystemExit("--parent-tree: check the parent commit out, build its liblance_hip.so and pass the directory")
    if a.repeats < 3:
        raise SystemExit("--repeats: the parent's spread needs at least three repeats")
    recs = {"parent": [], "this": []}
    for _ in range(a.repeats):
        for side in ("parent", "this"):          # alternating: both see the same neighbours on a shared host
            env = dict(os.environ)
            env.pop("LANCE_HIP_LIB", None)
            cmd = [sys.executable, os.path.abspath(__file__), "--one", "--warmup", str(a.warmup), "--reps", str(a.reps)]
            if side == "parent":
                cmd += ["--tree", os.path.abspath(a.parent_tree)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"the {side} child failed (exit {r.returncode}): nothing more is started")
            recs[side].append(json.loads(line[-1][6:]))
            print(side, json.dumps({n: s["search_ms_per_batch"] for n, s in recs[side][-1]["shapes"].items()}), flush=True)
    out = {"method": "HIP events on the context's stream around each search call of the whole batch; per child process %d warm-up and %d "
                     "timed calls; %d child processes per library, parent and this tree alternating" % (a.warmup, a.reps, a.repeats),
           "device": recs["this"][0]["device"], "shapes": {}}
    for name, s in SHAPES.items():
        pm = [r["shapes"][name]["search_ms_per_batch"]["unranged"]["median"] for r in recs["parent"]]
        tm = [r["shapes"][name]["search_ms_per_batch"]["unranged"]["median"] for r in recs["this"]]
        rm = [r["shapes"][name]["search_ms_per_batch"]["ranged"]["median"] for r in recs["this"]]
        spread = max(pm) - min(pm)
        out["shapes"][name] = {
            "shape": dict(s, metric="l2", dtype="float32"),
            "unranged_ms_parent_medians": pm, "unranged_ms_this_medians": tm,
            "parent_spread_ms": spread,
            "unranged_ms_parent": float(np.median(pm)), "unranged_ms_this": float(np.median(tm)),
            "excess_ms": float(np.median(tm) - np.median(pm)),
            "within_parent_spread": bool(np.median(tm) - np.median(pm) <= spread),
            "ranged_ms_this_medians": rm, "ranged_ms_this": float(np.median(rm)),
            "ranged_upper": recs["this"][0]["shapes"][name]["ranged_upper"],
            "ranged_rows_found_share": recs["this"][0]["shapes"][name]["ranged_rows_found_share"],
            "replayed_share_unranged": recs["this"][0]["shapes"][name]["replayed_share"],
        }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
