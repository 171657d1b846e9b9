"""Does the distance range cost the un-ranged flat scan anything, and what does a ranged scan cost?  Two built trees -- this one and a
checkout of the parent commit with its liblance_hip.so built (--parent-tree) -- measured ALTERNATING in fresh child processes on the
same device -> profiles/flat_range.json.  Not part of bench.py.  Needs an MI355X.

Shapes: C1 (1M x 128 f32, L2, k = 10) with one query (flat_small.hip) and with 10,000 queries (the short-row matrix-core filter), and
--long: 1000 queries x 1M x 1536, cosine (the long-row matrix-core filter).

Method, per child: lance_amd is imported from the tree under test; HIP events on the context's stream around every call, 3 warm-up and 15
timed calls; median / min / max.  Each tree runs in --repeats (at least three) child processes: the spread of the parent's own medians is
the noise floor, and the un-ranged median of this tree may exceed the parent's by no more than that spread.  The ranged calls are timed in
this tree only (the parent has no such entry): (None, median returned distance), (median of ALL distances, None) and both, recorded
beside the un-ranged figure with no threshold, each with the number of repair rounds (count:flat_repair) its calls took, which must be 0
on these shapes (`repair_free`; the script exits non-zero otherwise), and the number of chunks a lower bound handed from the matrix cores
to the exact filter (count:flat_lower_fallback).  A child that fails ends the run: nothing more is started on the device."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = {
    "c1_one_query": {"rows": 1_000_000, "d": 128, "queries": 1, "k": 10, "metric": "l2"},
    "c1_10000_queries": {"rows": 1_000_000, "d": 128, "queries": 10_000, "k": 10, "metric": "l2"},
    "long_1000_queries": {"rows": 1_000_000, "d": 1536, "queries": 1000, "k": 10, "metric": "cosine"},
}


def stats(v):
    return {"median": float(np.median(v)), "min": float(np.min(v)), "max": float(np.max(v))}


def child(a):
    sys.path.insert(0, os.path.abspath(a.tree) if a.tree else ROOT)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("flat_range_probe.py needs an MI355X: no HIP device is visible and there is no CPU fallback")
    import lance_amd
    from lance_amd.engine import Engine
    from lance_amd.testing import sift_like

    eng = Engine(use_torch_stream=True)
    dev = torch.device("cuda", torch.cuda.current_device())
    has_range = hasattr(eng.lib, "lance_hip_flat_topk_range")
    rec = {"tree": os.path.dirname(os.path.dirname(os.path.abspath(lance_amd.__file__))), "has_range": has_range,
           "device": torch.cuda.get_device_name(0), "shapes": {}}
    x128 = None
    for name in a.shapes.split(","):
        s = SHAPES[name]
        if s["d"] == 128:
            x = x128 = x128 if x128 is not None else sift_like(s["rows"], 128, seed=1, device=dev)
        else:
            x128 = None
            x = torch.randn((s["rows"], s["d"]), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
        if s["d"] == 128:
            qb = sift_like(s["queries"], 128, seed=2, device=dev).contiguous()
        else:
            qb = torch.randn((s["queries"], s["d"]), device=dev, generator=torch.Generator(device=dev).manual_seed(2))
        runs = {"unranged": lambda: eng.flat_topk(x, qb, s["k"], s["metric"])}
        out = {}
        if has_range:
            dists = runs["unranged"]()[1]
            upper = float(dists[torch.isfinite(dists)].median())
            # the median of ALL distances, estimated on a sample of the rows (the matrix is 10,000 x 1M)
            sample = x[torch.randperm(s["rows"], device=dev, generator=torch.Generator(device=dev).manual_seed(3))[:2048]].contiguous()
            every = eng.flat_topk(sample, qb[:64].contiguous(), 1024, s["metric"])[1]      # the 1024 nearest of 2048 sampled rows: the last one is the sample median
            lower = float(every[:, -1].median())
            both_hi = float(eng.flat_topk(x, qb[:64].contiguous(), s["k"], s["metric"], lower=lower)[1].max())
            runs["upper"] = lambda: eng.flat_topk(x, qb, s["k"], s["metric"], upper=upper)
            runs["lower"] = lambda: eng.flat_topk(x, qb, s["k"], s["metric"], lower=lower)
            runs["both"] = lambda: eng.flat_topk(x, qb, s["k"], s["metric"], lower=lower, upper=both_hi)
            out["bounds"] = {"upper": upper, "lower": lower, "both": [lower, both_hi]}
            out["rows_found_share"] = {n: float((runs[n]()[0] != -1).float().mean()) for n in ("upper", "lower", "both")}
        for _ in range(a.warmup):
            for run in runs.values():
                run()
        ms = {n: [] for n in runs}
        repairs = {n: 0 for n in runs}
        fallbacks = {n: 0 for n in runs}      # count:flat_lower_fallback: a lower bound's chunk handed from the matrix cores to the exact filter
        for _ in range(a.reps):
            for n, run in runs.items():
                r0 = eng.timing_query("count:flat_repair")[1] if has_range else 0
                f0 = eng.timing_query("count:flat_lower_fallback")[1] if has_range else 0
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                run()
                e1.record()
                e1.synchronize()
                ms[n].append(e0.elapsed_time(e1))
                repairs[n] += (eng.timing_query("count:flat_repair")[1] - r0) if has_range else 0
                fallbacks[n] += (eng.timing_query("count:flat_lower_fallback")[1] - f0) if has_range else 0
        out["ms_per_call"] = {n: stats(v) for n, v in ms.items()}
        out["repair_rounds"] = repairs if has_range else None      # (the parent keeps no count)
        out["lower_fallbacks"] = fallbacks if has_range else None
        rec["shapes"][name] = out
        del x, qb
    print("PROBE " + json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-tree", help="a checkout of the parent commit with its liblance_hip.so built")
    ap.add_argument("--repeats", type=int, default=3, help="child processes per library, alternating")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--long", action="store_true", help="also 1000 queries x 1M x 1536, cosine (6 GB of rows per child)")
    ap.add_argument("--shapes", help="comma-separated subset of " + ", ".join(SHAPES))
    ap.add_argument("--one", action="store_true", help="measure one tree (--tree, default: this one) and print the record")
    ap.add_argument("--tree")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_range.json"))
    a = ap.parse_args()
    if not a.shapes:
        a.shapes = "c1_one_query,c1_10000_queries" + (",long_1000_queries" if a.long else "")
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
            cmd = [sys.executable, os.path.abspath(__file__), "--one", "--warmup", str(a.warmup), "--reps", str(a.reps), "--shapes", a.shapes]
            if side == "parent":
                cmd += ["--tree", os.path.abspath(a.parent_tree)]
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.child_timeout)
            line = [ln for ln in r.stdout.splitlines() if ln.startswith("PROBE ")]
            if r.returncode != 0 or not line:
                sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
                raise SystemExit(f"the {side} child failed (exit {r.returncode}): nothing more is started")
            recs[side].append(json.loads(line[-1][6:]))
            print(side, json.dumps({n: s["ms_per_call"] for n, s in recs[side][-1]["shapes"].items()}), flush=True)
    out = {"method": "HIP events on the context's stream around each flat_topk call; per child process %d warm-up and %d timed calls; "
                     "%d child processes per library, parent and this tree alternating" % (a.warmup, a.reps, a.repeats),
           "device": recs["this"][0]["device"], "shapes": {}}
    for name in a.shapes.split(","):
        pm = [r["shapes"][name]["ms_per_call"]["unranged"]["median"] for r in recs["parent"]]
        tm = [r["shapes"][name]["ms_per_call"]["unranged"]["median"] for r in recs["this"]]
        spread = max(pm) - min(pm)
        first = recs["this"][0]["shapes"][name]
        out["shapes"][name] = {
            "shape": dict(SHAPES[name], dtype="float32"),
            "unranged_ms_parent_medians": pm, "unranged_ms_this_medians": tm,
            "parent_spread_ms": spread,
            "unranged_ms_parent": float(np.median(pm)), "unranged_ms_this": float(np.median(tm)),
            "excess_ms": float(np.median(tm) - np.median(pm)),
            "within_parent_spread": bool(np.median(tm) - np.median(pm) <= spread),
            "ranged_ms_this": {n: float(np.median([r["shapes"][name]["ms_per_call"][n]["median"] for r in recs["this"]])) for n in ("upper", "lower", "both")},
            "ranged_ms_this_medians": {n: [r["shapes"][name]["ms_per_call"][n]["median"] for r in recs["this"]] for n in ("upper", "lower", "both")},
            "bounds": first["bounds"], "rows_found_share": first["rows_found_share"],
            "repair_rounds": {n: sum(r["shapes"][name]["repair_rounds"][n] for r in recs["this"]) for n in ("unranged", "upper", "lower", "both")},
            "lower_fallbacks": {n: sum(r["shapes"][name]["lower_fallbacks"][n] for r in recs["this"]) for n in ("unranged", "upper", "lower", "both")},
        }
        out["shapes"][name]["repair_free"] = not any(out["shapes"][name]["repair_rounds"].values())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
    print(json.dumps(out))
    bad = [n for n, s in out["shapes"].items() if not s["repair_free"]]
    if bad:
        raise SystemExit("repair rounds on " + ", ".join(bad) + ": count:flat_repair must stay 0 on these shapes")


if __name__ == "__main__":
    main()
