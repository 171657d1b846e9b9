"""Measurement helper (not a test): batched flat KNN on a float16 column, the f16 matrix-core route (lance_amd/csrc/flat_mfma_f16.hip)
against the routes from before it.  For each shape the same seeded call runs in two fresh child processes, alternated three times: one
with LANCE_HIP_NO_FLAT_F16_MC=1 (with the switch set a call takes the earlier route instruction for instruction: the stand-in for the
parent commit), one with the switch unset.  Each child runs under its own `timeout`; the script stops at the first non-zero exit status.
A child warms up, times a window of CALLS calls ending in a synchronise, then makes one timing run for the queued rows per query.  The
two children's answers must be equal.  Result: profiles/flat_f16_mc.json (ms per call, spread, queued rows per query).

    python scripts/flat_f16_probe.py [--n 1000000] [--nq 1000] [--k 10] [--dims 768,1536] [--metrics cosine,dot,l2]"""
import argparse
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCH = "LANCE_HIP_NO_FLAT_F16_MC"
CALLS, WARMUP, ROUNDS = 20, 3, 3


def child(a):
    sys.path.insert(0, ROOT)
    import time

    import torch

    from lance_amd.engine import Engine
    g = torch.Generator(device="cuda").manual_seed(1234 + a.d)
    centers = torch.randn(256, a.d, device="cuda", generator=g)

    def make(m):      # clustered unit vectors, generated in slices: the f32 intermediate of 1M x 1536 would not be small
        out = torch.empty(m, a.d, device="cuda", dtype=torch.float16)
        for s in range(0, m, 65536):
            e = min(m, s + 65536)
            v = centers[torch.randint(0, 256, (e - s,), device="cuda", generator=g)] + 0.5 * torch.randn(e - s, a.d, device="cuda", generator=g)
            out[s:e] = (v / v.norm(dim=1, keepdim=True)).half()
        return out

    x, q = make(a.n), make(a.nq)
    eng = Engine()
    for _ in range(WARMUP):
        ids, dist = eng.flat_topk(x, q, a.k, a.metric)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(CALLS):
        ids, dist = eng.flat_topk(x, q, a.k, a.metric)
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / CALLS
    eng.timing(True)
    before = (eng.timing_query("count:flat_mfma_f16_queued")[1], eng.timing_query("count:flat_mfma_f16")[1], eng.timing_query("count:flat_repair")[1])
    eng.flat_topk(x, q, a.k, a.metric)
    eng.synchronize()
    after = (eng.timing_query("count:flat_mfma_f16_queued")[1], eng.timing_query("count:flat_mfma_f16")[1], eng.timing_query("count:flat_repair")[1])
    eng.timing(False)
    h = hashlib.sha1(ids.cpu().numpy().tobytes() + dist.cpu().numpy().tobytes()).hexdigest()
    print("RESULT " + json.dumps({"ms": ms, "sha1": h, "queued_per_query": (after[0] - before[0]) / a.nq, "mc_epochs": after[1] - before[1],
                                  "repairs": after[2] - before[2]}), flush=True)
    eng.close()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--child", action="store_true")
    p.add_argument("--n", type=int, default=1_000_000)
    p.add_argument("--nq", type=int, default=1000)
    p.add_argument("--k", type=int, default=10)
    p.add_argument("--d", type=int, default=768)
    p.add_argument("--metric", default="cosine")
    p.add_argument("--dims", default="768,1536")
    p.add_argument("--metrics", default="cosine,dot,l2")
    p.add_argument("--child-timeout", type=int, default=120)
    p.add_argument("--out", default=os.path.join(ROOT, "profiles", "flat_f16_mc.json"))
    a = p.parse_args()
    if a.child:
        return child(a)
    rows = []
    for d in (int(v) for v in a.dims.split(",")):
        for metric in a.metrics.split(","):
            runs = {"before": [], "after": []}
            for _ in range(ROUNDS):
                for name in ("before", "after"):
                    env = dict(os.environ)
                    env.pop(SWITCH, None)
                    if name == "before":
                        env[SWITCH] = "1"
                    cmd = ["timeout", "-k", "10", str(a.child_timeout), sys.executable, os.path.abspath(__file__), "--child", "--n", str(a.n),
                           "--nq", str(a.nq), "--k", str(a.k), "--d", str(d), "--metric", metric]
                    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, text=True)
                    if r.returncode != 0:
                        print(f"child {name} d={d} {metric} ended with status {r.returncode}: stopping", flush=True)
                        return r.returncode
                    runs[name].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:]))
            assert len({c["sha1"] for c in runs["before"] + runs["after"]}) == 1, (d, metric, "the two routes' answers differ")
            row = {"n": a.n, "nq": a.nq, "k": a.k, "d": d, "metric": metric}
            for name, cs in runs.items():
                ms = sorted(c["ms"] for c in cs)
                row[name] = {"ms_per_call": ms[len(ms) // 2], "spread": (ms[-1] - ms[0]) / ms[len(ms) // 2], "ms_all": ms}
            row["speedup"] = row["before"]["ms_per_call"] / row["after"]["ms_per_call"]
            row.update({key: runs["after"][0][key] for key in ("queued_per_query", "mc_epochs", "repairs")})
            rows.append(row)
            print(json.dumps(row), flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"calls_per_window": CALLS, "rounds": ROUNDS, "switch": SWITCH, "shapes": rows}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
