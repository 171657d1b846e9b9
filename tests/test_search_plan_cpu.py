"""The IVF-PQ search plan (lance_amd/csrc/search_plan.h) on the CPU: the header is compiled alone with g++ (it has no HIP in it) into
tests/c/search_plan_main.cpp, under AddressSanitizer + UBSan where the compiler has them, and asked for plans.

Part one is a table: every row of the decision table in DESIGN.md ("which kernels serve an IVF-PQ search batch"), one probe on each
side of every threshold, every switch -- the expected values are written by hand -- and the cases of tests/golden/search_routes.json,
whose recorded launches must be the ones the predicted route makes.  Part two sweeps shapes and asserts what used to be implicit.
Gates no cheap GPU case reaches (lists of 65,536 rows, the 2 GiB scratch limits, thousands of lists) are covered here only."""
import itertools
import os
import subprocess

import pytest

import search_routes_spec as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L2, COSINE, DOT = 0, 1, 2
F32, F16 = 0, 1
NOT_BUILT, USABLE, UNUSABLE = 0, 1, 2


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("search_plan") / "search_plan")
    base = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "lance_amd", "csrc"),
            os.path.join(ROOT, "tests", "c", "search_plan_main.cpp"), "-o", exe]
    r = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr:      # a g++ without the sanitizer runtimes: the same program without them
        r = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]

    def plan(cases):
        text = "\n".join(" ".join(f"{k}={v}" for k, v in c.items()) for c in cases) + "\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        out = []
        for line in r.stdout.splitlines():
            head, why = line.split(" why=", 1)
            d = dict(t.split("=", 1) for t in head.split())
            d["why"] = why
            out.append(d)
        assert len(out) == len(cases)
        return out
    return plan


def case(**kw):
    """the C2 shape (d 128, M 16, 256 lists, 10^6 rows, largest list 6000) and a 10,000 x 10 batch at k * refine = 100, unless said otherwise"""
    c = dict(metric=L2, dtype=F32, d=128, m=16, nbits=8, nlist=256, n=1000000, max_part=6000, finite=1, cb_mean=1, ms=USABLE,
             nq=10000, nprobes=10, keff=100)
    c.update(kw)
    return c


C3 = dict(d=768, m=96, nlist=256)      # a tiled shape (sd 8)
Q = lambda bound, main, lists=1, class_b="pair": dict(route="quantised", bound=bound, main=main, lists=str(lists), class_b=class_b)
QM8, QM4, PAIR, EXACT = dict(route="qm8"), dict(route="qm4"), dict(route="pair_scan"), dict(route="exact_only")

TABLE = [
    # ---- DESIGN.md, route table ----
    ("row 1: k * refine above the cap", case(keff=129), EXACT),
    ("row 1: at the cap", case(keff=128), Q("matrix", "matrix")),
    ("row 1 comes before row 2 (4-bit)", case(keff=129, nbits=4), EXACT),
    ("row 2: NO_PM", case(no_pm=1), QM8),
    ("row 2: 4-bit codes", case(nbits=4, d=64), QM4),
    ("row 2: distance range", case(range=1), QM8),
    ("row 2: sd = 2", case(d=32), QM8),
    ("row 2: sd = 32", case(d=512), QM8),
    ("row 2: M = 8", case(d=64, m=8), QM8),
    ("row 2: M = 24", case(d=96, m=24), QM8),
    ("row 2: M does not divide d", case(d=130), QM8),
    ("row 2: codes unaligned", case(a_codes=0), QM8),
    ("row 2: codebook unaligned", case(a_codebook=0), QM8),
    ("row 2: 4095 pairs, M = 16", case(nq=4095, nprobes=1, nlist=8), QM8),
    ("row 2: 4096 pairs, M = 16", case(nq=4096, nprobes=1, nlist=8), Q("matrix", "matrix")),
    ("row 2: 2047 pairs, M = 96", case(nq=2047, nprobes=1, **C3), QM8),
    ("row 2: 2048 pairs, M = 96", case(nq=2048, nprobes=1, **C3), Q("pt", "pt", class_b="rescan")),
    ("row 3: NO_QSCAN", case(no_qscan=1), dict(PAIR, pair_bound="1")),
    ("row 3: PM_NOBOUND", case(pm_nobound=1), dict(PAIR, pair_bound="0")),
    ("row 3: model not finite", case(finite=0), PAIR),
    ("row 4: NO_QSCAN, M = 96", case(no_qscan=1, **C3), QM8),
    ("row 4: PM_NOBOUND, M = 96", case(pm_nobound=1, **C3), QM8),
    ("row 4: model not finite, M = 96", case(finite=0, **C3), QM8),
    ("row 5: the bench line", case(), Q("matrix", "matrix")),
    ("row 5: cosine", case(metric=COSINE), Q("matrix", "matrix")),
    # ---- refusals of the quantised flow: the two scratch limits ----
    ("survivor segments at 2 GiB", case(nq=2097152, nprobes=1), Q("matrix", "matrix")),
    ("survivor segments above 2 GiB", case(nq=2097153, nprobes=1), PAIR),
    ("survivor segments above 2 GiB, M = 96", case(nq=2097153, nprobes=1, **C3), QM8),
    # item residuals, integer main pass (d = 256 has no matrix-core scan): (pairs / 4 + 4097) * 256 * 16 <= 2^31 (and pairs <= 2,097,152)
    ("item residuals at 2 GiB", case(d=256, nlist=4096, nq=2080764, nprobes=1, keff=10), Q("integer", "integer")),
    ("item residuals above 2 GiB", case(d=256, nlist=4096, nq=2080768, nprobes=1, keff=10), PAIR),
    # ... which the per-query tables and the matrix-core scan do not read: C3, 10,000 x 100 = (250,000 + 257) * 768 * 16 bytes
    ("item residuals unread by per-query tables", case(nq=10000, nprobes=100, **C3), Q("pt", "pt", class_b="rescan")),
    ("item residuals unread by the matrix-core scan", case(d=128, m=32, nq=2097152, nprobes=1, nlist=16384), Q("matrix", "matrix")),
    ("item residuals read by the tiled scan", case(nq=10000, nprobes=100, qpt=0, **C3), QM8),
    # ---- main pass ----
    ("main: NO_MSCAN", case(no_mscan=1), Q("integer", "integer")),
    ("main: d = 64, M = 16", case(d=64), Q("matrix", "matrix")),
    ("main: d = 128, M = 32", case(m=32), Q("matrix", "matrix")),
    ("main: d = 64, M = 32 is no matrix-core shape", case(d=64, m=32), QM8),
    ("main: d = 256, M = 16", case(d=256), Q("integer", "integer")),
    ("main: d = 256, M = 32", case(d=256, m=32), Q("integer", "integer")),
    ("main: all-zero codebook", case(ms=UNUSABLE), Q("integer", "integer")),
    ("main: constants not built yet", case(ms=NOT_BUILT), dict(Q("matrix", "matrix"), wants_ms="1")),
    ("main: constants built", case(), dict(wants_ms="0")),
    ("main: 95 pairs per list", case(nq=95 * 256, nprobes=1), Q("integer", "integer")),
    ("main: 96 pairs per list", case(nq=96 * 256, nprobes=1), Q("matrix", "matrix")),
    ("main: MSCAN_MINQ = 8", case(nq=8 * 256 * 2, nprobes=1, mscan_minq=8), Q("matrix", "matrix")),
    ("main: thousands of lists (C4: 10,000 x 10 over 4096)", case(nlist=4096), Q("integer", "integer")),
    ("main: per-query tables", case(**C3), Q("pt", "pt", class_b="rescan")),
    ("main: QPT = 1", case(qpt=1, **C3), Q("integer", "pt", class_b="rescan")),
    ("main: QPT = 0", case(qpt=0, **C3), Q("integer", "tiled", class_b="rescan")),
    ("main: f16 column, M = 96", case(dtype=F16, **C3), Q("integer", "tiled", class_b="rescan")),
    ("main: M = 48", case(d=192, m=48), Q("pt", "pt", class_b="rescan")),
    ("main: M = 64, sd 16", case(d=1024, m=64), Q("pt", "pt", class_b="rescan")),
    # ---- bound pass ----
    ("bound: EXACT_BOUND", case(exact_bound=1), Q("exact_pair", "matrix")),
    ("bound: EXACT_BOUND, integer main", case(exact_bound=1, no_mscan=1), Q("exact_pair", "integer")),
    ("bound: EXACT_BOUND has no M = 96 kernel", case(exact_bound=1, **C3), Q("pt", "pt", class_b="rescan")),
    ("bound: NO_MSBOUND", case(no_msbound=1), Q("integer", "matrix")),
    ("bound: no codebook means", case(cb_mean=0), Q("integer", "matrix")),
    ("bound: largest list 65,535 rows", case(max_part=65535), Q("matrix", "matrix")),
    ("bound: largest list 65,536 rows", case(max_part=65536), Q("integer", "matrix")),
    ("bound: queries unaligned", case(a_query=0), Q("integer", "matrix")),
    ("bound: centroids unaligned", case(a_centroids=0), Q("integer", "matrix")),
    ("bound lists: BOUND_LISTS = 2", case(bound_lists=2), Q("matrix", "matrix", lists=2)),
    ("bound lists: BOUND_LISTS = 9 -> 4", case(bound_lists=9), Q("matrix", "matrix", lists=4)),
    ("bound lists: BOUND_LISTS only on the matrix cores", case(bound_lists=2, no_msbound=1), Q("integer", "matrix", lists=1)),
    ("bound lists: BOUND_LISTS, EXACT_BOUND", case(bound_lists=2, exact_bound=1), Q("exact_pair", "matrix", lists=1)),
    ("bound lists: at most nprobes", case(bound_lists=3, nq=50000, nprobes=2), Q("matrix", "matrix", lists=2)),
    # ---- dot ----
    ("dot: the flow", case(metric=DOT), Q("matrix", "matrix", lists=3)),
    ("dot: one probe", case(metric=DOT, nq=100000, nprobes=1), Q("matrix", "matrix", lists=1)),
    ("dot: DOT_BOUND_LISTS = 2", case(metric=DOT, dot_bound_lists=2), Q("matrix", "matrix", lists=2)),
    ("dot: EXACT_BOUND is L2 only", case(metric=DOT, exact_bound=1), Q("matrix", "matrix", lists=3)),
    ("dot: largest list 65,536 rows", case(metric=DOT, max_part=65536), Q("matrix", "matrix", lists=3)),
    ("dot: NO_DOT_FLOW", case(metric=DOT, no_dot_flow=1), PAIR),
    ("dot: NO_MSBOUND", case(metric=DOT, no_msbound=1), PAIR),
    ("dot: NO_MSCAN", case(metric=DOT, no_mscan=1), PAIR),
    ("dot: NO_QSCAN", case(metric=DOT, no_qscan=1), PAIR),
    ("dot: 95 pairs per list", case(metric=DOT, nq=95 * 256, nprobes=1), PAIR),
    ("dot: no codebook means", case(metric=DOT, cb_mean=0), PAIR),
    ("dot: all-zero codebook", case(metric=DOT, ms=UNUSABLE), PAIR),
    ("dot: queries unaligned", case(metric=DOT, a_query=0), PAIR),
    ("dot: centroids unaligned", case(metric=DOT, a_centroids=0), PAIR),
    ("dot: d = 256 has no matrix-core scan", case(metric=DOT, d=256), PAIR),
    ("dot: M = 96", case(metric=DOT, **C3), QM8),
    ("dot: skew 8.2 under DOT_FLOW_SKEW = 8", case(metric=DOT, max_part=32032, dot_flow_skew=8), PAIR),
    ("dot: skew 7.9 under DOT_FLOW_SKEW = 8", case(metric=DOT, max_part=30859, dot_flow_skew=8), Q("matrix", "matrix", lists=3)),
    ("dot: skew 21 without a guard", case(metric=DOT, max_part=82424), Q("matrix", "matrix", lists=3)),
    # ---- pool ----
    ("pool: nprobes * (keff + 28) = 1280", case(), dict(pool="1280")),
    ("pool: floor 512", case(nq=5000, nprobes=1, keff=1, nlist=8), dict(pool="512")),
    ("pool: 580 rounded up to 256s", case(nprobes=10, keff=30), dict(pool="768")),
    ("pool: cap 8192", case(nprobes=100), dict(pool="8192")),
    ("pool: pair scan", case(no_qscan=1, nprobes=100), dict(pool="8192")),
    ("pool: M = 96 follows nprobes", case(nq=1000, nprobes=100, **C3), dict(pool="12800")),
    ("pool: M = 96 cap", case(nq=1000, nprobes=512, keff=128, d=768, m=96, nlist=1024), dict(route="quantised", pool="65536")),
    ("pool: M = 96 within 1 GiB", case(nq=5000, nprobes=256, keff=128, **C3), dict(route="quantised", pool="16384")),
    # ---- the index-only part (lance_hip_index_prewarm) ----
    ("prewarm: the bench index", case(ms=NOT_BUILT), dict(prewarm_ms="1")),
    ("prewarm: NO_MSCAN", case(ms=NOT_BUILT, no_mscan=1), dict(prewarm_ms="0")),
    ("prewarm: M = 96", case(ms=NOT_BUILT, **C3), dict(prewarm_ms="0")),
    ("prewarm: 4-bit", case(ms=NOT_BUILT, nbits=4), dict(prewarm_ms="0")),
    ("prewarm: model not finite", case(ms=NOT_BUILT, finite=0), dict(prewarm_ms="0")),
    ("prewarm: dot", case(ms=NOT_BUILT, metric=DOT), dict(prewarm_ms="1")),
    ("prewarm: dot, NO_DOT_FLOW", case(ms=NOT_BUILT, metric=DOT, no_dot_flow=1), dict(prewarm_ms="0")),
    ("prewarm: dot, uneven lists under a guard", case(ms=NOT_BUILT, metric=DOT, max_part=82424, dot_flow_skew=8), dict(prewarm_ms="0")),
]


def test_decision_table(planner):
    got = planner([c for _, c, _ in TABLE])
    bad = [(name, {k: g[k] for k in want}, want) for (name, _, want), g in zip(TABLE, got) if any(g[k] != v for k, v in want.items())]
    assert not bad, "\n".join(f"{n}: planned {g}, expected {w}" for n, g, w in bad)
    assert all(g["why"] != "(null)" for g in got)
    assert all(g["why"] for (_, _, want), g in zip(TABLE, got) if want.get("route") in ("qm8", "qm4", "pair_scan", "exact_only")), "a slower route names its reason"


# the launches a route makes (stage counters of one call, without the coarse quantiser, refine and graph bookkeeping)
_PAIR = {"pm_group": 1, "ivfpq_scan_c0": 1, "ivfpq_scan_c1": 1, "ivfpq_merge": 1, "ivfpq_exact": 1}
_FLOW = {"pm_group": 2, "ivfpq_scan_c0": 1, "q_residual": 1, "ivfpq_scan_c1": 1, "ivfpq_scan_cb": 1, "ivfpq_merge": 1, "ivfpq_exact": 1}


def launches(p):
    if p["route"] == "exact_only":
        return {"ivfpq_exact": 1}
    if p["route"] in ("qm8", "qm4"):
        return {"ivfpq_scan": 1, "ivfpq_merge": 1, "ivfpq_exact": 1}
    if p["route"] == "pair_scan":
        return dict(_PAIR)
    s = dict(_FLOW)
    if p["bound"] == "matrix":
        s["ivfpq_msbound"] = 1
    if p["main"] == "matrix":
        s["ivfpq_mscan"] = 1
    if p["main"] == "pt" and p["bound"] != "pt":
        s.update(q_pt_tables=1, q_pt_table_only=1)
    return s


_ENV = {"LANCE_HIP_NO_MSCAN": "no_mscan", "LANCE_HIP_NO_MSBOUND": "no_msbound", "LANCE_HIP_NO_QSCAN": "no_qscan", "LANCE_HIP_PM_NOBOUND": "pm_nobound",
        "LANCE_HIP_EXACT_BOUND": "exact_bound", "LANCE_HIP_QPT": "qpt", "LANCE_HIP_NO_PM": "no_pm", "LANCE_HIP_NO_DOT_FLOW": "no_dot_flow"}


def test_recorded_gpu_routes_are_the_predicted_ones(planner):
    """tests/golden/search_routes.json (the launches of every grid case, recorded on a GPU): the plan of the same case predicts them."""
    golden = R.golden()
    names, cases = [], []
    for group, table in sorted(golden.items()):
        env = {} if group == "default" else R.SWITCHED[group][0]
        for name in sorted(table):
            index, nq, k, nprobes, rf, kind = R.CASES[name]
            metric, dtype, d, m, nbits, nlist, n, cbk = R.INDEXES[index]
            c = dict(metric={"l2": L2, "cosine": COSINE, "dot": DOT}[metric], dtype=F16 if dtype == "float16" else F32, d=d, m=m, nbits=nbits, nlist=nlist, n=n,
                     max_part=n // 2, finite=1, cb_mean=int(nbits == 8), ms=UNUSABLE if cbk == "zero" else USABLE, nq=nq, nprobes=nprobes, keff=k * max(rf, 1),
                     range=int(kind == "range"))
            c.update({_ENV[k_]: int(v) for k_, v in env.items()})
            names.append((group, name)); cases.append(c)
    assert set(golden["default"]) == set(R.CASES) and set(golden) == {"default"} | set(R.SWITCHED)
    skip = ("select_probes", "coarse_groups", "refine", "refine_u8", "graph_capture", "graph_replay")
    for (group, name), p in zip(names, planner(cases)):
        for call, rec in enumerate(golden[group][name]):
            assert {k: v for k, v in rec.items() if k not in skip} == launches(p), (group, name, call, p)
        assert "graph_capture" in golden[group][name][1] and "graph_replay" in golden[group][name][2], (group, name)
    routes = {p["route"] for p in planner(cases)}
    assert routes == {"qm8", "qm4", "exact_only", "pair_scan", "quantised"}, "the grid reaches every route"


def test_sweep_invariants(planner):
    cases = []
    batches = [(1, 1), (64, 4), (512, 4), (1024, 4), (10000, 10), (10000, 50)]
    for metric, dtype, m, sd, nbits, (nq, nprobes), ms, nlist in itertools.product((L2, COSINE, DOT), (F32, F16), (8, 16, 32, 48, 64, 96), (4, 8, 16), (8, 4),
                                                                                 batches, (NOT_BUILT, USABLE, UNUSABLE), (8, 256)):
        for sw in ({}, {"no_mscan": 1}, {"no_msbound": 1}, {"qpt": 0}, {"qpt": 1}, {"exact_bound": 1}, {"finite": 0}, {"keff": 200}):
            cases.append(case(metric=metric, dtype=dtype, d=m * sd, m=m, nbits=nbits, nq=nq, nprobes=nprobes, ms=ms, nlist=nlist, **sw))
    plans = planner(cases)
    for c, p in zip(cases, plans):
        tiled, dot, q = c["m"] >= 48, c["metric"] == DOT, p["route"] == "quantised"
        ctx = (c, p)
        assert (p["route"] == "exact_only") == (c["keff"] > 128), ctx
        assert (p["route"] == "qm4") == (c["nbits"] == 4 and c["keff"] <= 128), ctx
        if dot and q:
            assert p["bound"] == "matrix" and p["main"] == "matrix", ("dot never gets an integer pass", ctx)
        if tiled:
            assert p["route"] != "pair_scan" and p["bound"] != "exact_pair", ("tiled shapes never get the pair kernel", ctx)
            assert not q or (p["class_b"] == "rescan" and p["main"] in ("tiled", "pt")), ctx
        elif q:
            assert p["class_b"] == "pair" and p["main"] in ("matrix", "integer"), ctx
        if not c["finite"]:
            assert not q, ("a non-finite model never gets a filter scan", ctx)
        if q and "pt" in (p["bound"], p["main"]):
            assert c["dtype"] != F16 and not dot and tiled and c.get("qpt", 2) != 0, ("per-query tables never go with f16 or dot", ctx)
            assert (p["bound"] == "pt") == (c.get("qpt", 2) == 2) and p["main"] == "pt", ctx
        if q and "matrix" in (p["bound"], p["main"]):
            assert (c["d"], c["m"]) in ((128, 16), (128, 32), (64, 16)) and c["ms"] != UNUSABLE and p["main"] == "matrix", ctx
            assert c["nq"] * c["nprobes"] >= 96 * c["nlist"], ctx
        assert (p["wants_ms"] == "1") == (q and p["main"] == "matrix" and c["ms"] == NOT_BUILT), ctx
        if q:
            assert 1 <= int(p["lists"]) <= min(4, c["nprobes"]) and int(p["pool"]) % 256 == 0 and int(p["pool"]) >= 512, ctx
            # a plan is final once the constants exist: planning again with them built changes nothing but wants_ms
    again = planner([dict(c, ms=USABLE) if c["ms"] == NOT_BUILT else c for c in cases])
    for c, p, p2 in zip(cases, plans, again):
        if c["ms"] == NOT_BUILT:
            assert {k: v for k, v in p.items() if k != "wants_ms"} == {k: v for k, v in p2.items() if k != "wants_ms"}, (c, p, p2)
