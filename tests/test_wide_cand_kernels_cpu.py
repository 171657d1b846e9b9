"""The candidate kernels of IVF_SQ / IVF_RQ (lance_amd/csrc/pair_cand.cuh and their instances in the search blocks of sq.hip / rq.hip: scan,
merge and heap replay for keff <= 768) run on the CPU, lane by lane (tests/c/simt_emu), as a stand-alone program under AddressSanitizer +
UBSan, against tests/sq_spec.py / tests/rq_spec.py at k = keff bit for bit.  The kernels' text and the functions that size their launches
are cut out of the sources at test time, so what runs here is what the GPU compiles.  The candidate buffer's capacity is a launch
parameter.  The wide cases (128 < keff) run at the smallest wide one (1024 = 768 kept + one 256-row chunk), where the buffer is sorted
most often and, at keff = 768, filled to its last entry; the narrow cases (keff = 128) run at the capacity the library picks for them:
512, and 1024 once IVF_RQ's rotated query (4 d bytes, parked in the buffer before the scan) no longer fits 512 entries."""
import os
import re
import subprocess

import numpy as np
import pytest

import refine_spec as F
import rq_spec as R
import sq_spec as S
from test_sq_kernels_cpu import function_text, pair_cand_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lance_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "c", "simt_emu")
f32 = np.float32
CAP = F.MIN_CAP


def between(src, a, b):
    i = src.index(a)
    return src[i:src.index(b, i)]


def device_code():
    read = lambda name: open(os.path.join(CSRC, name)).read()
    exact, common, sq, rq = read("exact.cuh"), read("search_common.cuh"), read("sq.hip"), read("rq.hip")
    parts = [function_text(exact, n) for n in ("order_key", "key_to_float")]
    parts += [function_text(common, n) for n in ("row_allowed", "bitonic_sort_kr", "heap_sift_up", "heap_push", "heap_pop")]
    parts += [function_text(sq, n) for n in ("sq_udot4", "sq_row_xq", "sq_finish", "sq_sum")]
    parts.append(between(rq, "constexpr int RQ_BATCH", "// out[i][j] = in[j][i]"))                          # RQ_BATCH, the branches, rq_rot_dot
    parts.append(between(rq, "struct RqQuery {", "// distance_all (quantised != 0) or distance of every row"))   # rq_prepare, rq_row_distance
    parts.append(pair_cand_code())
    parts.append(between(sq, "// ---- IVF_SQ search", "// ---- host side"))
    parts.append(between(rq, "// ---- IVF_RQ search", "// ---- host side"))
    code = "".join(parts).replace("extern __shared__ __attribute__((aligned(16))) char smem[];", "")
    return code


def test_device_code_is_found():
    code = device_code()
    for name in ("cand_sort_truncate", "cand_scan_pair", "cand_merge_kernel", "cand_replay_query", "cand_scan_cap", "sq_scan_kernel", "sq_exact_kernel",
                 "rq_scan_kernel", "rq_exact_kernel", "rq_scan_cap", "rq_replay_lds", "rq_prepare", "rq_row_distance", "sq_row_xq", "heap_pop"):
        assert name in code, name
    assert "hipLaunchKernelGGL" not in code and "LH_REQUIRE" not in code and "extern __shared__" not in code, "host code must stay out"


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    work = tmp_path_factory.mktemp("wide_emu")
    (work / "pair_device_code.inc").write_text(device_code())
    exe = str(work / "pair_cand")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", str(work), "-I", EMU, os.path.join(EMU, "pair_cand_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("g++ without sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, work


def allow_bits(stored_ids, prefilter):
    bits = np.zeros(len(stored_ids) // 32 + 4, np.uint32)
    ok = stored_ids < prefilter.size
    ok[ok] = prefilter[stored_ids[ok]]
    for i in np.nonzero(ok)[0]:
        bits[i >> 5] |= np.uint32(1 << (i & 31))
    return bits


def run(emulator, kind, head, offs, stored_ids, probes, bits, payload, nq, keff):
    exe, work = emulator
    inp, outp = str(work / "in.bin"), str(work / "out.bin")
    with open(inp, "wb") as fh:
        np.array(head, np.uint32).tofile(fh)
        offs.astype(np.uint32).tofile(fh); stored_ids.astype(np.uint64).tofile(fh); probes.astype(np.uint32).tofile(fh)
        if bits is not None:
            bits.tofile(fh)
        for a in payload:
            np.ascontiguousarray(a).tofile(fh)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-1000:] + r.stderr[-4000:]
    raw = np.fromfile(outp, np.uint8)
    pos = 0

    def take(count, dt):
        nonlocal pos
        a = raw[pos:pos + count * np.dtype(dt).itemsize].view(dt)
        pos += count * np.dtype(dt).itemsize
        return a
    pairs = nq * probes.shape[1]
    out = {"pkey": take(pairs * keff, np.uint32).reshape(pairs, keff), "ppos": take(pairs * keff, np.uint32).reshape(pairs, keff),
           "pcnt": take(pairs, np.uint32), "pamb": take(pairs, np.uint32),
           "fast_ids": take(nq * keff, np.uint64).reshape(nq, keff), "fast_dists": take(nq * keff, f32).reshape(nq, keff),
           "flags": take(nq + 1, np.uint32), "ids": take(nq * keff, np.uint64).reshape(nq, keff), "dists": take(nq * keff, f32).reshape(nq, keff)}
    assert pos == raw.size
    out["cap"] = int(re.search(r"^cap (\d+)$", r.stdout, flags=re.M).group(1))      # the capacity the scan ran at (head cap = 0: the library's)
    return out


def check(out, oi, od, nq):
    assert (out["ids"] == oi).all(), np.argwhere(out["ids"] != oi)[:4]
    assert (out["dists"].view(np.uint32) == od.view(np.uint32)).all()
    kept = out["flags"][:nq] == 0
    assert (out["fast_ids"][kept] == oi[kept]).all() and (out["fast_dists"][kept].view(np.uint32) == od[kept].view(np.uint32)).all()
    assert out["flags"][nq] == (~kept).sum()
    return int(out["flags"][nq])


def run_rq(emulator, oracle, x, q, cent, P, metric, keff, nprobes, row_ids, prefilter=None, cap=CAP, built=None):
    x, q, cent, P = (np.ascontiguousarray(a, f32) for a in (x, q, cent, P))
    d, nq, nlist = x.shape[1], q.shape[0], cent.shape[0]
    part, codes, add, scale = built or R.build(oracle, x, cent, P, metric)
    offs, perm = oracle.partition_layout(part, nlist)
    probes, pd = oracle.find_partitions(q, cent, nprobes, metric)
    stored_ids = row_ids[perm]
    bits = None if prefilter is None else allow_bits(stored_ids, prefilter)
    head = [1, len(perm), d, nlist, nq, nprobes, keff, cap, int(metric == "dot"), int(prefilter is not None)]
    out = run(emulator, "rq", head, offs, stored_ids, probes, bits,
              [codes[perm], add[perm], scale[perm], pd.astype(f32), q, cent, np.ascontiguousarray(P.T)], nq, keff)
    oi, od = R.search(oracle, codes, add, scale, part, cent, P, q, keff, nprobes, metric, row_ids=row_ids, prefilter=prefilter)
    return check(out, oi, od, nq), out


def run_sq(emulator, oracle, x, q, cent, metric, keff, nprobes, bounds, row_ids, prefilter=None, cap=CAP):
    xs, part = S.prepare_rows(oracle, x, cent, metric)
    qs = oracle.normalize(q) if metric == "cosine" else q
    d, nq, nlist = x.shape[1], q.shape[0], cent.shape[0]
    ld = (d + 15) // 16 * 16
    codes = S.encode(xs, *bounds)
    offs, perm = oracle.partition_layout(part, nlist)
    probes, _ = oracle.find_partitions(qs, cent, nprobes, "l2" if metric == "cosine" else metric)
    pad = lambda c: np.ascontiguousarray(np.pad(c, ((0, 0), (0, ld - d))))
    stored, qc = pad(codes[perm]), pad(S.encode(qs, *bounds))
    sq = lambda c: (c.astype(np.uint32) ** 2).sum(axis=1, dtype=np.uint32)
    stored_ids = row_ids[perm]
    bits = None if prefilter is None else allow_bits(stored_ids, prefilter)
    r = f32(bounds[1] - bounds[0])
    head = [0, len(perm), d, nlist, nq, nprobes, keff, cap, int(metric == "dot"), int(prefilter is not None)]
    out = run(emulator, "sq", head, offs, stored_ids, probes, bits, [np.array([r * r], f32), stored, sq(stored), qc, sq(qc)], nq, keff)
    oi, od = S.search(oracle, codes, part, cent, q, keff, nprobes, metric, *bounds, row_ids=row_ids, prefilter=prefilter)
    return check(out, oi, od, nq), out


def half_mask(rid, seed):
    m = np.zeros(int(rid.max()) + 1, bool)
    m[rid[np.random.default_rng(seed).random(len(rid)) < 0.5]] = True
    return m


def pair_contract(out, f, keff, allow_rows=None):
    """the design query's first pair (query 0, partition 0 = storage positions 0..N-1): the keff best (key, position) and the cut-tie flag"""
    keys = f["keys"]
    pos = np.arange(f["N"])
    if allow_rows is not None:
        keys, pos = keys[allow_rows], pos[allow_rows]
    order = np.lexsort((pos, keys))[:keff]
    got = int(out["pcnt"][0])
    assert got == min(keff, len(keys))
    assert (out["pkey"][0, :got] == keys[order]).all() and (out["ppos"][0, :got] == pos[order]).all()
    assert out["pamb"][0] == int(R.kth_is_tied(keys, keff))


# N % 32 = 0, 1, 31 over the cases; every N is past the buffer plus two chunks.  keff = 768 in descending order fills the buffer to its
# last entry: 768 kept after a cut, and every one of the next 256 rows enters.
ORDERED = [("descending", 129, 1568), ("descending", 768, 1569), ("ascending", 129, 1599), ("ascending", 768, 1568),
           ("staircase", 129, 1569), ("staircase", 768, 1599), ("tie_cut", 129, 1568), ("tie_cut", 768, 1599)]


@pytest.mark.parametrize("order,keff,N", ORDERED)
def test_rq_ordered_partitions(emulator, oracle, order, keff, N):
    metric = "dot" if keff == 129 else "l2"
    f = F.ordered_partition(oracle, "rq", order, metric, keff, CAP, N)
    q = np.ascontiguousarray(np.stack([f["q"], f["x"][5] + f32(0.1)]))
    rid = R.permuted_ids(len(f["x"]), 4)
    replays, out = run_rq(emulator, oracle, f["x"], q, f["cent"], f["P"], metric, keff, 2, rid)
    pair_contract(out, f, keff)
    assert f["cut_tie"] == (order == "tie_cut") and out["flags"][0] == int(f["cut_tie"])       # the design query is replayed iff its tie is cut


@pytest.mark.parametrize("order,keff,N", [("tie_cut", 129, 1599), ("descending", 768, 1568), ("staircase", 768, 1569)])
def test_rq_ordered_partitions_masked(emulator, oracle, order, keff, N):
    """under a prefilter every row takes the f32 fold; an all-selected mask keeps the order's properties, a half mask keeps the check"""
    f = F.ordered_partition(oracle, "rq", order, "l2", keff, CAP, N, prefiltered=True)
    q = np.ascontiguousarray(f["q"][None])
    rid = R.permuted_ids(len(f["x"]), 4)
    replays, out = run_rq(emulator, oracle, f["x"], q, f["cent"], f["P"], "l2", keff, 2, rid, prefilter=np.ones(int(rid.max()) + 1, bool))
    pair_contract(out, f, keff)
    assert out["flags"][0] == int(f["cut_tie"])
    m = half_mask(rid, 8)
    _, out = run_rq(emulator, oracle, f["x"], q, f["cent"], f["P"], "l2", keff, 2, rid, prefilter=m)
    pair_contract(out, f, keff, allow_rows=m[rid[:N]])


@pytest.mark.parametrize("order,keff,N", ORDERED)
def test_sq_ordered_partitions(emulator, oracle, order, keff, N):
    metric = "dot" if keff == 129 else "l2"
    f = F.ordered_partition(oracle, "sq", order, metric, keff, CAP, N)
    q = np.ascontiguousarray(np.stack([f["q"], f["x"][5] + f32(0.1)]))
    rid = S.permuted_ids(len(f["x"]), 4)
    replays, out = run_sq(emulator, oracle, f["x"], q, f["cent"], metric, keff, 2, f["bounds"], rid)
    pair_contract(out, f, keff)
    assert out["flags"][0] == 1 or not f["cut_tie"]
    if order == "tie_cut":
        m = half_mask(rid, 8)
        _, out = run_sq(emulator, oracle, f["x"], q[:1], f["cent"], metric, keff, 2, f["bounds"], rid, prefilter=m)
        pair_contract(out, f, keff, allow_rows=m[rid[:N]])


@pytest.mark.parametrize("keff", [129, 768])
def test_fewer_rows_than_keff(emulator, oracle, keff):
    """partitions of 64, 33, 31, 0 and 258 rows: every list is short, the merged answer of five probes is padded at keff = 768 (386 rows);
    d = 24 reads RQ rows byte by byte and SQ rows with a zero-padded tail"""
    x, cent = R.sized_partitions([64, 33, 31, 0, 258], 24, seed=24)
    rng = np.random.default_rng(1)
    q = np.ascontiguousarray((x[rng.integers(0, len(x), 2)] + rng.standard_normal((2, 24)) * 0.2).astype(f32))
    rid = R.permuted_ids(len(x), 2)
    P = R.rotations(24, seed=3)["qr"]
    mask = np.ones(int(rid.max()) // 2, bool)                    # ids past the mask's end are not selected (and never read)
    metric = "l2" if keff == 768 else "dot"
    _, out = run_rq(emulator, oracle, x, q, cent, P, metric, keff, 5, rid)
    assert ((out["ids"] == F.UNSET).any(axis=1) == (keff == 768)).all() and int(out["pcnt"].max()) == min(keff, 258)
    run_rq(emulator, oracle, x, q, cent, P, metric, keff, 3, rid, prefilter=mask)
    if keff == 768:
        run_sq(emulator, oracle, x, q, oracle.normalize(cent), "cosine", keff, 5, S.bounds(oracle.normalize(x)[:64]), rid)
    else:
        run_sq(emulator, oracle, x, q, cent, "dot", keff, 5, S.bounds(x[:64]), rid)
    run_sq(emulator, oracle, x, q, cent, "l2", keff, 5, S.bounds(x[:64]), rid, prefilter=mask)


def test_mass_ties_are_replayed(emulator, oracle):
    """IVF_SQ on a four-value grid (sq_spec.tie_fixture): far more rows tie at a partition's keff-th distance than fit"""
    x, q, rid = S.tie_fixture(n=2400, nq=3)
    cent = np.ascontiguousarray(x[[0, 700, 1400]])
    replays, _ = run_sq(emulator, oracle, x, q, cent, "l2", 200, 1, S.bounds(x), rid)       # one probe: a cut tie of the pair is the answer's
    assert replays > 0
    run_sq(emulator, oracle, x, q, cent, "l2", 200, 3, S.bounds(x), rid)



# ---- the narrow capacity: keff = 128, the buffer the library picks (cap = 0 in the problem file) -------------------------------------
# Every N is past the buffer plus two chunks, N % 32 = 0, 1, 31, 0 over the four orders.  IVF_RQ at d = 1024: the rotated query fills the
# 512-entry buffer it borrows to its last byte; d = 1032 is the first dimension that takes 1024 entries.
NARROW_K = 128
NARROW = {512: list(zip(F.ORDERS, (1056, 1057, 1087, 1056))), 1024: list(zip(F.ORDERS, (1568, 1569, 1599, 1568)))}


@pytest.mark.parametrize("order,N", NARROW[512])
def test_sq_narrow_ordered_partitions(emulator, oracle, order, N):
    f = F.ordered_partition(oracle, "sq", order, "l2", NARROW_K, 512, N)
    q = np.ascontiguousarray(np.stack([f["q"], f["x"][5] + f32(0.1)]))
    rid = S.permuted_ids(len(f["x"]), 4)
    replays, out = run_sq(emulator, oracle, f["x"], q, f["cent"], "l2", NARROW_K, 2, f["bounds"], rid, cap=0)
    assert out["cap"] == 512
    pair_contract(out, f, NARROW_K)
    assert out["flags"][0] == 1 or not f["cut_tie"]


@pytest.mark.parametrize("d,cap,order,N", [(1024, 512, o, n) for o, n in NARROW[512]] + [(1032, 1024, o, n) for o, n in NARROW[1024]])
def test_rq_narrow_ordered_partitions(emulator, oracle, d, cap, order, N):
    f = F.ordered_partition(oracle, "rq", order, "l2", NARROW_K, cap, N, d=d)
    q = np.ascontiguousarray(np.stack([f["q"], f["x"][5] + f32(0.1)]))
    rid = R.permuted_ids(len(f["x"]), 4)
    replays, out = run_rq(emulator, oracle, f["x"], q, f["cent"], f["P"], "l2", NARROW_K, 2, rid, cap=0, built=f["built"])
    assert out["cap"] == cap
    pair_contract(out, f, NARROW_K)
    assert f["cut_tie"] == (order == "tie_cut") and out["flags"][0] == int(f["cut_tie"])


def test_rq_narrow_tie_cut_masked(emulator, oracle):
    """an all-selected mask (every row through the f32 fold): every one of the first 512 rows is a candidate, so the first cut finds the
    512-entry buffer filled to its last entry (ordered_partition asserts that the cut at storage position 511 cuts the tie block)"""
    f = F.ordered_partition(oracle, "rq", "tie_cut", "l2", NARROW_K, 512, 1087, prefiltered=True)
    rid = R.permuted_ids(len(f["x"]), 4)
    replays, out = run_rq(emulator, oracle, f["x"], np.ascontiguousarray(f["q"][None]), f["cent"], f["P"], "l2", NARROW_K, 2, rid,
                          prefilter=np.ones(int(rid.max()) + 1, bool), cap=0)
    assert out["cap"] == 512
    pair_contract(out, f, NARROW_K)
    assert f["cut_tie"] and out["flags"][0] == 1 and replays == 1
