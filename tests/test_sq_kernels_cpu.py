"""The DEVICE code of lance_amd/csrc/sq.hip run on the CPU, lane by lane (tests/c/simt_emu: a thread per lane, a barrier for
__syncthreads), under AddressSanitizer + UBSan, against tests/sq_spec.py bit for bit: bounds, codes, distances through both row
readers, and the search -- per-pair selection, merge, the replay decision and the heap replay (pair_cand.cuh at the capacity of k <= 128 and,
in one large-sum case, at the wide one; the dynamic LDS of every launch sized by the library's own functions and guarded).  Integer sums
past 2^24 (sq_spec.large_sum_partition at d = 516) are answered like the specification, and a second build of the same text whose key is
taken before the scaling FAILS that case: the fixture tells the keys apart in the kernels' own code.  The kernels' text is cut out of the
sources at test time, so what runs here is what the GPU compiles, minus the packed dot instruction (its portable definition in
sq.hip stands in).  This checks the logic and the memory safety of the kernels without a device; the arithmetic of the device's own
instructions is what tests/test_zz_gpu_sq.py checks."""
import os
import re
import subprocess

import numpy as np
import pytest

import sq_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lance_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "c", "simt_emu")
f32 = np.float32


def function_text(src, name):
    """the definition of the __device__ function `name` (with its template line, if any), found by name and brace matching"""
    m = re.search(r"^(template <[^\n]*>\n)?__device__ [^\n;{]*\b" + re.escape(name) + r"\(", src, flags=re.M)
    assert m, name
    depth, i = 0, src.index("{", m.end())
    while True:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
        if depth == 0:
            return src[m.start():i] + "\n"


def pair_cand_code():
    """what the IVF_SQ / IVF_RQ search kernels instantiate (pair_cand.cuh): the device code and the launch-size functions behind it"""
    src = open(os.path.join(CSRC, "pair_cand.cuh")).read()
    i = src.index("// ---- pair candidates: device code")
    return src[i:src.index("// ---- pair candidates: end of the code the emulator programs compile", i)]


def device_code(mutant=False):
    """mutant: the scan's and the replay's key taken from (float)sum, before the multiply by r^2 and the divide by 65025 -- the wrong
    kernel tests/sq_spec.py's unscaled_select describes (L2; the distances it reports are not compared)"""
    read = lambda name: open(os.path.join(CSRC, name)).read()
    exact, common, sq = read("exact.cuh"), read("search_common.cuh"), read("sq.hip")
    parts = [function_text(exact, n) for n in ("order_key", "key_to_float")]
    parts += [function_text(common, n) for n in ("row_allowed", "bitonic_sort_kr", "heap_sift_up", "heap_push", "heap_pop")]
    parts.append(pair_cand_code())
    body = sq[sq.index("constexpr uint32_t SQ_MAX_DIM"):sq.index("// ---- host side")]
    body = body.replace("LANCE_HIP_SQ_MAX_DIM", "16384")
    assert "__global__" in body and "smem" in body
    if mutant:
        body, count = re.subn(r"order_key\(sq_finish\(a\.dot, (sq_sum\([^;]*\)), a\.r2\)\)", r"order_key((float)(\1))", body)
        assert count == 2, "the key of sq_scan_kernel and of SqDist::key"
    return ("".join(parts) + body).replace("extern __shared__ __attribute__((aligned(16))) char smem[];", "")


def build_emulator(work, mutant=False):
    (work / "sq_device_code.inc").write_text(device_code(mutant))
    exe = str(work / "sq_kernels")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", str(work), "-I", EMU, os.path.join(EMU, "sq_kernels_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("g++ without sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, work


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory.mktemp("sq_emu"))


@pytest.fixture(scope="module")
def mutant_emulator(tmp_path_factory):
    return build_emulator(tmp_path_factory.mktemp("sq_emu_mutant"), mutant=True)


def run_case(emulator, oracle, x, q, cent, metric, k, nprobes, bounds, row_ids, prefilter=None, shift=0, want_wide=None, want_cap=None, ids_only=False):
    exe, work = emulator
    xs, part = S.prepare_rows(oracle, x, cent, metric)
    qs = oracle.normalize(q) if metric == "cosine" else q
    xs32, qs32 = np.ascontiguousarray(xs, f32), np.ascontiguousarray(qs, f32)
    n, d = xs32.shape
    nq, nlist = qs32.shape[0], cent.shape[0]
    nprobes = min(nprobes, nlist)
    offs, perm = oracle.partition_layout(part, nlist)
    probes, _ = oracle.find_partitions(qs, cent, nprobes, "l2" if metric == "cosine" else metric)
    bits = np.zeros(len(perm) // 32 + 4, np.uint32)
    if prefilter is not None:
        stored = row_ids[perm]
        ok = stored < prefilter.size
        ok[ok] = prefilter[stored[ok]]
        for i in np.nonzero(ok)[0]:
            bits[i >> 5] |= np.uint32(1 << (i & 31))
    inp, outp = str(work / "in.bin"), str(work / "out.bin")
    with open(inp, "wb") as fh:
        np.array([n, d, nlist, nq, nprobes, k, int(metric == "dot"), int(prefilter is not None)], np.uint32).tofile(fh)
        np.array(bounds, np.float64).tofile(fh)
        xs32.tofile(fh); qs32.tofile(fh)
        np.array([len(perm)], np.uint32).tofile(fh); perm.astype(np.uint32).tofile(fh); offs.astype(np.uint32).tofile(fh)
        row_ids.astype(np.uint64).tofile(fh); probes.astype(np.uint32).tofile(fh)
        if prefilter is not None:
            bits.tofile(fh)
    r = subprocess.run([exe, inp, outp] + ([str(shift)] if shift else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-1000:] + r.stderr[-4000:]
    if want_wide is not None:
        assert f"sq_distance wide {int(want_wide)}" in r.stdout, r.stdout
    if want_cap is not None:
        assert f"scan capacity {want_cap}\n" in r.stdout, r.stdout
    raw = np.fromfile(outp, np.uint8)
    if shift:
        return raw
    pos = 0

    def take(count, dt):
        nonlocal pos
        a = raw[pos:pos + count * np.dtype(dt).itemsize].view(dt)
        pos += count * np.dtype(dt).itemsize
        return a
    fold = take(2, np.float64)
    codes = take(n * d, np.uint8).reshape(n, d)
    dist_words, dist_wide = take(nq * n, f32).reshape(nq, n), take(nq * n, f32).reshape(nq, n)
    ids, dists = take(nq * k, np.uint64).reshape(nq, k), take(nq * k, f32).reshape(nq, k)
    flags = take(nq + 1, np.uint32)
    fast_ids = take(nq * k, np.uint64).reshape(nq, k)
    assert pos == raw.size
    if ids_only:
        return ids
    # bounds, codes, distances
    assert tuple(fold) == S.bounds(xs32)
    want_codes = S.encode(xs32, *bounds)
    assert (codes == want_codes).all()
    want_d = S.distances(want_codes, qs32, metric, *bounds)
    assert (dist_words.view(np.uint32) == want_d.view(np.uint32)).all()
    assert d % 16 != 0 or (dist_wide.view(np.uint32) == want_d.view(np.uint32)).all()
    # the search: the final answer, and the fast path's answer for every query it did not hand to the replay
    oi, od = S.search(oracle, want_codes, part, cent, q, k, nprobes, metric, *bounds, row_ids=row_ids, prefilter=prefilter)
    assert (ids == oi).all() and (dists.view(np.uint32) == od.view(np.uint32)).all()
    kept = flags[:nq] == 0
    assert (fast_ids[kept] == oi[kept]).all()
    assert flags[nq] == (~kept).sum()
    return int(flags[nq])


def test_device_code_is_found():
    code = device_code()
    for name in ("sq_bounds_kernel", "sq_encode_kernel", "sq_distance_kernel", "sq_scan_kernel", "cand_merge_kernel", "sq_exact_kernel",
                 "cand_scan_pair", "cand_sort_truncate", "cand_replay_query", "sq_scan_lds", "sq_gather_kernel", "sq_norms_kernel", "heap_pop", "bitonic_sort_kr", "order_key"):
        assert name in code, name
    assert "hipLaunchKernelGGL" not in code and "LH_REQUIRE" not in code, "host code must stay out"


def test_ties_are_replayed(emulator, oracle):
    x, q, rid = S.tie_fixture(n=900, nq=4)
    cent = S.centroids_with_gaps(x, 4, seed=3)
    b = S.bounds(x)
    assert run_case(emulator, oracle, x, q, cent, "l2", 10, 3, b, rid) > 0
    assert run_case(emulator, oracle, x, q, cent, "l2", 128, 4, b, rid, prefilter=np.arange(int(rid.max()) + 1) % 3 != 0) > 0


@pytest.mark.parametrize("metric,kind,d,k,nprobes", [("l2", "f32", 20, 10, 3), ("dot", "f16", 32, 128, 8), ("cosine", "f32", 16, 1, 1),
                                                     ("l2", "f32", 1, 10, 3), ("cosine", "f16", 17, 10, 3)])
def test_gaussian_rows(emulator, oracle, metric, kind, d, k, nprobes):
    x, q = S.gaussian(700, d, 3, seed=5, kind=kind)
    x[650, min(2, d - 1)] = np.nan                        # a row without a partition
    rid = S.permuted_ids(700, 2)
    cent = S.centroids_with_gaps(oracle.normalize(x[:600]) if metric == "cosine" else x[:600], 8, seed=1)
    xs, _ = S.prepare_rows(oracle, x, cent, metric)
    b = S.bounds(np.asarray(xs, f32)[100:164])            # a sample's bounds: later rows saturate
    replays = run_case(emulator, oracle, x, q, cent, metric, k, nprobes, b, rid)
    assert replays < 3 or d == 1                          # (one column: 700 rows on 256 codes tie everywhere)
    half = np.zeros(int(rid.max()) + 1, bool)
    half[rid[::2]] = True
    run_case(emulator, oracle, x, q, cent, metric, k, 8, b, rid, prefilter=half)
    run_case(emulator, oracle, x, q, cent, metric, k, 8, b, rid, prefilter=np.zeros(5, bool))


def test_row_addresses(emulator, oracle):
    """Row ids as a table of several fragments has them (tests/rowid_fixtures.py: fragment << 32 | offset, up to fragment 2^31 - 1, low
    words that repeat across fragments and order the other way round): the merge and the heap replay compare and carry all 64 bits,
    and a prefilter mask far shorter than every id selects nothing."""
    import rowid_fixtures as R
    x, q, _ = S.tie_fixture(n=450, nq=2)               # (half the rows and queries of the cases above: each run starts a thread per lane)
    rid = R.row_addresses(450, 21)
    cent = S.centroids_with_gaps(x, 4, seed=3)
    b = S.bounds(x)
    assert run_case(emulator, oracle, x, q, cent, "l2", 10, 3, b, rid) > 0
    run_case(emulator, oracle, x, q, cent, "l2", 10, 3, b, rid, prefilter=np.ones(1000, bool))
    x, q = S.gaussian(350, 20, 2, seed=5)
    rid = R.row_addresses(350, 22)
    cent = S.centroids_with_gaps(x[:300], 8, seed=1)
    b = S.bounds(x[100:164])
    assert run_case(emulator, oracle, x, q, cent, "l2", 10, 3, b, rid) < 2
    run_case(emulator, oracle, x, q, cent, "l2", 128, 8, b, rid, prefilter=np.ones(1000, bool))


@pytest.mark.parametrize("d", [16, 20])
def test_offset_bases(emulator, oracle, d):
    """Caller-owned bases 1, 4 and 8 bytes off the 16-byte grid: the codes handed to sq_distance (both readers; at d = 16 the host's
    gate must leave the 16-byte reader), and at 4 and 8 the f32 rows and keys read by the bounds and encode kernels.  Every buffer ends
    with its last element, so the sanitizers see a read past a row or a misaligned wide load; every output byte equals the aligned run's."""
    src = open(os.path.join(CSRC, "sq.hip")).read()
    gate = "const bool wide = d % 16 == 0 && (reinterpret_cast<uintptr_t>(codes) & 15) == 0;"
    assert gate in src, f"sq.hip no longer holds {gate!r} (the gate of lance_hip_sq_distance): tests/c/simt_emu/sq_kernels_main.cpp mirrors it, update both"
    x, q = S.gaussian(300, d, 2, seed=8)
    rid = S.permuted_ids(300, 3)
    cent = S.centroids_with_gaps(x[:250], 4, seed=2)
    b = S.bounds(x[50:114])
    args = (emulator, oracle, x, q, cent, "l2", 10, 3, b, rid)
    run_case(*args, want_wide=True if d == 16 else None)
    aligned = np.fromfile(str(emulator[1] / "out.bin"), np.uint8)
    for shift in (1, 4, 8):
        got = run_case(*args, shift=shift, want_wide=False if d == 16 else None)
        assert np.array_equal(got, aligned), shift


def test_constant_column(emulator, oracle):
    x = np.full((300, 5), 1.25, f32)
    cent = np.ascontiguousarray(np.stack([x[0], x[0] + 1, x[0] - 1]))
    rid = S.permuted_ids(300, 4)
    assert run_case(emulator, oracle, x, x[:2], cent, "l2", 10, 3, (0.0, 2.0), rid) == 2
    assert run_case(emulator, oracle, x, x[:2], cent, "l2", 128, 1, (1.25, 1.25), rid) == 2      # start == end


# ---- integer sums past 2^24 (sq_spec.large_sum_partition; its conditions are checked by tests/test_sq_spec.py at the sizes of the GPU file) ----
def large_sum_case(oracle):
    """d = 516 with 426 + 24 rows; the design query's partition cuts a tie at k = 10, 128 and 129"""
    f = S.large_sum_partition(516, "l2", 426)
    _, keys = S.large_sum_keys(f, "l2")
    for k in (10, 128, 129):
        s = np.sort(keys)
        assert s[k - 1] == s[k]
    return f, (oracle, f["x"], f["q"][:2], f["cent"], "l2")


@pytest.mark.parametrize("k,nprobes,cap", [(10, 2, 512), (128, 1, 512), (129, 2, 4096)])
def test_large_sums(emulator, oracle, k, nprobes, cap):
    """sums above 2^24 that are one float: the cut ties are replayed, and the answer is the heap's.  k = 129 runs the scan at the wide
    capacity (4096 entries beside the 528 bytes of the query) and the wide merge instance"""
    f, args = large_sum_case(oracle)
    assert run_case(emulator, *args, k, nprobes, f["bounds"], f["rid"], want_cap=cap) >= 1
    if k == 128:
        half = np.zeros(int(f["rid"].max()) + 1, bool)
        half[f["rid"][::2]] = True
        run_case(emulator, *args, k, 2, f["bounds"], f["rid"], prefilter=half)


def test_large_sums_fail_a_kernel_keyed_on_the_unscaled_sum(mutant_emulator, oracle):
    """the same device text with order_key((float)sum) for a key: its ids at d = 516 are not the reference's -- they are the ones
    sq_spec.unscaled_select predicts -- so the fixture tells the two keys apart in the kernels' own code.  (One probe: with two the
    mutant also merges by the wrong key.)"""
    f, args = large_sum_case(oracle)
    _, part = S.prepare_rows(oracle, f["x"], f["cent"], "l2")
    spec = (oracle, f["codes"], part, f["cent"], f["q"][:2], 128, 1, "l2") + f["bounds"]
    want, _ = S.search(*spec, row_ids=f["rid"])
    wrong, _ = S.search(*spec, row_ids=f["rid"], select=S.unscaled_select)
    got = run_case(mutant_emulator, *args, 128, 1, f["bounds"], f["rid"], ids_only=True)
    differ = (np.sort(got, axis=1) != np.sort(want, axis=1)).any(axis=1)
    assert differ.all(), "the mutant kernel must fail both design queries"
    assert (np.sort(got, axis=1) == np.sort(wrong, axis=1)).all()
    with pytest.raises(AssertionError):
        run_case(mutant_emulator, *args, 128, 1, f["bounds"], f["rid"])
