"""The DEVICE code of lance_amd/csrc/rq.hip run on the CPU, lane by lane (tests/c/simt_emu: a thread per lane, a barrier for
__syncthreads), under AddressSanitizer + UBSan, against tests/rq_spec.py bit for bit: the encoder, the query preparation, the three
distance branches (packed rows through the u8 table, the f32 remainder, the f32 fold under a prefilter) and the search -- per-pair
selection, the merge kernel, the replay decision and the heap replay (pair_cand.cuh at the capacity of k <= 128, the dynamic LDS of
every launch sized by the library's own functions and guarded).  The kernels' text is cut out of the sources at
test time, so what runs here is what the GPU compiles.  This checks the logic and the memory safety of the kernels without a device;
the arithmetic of the device's own instructions is what tests/test_zz_gpu_rq.py checks."""
import os
import re
import subprocess

import numpy as np
import pytest

import rq_spec as R
from test_sq_kernels_cpu import function_text, pair_cand_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lance_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "c", "simt_emu")
f32 = np.float32


def device_code():
    read = lambda name: open(os.path.join(CSRC, name)).read()
    exact, common, rq = read("exact.cuh"), read("search_common.cuh"), read("rq.hip")
    parts = [function_text(exact, n) for n in ("order_key", "key_to_float")]
    parts += [function_text(common, n) for n in ("row_allowed", "bitonic_sort_kr", "heap_sift_up", "heap_push", "heap_pop")]
    parts.append(pair_cand_code())
    body = rq[rq.index("constexpr uint32_t RQ_MAX_DIM"):rq.index("// ---- host side")]
    body = body.replace("LANCE_HIP_RQ_MAX_DIM", "2048")
    code = "".join(parts) + body
    code = code.replace("extern __shared__ __attribute__((aligned(16))) char smem[];", "")
    assert "__global__" in code and "smem" in code
    return code


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    work = tmp_path_factory.mktemp("rq_emu")
    (work / "rq_device_code.inc").write_text(device_code())
    exe = str(work / "rq_kernels")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", str(work), "-I", EMU, os.path.join(EMU, "rq_kernels_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("g++ without sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, work


def run_case(emulator, oracle, x, q, cent, P, metric, k, nprobes, row_ids, prefilter=None, shift=0):
    exe, work = emulator
    x, q, cent, P = (np.ascontiguousarray(a, f32) for a in (x, q, cent, P))
    n, d = x.shape
    nq, nlist = q.shape[0], cent.shape[0]
    nprobes = min(nprobes, nlist)
    part, dvc = R.prepare_rows(oracle, x, cent, metric)
    offs, perm = oracle.partition_layout(part, nlist)
    probes, pd = oracle.find_partitions(q, cent, nprobes, metric)
    every, every_d = oracle.find_partitions(q, cent, nlist, metric)
    dqc_all = np.empty((nq, nlist), f32)
    np.put_along_axis(dqc_all, every.astype(np.int64), every_d, axis=1)
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
        x.tofile(fh); q.tofile(fh); cent.tofile(fh); P.tofile(fh)
        part.astype(np.uint32).tofile(fh); dvc.astype(f32).tofile(fh)
        np.array([len(perm)], np.uint32).tofile(fh); perm.astype(np.uint32).tofile(fh); offs.astype(np.uint32).tofile(fh)
        row_ids.astype(np.uint64).tofile(fh); probes.astype(np.uint32).tofile(fh); pd.astype(f32).tofile(fh); dqc_all.tofile(fh)
        if prefilter is not None:
            bits.tofile(fh)
    r = subprocess.run([exe, inp, outp] + ([str(shift)] if shift else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-1000:] + r.stderr[-4000:]
    raw = np.fromfile(outp, np.uint8)
    if shift:
        return raw, int(re.search(r"refused (\d+)", r.stdout).group(1))
    pos = 0

    def take(count, dt):
        nonlocal pos
        a = raw[pos:pos + count * np.dtype(dt).itemsize].view(dt)
        pos += count * np.dtype(dt).itemsize
        return a
    cb = d // 8
    codes, add, scale = take(n * cb, np.uint8).reshape(n, cb), take(n, f32), take(n, f32)
    want_codes, want_add, want_scale = R.encode(x, part, dvc, cent, P, metric)
    assert (codes == want_codes).all()
    assert (add.view(np.uint32) == want_add.view(np.uint32)).all() and (scale.view(np.uint32) == want_scale.view(np.uint32)).all()
    for p in range(nlist):
        rows = perm[int(offs[p]):int(offs[p + 1])]
        if len(rows) == 0:
            continue
        for quantised in (True, False):
            got = take(nq * len(rows), f32).reshape(nq, len(rows))
            want = R.distances(want_codes[rows], want_add[rows], want_scale[rows], q - cent[p], dqc_all[:, p], P, metric, quantised)
            assert (got.view(np.uint32) == want.view(np.uint32)).all(), (p, quantised)
    ids, dists = take(nq * k, np.uint64).reshape(nq, k), take(nq * k, f32).reshape(nq, k)
    flags = take(nq + 1, np.uint32)
    fast_ids = take(nq * k, np.uint64).reshape(nq, k)
    assert pos == raw.size
    oi, od = R.search(oracle, want_codes, want_add, want_scale, part, cent, P, q, k, nprobes, metric, row_ids=row_ids, prefilter=prefilter)
    assert (ids == oi).all() and (dists.view(np.uint32) == od.view(np.uint32)).all()
    kept = flags[:nq] == 0
    assert (fast_ids[kept] == oi[kept]).all()
    assert flags[nq] == (~kept).sum()
    return int(flags[nq])


def test_device_code_is_found():
    code = device_code()
    for name in ("rq_transpose_kernel", "rq_encode_kernel", "rq_prepare", "rq_row_distance", "rq_distance_kernel", "rq_scan_kernel", "rq_exact_kernel",
                 "cand_scan_pair", "cand_sort_truncate", "cand_replay_query", "rq_scan_cap", "rq_gather_kernel", "cand_merge_kernel", "heap_pop", "bitonic_sort_kr", "order_key"):
        assert name in code, name
    assert "hipLaunchKernelGGL" not in code and "LH_REQUIRE" not in code, "host code must stay out"


def queries(x, cent, nq, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray((x[rng.integers(0, len(x), nq)] + rng.standard_normal((nq, x.shape[1])) * 0.2).astype(f32))


@pytest.mark.parametrize("metric,d,rot,k,nprobes", [("l2", 128, "qr", 10, 3), ("dot", 8, "signed_perm", 128, 5), ("l2", 24, "identity", 1, 1)])
def test_three_branches(emulator, oracle, metric, d, rot, k, nprobes):
    """partitions of 64, 33, 31 and 0 rows and one of 258 (n % 32 = 0, 1, 31, 2; more than one 256-row chunk): packed rows, remainder
    rows and -- under the prefilter -- the f32 fold; d = 128 reads rows as 16-byte words, d = 8 / 24 byte by byte (d = 24 also takes
    the dot's tail).  The mask is half as long as the largest row id: about half the rows are selected, the ids of the others lie
    past its end (not selected, and never read).  (Each run starts a thread per lane: two runs per shape.)"""
    x, cent = R.sized_partitions([64, 33, 31, 0, 258], d, seed=d)
    q = queries(x, cent, 2, seed=1)
    P = R.rotations(d, seed=3)[rot]
    rid = R.permuted_ids(len(x), 2)
    run_case(emulator, oracle, x, q, cent, P, metric, k, nprobes, rid)
    run_case(emulator, oracle, x, q, cent, P, metric, k, 5, rid, prefilter=np.ones(int(rid.max()) // 2, bool))


@pytest.mark.parametrize("d", [64, 128])
def test_offset_bases(emulator, oracle, d):
    """Caller-owned bases 1, 4 and 8 bytes off the 16-byte grid.  d = 64: rows of 8 code bytes, read byte by byte from any base; d = 128:
    rows of one 16-byte word, which lance_hip_rq_distance refuses off the grid -- the program counts the refusals and never hands the
    16-byte reader such a base.  At 4 and 8 the f32 rows of rq_encode move too.  Every output byte equals the aligned run's."""
    src = open(os.path.join(CSRC, "rq.hip")).read()
    gate = 'LH_REQUIRE(d % 128 != 0 || (reinterpret_cast<uintptr_t>(codes) & 15) == 0, "rq_distance: codes of 16-byte rows must be 16-byte aligned");'
    assert gate in src, f"rq.hip no longer holds {gate!r} (the refusal of lance_hip_rq_distance): tests/c/simt_emu/rq_kernels_main.cpp mirrors it, update both"
    x, cent = R.sized_partitions([40, 33], d, seed=d + 1)
    q = queries(x, cent, 2, seed=4)
    P = R.rotations(d, seed=5)["qr"]
    rid = R.permuted_ids(len(x), 2)
    args = (emulator, oracle, x, q, cent, P, "l2", 10, 2, rid)
    run_case(*args)
    aligned = np.fromfile(str(emulator[1] / "out.bin"), np.uint8)
    for shift in (1, 4, 8):
        got, refused = run_case(*args, shift=shift)
        assert np.array_equal(got, aligned), shift
        assert refused == (2 if d == 128 else 0)


def test_row_addresses(emulator, oracle):
    """Lance row addresses (fragment << 32 | offset, tests/rowid_fixtures.py): the merge and the replay carry all 64 bits, and a mask
    far shorter than every id selects nothing"""
    import rowid_fixtures as F
    x, cent = R.sized_partitions([40, 65], 16, seed=9)
    q = queries(x, cent, 2, seed=3)
    rid = F.row_addresses(len(x), 5)
    P = R.rotations(16, seed=2)["qr"]
    run_case(emulator, oracle, x, q, cent, P, "l2", 10, 2, rid)
    run_case(emulator, oracle, x, q, cent, P, "l2", 10, 2, rid, prefilter=np.ones(1000, bool))


def test_ties_are_replayed(emulator, oracle):
    """a block of identical rows: more rows tie at a partition's k-th distance than fit, the heap decides which stay"""
    x, cent = R.sized_partitions([40, 300], 16, seed=4, dup_block=200)
    q = queries(x, cent, 2, seed=2)
    rid = np.random.default_rng(6).permutation(len(x)).astype(np.uint64) * np.uint64(5) + np.uint64(1)
    P = R.rotations(16, seed=1)["qr"]
    assert run_case(emulator, oracle, x, q, cent, P, "l2", 10, 2, rid) > 0
    assert run_case(emulator, oracle, x, q, cent, P, "l2", 128, 2, rid, prefilter=np.arange(int(rid.max()) + 1) % 3 != 0) > 0


# ---- past two chunks: the mid-scan threshold and the ties it cuts (rq_spec.ordered_partition) ---------------------------------------
@pytest.mark.parametrize("order,k,prefiltered", [("staircase", 10, False), ("tie_then_closer", 10, False), ("tie_wide", 128, True),
                                                 ("tie_across_remainder", 10, False), ("tie_across_remainder", 10, True)])
def test_scan_past_two_chunks(emulator, oracle, order, k, prefiltered):
    """a partition of ~800 rows (four 256-row chunks) stored in an order chosen for the first query: after its first truncation the
    scan admits rows by its threshold alone.  staircase: every later row is exactly the new k-th (a threshold one rank too tight loses
    them); tie_then_closer: a tie cut at the first truncation is still the k-th key at the end; tie_wide: 300 copies over two chunks at
    k = 128; tie_across_remainder: copies on both sides of the packed / remainder boundary, one key under a prefilter, two without"""
    f = R.ordered_partition(oracle, order, "l2", k, prefiltered=prefiltered)
    x, cent = f["x"], f["cent"]
    q = np.ascontiguousarray(np.stack([f["q"], queries(x, cent, 1, seed=5)[0]]))
    rid = R.permuted_ids(len(x), 4)
    mask = np.ones(int(rid.max()) + 1, bool) if prefiltered else None
    replays = run_case(emulator, oracle, x, q, cent, f["P"], "l2", k, 2, rid, prefilter=mask)
    if f["cut_tie"]:
        assert replays > 0
    assert f["cut_tie"] or order in ("staircase", "tie_across_remainder")


def test_d136(emulator, oracle):
    """d = 136: eight full 16-blocks and a tail of 8 in every rotation dot, 17 code bytes per row (read byte by byte, rows not 16-byte
    aligned), 34 tables; one query is a centroid (zero residual in that partition: qmin == qmax there, not in the others)"""
    d = 136
    x, cent = R.sized_partitions([33, 0, 97], d, seed=d)
    q = queries(x, cent, 2, seed=7)
    q[1] = cent[2]
    run_case(emulator, oracle, x, q, cent, R.rotations(d, seed=6)["qr"], "l2", 10, 3, R.permuted_ids(len(x), 8))
