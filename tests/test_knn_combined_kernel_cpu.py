"""The DEVICE code of lance_amd/csrc/combine.hip (take_flat_knn_kernel) run on the CPU, lane by lane (tests/c/simt_emu: a thread per
lane, a barrier for __syncthreads), under AddressSanitizer + UBSan, against the take_flat_knn model of tests/knn_combined_spec.py bit for
bit.  The kernel's text and the exact.cuh / search_common.cuh functions it calls are cut out of the sources at test time, so what runs
here is what the GPU compiles; the launch geometry and the dynamic LDS come from the library's own sizing functions, with guard bytes
behind the LDS; the column is allocated to the byte, so a read past a row -- or of a row id beyond the column -- is reported.  This
checks the logic and the memory safety without a device; the device's own arithmetic is what tests/test_zz_gpu_knn_combined.py checks."""
import os
import re
import subprocess

import numpy as np
import pytest

import flat_order_spec as FO
import knn_combined_spec as KC
from test_sq_kernels_cpu import function_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lance_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "c", "simt_emu")
f32 = np.float32
DTYPES = {"float32": 0, "float16": 1, "int8": 2}
METRIC_CODES = {"l2": 0, "cosine": 1, "dot": 2}


def flag_line(common):
    """the definition of the per-query flag bits in search_common.cuh, as it stands there"""
    m = re.search(r"^constexpr uint32_t [^\n;]*\bFLAG_BADROW = \d+u[^\n;]*;", common, flags=re.M)
    assert m, "search_common.cuh no longer defines FLAG_BADROW on one line"
    return m.group(0)


def flag_badrow():
    return int(re.search(r"FLAG_BADROW = (\d+)u", flag_line(open(os.path.join(CSRC, "search_common.cuh")).read())).group(1))


def device_code():
    read = lambda name: open(os.path.join(CSRC, name)).read()
    exact, common, combine = read("exact.cuh"), read("search_common.cuh"), read("combine.hip")
    parts = [flag_line(common) + "\n"] + [function_text(exact, n) for n in ("order_key", "key_to_float")]
    parts += [m.group(0) + "\n" for m in re.finditer(r"^__device__ __forceinline__ float ld_elem\([^\n]*$", exact, flags=re.M)]
    parts += [function_text(exact, n) for n in ("dist_exact_rt", "cosine_finish", "norm_l2_rt", "cosine_scalar32_rt", "reduce8_tree",
                                                "cosine_exact_rt", "finish_metric")]
    parts.append(function_text(common, "bitonic_sort_kr"))
    i = combine.index("// ---- take_flat_knn: device code")
    parts.append(combine[i:combine.index("// ---- take_flat_knn: end of the code the emulator program compiles", i)])
    return "".join(parts).replace("extern __shared__ __attribute__((aligned(16))) char smem[];", "")


def test_device_code_is_found():
    code = device_code()
    assert code.count("float ld_elem(") == 3
    for name in ("take_flat_knn_kernel", "tfk_distance", "take_flat_knn_bytes", "tfk_rows_per_step", "bitonic_sort_kr", "cosine_exact_rt", "dist_exact_rt"):
        assert name in code, name
    assert "hipLaunchKernelGGL" not in code and "LH_REQUIRE" not in code, "host code must stay out"


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    work = tmp_path_factory.mktemp("take_emu")
    (work / "take_device_code.inc").write_text(device_code())
    exe = str(work / "take_flat_knn")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", str(work), "-I", EMU, os.path.join(EMU, "take_flat_knn_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("g++ without sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, work


def run_case(emulator, oracle, x, q, a, k, metric, b=None, db=None, lower=None, upper=None, shift=0, want=None, bad=()):
    """-> the emulator's stdout; the outputs are compared with the model (want=None) unless `bad` names the flagged queries"""
    exe, work = emulator
    n, d = x.shape
    nq = q.shape[0]
    ca, cb = a.shape[1], 0 if b is None else b.shape[1]
    key = lambda v: 0 if v is None else int(FO.keys(np.asarray([v], f32))[0])
    inp, outp = str(work / "in.bin"), str(work / "out.bin")
    with open(inp, "wb") as fh:
        np.array([DTYPES[x.dtype.name], METRIC_CODES[metric], n, d, nq, ca, cb, int(db is not None), int(lower is not None), int(upper is not None),
                  k, shift], np.uint32).tofile(fh)
        np.array([key(lower), key(upper)], np.uint32).tofile(fh)
        np.ascontiguousarray(x).tofile(fh)
        np.ascontiguousarray(q.astype(x.dtype).astype(f32)).tofile(fh)
        np.ascontiguousarray(a, np.uint64).tofile(fh)
        if b is not None:
            np.ascontiguousarray(b, np.uint64).tofile(fh)
        if db is not None:
            np.ascontiguousarray(db, f32).tofile(fh)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-1000:] + r.stderr[-4000:]
    raw = np.fromfile(outp, np.uint8)
    ids = raw[:nq * k * 8].view(np.uint64).reshape(nq, k)
    dists = raw[nq * k * 8:nq * k * 12].view(f32).reshape(nq, k)
    flags = raw[nq * k * 12:].view(np.uint32)
    assert flags.size == nq
    assert (flags != 0).tolist() == [i in bad for i in range(nq)] and set(flags.tolist()) <= {0, flag_badrow()}
    if not bad:
        want = KC.take_flat_knn(oracle, x, q, a, k, metric, ids_b=b, dists_b=db, lower=lower, upper=upper) if want is None else want
        assert (ids == want[0]).all() and (dists.view(np.uint32) == want[1].view(np.uint32)).all()
    return r.stdout


def _rows(n, d, nq, seed, dtype="float32"):
    rng = np.random.default_rng(seed)
    if dtype == "int8":
        return rng.integers(-100, 101, (n, d)).astype(np.int8), rng.integers(-100, 101, (nq, d)).astype(np.int8)
    return (rng.standard_normal((n, d)) * 1.5 + 0.25).astype(dtype), (rng.standard_normal((nq, d)) * 1.5 - 0.25).astype(dtype)


def _lists(n, nq, ca, cb, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, n, (nq, ca)).astype(np.uint64)
    b = rng.integers(0, n, (nq, cb)).astype(np.uint64)
    a[rng.random(a.shape) < 0.1] = KC.UNSET
    b[rng.random(b.shape) < 0.1] = KC.UNSET
    b[:, 0] = a[:, 1]
    return a, b


@pytest.mark.parametrize("dtype,d,metric,vec", [("float32", 20, "l2", 1), ("float32", 3, "cosine", 0), ("float32", 32, "cosine", 1), ("float32", 17, "dot", 0),
                                                ("float16", 40, "cosine", 1), ("float16", 33, "dot", 0), ("float16", 8, "l2", 1),
                                                ("int8", 48, "l2", 1), ("int8", 5, "dot", 0)])
def test_rows_through_both_readers(emulator, oracle, dtype, d, metric, vec):
    """whole 16-byte words and element by element; several steps per wave (70 candidates of up to 160-byte rows: one step; see below)"""
    x, q = _rows(120, d, 2, d, dtype)
    a, b = _lists(120, 2, 40, 30, d + 1)
    out = run_case(emulator, oracle, x, q, a, 10, metric, b=b)
    assert f"vec {vec}\n" in out
    out = run_case(emulator, oracle, x, q, a, 10, metric, b=b, shift=4 if dtype == "float32" else 2 if dtype == "float16" else 1)
    assert "vec 0\n" in out                                 # off the 16-byte grid: the same answer, element by element


def test_several_steps_and_rows_in_place(emulator, oracle):
    """d = 700: two rows per wave and step, 9 steps for 70 candidates; d = 2100: rows longer than a slice, read in place, no stage in the LDS"""
    for d, rps in ((700, 2), (2100, 0)):
        x, q = _rows(90, d, 2, d)
        a, b = _lists(90, 2, 40, 30, d + 1)
        out = run_case(emulator, oracle, x, q, a, 7, "l2", b=b)
        assert f"rows_per_step {rps} " in out
        assert ("lds 34832 " if rps else "lds 2064 ") in out      # 128 entries x 16 + 16 (+ 4 slices of 8 KiB)


def test_bounds_given_distances_and_limits(emulator, oracle):
    x, q = _rows(200, 12, 2, 3)
    a, b = _lists(200, 2, 50, 30, 5)
    free = KC.take_flat_knn(oracle, x, q, a, 80, "l2", ids_b=b)
    lo, hi = float(free[1][0][4]), float(free[1][0][30])
    for lower, upper in ((lo, hi), (lo, None), (None, hi), (lo, lo)):
        run_case(emulator, oracle, x, q, a, 10, "l2", b=b, lower=lower, upper=upper)
    # list B's distances handed over: taken as they are (here the model's own: the same bits either way)
    db = np.full(b.shape, np.inf, f32)
    for i in range(2):
        for j, r in enumerate(b[i]):
            if r != KC.UNSET:
                db[i, j] = KC.take_flat_knn(oracle, x, q[i:i + 1], np.array([[r]], np.uint64), 1, "l2")[1][0, 0]
    run_case(emulator, oracle, x, q, a, 10, "l2", b=b, db=db, lower=lo, upper=hi, want=KC.take_flat_knn(oracle, x, q, a, 10, "l2", ids_b=b, lower=lo, upper=hi))
    # the limits: one candidate; 4096 candidates and k = 1024 (64 KiB of entries beside the slices)
    run_case(emulator, oracle, x, q[:1], np.array([[7]], np.uint64), 3, "dot")
    rng = np.random.default_rng(9)
    big = rng.integers(0, 200, (1, 4096)).astype(np.uint64)
    out = run_case(emulator, oracle, x, q[:1], big[:, :3072], 1024, "l2", b=big[:, 3072:])
    assert "lds 98320 " in out


def test_a_row_id_beyond_the_column_is_flagged_and_never_read(emulator, oracle):
    """the column ends with its last row (ASan guards the byte behind it): ids n, 2^40 and 2^64 - 2 set the query's flag and nothing else"""
    x, q = _rows(64, 16, 3, 11)
    a, b = _lists(64, 3, 20, 10, 13)
    a[1, 5], b[2, 3] = 64, 2 ** 40
    run_case(emulator, oracle, x, q, a, 5, "l2", b=b, bad=(1, 2))
    a[0, 0] = 2 ** 64 - 2
    run_case(emulator, oracle, x, q, a, 5, "cosine", b=b, db=np.zeros(b.shape, f32), bad=(0, 1, 2))
