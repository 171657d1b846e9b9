"""The DEVICE code of lance_amd/csrc/rebalance.hip run on the CPU, lane by lane (tests/c/simt_emu), as a stand-alone program under
AddressSanitizer + UBSan, against tests/rebalance_spec.py bit for bit.  The kernel's text, the exact.cuh functions it calls and the host's
choice between the staged and the in-place route are cut out of the sources at test time, so what runs here is what the GPU compiles.
Every buffer has the size the library's contract gives it and the LDS block ends where the launch's request ends: this is the
memory-safety check of the gather by row id, the segment search and the LDS layout."""
import collections
import os
import re
import subprocess

import numpy as np
import pytest

import rebalance_spec as R
from test_sq_kernels_cpu import function_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lance_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "c", "simt_emu")
METRIC = {"l2": 0, "cosine": 1, "dot": 2}


def device_code():
    exact, src = open(os.path.join(CSRC, "exact.cuh")).read(), open(os.path.join(CSRC, "rebalance.hip")).read()
    parts = ["enum { METRIC_L2 = 0, METRIC_COSINE = 1, METRIC_DOT = 2 };\n"]
    parts += [function_text(exact, n) for n in ("order_key", "key_to_float", "ld_elem", "dist_exact_rt", "norm_l2_rt", "reduce8_tree",
                                                "cosine_exact_rt", "finish_metric")]
    body = src[src.index("// ---- device code"):src.index("// ---- host side")]
    parts.append(body.replace("extern __shared__ __attribute__((aligned(16))) char smem[];", ""))
    m = re.search(r"^static int64_t rb_lds_bytes\(", src, flags=re.M)
    depth, i = 0, src.index("{", m.end())
    while True:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
        if depth == 0:
            break
    parts.append(src[m.start():i] + "\n")
    return "".join(parts)


def test_device_code_is_found():
    code = device_code()
    for name in ("rb_reassign_kernel", "rb_dist", "rb_lds_bytes", "cosine_exact_rt", "dist_exact_rt", "norm_l2_rt", "order_key"):
        assert name in code, name
    assert "hipLaunchKernelGGL" not in code and "LH_REQUIRE" not in code and "extern __shared__" not in code, "host code must stay out"
    for intrinsic in ("__shfl", "__ballot", "__popc", "atomic"):
        assert intrinsic not in code, f"the decision kernel uses no cross-lane operation and no atomic: {intrinsic}"


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    work = tmp_path_factory.mktemp("rebalance_emu")
    (work / "rebalance_device_code.inc").write_text(device_code())
    exe = str(work / "rebalance_kernels")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", str(work), "-I", EMU, os.path.join(EMU, "rebalance_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("g++ without sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, work


def run(emulator, metric, mode, raw, ids, seg_offs, seg_cent, cand_ids, c12, part1, part2, shift=0):
    """-> (flag, staged, dest)"""
    exe, work = emulator
    inp, outp = str(work / "in.bin"), str(work / "out.bin")
    d, C = raw.shape[1], len(cand_ids)
    with open(inp, "wb") as fh:
        np.array([METRIC[metric], mode, d, len(raw), len(ids), C, part1, part2], np.uint32).tofile(fh)
        np.ascontiguousarray(raw, np.float32).tofile(fh); np.asarray(ids, np.uint64).tofile(fh); np.asarray(seg_offs, np.uint32).tofile(fh)
        np.ascontiguousarray(seg_cent, np.float32).tofile(fh); np.asarray(cand_ids, np.uint32).tofile(fh)
        if mode == R.SPLIT:
            np.ascontiguousarray(c12, np.float32).tofile(fh)
    r = subprocess.run([exe, inp, outp] + ([str(shift)] if shift else []), capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-1000:] + r.stderr[-4000:]
    out = np.fromfile(outp, np.uint32)
    assert out.size == 2 + len(ids)
    return int(out[0]), int(out[1]), out[2:]


def split_both(emulator, c):
    want = R.split_dest(c["metric"], c["centroids"], c["offs"], c["ids"], c["part"], c["raw"], c["c12"])
    flag, staged, dest = run(emulator, c["metric"], R.SPLIT, c["raw"], c["ids"][want["pos"]], want["seg_offs"], want["seg_cent"], want["cands"],
                             c["c12"], c["part"], len(c["centroids"]))
    return want, flag, staged, dest


# d = 20: a tail of 4 after one chunk of 16; 8 and 16: cosine_once; 33: an odd length; n = 700 / 1900: the last tile of either workgroup is partial
@pytest.mark.parametrize("metric", ["l2", "cosine", "dot"])
@pytest.mark.parametrize("nlist,d", [(1, 8), (2, 16), (5, 20), (70, 33)])
def test_split_dest_equals_the_specification(emulator, metric, nlist, d):
    c = R.make_case(3, nlist, d, metric, n=1900 if nlist == 5 else 700)
    want, flag, staged, dest = split_both(emulator, c)
    assert flag == 0 and staged == 1 and len(want["cands"]) == min(64, nlist - 1)
    assert np.array_equal(dest, want["dest"]), collections.Counter(np.asarray(want["what"])[dest != want["dest"]])
    seen = collections.Counter(want["what"])
    if nlist == 5:
        assert all(seen[o] > 0 for o in R.OUTCOMES), seen


@pytest.mark.parametrize("metric", ["l2", "cosine", "dot"])
@pytest.mark.parametrize("tie", ["c1=c0", "c1=c2", "candidates"])
def test_ties_take_the_less_or_equal_branches(emulator, metric, tie):
    c = R.make_case(29, 5, 20, metric, n=500, tie=tie)
    want, flag, _, dest = split_both(emulator, c)
    assert flag == 0 and np.array_equal(dest, want["dest"])
    if tie == "c1=c2":
        assert set(dest.tolist()) <= {c["part"], R.NONE} | set(want["cands"]) and (dest == c["part"]).any()


# the largest d at which 64 candidates are staged in LDS, and the first one past it
@pytest.mark.parametrize("metric,d,staged", [("l2", 141, 1), ("cosine", 141, 1), ("l2", 142, 0), ("cosine", 143, 0), ("dot", 142, 0)])
def test_the_in_place_route_past_64_kib(emulator, metric, d, staged):
    c = R.make_case(7, 70, d, metric, n=400, shaped=False)
    want, flag, took, dest = split_both(emulator, c)
    assert flag == 0 and took == staged and len(want["cands"]) == 64
    assert np.array_equal(dest, want["dest"])


@pytest.mark.parametrize("metric", ["l2", "cosine", "dot"])
@pytest.mark.parametrize("nlist,d", [(2, 8), (5, 20), (70, 16), (70, 150)])
def test_join_dest_equals_the_specification(emulator, metric, nlist, d):
    c = R.make_case(11, nlist, d, metric, n=600, shaped=False)
    want = R.join_dest(metric, c["centroids"], c["offs"], c["ids"], c["part"], c["raw"])
    flag, staged, dest = run(emulator, metric, R.JOIN, c["raw"], c["ids"][want["pos"]], want["seg_offs"], want["seg_cent"], want["cand_ids"],
                             None, 0, 0)
    assert flag == 0 and staged == (d < 100) and len(dest) > 32
    assert np.array_equal(dest, want["dest"])
    assert set(dest.tolist()) <= set(want["cand_ids"].tolist()) and dest.max() < nlist - 1      # the numbering without the joined partition


@pytest.mark.parametrize("metric,nlist,d,staged", [("l2", 5, 20, 1), ("cosine", 5, 16, 1), ("dot", 70, 142, 0)])
def test_raw_off_the_16_byte_grid(emulator, metric, nlist, d, staged):
    """The raw vectors are the caller's: a slice of an f32 column starts on a 4-byte boundary only.  Both readers of `raw` (the copy into
    LDS and the in-place route past 64 KiB) with the base 4 and 8 bytes off the grid, the block ending with the last row: the same
    destinations as the aligned run and the specification, nothing read past a row, no access wider than the element."""
    c = R.make_case(17, nlist, d, metric, n=400, shaped=nlist == 5)
    want = R.split_dest(metric, c["centroids"], c["offs"], c["ids"], c["part"], c["raw"], c["c12"])
    args = (emulator, metric, R.SPLIT, c["raw"], c["ids"][want["pos"]], want["seg_offs"], want["seg_cent"], want["cands"], c["c12"], c["part"],
            len(c["centroids"]))
    aligned = run(*args)
    assert aligned[0] == 0 and aligned[1] == staged and np.array_equal(aligned[2], want["dest"])
    for shift in (4, 8):
        flag, took, dest = run(*args, shift=shift)
        assert flag == 0 and took == staged and np.array_equal(dest, aligned[2]), shift


def test_row_ids_out_of_range_raise_the_flag_and_are_never_read(emulator):
    c = R.make_case(13, 5, 20, "l2", n=300)
    want = R.split_dest("l2", c["centroids"], c["offs"], c["ids"], c["part"], c["raw"], c["c12"])
    ids = c["ids"][want["pos"]].copy()
    n_raw = len(c["raw"])
    bad = [0, 31, 32, len(ids) - 1]
    ids[bad] = [n_raw, n_raw + 1, 1 << 40, 2 ** 64 - 1]
    spec, what = R.reassign("l2", R.SPLIT, c["raw"], ids, want["seg_offs"], want["seg_cent"], np.asarray(want["cands"], np.uint32), c["c12"],
                            c["part"], 5)
    flag, _, dest = run(emulator, "l2", R.SPLIT, c["raw"], ids, want["seg_offs"], want["seg_cent"], want["cands"], c["c12"], c["part"], 5)
    assert flag == 1 and np.array_equal(dest, spec) and (dest[bad] == R.NONE).all() and [what[b] for b in bad] == ["bad id"] * 4
