"""The kernels of the multivector ANN join (lance_amd/csrc/multivec_ann.hip: mva_sort_kernel, mva_score_kernel, mva_select_kernel) run
on the CPU, lane by lane (tests/c/simt_emu), as a stand-alone program under AddressSanitizer + UBSan, against tests/multivec_ann_spec.py
bit for bit.  The kernels' text is cut out of the source at test time, so what runs here is what the GPU compiles.  Every global buffer
has exactly the elements the library asks for, every launch states its dynamic LDS (checked against 64 KiB, the bytes behind it guarded).

The cases cover keff in {1, 2, 255, 256, 257, 4096} (the sort's power-of-two padding on either side of a boundary, the largest list) and
nqv in {1, 2, 64, 65, 256} (the limit; one more list than lanes in a wave), not their product: a lane is a thread here and a barrier
costs a millisecond."""
import os
import subprocess

import numpy as np
import pytest

import multivec_ann_spec as A
from test_sq_kernels_cpu import function_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lance_amd", "csrc")
EMU = os.path.join(ROOT, "tests", "c", "simt_emu")
f32 = np.float32


def device_code():
    read = lambda name: open(os.path.join(CSRC, name)).read()
    exact, src = read("exact.cuh"), read("multivec_ann.hip")
    i = src.index("// ---- multivector ANN: device code")
    body = src[i:src.index("// ---- multivector ANN: host side", i)]
    body = body.replace("extern __shared__ __attribute__((aligned(16))) char smem[];", "")
    return "".join(function_text(exact, n) for n in ("order_key", "key_to_float")) + body


def test_device_code_is_found():
    code = device_code()
    for name in ("mva_find", "mva_sort_kernel", "mva_score_kernel", "mva_select_kernel", "struct MvaArgs", "struct MvaSel", "order_key"):
        assert name in code, name
    assert "hipLaunchKernelGGL" not in code and "LH_REQUIRE" not in code and "extern __shared__" not in code, "host code must stay out"
    assert "__shared__" not in code, "static LDS would escape the launch's count"


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    work = tmp_path_factory.mktemp("mva_emu")
    (work / "multivec_ann_device_code.inc").write_text(device_code())
    exe = str(work / "multivec_ann")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", str(work), "-I", EMU, os.path.join(EMU, "multivec_ann_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("g++ without sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, work


def run(emulator, ids, dists, q_offsets, k_out):
    """the three kernels over the lists ids / dists [lists][keff] of the queries q_offsets -> (ids [B][k_out], dists, rows joined per query, stdout)"""
    exe, work = emulator
    inp, outp = str(work / "in.bin"), str(work / "out.bin")
    B, (lists, keff) = len(q_offsets) - 1, ids.shape
    with open(inp, "wb") as fh:
        np.array([B, keff, k_out, lists], np.uint32).tofile(fh)
        np.asarray(q_offsets, np.uint64).tofile(fh)
        np.ascontiguousarray(ids, np.uint64).tofile(fh)
        np.ascontiguousarray(dists, f32).tofile(fh)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-1000:] + r.stderr[-4000:]
    raw = np.fromfile(outp, np.uint8)
    n = B * k_out
    assert raw.size == n * 12 + B * 4
    return raw[:n * 8].view(np.uint64).reshape(B, k_out), raw[n * 8:n * 12].view(f32).reshape(B, k_out), raw[n * 12:].view(np.uint32), r.stdout


def check(emulator, ids, dists, q_offsets, k_out):
    gi, gd, joined, out = run(emulator, ids, dists, q_offsets, k_out)
    for b in range(len(q_offsets) - 1):
        sl = slice(int(q_offsets[b]), int(q_offsets[b + 1]))
        rows, _ = A.scores(ids[sl], dists[sl])
        oi, od = A.topk(ids[sl], dists[sl], k_out)
        assert joined[b] == rows.size, (b, joined[b], rows.size)          # every joined row emitted once, by the list that owns it
        assert (gi[b] == oi).all(), (b, np.argwhere(gi[b] != oi)[:4])
        assert (gd[b].view(np.uint32) == od.view(np.uint32)).all(), b
    return out


BIG = 1 << 40

# (nqv, keff, rows, k_out): the rows are fewer than the entries, so a row recurs inside a list and across lists
CASES = [(1, 1, 3, 1), (256, 2, 300, 10), (64, 255, 700, 100), (65, 256, 900, 10), (2, 257, 200, 1024), (5, 100, 150, 10)]


@pytest.mark.parametrize("nqv,keff,rows,k_out", CASES)
def test_against_the_specification(emulator, nqv, keff, rows, k_out):
    """full lists, short lists (padding behind the valid entries) and an empty one; row ids >= 2^40, three apart"""
    short = () if nqv < 2 else (1,) if nqv < 5 else (1, nqv - 1)
    ids, dists = A.random_lists(nqv, keff, rows, seed=100 + nqv + keff, id_base=BIG + 5, id_step=3, short=short, empty=(3,) if nqv >= 5 else ())
    check(emulator, ids, dists, [0, nqv], k_out)


def test_largest_list(emulator):
    """keff = 4096: the sort's 48 KiB; 2 x 4096 candidates over 3000 rows, k_out = 1024: four selection blocks, then two, then one"""
    ids, dists = A.random_lists(2, 4096, 3000, seed=7, id_base=BIG, id_step=7, short=(1,), dup=0.1)
    out = check(emulator, ids, dists, [0, 2], 1024)
    assert "largest dynamic LDS 49168 bytes, 3 selection rounds" in out


def test_all_duplicate_lists(emulator):
    """every entry of a list is the same row: one first occurrence per list, its sim the FIRST entry's, min_sim the LAST entry's"""
    rng = np.random.default_rng(3)
    lists = []
    for j in range(4):
        d = np.sort((rng.random(256) * 0.9).astype(f32))
        lists.append((np.full(256, BIG + (j % 2) * 11, np.uint64), d))
    ids, dists = A.pad_lists(lists, 256)
    check(emulator, ids, dists, [0, 4], 10)


def test_batch_of_queries(emulator):
    """three queries of 1, 5 and 2 vectors in one launch sequence; fewer joined rows than k_out in the first (padding)"""
    parts = [A.random_lists(n, 100, rows, seed=40 + n, id_base=BIG, short=(0,)) for n, rows in ((1, 20), (5, 300), (2, 150))]
    ids, dists = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    gi, gd, joined, _ = run(emulator, ids, dists, [0, 1, 6, 8], 40)
    assert joined[0] < 40 and (gi[0, joined[0]:] == A.U64_MAX).all() and np.isinf(gd[0, joined[0]:]).all()
    check(emulator, ids, dists, [0, 1, 6, 8], 40)


def test_order_fixture(emulator):
    ids, dists = A.order_fixture()
    check(emulator, ids, dists, [0, len(ids)], 400)
