"""The alignment gate of the lane-per-row residual + PQ encoder (lance_amd/csrc/encode_fused.hip) against the stores of its kernel, on
the CPU: `encode_fused_supported` and the statements that write a row's code bytes are cut out of the source at test time and run by
tests/c/encode_gate_main.cpp under AddressSanitizer + UBSan, for every instantiated shape and every byte offset of the caller's
`codes`.  A gate that lets a pointer through which the stores cannot take (the kernel writes 16-byte pieces at M = 16 / 32 and 4-byte
words at M = 8) is a misaligned-store report here, without a GPU.  tests/test_zz_gpu_unaligned.py::test_ivfpq_encode asserts the same
gate through the launch counters on the device."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "lance_amd", "csrc", "encode_fused.hip")


def braces(src, start):
    depth, i = 0, src.index("{", start)
    while True:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
        if depth == 0:
            return i


def anchor(src, text, what):
    assert text in src, f"encode_fused.hip no longer holds {text!r} ({what}): update the anchor in {os.path.basename(__file__)}"
    return src.index(text)


def gate_and_stores():
    src = open(SRC).read()
    g = anchor(src, "bool encode_fused_supported(", "the host's gate")
    gate = src[g:braces(src, g)]
    s = anchor(src, "  if (valid) {\n    uint8_t *dst = codes + row * M;", "the start of the kernel's code-row stores")
    stores = src[s:braces(src, s)]
    assert "reinterpret_cast<uint4 *>(dst" in stores and "reinterpret_cast<uint32_t *>(dst" in stores, "the kernel's code stores have changed shape"
    return gate + "\ntemplate <int M>\nstatic void store_row(uint8_t *codes, int64_t row, const uint32_t *packed) {\n  const bool valid = true;\n" + stores + "\n}\n"


def test_the_gate_admits_only_what_the_stores_can_take(tmp_path):
    (tmp_path / "encode_gate.inc").write_text(gate_and_stores())
    exe = str(tmp_path / "encode_gate")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-Wno-unknown-pragmas", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(tmp_path),
           "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "c", "encode_gate_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("g++ without sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env={k: v for k, v in os.environ.items() if k != "LANCE_HIP_NO_FUSED_ENCODE"})
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-1000:] + r.stderr[-3000:]
    # codes: 2 of 32 offsets at M = 16 / 32 (three shapes), 8 of 32 at M = 8 (two shapes); rows: 2 + 4 + 8 accepted starts of 32 bytes
    accepted = int(re.search(r"accepted (\d+)", r.stdout).group(1))
    assert accepted == (3 * 2 + 2 * 8) * (2 + 4 + 8)
