"""The DEVICE code of lance_amd/csrc/index_update.hip run on the CPU, lane by lane (tests/c/simt_emu), as a stand-alone program under
AddressSanitizer + UBSan, against tests/index_update_spec.py byte for byte.  The kernels' text -- and the host's choice of the access
width -- is cut out of the source at test time, so what runs here is what the GPU compiles.  This is the memory-safety check of the
gather / scatter indices of merge, remap and the unpadding export; stable_group is replaced by a host stable sort."""
import os
import re
import subprocess

import numpy as np
import pytest

import index_update_spec as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "lance_amd", "csrc", "index_update.hip")
EMU = os.path.join(ROOT, "tests", "c", "simt_emu")


def device_code():
    src = open(SRC).read()
    body = src[src.index("// ---- device code"):src.index("// ---- host side")]
    m = re.search(r"^static int iu_width\(", src, flags=re.M)
    depth, i = 0, src.index("{", m.end())
    while True:
        depth += {"{": 1, "}": -1}.get(src[i], 0)
        i += 1
        if depth == 0:
            break
    return body + src[m.start():i] + "\n"


def test_device_code_is_found():
    code = device_code()
    for name in ("iu_copy_rows_kernel", "iu_remap_keys_kernel", "iu_check_ascending_kernel", "iu_words_differ_kernel", "iu_partition_of", "iu_width"):
        assert name in code, name
    assert "hipLaunchKernelGGL" not in code and "LH_REQUIRE" not in code, "host code must stay out"
    for intrinsic in ("__shfl", "__ballot", "__any", "__popc", "atomic"):
        assert intrinsic not in code, f"the new kernels are plain loads and stores: {intrinsic}"


@pytest.fixture(scope="module")
def emulator(tmp_path_factory):
    work = tmp_path_factory.mktemp("index_update_emu")
    (work / "index_update_device_code.inc").write_text(device_code())
    exe = str(work / "index_update_kernels")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-pthread",
           "-I", str(work), "-I", EMU, os.path.join(EMU, "index_update_main.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    if r.returncode != 0 and "sanitize" in r.stderr:
        pytest.skip("g++ without sanitizer runtimes")
    assert r.returncode == 0, r.stderr[-3000:]
    return exe, work


def run(emulator, mode, nlist, sources, shift=0, unpad=0, mapping=None):
    """sources: [(offs, ids, payload [n, stride] u8, aux u32 | None)] -> (refused, offs, payload, ids, aux, unpadded, widths used)"""
    exe, work = emulator
    stride = sources[0][2].shape[1]
    has_aux = sources[0][3] is not None
    inp, outp = str(work / "in.bin"), str(work / "out.bin")
    with open(inp, "wb") as fh:
        np.array([mode, nlist, stride, shift, int(has_aux), unpad, len(sources)], np.uint32).tofile(fh)
        for offs, ids, payload, aux in sources:
            np.array([len(ids)], np.uint32).tofile(fh)
            offs.astype(np.uint32).tofile(fh); np.ascontiguousarray(payload, np.uint8).tofile(fh); ids.astype(np.uint64).tofile(fh)
            if has_aux:
                aux.astype(np.uint32).tofile(fh)
        if mode == 1:
            old, new = mapping
            np.array([len(old)], np.uint32).tofile(fh); old.astype(np.uint64).tofile(fh); new.astype(np.uint64).tofile(fh)
    r = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout[-1000:] + r.stderr[-4000:]
    raw = np.fromfile(outp, np.uint8)
    pos = 0

    def take(count, dt):
        nonlocal pos
        a = raw[pos:pos + count * np.dtype(dt).itemsize].view(dt)
        pos += count * np.dtype(dt).itemsize
        return a
    refused, n_out = take(2, np.uint32)
    offs = take(nlist + 1, np.uint32)
    payload = take(n_out * stride, np.uint8).reshape(n_out, stride)
    ids = take(n_out, np.uint64)
    aux = take(n_out, np.uint32) if has_aux else None
    flat = take(n_out * unpad, np.uint8).reshape(n_out, unpad) if unpad else None
    assert pos == raw.size
    return int(refused), offs, payload, ids, aux, flat, [int(w) for w in re.findall(r"copy width (\d+)", r.stdout)]


def sources_for(stride, sizes, nlist=5, seed=0, aux=False):
    rng = np.random.default_rng(seed + stride)
    out = []
    for j, n in enumerate(sizes):
        offs, ids, payload = S.random_storage(rng, nlist, n, stride, empty=(3,) if j != 1 else (3, 0), id_base=1000 * j)
        out.append((offs, ids, payload, rng.integers(0, 1 << 31, n).astype(np.uint32) if aux else None))
    return out


# strides: 8 (4-bit M=16), 12 (d=24, M=12), 16, 96 (an IVF_FLAT row of d=24), 32 (IVF_SQ d=20 padded, with its sums and an unpadding export)
@pytest.mark.parametrize("stride,shift,aux,unpad,width", [(8, 0, False, 0, 8), (12, 0, False, 0, 4), (16, 0, False, 0, 16), (96, 0, False, 0, 16),
                                                           (32, 0, True, 20, 16), (16, 4, False, 0, 4), (16, 1, False, 0, 1), (8, 8, False, 0, 8),
                                                           (16, 8, False, 0, 8), (96, 4, False, 0, 4), (96, 1, False, 0, 1), (8, 4, False, 0, 4)])
def test_merge_three_sources_one_empty(emulator, stride, shift, aux, unpad, width):
    srcs = sources_for(stride, (300, 0, 41), aux=aux)
    refused, offs, payload, ids, xx, flat, widths = run(emulator, 0, 5, srcs, shift=shift, unpad=unpad)
    cols = lambda s: [s[1], s[2]] + ([s[3]] if aux else [])
    want_offs, want = S.merge_storage([(s[0], cols(s)) for s in srcs])
    assert refused == 0 and np.array_equal(offs, want_offs)
    assert np.array_equal(ids, want[0]) and np.array_equal(payload, want[1])
    assert widths[0] == width and 8 in widths                    # the payload's pieces, and the row ids as 8-byte words
    if aux:
        assert np.array_equal(xx, want[2]) and 4 in widths
    if unpad:
        assert np.array_equal(flat, want[1][:, :unpad]) and widths[-1] == 4


@pytest.mark.parametrize("stride,shift,aux", [(8, 0, False), (12, 0, False), (16, 0, False), (96, 0, False), (32, 0, True), (16, 1, False), (16, 4, False),
                                              (16, 8, False)])
def test_remap(emulator, stride, shift, aux):
    (offs, ids, payload, xx), = sources_for(stride, (330,), aux=aux, seed=9)
    first, last = int(ids[0]), int(ids[-1])
    mapping = {first: None, last: None, int(ids[7]): int(ids[8]), int(ids[8]): int(ids[7]), int(ids[20]): (1 << 40) + 3, 10 ** 15: 1}
    mapping.update({int(i): None for i in ids[offs[1]:offs[2]]})           # a whole partition
    cols = [payload] + ([xx] if aux else [])
    for mp in (mapping, {}, {int(i): None for i in ids}):
        refused, o2, p2, i2, x2, _, _ = run(emulator, 1, 5, [(offs, ids, payload, xx)], shift=shift, mapping=S.mapping_arrays(mp))
        wo, wi, wc = S.remap_storage(offs, ids, cols, mp)
        assert refused == 0 and np.array_equal(o2, wo) and np.array_equal(i2, wi) and np.array_equal(p2, wc[0])
        assert not aux or np.array_equal(x2, wc[1])


def test_remap_refuses_unsorted_and_duplicate_old_ids(emulator):
    (offs, ids, payload, _), = sources_for(16, (100,), seed=3)
    for old in ([5, 3, 9], [3, 5, 5], [0] * 600 + [1, 1]):
        old = np.array(old, np.uint64)
        refused, o2, p2, i2, _, _, _ = run(emulator, 1, 5, [(offs, ids, payload, None)], mapping=(old, np.zeros(old.size, np.uint64)))
        assert refused == 1 and i2.size == 0 and p2.size == 0 and not o2.any()
    old = np.arange(700, dtype=np.uint64) * 3                              # ascending across the workgroups' boundary
    assert run(emulator, 1, 5, [(offs, ids, payload, None)], mapping=(old, old))[0] == 0
