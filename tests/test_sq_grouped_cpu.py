"""The partition-major IVF_SQ scan (lance_amd/csrc/sq_pm.cuh) without a device: the identity that takes the signed matrix product back to
the unsigned sum of products, in the int32 arithmetic the kernel uses, and the plan that chooses the scan."""
import numpy as np
import pytest


@pytest.mark.parametrize("ld", [16, 16384])
@pytest.mark.parametrize("codes", ["zeros", "full", "random"])
def test_offset_identity_stays_inside_int32(ld, codes):
    """xq = S + 128 sum(x) + 128 sum(q) - 16384 ld with S = sum((x - 128)(q - 128)) over the ld staged bytes: every operation is done in
    int32 with numpy's overflow checks on, in the kernel's order, and the result is the u8 dot product"""
    rng = np.random.default_rng(ld)
    make = {"zeros": lambda: np.zeros(ld, np.uint8), "full": lambda: np.full(ld, 255, np.uint8), "random": lambda: rng.integers(0, 256, ld).astype(np.uint8)}[codes]
    for x, q in ((make(), make()), (make(), 255 - make())):
        sx, sq = (x ^ 0x80).view(np.int8).astype(np.int32), (q ^ 0x80).view(np.int8).astype(np.int32)      # the staged operands: bit 7 flipped
        with np.errstate(over="raise"):
            S = np.int32(0)
            for lo in range(0, ld, 32):                          # the accumulator after every K step of the matrix instruction
                S = S + np.sum(sx[lo:lo + 32] * sq[lo:lo + 32], dtype=np.int32)
                assert abs(int(S)) <= ld * 128 * 128
            qterm = np.int32(128) * np.sum(q, dtype=np.int32) - np.int32(16384) * np.int32(ld)
            xq = S + np.int32(128) * np.sum(x, dtype=np.int32) + qterm
        assert int(xq) == int(np.dot(x.astype(np.int64), q.astype(np.int64)))


def test_plan():
    from lance_amd import _lib
    plan = _lib.load().lance_hip_ivfsq_plan
    G = 64                                                       # SQPM_MIN_PAIRS_PER_LIST
    assert plan(10000, 10, 256, 10, 0) == 1                      # the measured shape: 390 pairs per partition
    assert plan(10000, 10, 256, 128, 0) == 1 and plan(10000, 10, 256, 129, 0) == 0
    assert plan(10000, 10, 256, 10, 1) == 0                      # LANCE_HIP_NO_SQ_GROUPED
    assert plan(G * 256 // 2, 2, 256, 10, 0) == 1 and plan(G * 256 // 2 - 1, 2, 256, 10, 0) == 0      # nq * nprobes against G * nlist
    assert plan(96, 2, 3, 10, 0) == 1 and plan(95, 2, 3, 10, 0) == 0
    assert plan(100, 4, 16, 20, 0) == 0                          # 25 pairs per partition
    assert plan(65535, 65, 65536, 128, 0) == 1 and plan(65535, 64, 65536, 128, 0) == 0      # 64-bit products
