"""The partition-major IVF_RQ scan (lance_amd/csrc/rq_pm.cuh) without a device: the identity that turns the u8 table lookups of a row
into a signed matrix product of its one-hot expansion, in the int32 arithmetic the kernel uses, and the plan that chooses the scan."""
import numpy as np
import pytest

import rq_spec as R


@pytest.mark.parametrize("d", [8, 256, 2048])
@pytest.mark.parametrize("table", ["zeros", "full", "random"])
def test_onehot_product_is_the_lookup_sum(d, table):
    """per K step (one code byte: segments 2b and 2b + 1) the accumulator gains onehot . (etab ^ 0x80 as i8); acc + 32 d is the lookup sum
    of rq_spec, and min(., 65535) behind it is the reference's saturating u16 sum"""
    rng = np.random.default_rng(d)
    e = {"zeros": np.zeros((d // 4, 16), np.uint8), "full": np.full((d // 4, 16), 255, np.uint8),
         "random": rng.integers(0, 256, (d // 4, 16)).astype(np.uint8)}[table]
    codes = rng.integers(0, 256, (5, d // 8)).astype(np.uint8)
    calc = R.Query(np.ones(d, np.float32), 0.0, np.eye(d, dtype=np.float32), "l2")
    calc.e, calc.qmin, calc.qmax = e, np.float32(0.0), np.float32(255.0)          # range 1, sum_min 0: raw_packed returns the saturated sum
    want = calc.raw_packed(codes)
    signed = (e ^ 0x80).view(np.int8).astype(np.int32)
    for row, w in zip(codes, want):
        with np.errstate(over="raise"):
            acc = np.int32(0)
            for b, code in enumerate(row):
                onehot = np.zeros((2, 16), np.int32)
                onehot[0, code & 15] = onehot[1, code >> 4] = 1
                acc = acc + np.sum(onehot * signed[2 * b:2 * b + 2], dtype=np.int32)
                assert abs(int(acc)) <= 128 * 2 * (b + 1)
            s = acc + np.int32(32 * d)
        b = np.arange(d // 8)
        assert int(s) == int(e[2 * b, row & 15].astype(np.int64).sum() + e[2 * b + 1, row >> 4].astype(np.int64).sum())
        assert np.float32(min(int(s), 65535)) == w
    if table == "full":
        assert (want == 65535).all() == (d == 2048)                    # 255 d / 4 passes 65535 from d = 1032 on


def test_plan():
    from lance_amd import _lib
    plan = _lib.load().lance_hip_ivfrq_plan
    G, DMAX = 128, 584                                            # rq_pm.cuh: RQPM_MIN_PAIRS_PER_LIST; the last d whose block fits 160 KiB of LDS
    assert plan(10000, 10, 256, 10, 128, 0, 0) == 1              # the measured shape: 390 pairs per partition
    assert plan(10000, 10, 256, 128, 128, 0, 0) == 1 and plan(10000, 10, 256, 129, 128, 0, 0) == 0
    assert plan(10000, 10, 256, 10, 128, 1, 0) == 0              # a prefilter: every row takes the f32 fold
    assert plan(10000, 10, 256, 10, 128, 0, 1) == 0              # LANCE_HIP_NO_RQ_GROUPED
    assert plan(10000, 10, 256, 10, DMAX, 0, 0) == 1 and plan(10000, 10, 256, 10, DMAX + 8, 0, 0) == 0
    assert all(plan(10000, 10, 256, 10, d, 0, 0) == 1 for d in range(8, 257, 8)) and plan(10000, 10, 256, 10, 2048, 0, 0) == 0
    assert plan(G * 256 // 2, 2, 256, 10, 64, 0, 0) == 1 and plan(G * 256 // 2 - 1, 2, 256, 10, 64, 0, 0) == 0      # nq * nprobes against G * nlist
    assert plan(G * 3 // 2, 2, 3, 10, 8, 0, 0) == 1 and plan(G * 3 // 2 - 1, 2, 3, 10, 8, 0, 0) == 0
    assert plan(65535, 129, 65536, 128, 128, 0, 0) == 1 and plan(65535, 128, 65536, 128, 128, 0, 0) == 0              # 64-bit products
    assert plan(2 ** 31, 4, 65536, 10, 128, 0, 0) == 1                                                               # (2^33 pairs: 0 in 32 bits)
