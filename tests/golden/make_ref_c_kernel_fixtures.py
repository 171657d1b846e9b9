"""Generates tests/golden/ref_c_kernels.npz: what the reference's two stand-alone C kernels (oracle/_ref, built by
`make -C oracle ref` where the reference tree is present) return on the seeded inputs of
tests/test_oracle_golden.py::test_sum_4bit_dist_table_known_answer_and_reference_c and ::test_f16_kernels_against_reference_c,
so that those tests check the oracle against the reference's numbers on every machine.  Only outputs are stored; the tests
regenerate the inputs from the same seeds.

Run from the repository root after `make -C oracle ref`: python tests/golden/make_ref_c_kernel_fixtures.py
"""
import ctypes as C
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.join(os.path.dirname(os.path.dirname(HERE)), "oracle", "_ref")
F16_DIMS = (4, 16, 20, 128, 333, 1536)
DT_CODE_LENS = (2, 4, 8)


def dist_table_outputs(ref):
    rng = np.random.default_rng(0)
    outs = []
    for code_len in DT_CODE_LENS:
        codes = rng.integers(0, 256, 32 * code_len, dtype=np.uint8)
        dt = rng.integers(0, 256, code_len * 32, dtype=np.uint8)
        out = np.zeros(32, np.uint16)
        ref.sum_4bit_dist_table_32bytes_batch_avx512(codes.ctypes.data_as(C.c_void_p), C.c_size_t(codes.size),
                                                     dt.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        outs.append(out)
    return np.stack(outs)


def f16_outputs(ref):
    """Per dimension: l2, dot, norm, cosine on the integer-valued pair, then l2, dot, norm, cosine on the real-valued pair
    (cosine of the integer pair is NaN where a vector is all zeros: the test does not call it there)."""
    for fn in (ref.l2_f16_avx2, ref.dot_f16_avx2, ref.norm_l2_f16_avx2, ref.cosine_f16_avx2):
        fn.restype = C.c_float
    ref.cosine_f16_avx2.argtypes = [C.c_void_p, C.c_float, C.c_void_p, C.c_uint32]
    rng = np.random.default_rng(12)
    rows = []
    for d in F16_DIMS:
        row = []
        xi = rng.integers(-6, 7, d).astype(np.float16)
        yi = rng.integers(-6, 7, d).astype(np.float16)
        for pair in ("int", "real"):
            if pair == "real":
                x = (rng.standard_normal(d) * 2).astype(np.float16)
                y = (rng.standard_normal(d) * 2).astype(np.float16)
            else:
                x, y = xi, yi
            px, py = x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p)
            n = ref.norm_l2_f16_avx2(px, C.c_uint32(d))
            cos = ref.cosine_f16_avx2(px, C.c_float(n), py, C.c_uint32(d)) if (x != 0).any() and (y != 0).any() else np.nan
            row += [ref.l2_f16_avx2(px, py, C.c_uint32(d)), ref.dot_f16_avx2(px, py, C.c_uint32(d)), n, cos]
        rows.append(row)
    return np.array(rows, np.float32)


if __name__ == "__main__":
    dt = dist_table_outputs(C.CDLL(os.path.join(REF, "libref_dist_table.so")))
    f16 = f16_outputs(C.CDLL(os.path.join(REF, "libref_f16.so")))
    np.savez(os.path.join(HERE, "ref_c_kernels.npz"), dist_table_u16=dt, dist_table_code_lens=np.array(DT_CODE_LENS),
             f16_values=f16, f16_dims=np.array(F16_DIMS))
    print("wrote", os.path.join(HERE, "ref_c_kernels.npz"), dt.shape, f16.shape)
