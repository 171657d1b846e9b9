"""The CPU specification of IVF_RQ (tests/rq_spec.py) checked against itself and against the oracle's sums: no GPU involved.  The GPU
kernels are held to this specification bit for bit by tests/test_zz_gpu_rq.py, their source run on the CPU by
tests/test_rq_kernels_cpu.py."""
import itertools

import numpy as np
import pytest

import rq_spec as R

f32, f64 = np.float32, np.float64


@pytest.mark.parametrize("d", [8, 16, 24, 40, 64, 128])
def test_dot16_is_the_oracles_dot(oracle, d):
    """the vectorised restatement of lance_linalg::distance::dot used for the rotation equals the oracle's scalar one, tail included"""
    rng = np.random.default_rng(d)
    a = rng.standard_normal((6, d)).astype(f32) * f32(3.0)
    b = rng.standard_normal(d).astype(f32)
    got = R.dot16(a, b[None, :])
    want = np.array([oracle.dot(a[i], b) for i in range(6)], f32)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    assert (R.rotate(a, b[None])[0].view(np.uint32) == want.view(np.uint32)).all()


def test_lowbit_table_is_the_subset_sums():
    """t[s][j] = sum of rq[4 s + i] over the bits i of j: on small integers every partial sum is exact, so any order gives it"""
    rq = np.random.default_rng(1).integers(-50, 50, 32).astype(f32)
    t = R.dist_table(rq)
    assert t.shape == (8, 16)
    for s, j in itertools.product(range(8), range(16)):
        assert t[s, j] == sum(float(rq[4 * s + i]) for i in range(4) if j >> i & 1)


def test_quantised_table_rounds_half_away_and_saturates_like_as_u8():
    t = np.array([[0.0, 0.5, 1.5, 2.5, 254.5, 255.0] + [1.0] * 10], f32)
    qmin, qmax, e = R.quantise_table(t)
    assert (qmin, qmax) == (0.0, 255.0)
    assert list(e[0, :6]) == [0, 1, 2, 3, 255, 255]          # half-even would give 0, 2, 2, 254
    qmin, qmax, e = R.quantise_table(np.zeros((2, 16), f32))
    assert qmin == qmax and not e.any()
    t = np.zeros((1, 16), f32); t[0, 3] = -0.0                # total_cmp: -0.0 < +0.0, but they compare equal -> all zero
    qmin, qmax, e = R.quantise_table(t)
    assert np.signbit(qmin) and not np.signbit(qmax) and not e.any()


def test_packed_and_remainder_branches_agree_on_an_integer_table():
    """P = I and a query whose table holds integers with qmax - qmin = 255: factor and range are exactly 1, every quantised entry
    is t - qmin exactly, so the integer branch and the f32 branch give the same distance for every row"""
    d = 64
    qr = np.random.default_rng(2).integers(0, 4, d).astype(f32)
    qr[:4] = [97.0, 60.0, 50.0, 45.0]                         # segment 0 spans 0 .. 252
    qr[8] = -3.0                                              # the smallest entry of the whole table: 252 - (-3) = 255
    c = R.Query(qr, 0.0, np.eye(d, dtype=f32), "l2")
    assert c.qmax - c.qmin == 255.0 and (c.table == np.rint(c.table)).all()
    codes = np.random.default_rng(3).integers(0, 256, (64, d // 8)).astype(np.uint8)
    packed, flat = c.raw_packed(codes), c.raw_f32(codes, 0.0)
    assert (packed.view(np.uint32) == flat.view(np.uint32)).all()
    add = np.arange(64, dtype=f32); scale = -np.ones(64, f32)
    both = c.distance_all(codes, add, scale)                  # 64 rows: all packed
    one_by_one = c.distance(codes, add, scale)
    assert (both.view(np.uint32) == one_by_one.view(np.uint32)).all()
    mixed = c.distance_all(codes[:33], add[:33], scale[:33])  # 32 packed + 1 remainder
    assert (mixed.view(np.uint32) == one_by_one[:33].view(np.uint32)).all()


def test_u16_sum_saturates():
    d = 1536
    c = R.Query(np.ones(d, f32), 0.0, np.eye(d, dtype=f32), "l2")      # every table spans 0 .. 4: e = round(t * 63.75)
    assert c.e.max() == 255
    ones = np.full((1, d // 8), 255, np.uint8)
    raw = c.raw_packed(ones)
    assert raw[0] == f32(65535.0) * c.table.max() / f32(255.0) and d // 4 * 255 == 97920


@pytest.mark.parametrize("metric", ["l2", "dot"])
def test_formula_reproduces_the_reconstruction_with_identity_rotation(oracle, metric):
    """P = I and inputs on which every operation is exact (small dyadic rationals, d = 16 so that sqrt(d) = 4): the estimator is
    |q - v^|^2 (L2) or 1 - q . v^ (dot) for the reconstruction v^ = c + (res2 / (ip sqrt d)) sign(r) the factors define, in f64."""
    d = 16
    rng = np.random.default_rng(4)
    cent = rng.integers(-2, 3, (2, d)).astype(f32)
    x = (cent[rng.integers(0, 2, 12)] + rng.choice([-0.5, 0.5], (12, d))).astype(f32)      # |r_i| = 0.5: ip = 8 / 4 = 2, res2 = 4
    part = np.array([int(np.argmin([np.abs(np.abs(x[i] - c) - 0.5).sum() for c in cent])) for i in range(12)], np.uint32)
    r = x - cent[part]
    assert (np.abs(r) == 0.5).all()
    dvc = np.array([oracle.l2(x[i], cent[part[i]]) if metric == "l2" else 1.0 - oracle.dot(x[i], cent[part[i]]) for i in range(12)], f32)
    codes, add, scale = R.encode(x, part, dvc, cent, np.eye(d, dtype=f32), metric)
    assert (np.unpackbits(codes, axis=1, bitorder="little").astype(bool) == (r > 0)).all()
    q = rng.integers(-3, 4, (5, d)).astype(f32)
    for qi in range(5):
        for p in range(2):
            rows = np.nonzero(part == p)[0]
            dqc = oracle.l2(q[qi], cent[p]) if metric == "l2" else 1.0 - oracle.dot(q[qi], cent[p])
            calc = R.Query(q[qi] - cent[p], dqc, np.eye(d, dtype=f32), metric)
            got = calc.distance(codes[rows], add[rows], scale[rows])
            vhat = cent[p].astype(f64) + (4.0 / (2.0 * 4.0)) * np.sign(r[rows].astype(f64))
            want = ((q[qi].astype(f64) - vhat) ** 2).sum(axis=1) if metric == "l2" else 1.0 - vhat @ q[qi].astype(f64)
            assert (got.astype(f64) == want).all(), (metric, qi, p)


def test_zero_residual_and_signed_zero_bits():
    d = 8
    cent = np.ones((1, d), f32)
    x = np.ones((3, d), f32)
    x[1, 0] = 1.5
    x[2] = [1.0, 0.5, 1.0, 1.0, 2.0, 1.0, 1.0, 1.0]
    # a product -1 * (+0.0) = -0.0 does not survive the dot: its accumulators start at +0.0 and (+0.0) + (-0.0) = +0.0, so a rotated
    # component is never -0.0 and a zero component always sets its bit (is_sign_positive(+0.0))
    P = np.eye(d, dtype=f32); P[3, 3] = -1.0
    part = np.zeros(3, np.uint32)
    codes, add, scale = R.encode(x, part, np.array([0.0, 0.25, 1.25], f32), cent, P, "l2")
    assert codes[0, 0] == 0b11111111 and scale[0] == 0.0 and not np.signbit(scale[0])       # ip == 0
    assert codes[2, 0] == 0b11111101 and codes[1, 0] == 0b11111111
    _, _, sd = R.encode(x, part, np.zeros(3, f32), cent, P, "dot")
    assert sd[0] == 0.0 and np.signbit(sd[0])                 # the reference negates unwrap_or_default()


# ---- the ordered partitions of the scan tests (rq_spec.ordered_partition asserts what each order is for) -------------------------
ORDERED = [(order, k) for order, (_, ks) in R.ORDERS.items() for k in ks]


def chunked_scan(keys, k, tight=0):
    """the selection rq_scan_kernel makes over one partition, every row a candidate: candidates pile up chunk by chunk, are sorted by
    (key, position) and cut to k once more than CHUNK are held, and from then on a row enters only with key <= the k-th key kept.
    tight = 1 takes the (k - 1)-th key as that threshold: the fault a scan test must notice.  -> positions kept"""
    held, thr = [], None
    for base in range(0, len(keys), R.CHUNK):
        held += [(int(keys[p]), p) for p in range(base, min(base + R.CHUNK, len(keys))) if thr is None or keys[p] <= thr]
        if len(held) > R.CHUNK:
            held = sorted(held)[:k]
            thr = held[k - 1 - tight][0]
    return [p for _, p in sorted(held)[:k]]


@pytest.mark.parametrize("prefiltered", [False, True])
@pytest.mark.parametrize("metric", ["l2", "dot"])
@pytest.mark.parametrize("order,k", ORDERED)
def test_ordered_partition(oracle, order, k, metric, prefiltered):
    f = R.ordered_partition(oracle, order, metric, k, prefiltered=prefiltered)
    keys, N = f["keys"], f["N"]
    assert f["x"].shape == (N + 40, 64) and N == R.ORDERS[order][0] and N > R.FIRST_CUT + R.CHUNK
    want = list(np.lexsort((np.arange(N), keys))[:k])
    assert chunked_scan(keys, k) == want
    if order == "staircase":
        assert chunked_scan(keys, k, tight=1) != want          # a threshold one rank too tight loses the rows of the last chunk
    if order in ("tie_then_closer", "tie_across_chunk", "tie_wide") or (order == "tie_across_remainder" and prefiltered):
        assert f["cut_tie"]
    if order in ("descending", "ascending", "staircase", "tie_then_displaced"):
        assert not f["cut_tie"]
    again = R.ordered_partition(oracle, order, metric, k, prefiltered=prefiltered)
    assert (again["x"].view(np.uint32) == f["x"].view(np.uint32)).all() and (again["q"] == f["q"]).all()      # seeded: every caller gets the same


RECALL_AT_10 = 0.2867


def test_recall_sanity(oracle):
    """Clustered Gaussian rows 4000 x 64, 8 lists, every list probed, k = 10, L2, the seeded QR rotation: recall@10 of the CPU
    specification against the exact flat search, measured once: 0.2867 over 30 queries (86 of 300).  One bit per dimension in 64 dimensions
    ranks coarsely (the reference re-ranks IVF_RQ candidates for that reason); what this guards is the formula's sign conventions --
    a flipped sign of scale, sum_q or q_factor drops the recall to the level of chance (k / n = 0.0025)."""
    x, q = R.clustered(4000, 64, 30, seed=7)
    rng = np.random.default_rng(8)
    cent = np.ascontiguousarray(x[rng.choice(4000, 8, replace=False)])
    P = R.rotation(64, 9)
    part, codes, add, scale = R.build(oracle, x, cent, P, "l2")
    ids, _ = R.search(oracle, codes, add, scale, part, cent, P, q, 10, 8, "l2")
    exact, _ = oracle.flat_knn(x, q, 10, "l2")
    recall = np.mean([len(set(ids[i]) & set(np.asarray(exact[i], np.uint64))) / 10.0 for i in range(len(q))])
    print("recall@10", recall)
    assert recall >= RECALL_AT_10 - 0.02
