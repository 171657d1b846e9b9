"""The front end of a batched IVF-PQ search: the coarse quantiser's fused kernel (mfma_assign.hip: coarse_fused_kernel) and the matrix-core
scan's residual pre-pass (search_ms.hip: ms_prep_rows_kernel, with ms_prep_kernel as its fall-back).

Coarse quantiser: a workgroup owns CF_ROWS = 32 queries and its CF_WAVES = 16 waves answer rows w and w + 16, so the row counts below sit on
both sides of every multiple of 16 up to two workgroups, and the batch of special rows (NaN, all-inf, more candidates than the kernel keeps)
is run twice, with the halves of every workgroup swapped: each kind of row is a wave's first row once and its second row once, beside a
normal partner, beside another special one and beside no partner at all.  Ids (uint32) and distances (bit patterns) must equal
`oracle.find_partitions`; `count:coarse_fused` rises by one per call.

Pre-pass: searches sized for the matrix-core route (pairs >= 4096 and >= 96 x lists).  `count:ivfpq_mscan` and `count:ms_prep_rows` rise by
one per search; with the query tensor 4 bytes off the 16-byte grid the element-wise kernel serves the batch (the second counter stays) and
the answers are the same.  A wave of the new kernel carries 16 pairs at d = 128 and 32 at d = 64: 32 consecutive query counts at 5 probes
walk the pair count through every remainder of both.  Ids and distances must equal the oracle's bit for bit.

LANCE_HIP_MFMA_COARSE=1 is read once per process: every group runs in a fresh child, in the manner of test_zz_gpu_coarse_fused.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CF_ROWS, CF_WAVES = 32, 16      # mfma_assign.hip
GATE = 960                      # mfma_assign.hip: CF_MAX_LISTS
# every row count one below, at and one above a multiple of CF_WAVES, up to two workgroups and one row
ROW_COUNTS = sorted({1, 2 * CF_ROWS + 1} | {n for b in range(CF_WAVES, 2 * CF_ROWS + 1, CF_WAVES) for n in (b - 1, b, b + 1)})


def _setup():
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle
    from lance_amd.engine import Engine
    oracle.lib()
    return oracle, Engine()


def _count(eng, name):
    return eng.timing_query("count:" + name)[1]


# ---- coarse quantiser ---------------------------------------------------------------------------------------------------------------
def _fp_eq(eng, oracle, q, cent, nprobes, metric, tag, ref=None):
    before = _count(eng, "coarse_fused")
    ids, d = eng.find_partitions(q, cent, nprobes, metric)
    served = _count(eng, "coarse_fused") - before
    oi, od = ref if ref is not None else oracle.find_partitions(q, cent, nprobes, metric)
    oi, od = oi[:len(q)], od[:len(q)]
    ids = ids.cpu().numpy().view(np.uint32); d = d.cpu().numpy()
    assert np.array_equal(ids, oi), (tag, "ids", np.argwhere(ids != oi)[:5])
    assert np.array_equal(d.view(np.uint32), od.view(np.uint32)), (tag, "distances", np.argwhere(d.view(np.uint32) != od.view(np.uint32))[:5])
    assert served == 1, (tag, "count:coarse_fused", served)


def _coarse_rows():
    """Child: d x lists x metric x nprobes, every row count of ROW_COUNTS (the oracle answers the longest batch once: queries are independent)"""
    oracle, eng = _setup()
    rng = np.random.default_rng(1601)
    n = 0
    for d in (64, 128):
        for nlist in (33, 256, GATE):
            for metric in ("l2", "dot"):
                cent = (rng.standard_normal((nlist, d)) * 3).astype(f32)
                q = (cent[rng.integers(0, nlist, max(ROW_COUNTS))] + rng.standard_normal((max(ROW_COUNTS), d)).astype(f32)).astype(f32)
                for nprobes in (1, 10, 64):
                    if nprobes > nlist:
                        continue
                    ref = oracle.find_partitions(q, cent, nprobes, metric)
                    for nq in ROW_COUNTS:
                        _fp_eq(eng, oracle, q[:nq], cent, nprobes, metric, (d, nlist, metric, nprobes, nq), ref)
                        n += 1
    eng.close()
    print(f"front end coarse rows ok: {n} calls")


def _coarse_mixed():
    """Child: d 64, 512 lists, integer-valued (the recipe of test_zz_gpu_coarse_fused._ties): rows that share a wave take different paths"""
    oracle, eng = _setup()
    rng = np.random.default_rng(2026)
    d, nlist = 64, 512
    cent = np.rint(rng.uniform(0, 40, (nlist, d))).astype(f32)
    cent[100:260] = cent[100]                      # 160 identical centroids > 128 candidates: the exact path inside the kernel
    nq = CF_ROWS + CF_WAVES // 2                   # the second workgroup's rows have no partner: w + 16 lies beyond nq
    q = np.rint(rng.uniform(0, 40, (nq, d))).astype(f32)
    nan_row = q[0].copy(); nan_row[2] = np.nan
    many_row = cent[100].copy()
    inf_row = np.full(d, np.inf, f32)
    kinds = {"nan": nan_row, "many": many_row, "inf": inf_row}
    # wave w: rows w and w + 16 of the first workgroup.  (first row, second row) per wave; None = a normal row
    plan = [("nan", None), ("many", None), ("inf", None), (None, "nan"), (None, "many"), (None, "inf"),
            ("nan", "many"), ("many", "inf"), ("inf", "nan"), ("many", "many"), ("nan", "nan"), ("inf", "inf")]
    special = np.zeros(nq, bool)
    for w, (a, b) in enumerate(plan):
        if a: q[w] = kinds[a]; special[w] = True
        if b: q[w + CF_WAVES] = kinds[b]; special[w + CF_WAVES] = True
    # ... and without a partner (second workgroup): one of each kind, normal rows between them
    for w, kind in ((1, "nan"), (3, "many"), (5, "inf")):
        q[CF_ROWS + w] = kinds[kind]; special[CF_ROWS + w] = True
    swapped = q.copy()                             # the halves of the first workgroup trade places: every kind in the other slot of its wave
    swapped[:CF_WAVES], swapped[CF_WAVES:CF_ROWS] = q[CF_WAVES:CF_ROWS], q[:CF_WAVES]
    # dot takes only the finite rows (inf x 0 and 1 - NaN carry a platform-dependent NaN sign: tests/test_zz_gpu_coarse_mfma.py)
    fin = np.rint(rng.uniform(0, 40, (nq, d))).astype(f32)
    for name, batch in (("as built", q), ("halves swapped", swapped)):
        bd = batch.copy()
        nonfinite = ~np.isfinite(bd).all(axis=1)
        bd[nonfinite] = fin[nonfinite]
        for nprobes in (1, 10, 64):
            with np.errstate(all="ignore"):
                _fp_eq(eng, oracle, batch, cent, nprobes, "l2", ("mixed", name, nprobes))
                _fp_eq(eng, oracle, bd, cent, nprobes, "dot", ("mixed dot", name, nprobes))
                # one row in the second workgroup: fifteen of its waves have no row at all
                _fp_eq(eng, oracle, batch[:CF_ROWS + 1], cent, nprobes, "l2", ("mixed, partner beyond nq", name, nprobes))
    assert special.sum() == 21
    eng.close()
    print("front end coarse mixed ok")


# ---- residual pre-pass --------------------------------------------------------------------------------------------------------------------
def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _off_view(t, nbytes):
    """a copy of the contiguous device tensor t that starts `nbytes` after a 256-byte boundary"""
    import torch
    size = t.numel() * t.element_size()
    buf = torch.empty(size + 512, dtype=torch.uint8, device=t.device)
    start = (-buf.data_ptr()) % 256 + nbytes
    v = buf[start:start + size].view(t.dtype).view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == nbytes % 16 and v.is_contiguous()
    return v


def _build(eng, oracle, x, cent, m, metric, seed=2):
    from lance_amd.engine import DeviceIndex
    km = "l2" if metric == "cosine" else metric
    xs = oracle.normalize(x.astype(f32)) if metric == "cosine" else x
    cent = cent.astype(x.dtype)
    part, _ = oracle.assign(xs, cent, km)
    res = oracle.residual(xs, cent, np.where(part == oracle.NONE, 0, part)) if km == "l2" else xs
    cb, _ = oracle.pq_train(res[:3072], m, max_iters=3, seed=seed)
    oidx = oracle.build_index(x, cent, cb, metric)
    gpart, gcodes, _ = eng.ivfpq_encode(x, cent, cb, metric)
    return DeviceIndex.create(eng, metric, cent, cb, gpart, gcodes, None, raw=x), oidx


def _trained(eng, oracle, x, nlist, m, metric):
    km = "l2" if metric == "cosine" else metric
    xs = oracle.normalize(x.astype(f32)) if metric == "cosine" else x
    cent, _, _, _ = oracle.kmeans_train(xs[:2048].astype(f32), nlist, max_iters=4, seed=1, metric=km)
    return _build(eng, oracle, x, cent, m, metric)


def _rows(n, d, seed, dot=False):      # tests/search_routes_spec.py: _rows
    rng = np.random.default_rng(seed)
    centers = rng.uniform(0, 128, (24, d))
    x = np.clip(np.rint(centers[rng.integers(0, 24, n)] + rng.normal(0, 20, (n, d))), 0, 218).astype(f32)
    return x - f32(64.0) if dot else x


def _search_eq(eng, gidx, qd, ref, k, nprobes, rf, rows_expected, tag):
    """one search of the device tensor qd; ref = the oracle's (ids, distances) for a superset of the rows; rows_expected: how often the
    whole-row pre-pass must have run (None: either kernel)"""
    before = (_count(eng, "ivfpq_mscan"), _count(eng, "ms_prep_rows"))
    gi, gd = gidx.search(qd, k, nprobes, rf, engine=eng)
    eng.synchronize()
    ran = (_count(eng, "ivfpq_mscan") - before[0], _count(eng, "ms_prep_rows") - before[1])
    nq = qd.shape[0]
    gi = gi.cpu().numpy().view(np.uint64); gd = gd.cpu().numpy().view(np.uint32)
    oi, od = ref[0][:nq], ref[1][:nq].view(np.uint32)
    bad = np.nonzero((gi != oi).any(axis=1))[0]
    assert bad.size == 0, (tag, f"ids differ for {bad.size} of {nq} queries (first {bad[:5]})")
    bad = np.nonzero((gd != od).any(axis=1))[0]
    assert bad.size == 0, (tag, f"distances differ for {bad.size} of {nq} queries (first {bad[:5]})")
    assert ran[0] == 1 and rows_expected in (None, ran[1]), (tag, "count:ivfpq_mscan, count:ms_prep_rows", ran)


def _prep_shapes():
    """Child: every shape x metric of the matrix-core scan, 8 lists, 1024 queries x 4 probes = 4096 pairs; aligned and 4 bytes off"""
    oracle, eng = _setup()
    for d, m in ((128, 16), (128, 32), (64, 16)):
        for metric in ("l2", "cosine", "dot"):
            x = _rows(4000, d, 7 + d + m, metric == "dot") + (f32(1.0) if metric == "cosine" else f32(0.0))
            q = _rows(1024, d, 8 + d + m, metric == "dot") + (f32(1.0) if metric == "cosine" else f32(0.0))
            gidx, oidx = _trained(eng, oracle, x, 8, m, metric)
            qd = _dev(q)
            for k, rf in ((10, 0), (10, 2)):
                ref = oidx.search(q, k, 4, refine=rf, raw=x if rf else None)
                _search_eq(eng, gidx, qd, ref, k, 4, rf, 1, (d, m, metric, k, rf))
            # 4 bytes off: dot leaves the matrix-core route (search_plan.h); cosine normalises the queries into a buffer of the library's
            # own, which is on the grid again: only the answers are asserted there
            if metric != "dot":
                _search_eq(eng, gidx, _off_view(qd, 4), ref, 10, 4, 2, 0 if metric == "l2" else None, (d, m, metric, "q + 4 bytes"))
            gidx.close()
    eng.close()
    print("front end prep shapes ok")


def _prep_f16():
    """Child: an f16 column: the residual is rounded to f16 before anything else (round_f16)"""
    oracle, eng = _setup()
    rng = np.random.default_rng(19)
    n, d, m, nlist, nq = 8000, 128, 16, 8, 1024
    c = rng.standard_normal((16, d)) * 2
    x = (c[rng.integers(0, 16, n)] + rng.standard_normal((n, d)) * 0.7).astype(np.float16)
    q = (c[rng.integers(0, 16, nq)] + rng.standard_normal((nq, d)) * 0.7).astype(np.float16)
    gidx, oidx = _build(eng, oracle, x, x[rng.choice(n, nlist, replace=False)].copy(), m, "l2")
    for k, nprobes, rf in ((10, 4, 0), (10, 5, 3)):
        ref = oidx.search(q, k, nprobes, refine=rf, raw=x.astype(f32) if rf else None)
        _search_eq(eng, gidx, _dev(q), ref, k, nprobes, rf, 1, ("f16", k, nprobes, rf))
    gidx.close()
    eng.close()
    print("front end prep f16 ok")


def _prep_remainders():
    """Child: 5 probes x 32 consecutive query counts: the pair count takes every remainder of 16 and of 32 pairs per wave"""
    oracle, eng = _setup()
    for d in (128, 64):
        x = _rows(4000, d, 31 + d)
        q = _rows(832 + 32, d, 32 + d)
        gidx, oidx = _trained(eng, oracle, x, 8, 16, "l2")
        ref = oidx.search(q, 10, 5)
        qd = _dev(q)
        for nq in range(832, 832 + 32):      # 832 x 5 = 4160 pairs = 130 x 32
            _search_eq(eng, gidx, qd[:nq].contiguous(), ref, 10, 5, 0, 1, (d, "nq", nq))
        gidx.close()
    eng.close()
    print("front end prep remainders ok")


def _uneven(oracle, rng, d):
    """12 lists of 400 rows where the queries are, 5 far-away lists: four of 40 rows and one of 4 (fewer than k: a query there has no bound)"""
    main = rng.uniform(0, 128, (12, d))
    far = np.full((5, d), 64.0)
    for i in range(5):
        far[i, 7 * i] += 3000.0 * (1 if i % 2 == 0 else -1)      # each along an axis of its own
    cent = np.rint(np.concatenate([main, far])).astype(f32)
    sizes = [400] * 12 + [40, 40, 40, 40, 4]
    x = np.concatenate([np.rint(cent[i] + rng.normal(0, 20, (s, d))) for i, s in enumerate(sizes)]).astype(f32)
    x = x[rng.permutation(len(x))]
    return x, cent


def _prep_uneven_and_special():
    """Child: lists that receive 1 to 3 pairs (a wave's pairs span many lists); an overflowing residual, a NaN query, a query without a bound"""
    oracle, eng = _setup()
    rng = np.random.default_rng(77)
    d, m, nlist, nq, nprobes, k = 128, 16, 17, 1100, 4, 10
    x, cent = _uneven(oracle, rng, d)
    gidx, oidx = _build(eng, oracle, x, cent, m, "l2")
    q = np.rint(cent[rng.integers(0, 12, nq)] + rng.normal(0, 20, (nq, d))).astype(f32)
    # far lists 12 .. 15 receive 1, 2, 3 and 1 queries (their other probes are main lists: the far lists lie along different axes)
    at = iter(range(100, 1000, 97))
    for lst, cnt in ((12, 1), (13, 2), (14, 3), (15, 1)):
        for _ in range(cnt):
            q[next(at)] = np.rint(cent[lst] + rng.normal(0, 20, d)).astype(f32)
    oi, _ = oracle.find_partitions(q, cent, nprobes, "l2")
    per_list = np.bincount(oi.ravel().astype(np.int64), minlength=nlist)
    assert ((per_list >= 1) & (per_list <= 3)).sum() >= 4, per_list
    assert nq * nprobes >= 4096 and nq * nprobes >= 96 * nlist
    ref = oidx.search(q, k, nprobes)
    _search_eq(eng, gidx, _dev(q), ref, k, nprobes, 0, 1, "uneven lists")
    ref = oidx.search(q, k, nprobes, refine=3, raw=x)
    _search_eq(eng, gidx, _dev(q), ref, k, nprobes, 3, 1, "uneven lists, refine")
    # the special queries, between normal ones
    qs = q.copy()
    qs[200] = cent[3]; qs[200, 5] += 30000.0       # |residual| sigma overflows binary16: the pair goes to the exact rescan
    qs[201] = cent[4]; qs[201, 9] = np.nan         # a NaN query
    qs[202] = cent[16]                             # its nearest list holds 4 rows < k: no bound (class B)
    with np.errstate(all="ignore"):
        ref = oidx.search(qs, k, nprobes)
    _search_eq(eng, gidx, _dev(qs), ref, k, nprobes, 0, 1, "special queries")
    _search_eq(eng, gidx, _off_view(_dev(qs), 4), ref, k, nprobes, 0, 0, "special queries, q + 4 bytes")
    gidx.close()
    eng.close()
    print("front end prep uneven ok")


def _child(call, **env):
    e = dict(os.environ, LANCE_HIP_MFMA_COARSE="1")
    for name in ("LANCE_HIP_NO_COARSE_FUSED", "LANCE_HIP_COARSE_GROUPS", "LANCE_HIP_COARSE_GROUPS_MA", "LANCE_HIP_NO_MS_PREP_ROWS", "LANCE_HIP_NO_MSCAN",
                 "LANCE_HIP_MSCAN_MINQ"):
        e.pop(name, None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", "import sys; sys.path.insert(0, %r); import tests.test_zz_gpu_front_end as t; t.%s" % (ROOT, call)],
                       cwd=ROOT, env=e, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_coarse_row_counts_around_every_wave_boundary():
    assert "front end coarse rows ok" in _child("_coarse_rows()")


def test_coarse_rows_sharing_a_wave_take_different_paths():
    assert "front end coarse mixed ok" in _child("_coarse_mixed()")


def test_prepass_every_shape_and_metric_aligned_and_four_bytes_off():
    assert "front end prep shapes ok" in _child("_prep_shapes()")


def test_prepass_f16_column():
    assert "front end prep f16 ok" in _child("_prep_f16()")


def test_prepass_pair_count_remainders():
    assert "front end prep remainders ok" in _child("_prep_remainders()")


def test_prepass_uneven_lists_and_special_queries():
    assert "front end prep uneven ok" in _child("_prep_uneven_and_special()")
