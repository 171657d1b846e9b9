"""Shared by tests/test_refine_spec.py (CPU), tests/test_wide_cand_kernels_cpu.py (CPU) and tests/test_zz_gpu_refine_sqrq.py (GPU): the
CPU specification of an IVF_SQ / IVF_RQ search with a refine_factor, and partitions whose storage order is chosen for one query at
any k.

The specification (scanner.rs:2884-2904, knn.rs:642): the ANN node is asked for keff = k * refine_factor rows -- sq_spec.search /
rq_spec.search with k = keff: a heap of keff per probed partition, the (dist, rowid) merge, fetch keff --, the rows are taken by row id
and re-scored by flat_knn in the index's metric with the ORIGINAL query: oracle.flat_knn(raw[cand], q, k, metric, row_ids=cand).  raw
is indexed by row id; f16 rows are taken as f16.  Missing slots are id ~0 and distance +inf."""
import numpy as np

import rq_spec as R
import sq_spec as S

f32 = np.float32
UNSET = np.uint64(np.iinfo(np.uint64).max)
CHUNK = 256
WIDE_MAX = 768                         # keff of the widest search
MIN_CAP = 1024                         # the smallest wide candidate buffer: 768 kept + one chunk


def refine(oracle, cand, raw, q, k, metric):
    """cand u64 [nq][keff] (~0 = none) -> (ids u64 [nq][k], dists f32 [nq][k]) by the exact distance of q to raw[cand]"""
    raw = np.asarray(raw)
    q = np.asarray(q).reshape(-1, raw.shape[1])
    out_i = np.full((q.shape[0], k), UNSET, np.uint64)
    out_d = np.full((q.shape[0], k), np.inf, f32)
    for qi in range(q.shape[0]):
        c = cand[qi][cand[qi] != UNSET]
        if len(c):
            out_i[qi], out_d[qi] = (a[0] for a in oracle.flat_knn(np.ascontiguousarray(raw[c.astype(np.int64)]), q[qi:qi + 1], k, metric, row_ids=c))
    return out_i, out_d


def rq_search_refine(oracle, codes, add, scale, part_ids, centroids, P, q, k, refine_factor, nprobes, metric, raw, row_ids=None, prefilter=None):
    cand, _ = R.search(oracle, codes, add, scale, part_ids, centroids, P, q, k * refine_factor, nprobes, metric, row_ids=row_ids, prefilter=prefilter)
    return refine(oracle, cand, raw, q, k, metric)


def sq_search_refine(oracle, codes, part_ids, centroids, q, k, refine_factor, nprobes, metric, start, end, raw, row_ids=None, prefilter=None):
    cand, _ = S.search(oracle, codes, part_ids, centroids, q, k * refine_factor, nprobes, metric, start, end, row_ids=row_ids, prefilter=prefilter)
    return refine(oracle, cand, raw, q, k, metric)


def raw_by_row_id(x, row_ids):
    """the column as set_raw takes it: raw[row_ids[i]] = x[i] (row ids below len(raw); rows no id names are zero)"""
    rid = np.asarray(row_ids, np.uint64).astype(np.int64)
    raw = np.zeros((int(rid.max()) + 1, x.shape[1]), x.dtype)
    raw[rid] = x
    return raw


def recall(ids, truth):
    return float(np.mean([len(set(a.tolist()) & set(b.tolist())) / len(b) for a, b in zip(ids, truth)]))


# ---- one partition whose storage order is chosen for one query, any k -----------------------------------------------------------------
# rq_spec.ordered_partition at any k and any buffer capacity.  A scan that holds `cap` candidates and reads CHUNK rows per step sorts and
# cuts to k once more than cap - CHUNK are held: with every row a candidate the first cut follows storage position cap - 1, and from then on
# a row enters only with a key <= the k-th key of the last cut.
ORDERS = ("descending", "ascending", "staircase", "tie_cut")
SQ_BOUNDS = (-2.0, 6.0)                # fixed quantiser bounds of the IVF_SQ fixtures (codes do not depend on which rows are stored)


class _Redraw(Exception):
    pass


def ordered_partition(oracle, kind, order, metric, k, cap, N, d=64, prefiltered=False, seed=0, small=40):
    """kind "rq" | "sq".  Partition 0 of two (explicit centroids 4 e_0, 4 e_1; partition 1 holds `small` rows): N rows stored in `order`
    for the design query q, by the keys of the branch the search will use.
        descending   farthest first: after the first cut every row enters at rank 0
        ascending    nearest first: nothing enters after the first cut
        staircase    the k - 1 nearest, then the rest farthest first: every later row is exactly the new k-th
        tie_cut      k + 8 copies of the row at rank k // 2 inside the first `cap` rows, the k // 2 nearer rows after them: the first cut
                     cuts the tie block, and the block still holds the k-th key at the end (the heap decides which copies stay)
    IVF_RQ without a prefilter scores the last N % 32 rows by another branch: they are the farthest rows by that branch, fixed first.
    -> dict: x [N + small][d] (input order = storage order), cent, q, keys u32 [N] (storage order), cut_tie, N; rq: P, built (rq_spec.build
    of x: at d = 1024 the numpy rotation takes seconds); sq: bounds"""
    assert kind in ("rq", "sq") and order in ORDERS and 2 <= k <= cap - CHUNK and cap % CHUNK == 0
    assert N > cap + 2 * CHUNK, "the scan passes two chunks after its first cut"
    for draw in range(16):
        try:
            return _ordered_partition(oracle, kind, order, metric, k, cap, N, d, prefiltered, seed, small, draw)
        except _Redraw:
            pass
    raise AssertionError("no usable draw")


def _ordered_partition(oracle, kind, order, metric, k, cap, N, d, prefiltered, seed, small, draw):
    cent = np.zeros((2, d), f32)
    cent[0, 0] = cent[1, 1] = 4.0
    P = R.rotation(d, seed + 5) if kind == "rq" else None
    rem = N % R.BATCH if kind == "rq" and not prefiltered else 0
    head_n = N - rem
    rng = np.random.default_rng([seed, k, cap, N, int(prefiltered), ORDERS.index(order), int(metric == "dot"), int(kind == "sq"), draw])
    gauss = lambda n: rng.standard_normal((n, d)).astype(f32) * f32(0.25)
    pool = N + 256                                         # spare rows: IVF_RQ rows whose key another row shares are left out
    rows, other, q = (cent[0] + gauss(pool)).astype(f32), (cent[1] + gauss(small)).astype(f32), (cent[0] + gauss(1)[0] + gauss(1)[0]).astype(f32)
    pr, pd = oracle.find_partitions(q[None], cent, 2, metric)
    assert pr[0, 0] == 0, "the design query's nearest partition is partition 0"

    def branch_keys(r):
        """(keys by the branch of the rows before the remainder, keys by the remainder's branch) of rows r as members of partition 0"""
        if kind == "sq":
            kk = R.order_key(S.distances(S.encode(r, *SQ_BOUNDS), q[None], metric, *SQ_BOUNDS)[0])
            return kk, kk
        calc = R.Query(q - cent[0], pd[0, 0], P, metric)
        part, codes, add, scale = R.build(oracle, r, cent, P, metric)
        assert (part == 0).all()
        if prefiltered:
            kk = R.order_key(calc.distance(codes, add, scale))
            return kk, kk
        return R.order_key(calc.finish(calc.raw_packed(codes), add, scale)), R.order_key(calc.finish(calc.raw_f32(codes, 0.0), add, scale))

    kh, kt = branch_keys(rows)
    keep = np.ones(pool, bool)
    while True:
        chosen = np.nonzero(keep)[0][:N]
        if len(chosen) < N:
            raise _Redraw("too many generated rows share a key")
        by_tail = chosen[np.argsort(kt[chosen], kind="stable")]
        tail = by_tail[head_n:]                            # the remainder rows: the farthest by the branch they will take
        asc = by_tail[:head_n][np.argsort(kh[by_tail[:head_n]], kind="stable")]      # the rows before them, nearest first
        members = np.concatenate([asc, tail])
        _, first = np.unique(np.concatenate([kh[asc], kt[tail]]), return_index=True)
        if len(first) == N or kind == "sq":                # (IVF_SQ keys are integer sums: equal keys are part of that fixture)
            break
        keep[members[np.setdiff1d(np.arange(N), first)]] = False
    if order == "descending":
        head = asc[::-1]
    elif order == "ascending":
        head = asc
    elif order == "staircase":
        head = np.concatenate([asc[:k - 1], asc[k - 1:][::-1]])
    else:
        j, copies = k // 2, k + 8
        assert 100 + copies <= cap and head_n >= cap + 50 + j
        src = asc[j]
        dst = asc[head_n - (copies - 1):]                  # the farthest rows become the copies
        rows[dst] = rows[src]
        tie = np.concatenate([[src], dst])
        near = asc[:j]
        rest = asc[j + 1:head_n - (copies - 1)]
        rest = rest[rng.permutation(len(rest))]
        head = np.concatenate([rest[:100], tie, rest[100:cap - copies + 50], near, rest[cap - copies + 50:]])
    layout = np.concatenate([head, tail]).astype(np.int64)
    assert len(layout) == N and len(np.unique(layout)) == N
    x = np.ascontiguousarray(np.concatenate([rows[layout], other]).astype(f32))

    # ---- the final layout, from scratch ---------------------------------------------------------------------------------------------
    if kind == "sq":
        _, part = S.prepare_rows(oracle, x, cent, metric)
        dist = S.distances(S.encode(x[:N], *SQ_BOUNDS), q[None], metric, *SQ_BOUNDS)[0]
    else:
        part, codes, add, scale = R.build(oracle, x, cent, P, metric)
        calc = R.Query(q - cent[0], pd[0, 0], P, metric)
        dist = calc.distance(codes[:N], add[:N], scale[:N]) if prefiltered else calc.distance_all(codes[:N], add[:N], scale[:N])
    keys = R.order_key(dist)
    assert (part[:N] == 0).all() and (part[N:] == 1).all()
    first = np.sort(keys[:cap])
    strict = kind == "rq"
    if order == "descending":
        later = keys[cap:head_n]
        assert (later[1:] < later[:-1]).all() if strict else (later[1:] <= later[:-1]).all()
        assert later[0] < keys[:cap].min() if strict else later[0] <= keys[:cap].min()     # every later row enters, at rank 0
    elif order == "ascending":
        assert (keys[cap:] > first[k - 1]).all() if strict else (keys[cap:] >= first[k - 1]).all()      # nothing needs to enter after the first cut
    elif order == "staircase":
        if strict:
            for p in (cap, cap + CHUNK, N - rem - 1):
                s = np.sort(keys[:p])
                assert s[k - 2] < keys[p] < s[k - 1]       # exactly the new k-th: the threshold falls step by step
    else:
        tk = keys[np.nonzero(layout == src)[0][0]]
        tied = np.nonzero(keys == tk)[0]
        assert len(tied) >= copies and (tied.max() < cap or not strict)
        assert first[k - 1] == tk and first[k] == tk       # the first cut cuts the tie
        final = np.sort(keys)
        assert final[k - 1] == tk and final[k] == tk and (keys < tk).sum() < k
        pos = np.arange(N, dtype=np.uint64)
        heap = set(oracle.heap_topk(dist, pos, k)[0].tolist())
        if heap == set(np.lexsort((pos, keys))[:k].tolist()):
            raise _Redraw("the heap happens to keep the first copies by position")
    out = {"x": x, "cent": cent, "q": q, "keys": keys, "cut_tie": bool(R.kth_is_tied(keys, k)), "N": N}
    if kind == "rq":
        out["P"], out["built"] = P, (part, codes, add, scale)
    else:
        out["bounds"] = SQ_BOUNDS
    return out
