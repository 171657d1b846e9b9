"""Index maintenance on the GPU (lance_amd/csrc/index_update.hip): merge / append, remap / delete and the row-major export for IVF_PQ,
IVF_FLAT and IVF_SQ, against tests/index_update_spec.py and against the code that existed before -- ONE `create` over the concatenated
(or surviving) shuffle columns.  Rows are moved, never recomputed: everything is compared for equality, every stored byte through
export_rows and the searches through their (ids, distances).  The kernels' indices are checked on the CPU first
(tests/test_index_update_kernels_cpu.py).  Sorted last: newest device code last.

Layout of the fixture (7 partitions, supplied centroids): partition 5 receives no row of any source (its centroid is out of reach),
partition 6 none of the base (only the delta's rows come from its cluster); the base's partitions exceed 256 rows, so IVF_FLAT's
block list has several entries per partition; the delta repeats rows of the base, so ties are ordered by the layout."""
import ctypes as C
import functools

import numpy as np
import pytest

import index_update_spec as S

pytestmark = pytest.mark.gpu
f32 = np.float32
NLIST, N_BASE, N_DELTA, N_THIRD = 7, 3000, 1500, 37
N_ALL = N_BASE + N_DELTA + N_THIRD
K = 10


def eng():
    import lance_amd
    return lance_amd.default_engine()


@functools.lru_cache(maxsize=None)
def data(d, metric="l2", kind="f32"):
    """-> (centroids [7, d], [base, delta, third] rows, [their row ids], queries): row ids continue across the sources"""
    rng = np.random.default_rng(100 + d)
    cent = rng.normal(0, 4, (NLIST, d)).astype(f32)
    if metric == "cosine":                                      # unit centroids: rows are assigned in L2 after normalisation
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    cent[5] = 0.0 if metric == "dot" else (6e4 if kind == "f16" else 1e6)      # never the nearest: a zero dot product / a far point
    spread = 0.1 if metric == "cosine" else 1.0
    draw = lambda n, clusters: (cent[rng.choice(clusters, n)] + rng.normal(0, spread, (n, d))).astype(f32)
    base = draw(N_BASE, [0, 1, 2, 3, 4])
    delta = draw(N_DELTA, [0, 1, 2, 3, 4, 6, 6])
    delta[:200] = base[100:300]                                # the same vectors again, later in every partition
    third = draw(N_THIRD, [0, 1])
    third[:5] = base[100:105]
    q = np.concatenate([base[100:108], delta[300:304], draw(4, [0, 6])])
    if kind == "f16":
        cent, base, delta, third, q = (a.astype(np.float16) for a in (cent, base, delta, third, q))
    xs = [base, delta, third]
    starts = np.cumsum([0] + [len(x) for x in xs])
    return cent, xs, [np.arange(starts[i], starts[i + 1], dtype=np.uint64) for i in range(3)], q


def transposed(offs, codes):
    """row-major codes -> the per-partition [code bytes][n_p] blocks lance_hip_index_export hands out"""
    return np.concatenate([codes[offs[p]:offs[p + 1]].T.reshape(-1) for p in range(len(offs) - 1)] + [np.zeros(0, np.uint8)])


def same(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


def same_search(a, b):
    import torch
    return torch.equal(a[0], b[0]) and torch.equal(a[1].view(torch.int32), b[1].view(torch.int32))


def layout_ok(offs_base, offs_delta):
    cnt = lambda o: np.diff(o.astype(np.int64))
    return cnt(offs_base)[5] == 0 and cnt(offs_delta)[5] == 0 and cnt(offs_base)[6] == 0 and cnt(offs_delta)[6] > 100 and cnt(offs_base)[:5].min() > 256


# ---- sources of one kind: device indices over base / delta / third / nothing, and the columns they were built from ----------------
class Sources:
    def __init__(self, kind, d, metric="l2", m=0, nbits=8, elem="f32"):
        import torch
        from lance_amd import vector as V
        from lance_amd.engine import DeviceFlatIndex, DeviceIndex, DeviceSqIndex, to_device
        self.kind, self.metric, self.e = kind, metric, eng()
        cent, xs, rids, q = data(d, metric, elem)
        self.q, self.x_all = q, np.concatenate(xs)
        self.cent = to_device(cent)
        self.cb = self.bounds = None
        if kind == "IVF_PQ":
            rng = np.random.default_rng(m + nbits)
            self.cb = to_device(rng.normal(0, 1.5, (m, 1 << nbits, d // m)).astype(cent.dtype))
        if kind == "IVF_SQ":
            self.bounds = self.e.sq_bounds(xs[0][:512])        # a sample's bounds: later rows clip
        self.cols = []                                          # (part ids, payload, row ids) per source, on the device
        for x, rid in zip(xs, rids):
            part, payload = V._transform_rows(self.e, kind, metric, to_device(x), self.cent, codebook=self.cb, bounds=self.bounds)
            self.cols.append((part, payload, to_device(rid)))
        none = (torch.full((1,), -1, dtype=torch.int32, device=self.cent.device), self.cols[0][1][:1], self.cols[0][2][:1])
        self.cols.append(none)                                  # a source with no rows: its one row has no partition
        self.ix = [self.create(*c) for c in self.cols]

    def create(self, part, payload, rid, raw=None, cb=None, bounds=None):
        from lance_amd.engine import DeviceFlatIndex, DeviceIndex, DeviceSqIndex
        if self.kind == "IVF_PQ":
            return DeviceIndex.create(self.e, self.metric, self.cent, self.cb if cb is None else cb, part, payload, rid, raw=raw)
        if self.kind == "IVF_FLAT":
            return DeviceFlatIndex.create(self.e, self.metric, self.cent, payload, part, rid)
        return DeviceSqIndex.create(self.e, self.metric, self.cent, payload, part, self.bounds if bounds is None else bounds, rid)

    def one_create(self, raw=None):
        """the yardstick: ONE create over the concatenated columns"""
        import torch
        return self.create(*(torch.cat([c[i] for c in self.cols]) for i in range(3)), raw=raw)

    @staticmethod
    def stored(ix):
        """export_rows as (offs, [row ids, payload, (sums)]) -- the spec's form"""
        out = ix.export_rows()
        return out[0], [out[-1]] + list(out[1:-1])


@functools.lru_cache(maxsize=None)
def sources(kind, d, metric="l2", m=0, nbits=8, elem="f32"):
    return Sources(kind, d, metric, m, nbits, elem)


PQ_CASES = [(32, 8, 8, "l2", "f32"), (32, 16, 8, "l2", "f32"), (32, 16, 4, "l2", "f32"), (24, 12, 8, "l2", "f32"), (32, 8, 8, "dot", "f32"),
            (32, 16, 4, "dot", "f32"), (32, 8, 8, "l2", "f16")]
FLAT_SQ_CASES = [("IVF_FLAT", 8, "l2"), ("IVF_FLAT", 20, "l2"), ("IVF_FLAT", 8, "cosine"), ("IVF_FLAT", 20, "cosine"), ("IVF_SQ", 20, "l2"),
                 ("IVF_SQ", 32, "l2"), ("IVF_SQ", 32, "dot")]
ONE_OF_EACH = [("IVF_PQ", 32, "l2", 8, 8), ("IVF_PQ", 32, "l2", 16, 4), ("IVF_FLAT", 20, "l2", 0, 8), ("IVF_SQ", 20, "l2", 0, 8)]


# ---- 4. merge, IVF_PQ ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d,m,nbits,metric,elem", PQ_CASES)
def test_merge_pq(d, m, nbits, metric, elem):
    from lance_amd.engine import DeviceIndex
    s = sources("IVF_PQ", d, metric, m, nbits, elem)
    before = [s.stored(ix) for ix in s.ix]
    assert layout_ok(before[0][0], before[1][0])
    merged = DeviceIndex.merge(s.ix, raw=s.x_all)
    want = s.one_create(raw=s.x_all)
    got = s.stored(merged)
    spec = S.merge_storage(before)
    assert np.array_equal(got[0], spec[0]) and same(got[1], spec[1])
    assert np.array_equal(got[0], s.stored(want)[0]) and same(got[1], s.stored(want)[1])
    assert got[1][1].shape == (N_ALL, m if nbits == 8 else m // 2)
    ex_got, ex_want = merged.export(), want.export()
    assert same(ex_got, ex_want) and np.array_equal(ex_got[1], transposed(spec[0], spec[1][1])) and np.array_equal(ex_got[2], spec[1][0])
    assert merged.info() == want.info() and merged.h.value != want.h.value
    allow = np.random.default_rng(1).random(N_ALL) < 0.5
    for nprobes in (1, 3, 7):
        plain = merged.search(s.q, K, nprobes)
        assert same_search(plain, want.search(s.q, K, nprobes))
        assert same_search(merged.search(s.q, K, nprobes, 3), want.search(s.q, K, nprobes, 3))
        assert same_search(merged.search_filtered(s.q, K, nprobes, allow), want.search_filtered(s.q, K, nprobes, allow))
        dd = plain[1].cpu().numpy()
        lo, hi = float(dd[:, 1].min()), float(dd[np.isfinite(dd)].max())
        assert same_search(merged.search_range(s.q, K, nprobes, lo, hi), want.search_range(s.q, K, nprobes, lo, hi))
    assert (plain[0][:8, :2].cpu().numpy() >= 0).all()          # the repeated rows: found, whichever source stored them
    assert all(same(s.stored(ix)[1], b[1]) for ix, b in zip(s.ix, before))


# ---- 5. merge, IVF_FLAT and IVF_SQ ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,metric", FLAT_SQ_CASES)
def test_merge_flat_and_sq(kind, d, metric):
    s = sources(kind, d, metric)
    before = [s.stored(ix) for ix in s.ix]
    assert layout_ok(before[0][0], before[1][0])
    merged = type(s.ix[0]).merge(s.ix)
    want = s.one_create()
    got, spec = s.stored(merged), S.merge_storage(before)
    assert len(got[1]) == (3 if kind == "IVF_SQ" else 2)        # IVF_SQ: the sums of squared codes travel with the rows
    assert np.array_equal(got[0], spec[0]) and same(got[1], spec[1])
    assert np.array_equal(got[0], s.stored(want)[0]) and same(got[1], s.stored(want)[1])
    assert got[1][1].shape == (N_ALL, d)
    allow = np.random.default_rng(2).random(N_ALL) < 0.5
    for nprobes in (1, 3, 7):
        assert same_search(merged.search(s.q, K, nprobes), want.search(s.q, K, nprobes))
        assert same_search(merged.search(s.q, K, nprobes, allow=allow), want.search(s.q, K, nprobes, allow=allow))
    one = type(s.ix[0]).merge([s.ix[0]])                        # a single source: an equal copy
    assert same(s.stored(one)[1], before[0][1]) and one.h.value != s.ix[0].h.value


# ---- 6. append through the wrappers ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,metric,m,nbits", ONE_OF_EACH + [("IVF_FLAT", 8, "cosine", 0, 8)])
def test_append_equals_one_shot_build(kind, d, metric, m, nbits, tmp_path):
    import lance_amd
    cent, xs, _, q = data(d, metric)
    x = np.concatenate(xs).copy()
    n0 = N_BASE
    x[0, 0], x[1, 1] = -30.0, 30.0                              # the column's extremes lie in the first batch: the same SQ bounds
    x[n0 + 5] = np.nan                                          # dropped, and the ids after it stay positions
    kw = dict(index_type=kind, metric=metric, num_partitions=NLIST, ivf_centroids=cent, max_iters=2)
    if kind == "IVF_PQ":
        cb = np.random.default_rng(3).normal(0, 1.5, (m, 1 << nbits, d // m)).astype(f32)
        kw.update(num_sub_vectors=m, num_bits=nbits, pq_codebook=cb)
    first = lance_amd.create_index(x[:n0], **kw)
    whole = lance_amd.create_index(x, **kw)
    before = first.export_rows()
    grown = first.append(x[n0:])
    got, want = grown.export_rows(), whole.export_rows()
    assert same(got, want) and len(got[-1]) == N_ALL - 1 and n0 + 5 not in got[-1] and n0 + 6 in got[-1]
    assert same(first.export_rows(), before)
    assert type(grown) is type(whole) and grown.part_ids is None
    a, b = grown.nearest(q, k=K, nprobes=3), whole.nearest(q, k=K, nprobes=3)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
    again = grown.append(x[:3])                                 # the count goes on: the next ids are N_ALL ..
    assert set(again.export_rows()[-1]) - set(got[-1]) == {N_ALL, N_ALL + 1, N_ALL + 2}
    with pytest.raises(ValueError):
        first.append(x[n0:], row_ids=np.arange(3))
    with pytest.raises(ValueError):
        first.append(x[n0:, :-1])
    # delete and remap through the wrapper: sugar over the same call
    gone = got[-1][::7]
    kept = grown.delete(gone)
    spec = S.remap_storage(got[0], got[-1], list(got[1:-1]), {int(g): None for g in gone})
    out = kept.export_rows()
    assert np.array_equal(out[0], spec[0]) and np.array_equal(out[-1], spec[1]) and same(out[1:-1], spec[2])
    moved = grown.remap({int(got[-1][0]): 1 << 40, int(got[-1][1]): None, 10 ** 14: 4})
    spec = S.remap_storage(got[0], got[-1], list(got[1:-1]), {int(got[-1][0]): 1 << 40, int(got[-1][1]): None, 10 ** 14: 4})
    assert np.array_equal(moved.export_rows()[-1], spec[1])
    pair = grown.remap((np.array([got[-1][1], got[-1][0]]), [-1, 1 << 40]))
    assert same(pair.export_rows(), moved.export_rows())
    with pytest.raises(ValueError):
        grown.remap((np.array([5, 5]), [1, 2]))
    if kind == "IVF_PQ":
        rid, part, codes = grown.shuffle_buffers()
        assert np.array_equal(rid, got[2]) and np.array_equal(part, S.part_ids(got[0])) and np.array_equal(codes, got[1])
        sub = grown.prefiltered(np.arange(N_ALL) % 2 == 0) if nbits == 8 else None      # (no retained columns: the stored rows)
        assert sub is None or set(sub.export_rows()[-1]) == {int(i) for i in got[-1] if i % 2 == 0}
    if kind != "IVF_SQ":                                        # an index opened from files knows no row count
        first.save(tmp_path / "ix")
        opened = lance_amd.load_index(tmp_path / "ix")
        with pytest.raises(ValueError):
            opened.append(x[n0:])
        regrown = opened.append(x[n0:], row_ids=np.arange(n0, N_ALL))
        assert same(regrown.export_rows(), want)
    both = lance_amd.merge_indices([first, first.delete(before[-1])])      # (a source with every row deleted)
    assert same(both.export_rows(), before)
    with pytest.raises(ValueError):
        both.append(x[:2])


# ---- 7. remap / delete ----------------------------------------------------------------------------------------------------------------
def remapped(s, ix, mapping):
    old, new = S.mapping_arrays(mapping)
    return ix.remap(old.view(np.int64), new.view(np.int64))


@pytest.mark.parametrize("kind,d,metric,m,nbits", ONE_OF_EACH + [("IVF_PQ", 24, "l2", 12, 8)])
def test_remap(kind, d, metric, m, nbits):
    import torch
    import rowid_fixtures as R
    s = sources(kind, d, metric, m, nbits)
    src, (part, payload, rid) = s.ix[0], s.cols[0]
    offs, (ids, *cols) = s.stored(src)
    big = R.row_addresses(64, 5)
    assert (big >= 1 << 31).all() and (big >= 1 << 32).any()
    p = 2
    cases = {
        "partition": {int(i): None for i in ids[offs[p]:offs[p + 1]]},
        "everything": {int(i): None for i in ids},
        "swap": {int(ids[0]): int(ids[-1]), int(ids[-1]): int(ids[0])},
        "addresses": {int(i): int(b) for i, b in zip(ids[5:69], big)},
        "absent": {10 ** 13: 7, 10 ** 13 + 1: None, int(ids[9]): None},
        "first and last": {int(ids[0]): None, int(ids[-1]): None, int(ids[offs[1]]): None, int(ids[offs[1] - 1]): 77777},
        "empty": {},
    }
    rid_h, part_h = rid.cpu().numpy().view(np.uint64), part.cpu().numpy()
    for name, mapping in cases.items():
        out = remapped(s, src, mapping)
        got = s.stored(out)
        wo, wi, wc = S.remap_storage(offs, ids, cols, mapping)
        assert np.array_equal(got[0], wo) and np.array_equal(got[1][0], wi) and same(got[1][1:], wc), name
        # ... and ONE create over the surviving rows in their original order, under their new ids
        keep = np.array([mapping.get(int(i), 0) is not None for i in rid_h])
        new_rid = np.array([mapping.get(int(i), int(i)) or 0 for i in rid_h], np.uint64)
        sel = torch.from_numpy(np.flatnonzero(keep)).to(part.device)
        if keep.any():
            want = s.create(part[sel], payload[sel], torch.from_numpy(new_rid[keep].view(np.int64)).to(part.device))
            assert np.array_equal(got[0], s.stored(want)[0]) and same(got[1], s.stored(want)[1]), name
            assert same_search(out.search(s.q, K, 3), want.search(s.q, K, 3)), name
        else:
            assert got[0].tolist() == [0] * (NLIST + 1) and got[1][0].size == 0
            assert (out.search(s.q, K, 3)[0].cpu().numpy() == -1).all()
        assert out.h.value != src.h.value
    assert cases["partition"] and offs[p + 1] - offs[p] > 256
    # the raw ABI refuses an unsorted or a repeating mapping, and hands out nothing
    import lance_amd
    e = s.e
    for old in ([5, 3, 9], [3, 5, 5]):
        o = torch.tensor(old, dtype=torch.int64, device=part.device)
        h = C.c_void_p()
        torch.cuda.synchronize()
        rc = e.lib.lance_hip_index_remap(e.h, src.h, C.c_void_p(o.data_ptr()), C.c_void_p(o.data_ptr()), 3, C.byref(h))
        assert rc == lance_amd._lib.EINVAL and h.value is None and b"ascending" in e.lib.lance_hip_last_error()
    assert same(s.stored(src)[1], [ids] + cols)


# ---- 8. sources untouched ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,d,metric,m,nbits", ONE_OF_EACH)
def test_sources_stay_as_they_are(kind, d, metric, m, nbits):
    s = sources(kind, d, metric, m, nbits)
    before = [s.stored(ix) for ix in s.ix]
    answers = [ix.search(s.q, K, 3) for ix in s.ix[:2]]
    answers = [(a[0].clone(), a[1].clone()) for a in answers]
    merged = type(s.ix[0]).merge(s.ix)
    gone = remapped(s, s.ix[0], {int(i): None for i in before[0][1][0][::2]})
    merged.search(s.q, K, 3)
    merged.close()
    gone.close()
    for ix, b in zip(s.ix, before):
        now = s.stored(ix)
        assert np.array_equal(now[0], b[0]) and same(now[1], b[1])
    for ix, a in zip(s.ix[:2], answers):
        assert same_search(ix.search(s.q, K, 3), a)


# ---- 9. files ---------------------------------------------------------------------------------------------------------------------------
def test_files_of_a_merged_pq_and_a_remapped_flat_index(tmp_path):
    import lance_amd
    from lance_amd.engine import DeviceFlatIndex, DeviceIndex
    s = sources("IVF_PQ", 32, "l2", 16, 8)
    merged = DeviceIndex.merge(s.ix)
    merged.save(tmp_path / "pq")
    opened = lance_amd.load_index(tmp_path / "pq")
    assert same(opened.export_rows(), merged.export_rows()) and same(opened.export_storage(), merged.export())
    assert same_search(opened.search_device(s.q, K, 3), merged.search(s.q, K, 3))
    f = sources("IVF_FLAT", 20, "l2")
    ids = f.stored(f.ix[0])[1][0]
    moved = remapped(f, f.ix[0], {int(ids[0]): None, int(ids[1]): (3 << 32) | 5, int(ids[300]): None})
    moved.save(tmp_path / "flat")
    back = DeviceFlatIndex.load(f.e, tmp_path / "flat")
    assert same(back.export_rows(), moved.export_rows()) and len(back.export_rows()[-1]) == N_BASE - 2
    assert same_search(back.search(f.q, K, 3), moved.search(f.q, K, 3))
    sq = sources("IVF_SQ", 20, "l2")
    with pytest.raises(NotImplementedError):
        type(sq.ix[0]).merge(sq.ix).save(tmp_path / "sq")


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------------
def refused(e, indices, word):
    import lance_amd
    from lance_amd.engine import _merge_handles
    with pytest.raises(lance_amd.LanceHipError) as ei:
        _merge_handles(e, indices)
    return ei.value.code == lance_amd._lib.EINVAL and word in str(ei.value)


def test_merge_refuses_what_does_not_fit():
    import lance_amd
    import torch
    from lance_amd import vector as V
    pq, pq4, flat, sq = sources("IVF_PQ", 32, "l2", 16, 8), sources("IVF_PQ", 32, "l2", 16, 4), sources("IVF_FLAT", 32, "l2"), sources("IVF_SQ", 32, "l2")
    e = pq.e
    cb2 = pq.cb.clone()
    cb2[3, 200, 1] += 1.0
    other_cb = pq.create(*pq.cols[1], cb=cb2)
    assert refused(e, [pq.ix[0], other_cb], "codebook")
    assert refused(e, [pq.ix[0], pq.ix[1], pq4.ix[1]], "nbits")
    assert refused(e, [pq.ix[0], flat.ix[1]], "kind") and refused(e, [flat.ix[0], sq.ix[1]], "kind")
    hi = float(np.nextafter(sq.bounds[1], np.inf))
    assert refused(e, [sq.ix[0], sq.create(*sq.cols[1], bounds=(sq.bounds[0], hi))], "bounds")
    assert refused(e, [], "n_srcs")
    other = sources("IVF_FLAT", 32, "dot")                      # (its unreachable centroid is another one)
    assert refused(e, [flat.ix[0], other.ix[0]], "metric")
    cent2 = flat.cent.clone()
    cent2[6, 0] = torch.nextafter(cent2[6, 0], cent2[6, 0] + 1)
    from lance_amd.engine import DeviceFlatIndex
    moved = DeviceFlatIndex.create(e, "l2", cent2, flat.cols[1][1], flat.cols[1][0], flat.cols[1][2])
    assert refused(e, [flat.ix[0], moved], "centroids")
    h = C.c_void_p()
    arr = (C.c_void_p * 2)(pq.ix[0].h.value, other_cb.h.value)
    assert e.lib.lance_hip_index_merge(e.h, arr, 2, C.byref(h)) == lance_amd._lib.EINVAL and h.value is None
    # the wrappers turn these into ValueError with the library's message
    params = V.IvfPqParams(NLIST, 16, 8, "l2")
    with pytest.raises(ValueError, match="codebook"):
        lance_amd.merge_indices([V.IvfPqIndex(pq.ix[0], params), V.IvfPqIndex(other_cb, params)])
    with pytest.raises(ValueError, match="one kind"):
        lance_amd.merge_indices([V.IvfPqIndex(pq.ix[0], params), V.IvfFlatIndex(flat.ix[0], params, None, None)])
    assert same(pq.stored(pq.ix[0])[1], pq.stored(DeviceIndexCopy(pq))[1])


def DeviceIndexCopy(s):
    """the first source merged with nothing else: what a refused merge must not have disturbed"""
    return type(s.ix[0]).merge([s.ix[0], s.ix[3]])
