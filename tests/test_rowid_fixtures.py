"""The row-address fixtures of tests/rowid_fixtures.py, checked on the CPU: the addresses have the properties their docstrings claim,
and every case tests/test_zz_gpu_row_addresses.py runs on the device CAN fail -- the oracle's own answer changes when ties are broken
by the low word of the id, by the high word, or by the storage position instead of the full 64-bit id (rowid_fixtures.mutants), when
a prefilter mask is indexed by the low word, and when refine reads the raw column by storage position.  These are conditions on the
fixtures, not measurements: a case that does not meet them gets more duplicated rows until it does."""
import types

import numpy as np
import pytest

import rowid_fixtures as R

f32 = np.float32
u64 = np.uint64
NQ = 16          # queries per mutant run: the routing shape matters only on the device


# ---- the addresses ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(16, 0), (17, 1), (300, 2), (2100, 3), (6000, 4), (9000, 5)])
def test_row_addresses_have_the_claimed_properties(n, seed):
    rid = R.row_addresses(n, seed)
    assert rid.dtype == u64 and rid.shape == (n,) and np.unique(rid).size == n
    assert (rid == R.row_addresses(n, seed)).all(), "deterministic"
    assert (rid < u64(1 << 63)).all() and (rid != R.NONE_ID).all()
    assert (rid.view(np.int64) >= 0).all(), "an id crosses Python as an int64 bit pattern; -1 is merge_topk's hole"
    hi, lo = rid >> u64(32), rid & u64(0xFFFFFFFF)
    frags = set(hi.tolist())
    assert len(frags) >= 4 and 0 in frags and 2 ** 31 - 1 in frags and any(2 <= f < 2 ** 31 - 1 for f in frags)
    assert (lo < u64(1 << 31)).any() and (lo >= u64(1 << 31)).any(), "offsets on both sides of 2^31"
    assert (rid >= u64(1 << 31)).all(), "no address indexes a raw column or a mask of n entries"
    # truncating to either half gives duplicates: a low word in several fragments, a high word in several rows
    assert np.unique(lo).size < n and np.unique(hi).size < n
    assert len({int(h) for h, l in zip(hi, lo) if (lo == l).sum() > 1}) >= 2
    # four pairwise different orders over the rows in storage order
    pos = np.arange(n)
    orders = {"full": np.argsort(rid, kind="stable"), "low": np.lexsort((pos, lo)), "high": np.lexsort((pos, hi)), "pos": pos}
    names = sorted(orders)
    for i, a in enumerate(names):
        for b in names[i + 1:]:
            assert (orders[a] != orders[b]).any(), (a, b)
    # among rows of different fragments the low-word order is roughly the reverse of the address order
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, n, 4000), rng.integers(0, n, 4000)
    diff = hi[a] != hi[b]
    reversed_ = ((rid[a] < rid[b]) & (lo[a] > lo[b])) | ((rid[a] > rid[b]) & (lo[a] < lo[b]))
    assert reversed_[diff].mean() > 0.75, reversed_[diff].mean()


def test_small_offset_addresses_and_ids_indexing_raw():
    n = 6000
    rid = R.small_offset_addresses(n, 3)
    hi, lo = rid >> u64(32), rid & u64(0xFFFFFFFF)
    assert np.unique(rid).size == n and (np.sort(lo) == np.arange(n)).all() and set(hi.tolist()) == set(R.FRAGMENTS)
    sel = R.selected_rows(np.ones(n, bool), rid)
    assert (sel == (hi == 0)).all() and 0 < sel.sum() < n
    p = R.ids_indexing_raw(n, 4)
    assert (np.sort(p) == np.arange(n)).all() and (p != np.arange(n)).any()
    x = np.arange(n * 2, dtype=f32).reshape(n, 2)
    raw = R.raw_by_id(x, p)
    assert (raw[p.astype(np.int64)] == x).all()


def test_mutants_are_order_isomorphic_to_the_wrong_keys():
    rid = R.row_addresses(300, 9)
    pos = np.arange(300)
    keys = {"low": rid & u64(0xFFFFFFFF), "high": rid >> u64(32), "pos": pos.astype(u64)}
    for name, (mid, back) in R.mutants(rid).items():
        assert (np.sort(mid) == pos).all()
        assert (back[mid.astype(np.int64)] == rid).all()
        assert (R.unmap(np.array([mid[3], R.NONE_ID]), back) == np.array([rid[3], R.NONE_ID])).all()
        order = np.argsort(mid)
        k = keys[name][order]
        assert (np.diff(k.astype(np.int64)) >= 0).all(), name                       # ascending in the wrong key ...
        same = np.diff(k.astype(np.int64)) == 0
        assert (np.diff(order)[same] > 0).all(), name                                  # ... and in storage position where it ties


# ---- every case can fail ------------------------------------------------------------------------------------------------------
def run_differs(got, true, back=None):
    """per run: some query's id list differs"""
    assert len(got) == len(true) and len(true) > 0
    return [bool(((gi if back is None else R.unmap(gi, back)) != ti).any()) for (gi, _), (ti, _) in zip(got, true)]


def differs(got, true, back=None):
    """some query's id list differs in some run"""
    return any(run_differs(got, true, back))


def assert_every_mutant_changes_the_answer(answers, rid, low_word_is_the_id=False, heap_decides=()):
    """answers(ids) -> [(ids, dists)] per run.  -> the true answer.  Per CASE every mutant changes the answer; per RUN -- each run is a
    kernel path of its own on the device (few-query split, the IVF_SQ fast path, another k) -- at least one of them does, so every
    run can fail.  heap_decides: the indices of the k = 1 runs over partitions: the reference's heap of ONE entry per partition keeps
    the first of equal rows in storage order (the copies of a row share a partition), the id order never decides there and no
    mutant can change such a run; it still carries 64-bit ids through the kernels.  low_word_is_the_id: ids that index a raw
    column are below 2^32, so the order by low word IS the order by id -- no wrong order to tell apart (asserted, not assumed)"""
    true = answers(rid)
    assert all((ti != R.NONE_ID).any() for ti, _ in true), "a run that finds nothing pins nothing"
    per_run = np.zeros(len(true), bool)
    for name, (mid, back) in R.mutants(rid).items():
        if name == "low" and low_word_is_the_id:
            assert (mid == rid).all()
            continue
        d = run_differs(answers(mid), true, back)
        assert any(d), f"ties broken by {name} give the oracle's own answer: the case cannot fail"
        per_run |= d
    per_run[list(heap_decides)] = True
    assert per_run.all(), f"runs {np.nonzero(~per_run)[0]} give the oracle's own answer under every wrong id order"
    return true


def k1_runs(runs):
    return [i for i, r in enumerate(runs) if r[-2] == 1]


def one_more(c):
    """the case asked for k + 1 results in every run"""
    v = dict(vars(c))
    if "ks" in v:
        v["ks"] = tuple(k + 1 for k in c.ks)
    else:
        v["runs"] = tuple(r[:-2] + (r[-2] + 1, r[-1]) for r in c.runs)
    return types.SimpleNamespace(**v)


def assert_ties_at_the_kth_place(wider, ks):
    """wider: the answers for k + 1.  In some run some query's (k + 1)-th distance equals its k-th: the cut falls inside a tie, and which
    of the tied rows is kept is the id order's decision"""
    assert any((np.atleast_2d(d)[:, k].view(np.uint32) == np.atleast_2d(d)[:, k - 1].view(np.uint32)).any() for (_, d), k in zip(wider, ks))


@pytest.mark.parametrize("name", sorted(R.FLAT_CASES))
def test_flat_cases_can_fail(oracle, name):
    c = R.flat_case(name)
    assert_every_mutant_changes_the_answer(lambda ids: R.flat_answers(oracle, c, ids, nq=NQ), c.rid)
    assert_ties_at_the_kth_place(R.flat_answers(oracle, one_more(c), c.rid, nq=NQ), c.ks)
    assert c.x.shape[0] == 6000 and np.unique(c.x, axis=0).shape[0] <= 2000      # every row three times


def test_ivfflat_case_can_fail(oracle):
    c = R.ivfflat_case()
    true = assert_every_mutant_changes_the_answer(lambda ids: R.ivfflat_answers(oracle, c, ids), c.rid)
    assert_ties_at_the_kth_place(R.ivfflat_answers(oracle, one_more(c), c.rid), [k for k, _ in c.runs])


@pytest.mark.parametrize("name", sorted(R.IVFPQ_CASES))
def test_ivfpq_cases_can_fail(oracle, name):
    c = R.ivfpq_case(name)
    true = assert_every_mutant_changes_the_answer(lambda ids: R.ivfpq_answers(oracle, c, ids, nq=NQ), c.rid, heap_decides=k1_runs(c.runs))
    assert_ties_at_the_kth_place(R.ivfpq_answers(oracle, one_more(c), c.rid, nq=NQ), [k for _, k, _ in c.runs])
    oidx = R.ivfpq_oracle_index(oracle, c, c.rid)
    # both ways a tie at the k-th place is decided occur: by the id order alone (the scan / merge kernels answer), and by one
    # partition's heap (the exact replay answers) -- except in the overflow case, which is all heap by design
    census = [R.ivfpq_tie_census(oracle, c, oidx, min(nq, 100), k, nprobes) for nq, k, nprobes in c.runs if nq >= 100 and k > 1]
    assert all(by_heap > 0 for _, by_heap, _ in census) and (name == "overflow" or all(by_id >= 3 for by_id, _, _ in census)), census
    assert (np.sort(oidx.row_ids) == np.sort(c.rid)).all() and (oidx.row_ids == c.rid[oidx.perm]).all()
    if name in R.OTHER_SEARCHES:     # the same ids under a distance range, and as candidate lists (k = keff): the GPU file's parameters
        _, k, nprobes = c.runs[0]
        lo, hi = R.range_bounds(oidx, c)
        assert_every_mutant_changes_the_answer(lambda ids: R.ivfpq_answers(oracle, c, ids, runs=((NQ, k, nprobes),), lower=lo, upper=hi), c.rid)
        assert_every_mutant_changes_the_answer(lambda ids: R.ivfpq_answers(oracle, c, ids, runs=((NQ, R.CANDIDATES_KEFF, nprobes),)), c.rid)


@pytest.mark.parametrize("kind", ["f32", "f32_frac", "int8"])
@pytest.mark.parametrize("name", sorted(R.REFINE_RUNS))
def test_refine_cases_can_fail(oracle, name, kind):
    c = R.ivfpq_case(name, "raw", kind)
    runs = ((NQ,) + R.REFINE_RUNS[name][1:],)
    for rf in R.REFINE_FACTORS:
        answers = lambda ids: R.ivfpq_answers(oracle, c, ids, refine=rf, raw=R.raw_by_id(c.x, ids), runs=runs)
        true = assert_every_mutant_changes_the_answer(answers, c.rid, low_word_is_the_id=True)
        # a refine that reads the raw column by storage position ranks other rows' vectors
        assert differs(R.ivfpq_answers(oracle, c, c.rid, refine=rf, raw=c.x, runs=runs), true), rf
    # the candidate lists of an index with a raw column: ids and PQ distances of search(k = keff)
    cand = ((NQ, R.REFINE_CANDIDATES[1], runs[0][2]),)
    assert_every_mutant_changes_the_answer(lambda ids: R.ivfpq_answers(oracle, c, ids, runs=cand), c.rid, low_word_is_the_id=True)


def assert_prefilter_by_low_word_is_seen(answers, rid, n):
    """answers(ids, mask) under the all-True mask of n entries: exactly the fragment-0 rows are found; a mask indexed by the LOW WORD
    would admit every row, and the answer with every row admitted is another one"""
    mask = np.ones(n, bool)
    true = answers(rid, mask)
    frag0 = set(rid[rid < u64(n)].tolist())
    found = set(np.concatenate([ti.ravel() for ti, _ in true]).tolist()) - {int(R.NONE_ID)}
    assert found and found <= frag0
    for name, (mid, back) in R.mutants(rid).items():
        if name == "low":            # every selected row lies in fragment 0, where the low word is the id: the wrong mask below is this case's low-word error
            continue
        assert differs(answers(mid, R.mask_by_id(R.selected_rows(mask, rid), mid)), true, back), name
    low = rid & u64(0xFFFFFFFF)                      # a permutation of 0 .. n-1: usable as ids, and every one inside the mask
    back = np.empty(n, u64)
    back[low.astype(np.int64)] = rid
    assert differs(answers(low, mask), true, back), "a mask indexed by the low word gives the same answer"


@pytest.mark.parametrize("name", ["query_major", "four_bit"])
def test_ivfpq_prefilter_by_id_can_fail(oracle, name):
    c = R.ivfpq_case(name, "small")
    assert_prefilter_by_low_word_is_seen(lambda ids, mask: R.ivfpq_answers(oracle, c, ids, nq=NQ, prefilter=mask), c.rid, c.x.shape[0])


def test_ivfflat_prefilter_by_id_can_fail(oracle):
    c = R.ivfflat_case("small")
    assert_prefilter_by_low_word_is_seen(lambda ids, mask: R.ivfflat_answers(oracle, c, ids, keep=R.selected_rows(mask, ids)), c.rid, c.x.shape[0])


def test_sq_prefilter_by_id_can_fail(oracle):
    c = R.sq_case("gaussian", "small")
    assert_prefilter_by_low_word_is_seen(lambda ids, mask: R.sq_answers(oracle, c, ids, nq=NQ, prefilter=mask), c.rid, c.x.shape[0])


@pytest.mark.parametrize("name", ["gaussian", "ties"])
def test_sq_cases_can_fail(oracle, name):
    c = R.sq_case(name)
    true = assert_every_mutant_changes_the_answer(lambda ids: R.sq_answers(oracle, c, ids, nq=NQ), c.rid, heap_decides=k1_runs(c.runs))
    assert_ties_at_the_kth_place(R.sq_answers(oracle, one_more(c), c.rid, nq=NQ), [k for k, _ in c.runs])
    # a mask much shorter than the ids selects nothing
    none = R.sq_answers(oracle, c, c.rid, nq=NQ, prefilter=np.ones(1000, bool))
    assert all((ti == R.NONE_ID).all() for ti, _ in none)


def test_pq_partition_case_can_fail(oracle):
    c = R.pq_partition_case()
    true = assert_every_mutant_changes_the_answer(lambda ids: R.pq_partition_answers(oracle, c, ids), c.rid, heap_decides=[c.ks.index(1)])
    assert_ties_at_the_kth_place(R.pq_partition_answers(oracle, one_more(c), c.rid), c.ks)


def test_multivec_case_can_fail(oracle):
    c = R.multivec_case()
    assert c.off.size - 1 > 2048
    true = assert_every_mutant_changes_the_answer(lambda ids: R.multivec_answers(oracle, c, ids), c.rid)
    assert_ties_at_the_kth_place(R.multivec_answers(oracle, one_more(c), c.rid), c.ks)


@pytest.mark.parametrize("exact", [False, True])
def test_merge_case_can_fail(oracle, exact):
    c = R.merge_case()
    filled = c.ids[c.ids != R.NONE_ID]
    assert (filled.view(np.int64) > 0).all() and (c.ids == R.NONE_ID).any()
    true = R.merge_answers(oracle, c, c.ids, exact)
    for name in ("low", "high", "pos"):              # a candidate's storage position is its slot
        m_ids, backs = c.ids.copy(), []
        for r in range(c.ids.shape[0]):
            ok = c.ids[r] != R.NONE_ID
            m_ids[r][ok], back = R.mutants(c.ids[r][ok])[name]
            backs.append(back)
        (gi, _), = R.merge_answers(oracle, c, m_ids, exact)
        assert (np.stack([R.unmap(gi[r], backs[r]) for r in range(gi.shape[0])]) != true[0][0]).any(), name
    wide = types.SimpleNamespace(**{**vars(c), "k": c.k + 1})
    assert_ties_at_the_kth_place(R.merge_answers(oracle, wide, c.ids, exact), [c.k])
