"""stable_group (lance_amd/csrc/group.hip) and the work-item tables (q_item_table_kernel / q_item_desc_kernel, lance_amd/csrc/search_q.hip)
called directly, through lance_hip_stable_group / lance_hip_work_items, on every route they have, and compared bit for bit with the numpy
specification in tests/group_spec.py (itself checked in tests/test_group_spec.py).

Every output buffer is filled with a sentinel and is GUARD entries longer than the call may touch.  Exact: starts[0 .. k] and
rows[0 .. starts[k]) of every active problem.  Still the sentinel afterwards: everything at index >= n (the padding up to out_stride, the
guard) and every output of an inactive problem.  rows[starts[k] .. n) is not compared.  The key buffers carry VALID keys behind the n keys
of a problem, so a kernel that read past n would count them.

Routes ("The grouping, tested directly"):
  fused scan       k <= 256 and <= 256 row blocks: test_fused_small, test_fused_vector_paths (64-wide, 16-wide and scalar count paths,
                   mixed inside one launch by (b * k + c) * nblocks % 4), test_batched (nblocks = 3)
  two-level scan   k > 256 (test_two_level_by_k: the 256-key rounds of the totals scan; n = 70000 is 69 row blocks, the carry across the
                   64-block rounds) or more than 256 row blocks (test_two_level_by_n: 257 blocks), test_batched (k = 300)
  wide             k > 16384: test_wide (k = 4194304 sends 16384 keys, 64 KiB of LDS, through the inner pass)
"""
import numpy as np
import pytest
import torch

from group_spec import NONE, check_group, check_items, group

pytestmark = pytest.mark.gpu

GUARD = 256
SENT = 0xA5A5A5A5                                  # above every row number, offset and partition of these cases
SENT_I32 = int(np.uint32(SENT).view(np.int32))
PATTERNS = ("uniform", "one", "none", "mixed", "asc", "desc", "mod64", "modk", "zipf", "last")


@pytest.fixture(scope="module")
def eng(engine):
    from lance_amd.engine import Engine
    e = Engine()
    yield e
    e.close()


def make_keys(pattern, n, k, seed):
    rng = np.random.default_rng([seed, n, k, PATTERNS.index(pattern)])
    r = np.arange(n, dtype=np.int64)
    if pattern == "uniform":
        keys = rng.integers(0, k, n)
    elif pattern == "one":                                     # 64 lanes, one key
        keys = np.full(n, k // 2)
    elif pattern == "none":
        keys = np.full(n, NONE)
    elif pattern == "mixed":                                   # ~10 % NONE, ~10 % just above k: below 2^kbits, and a valid low byte
        keys = rng.integers(0, k, n)
        u = rng.random(n)
        keys[u < 0.1] = NONE
        above = (u >= 0.1) & (u < 0.2)
        keys[above] = k + rng.integers(0, 300, int(above.sum()))
    elif pattern == "asc":
        keys = r * k // max(n, 1)
    elif pattern == "desc":
        keys = (r * k // max(n, 1))[::-1]
    elif pattern == "mod64":                                   # 64 lanes, 64 different keys (those >= k are dropped)
        keys = r % 64
    elif pattern == "modk":
        keys = r % k
    elif pattern == "zipf":
        keys = np.minimum(rng.zipf(1.5, n) - 1, k - 1) if n else r
    elif pattern == "last":
        keys = np.full(n, k - 1)
    return np.ascontiguousarray(keys).astype(np.uint32)


def _buf(entries):
    return torch.full((entries,), SENT_I32, dtype=torch.int32, device="cuda")


def _host(t):
    return t.cpu().numpy().view(np.uint32)


def run_group(eng, keys, n, k, batches=1, key_stride=None, out_stride=None, active=None, expect=None):
    """keys: uint32 [batches][key_stride or n].  Runs the call and checks everything the module docstring lists; with `expect` the call
    must fail with that code and a message, and every output must still be the sentinel."""
    from lance_amd import _lib
    ks = n if key_stride is None else key_stride
    os_ = n if out_stride is None else out_stride
    keys = np.ascontiguousarray(keys, dtype=np.uint32).reshape(batches, ks)
    dkeys = torch.from_numpy(np.concatenate([keys.reshape(-1), np.zeros(GUARD, np.uint32)]).view(np.int32)).cuda()
    starts, rows = _buf(batches * (k + 1) + GUARD), _buf(batches * os_ + GUARD)
    act = None if active is None else torch.tensor(list(active), dtype=torch.uint8).cuda()
    if expect is not None:
        with pytest.raises(_lib.LanceHipError) as err:
            eng.stable_group(dkeys, n, k, starts, rows, batches, key_stride, out_stride, act)
        assert err.value.code == expect and "stable_group" in str(err.value)
        assert (_host(starts) == SENT).all() and (_host(rows) == SENT).all(), "a refused call wrote to its outputs"
        return
    eng.stable_group(dkeys, n, k, starts, rows, batches, key_stride, out_stride, act)
    hs, hr = _host(starts), _host(rows)
    assert (hs[batches * (k + 1):] == SENT).all(), "starts: guard overwritten"
    assert (hr[batches * os_:] == SENT).all(), "rows: guard overwritten"
    for b in range(batches):
        sb, rb = hs[b * (k + 1):(b + 1) * (k + 1)], hr[b * os_:(b + 1) * os_]
        if active is not None and not active[b]:
            assert (sb == SENT).all() and (rb == SENT).all(), f"problem {b} is inactive and was written"
            continue
        check_group(sb, rb[:n], keys[b, :n], k)
        assert (rb[n:] == SENT).all(), f"problem {b}: rows written at or past n = {n}"


def sweep(eng, k, n, seed=0):
    for pattern in PATTERNS:
        try:
            run_group(eng, make_keys(pattern, n, k, seed), n, k)
        except AssertionError as e:
            raise AssertionError(f"k = {k}, n = {n}, keys '{pattern}': {e}") from None


# ---- stable_group: one problem ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 5, 16, 255, 256])
def test_fused_small(eng, k):
    """one row block; k = 1 has kbits = 0 (no ballot round); n = 0 launches one block that reads nothing"""
    for n in (0, 1, 63, 64, 65, 1023, 1024, 1025):
        sweep(eng, k, n)


@pytest.mark.parametrize("nb", [16, 17, 64, 67, 80, 256])
@pytest.mark.parametrize("k", [5, 256])
def test_fused_vector_paths(eng, k, nb):
    """a key's row of nb block counts starts at (b * k + c) * nb words: 16-byte aligned for every key at nb = 16, 64, 80, 256 and for every
    fourth key at nb = 17, 67, where the other keys take the scalar path over the whole row.  Aligned rows: nb = 16 one 16-wide round;
    17 = 16 + 1 scalar; 64 one 64-wide round; 67 = 64 + 3 scalar; 80 = 64 + 16; 256 four 64-wide rounds (and the route's last size)."""
    for n in (1024 * nb - 3, 1024 * nb):
        sweep(eng, k, n, seed=1)


@pytest.mark.parametrize("k", [257, 300, 513, 1000, 16384])
def test_two_level_by_k(eng, k):
    """k > 256: a wave per key, then the totals in rounds of 256 keys (257 = a round of one key; 16384 = 64 rounds, 64 KiB of LDS in the
    histogram and the scatter); n = 70000 is 69 row blocks: the second 64-block round starts from the first one's carry"""
    for n in (5000, 70000):
        sweep(eng, k, n, seed=2)


@pytest.mark.parametrize("k", [7, 256])
def test_two_level_by_n(eng, k):
    """257 row blocks take a key set the fused scan serves off it: four full 64-block rounds and a round of one block"""
    sweep(eng, k, 262145, seed=3)


@pytest.mark.parametrize("k", [16385, 20000, 65536, 131072, 4194304])
def test_wide(eng, k):
    """low byte, then the high bits, each a stable pass: a key >= k has a low byte that is a valid digit of the first pass and must be
    dropped before it ('mixed', 'none'); the high pass sees ceil(k / 256) keys (65 .. 16384: at k = 4194304 exactly 64 KiB of LDS) and
    reads how many rows the low pass kept from the low pass's own starts[256]"""
    sweep(eng, k, 50000, seed=4)
    for pattern in ("uniform", "none"):
        run_group(eng, make_keys(pattern, 0, k, 4), 0, k)


def test_refused_and_empty_calls(eng):
    from lance_amd import _lib
    n = 1000
    run_group(eng, make_keys("uniform", n, 4194305, 5), n, 4194305, expect=_lib.EINVAL)           # one key past the wide route's limit
    run_group(eng, np.stack([make_keys("uniform", n, 16385, 5)] * 2), n, 16385, batches=2, expect=_lib.EINVAL)
    run_group(eng, make_keys("uniform", n, 16385, 5), n, 16385, active=[1], expect=_lib.EINVAL)   # the wide route takes no mask
    run_group(eng, make_keys("uniform", n, 16, 5), n, 0, expect=_lib.EINVAL)
    run_group(eng, np.zeros((0, n), np.uint32), n, 16, batches=0)                                 # OK, and nothing written
    run_group(eng, np.zeros((0, n), np.uint32), n, 20000, batches=0)


# ---- stable_group: several problems -------------------------------------------------------------------------------------------------------
def _masks(batches):
    holes = [0 if b in (0, batches // 2, batches - 1) else 1 for b in range(batches)]
    return (None, [1] * batches, holes, [b % 2 for b in range(batches)])


@pytest.mark.parametrize("batches,k", [(3, 16), (3, 256), (16, 16), (16, 256), (3, 300)])
def test_batched(eng, batches, k):
    """the form PQ training uses: strides that are not n (odd ones: the problems' buffers are not 16-byte aligned to each other), and a
    mask; problem b holds pattern b of PATTERNS, the key padding holds valid keys.  k <= 256 is the fused scan, k = 300 the two-level one.
    (batches = 3: the mask with holes at the first, a middle and the last problem leaves nothing active -- nothing may be written.)"""
    n = 3000
    ks, os_ = n + 7, n + 5
    keys = np.zeros((batches, ks), np.uint32)
    for b in range(batches):
        keys[b, :n] = make_keys(PATTERNS[(b + k) % len(PATTERNS)], n, k, 6 + b)
    for active in _masks(batches):
        run_group(eng, keys, n, k, batches=batches, key_stride=ks, out_stride=os_, active=active)


# ---- work items ---------------------------------------------------------------------------------------------------------------------------
COUNT_PATTERNS = ("zero", "one_first", "one_mid", "one_last", "runs", "edges", "random")


def make_counts(pattern, nvp, G, seed):
    rng = np.random.default_rng([seed, nvp, G, COUNT_PATTERNS.index(pattern)])
    c = np.zeros(nvp, np.int64)
    if pattern == "one_first":
        c[0] = 37 * G + 5
    elif pattern == "one_mid":
        c[nvp // 2] = 37 * G + 5
    elif pattern == "one_last":
        c[nvp - 1] = 37 * G + 5
    elif pattern == "runs":                                   # empty runs before, between and after the occupied partitions
        for at, cnt in ((nvp // 3, G + 1), (nvp // 3 + 1, 1), ((2 * nvp) // 3, 2 * G + 3), ((5 * nvp) // 6, G)):
            c[min(at, nvp - 1)] = cnt             # (nvp = 1000: partitions 0 .. 332, 335 .. 665, 667 .. 832 and 834 .. 999 are empty)
    elif pattern == "edges":
        c[:] = np.array([G - 1, G, G + 1, 2 * G + 3])[np.arange(nvp) % 4]
    elif pattern == "random":
        c[:] = rng.integers(0, 3 * G + 1, nvp) * (rng.random(nvp) < 0.5)
    return c


def run_items(eng, pair_starts, G, max_items):
    ps = np.asarray(pair_starts, np.uint32)
    nvp = ps.size - 1
    dps = torch.from_numpy(ps.view(np.int32)).cuda()
    item_start, desc = _buf(nvp + 1 + GUARD), _buf(4 * max_items + GUARD)
    eng.work_items(dps, G, item_start, desc, max_items)
    hi, hd = _host(item_start), desc.cpu().numpy()
    check_items(hi[:nvp + 1], hd[:4 * max_items], ps, G, max_items)
    assert (hi[nvp + 1:] == SENT).all(), "item_start: guard overwritten"
    assert (hd[4 * max_items:] == SENT_I32).all(), "desc: guard overwritten"


@pytest.mark.parametrize("nvp", [1, 255, 256, 257, 1000, 131072])
@pytest.mark.parametrize("G", [4, 32, 64])
def test_work_items(eng, G, nvp):
    """G = Q_G, SQPM_QB / RQPM_QB, MSB_BQ.  The item table is scanned in rounds of 256 partitions (255 / 256 / 257: one short of a round,
    a round, a round and one), the descriptors are written by blocks of 256 items: max_items takes the item total (0 for 'zero': no
    launch at all), total + 1, the next multiple of 256 above it, and the bound the searches pass, pairs / G + nvp + 1."""
    for pattern in COUNT_PATTERNS:
        counts = make_counts(pattern, nvp, G, 7)
        ps = np.concatenate([[0], np.cumsum(counts)])
        total = int(((counts + G - 1) // G).sum())
        for max_items in sorted({total, total + 1, (total // 256 + 1) * 256, int(ps[-1]) // G + nvp + 1}):
            try:
                run_items(eng, ps, G, max_items)
            except AssertionError as e:
                raise AssertionError(f"G = {G}, nvp = {nvp}, counts '{pattern}', max_items = {max_items}: {e}") from None


def test_work_items_refused(eng):
    from lance_amd import _lib
    ps = torch.from_numpy(np.array([0, 5, 9], np.int32)).cuda()
    item_start, desc = _buf(3 + GUARD), _buf(4 * 8 + GUARD)
    with pytest.raises(_lib.LanceHipError) as err:
        eng.work_items(ps, 0, item_start, desc, 8)
    assert err.value.code == _lib.EINVAL and "work_items" in str(err.value)
    with pytest.raises(_lib.LanceHipError) as err:
        eng.work_items(ps, 4, item_start, desc[1:], 8)      # 4 bytes off the 16-byte grid: the records are written as int4
    assert err.value.code == _lib.EINVAL and "aligned" in str(err.value)
    assert (_host(item_start) == SENT).all() and (_host(desc) == SENT).all()


# ---- the two together, as a grouped search uses them ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nlist,nq,nprobes", [(3, 700, 2), (20000, 1000, 20)])
def test_probes_to_items(eng, nlist, nq, nprobes):
    """(query, probed partition) pairs grouped by partition (nlist = 3: fused scan; 20000: wide route), the device's own starts cut into
    items of G = 32: every pair lies in exactly one item's range, and that item is its partition's"""
    G = 32
    rng = np.random.default_rng(8)
    probes = rng.integers(0, nlist, (nq, nprobes)).astype(np.uint32)
    npairs = nq * nprobes
    dkeys = torch.from_numpy(probes.reshape(-1).view(np.int32)).cuda()
    starts, rows = _buf(nlist + 1), _buf(npairs + GUARD)
    eng.stable_group(dkeys, npairs, nlist, starts, rows)
    check_group(_host(starts), _host(rows)[:npairs], probes.reshape(-1), nlist)
    max_items = npairs // G + nlist + 1
    item_start, desc = _buf(nlist + 1 + GUARD), _buf(4 * max_items + GUARD)
    eng.work_items(starts, G, item_start, desc, max_items)
    hd = desc.cpu().numpy()[:4 * max_items].reshape(max_items, 4)
    total = int(_host(item_start)[nlist])
    assert 0 < total <= max_items and (hd[:total, 0] >= 0).all() and (hd[total:] == [-1, 0, 0, 0]).all()
    vp, first, cnt = hd[:total, 0].astype(np.int64), hd[:total, 1].astype(np.int64), hd[:total, 2].astype(np.int64)
    assert (cnt >= 1).all() and (cnt <= G).all() and (first >= 0).all() and (first + cnt <= npairs).all()
    owner = np.repeat(np.arange(total), cnt)
    slot = np.repeat(first, cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    assert (np.bincount(slot, minlength=npairs) == 1).all(), "a pair in no item, or in two"
    pair = _host(rows)[slot]
    assert (probes.reshape(-1)[pair] == vp[owner]).all(), "an item holds a pair of another partition"
    assert (np.sort(pair) == np.arange(npairs)).all()
