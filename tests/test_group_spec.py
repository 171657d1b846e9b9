"""tests/group_spec.py is what tests/test_zz_gpu_grouping.py holds the grouping kernels against, so it is checked here first, without a
GPU: the numpy spec against a brute-force definition written with Python loops, and the two checkers against answers that are wrong in
the ways a grouping kernel goes wrong -- each must be rejected, and the right answer accepted."""
import numpy as np
import pytest

from group_spec import NONE, check_group, check_items, group, work_items


def brute_group(keys, k):
    lists = [[] for _ in range(k)]
    for r, key in enumerate(keys):
        if int(key) < k:
            lists[int(key)].append(r)
    starts, rows = [0], []
    for members in lists:
        rows += members
        starts.append(len(rows))
    return starts, rows


def brute_items(pair_starts, G, max_items):
    item_start, desc = [0], []
    for vp in range(len(pair_starts) - 1):
        at, end = int(pair_starts[vp]), int(pair_starts[vp + 1])
        while at < end:
            desc.append([vp, at, min(G, end - at), 0])
            at += G
        item_start.append(len(desc))
    desc = (desc + [[-1, 0, 0, 0]] * max_items)[:max_items]
    return item_start, desc


def _key_sets():
    rng = np.random.default_rng(11)
    yield np.zeros(0, np.uint32), 1
    yield np.zeros(0, np.uint32), 5
    yield np.zeros(7, np.uint32), 1
    yield np.array([NONE], np.uint32), 3
    yield np.array([2, 2, 0, NONE, 5, 1, 2, 4, 3, 0], np.uint32), 3      # keys 3, 4, 5 are below 2^kbits = 4 or above: all dropped
    yield np.full(70, 4, np.uint32), 5
    yield np.arange(70, dtype=np.uint32)[::-1].copy(), 64
    for k in (1, 2, 7, 300):
        keys = rng.integers(0, k + 3, 200).astype(np.uint32)
        keys[rng.random(200) < 0.1] = NONE
        yield keys, k


@pytest.mark.parametrize("case", range(11))
def test_group_matches_brute_force(case):
    keys, k = list(_key_sets())[case]
    starts, rows = group(keys, k)
    bs, br = brute_group(keys, k)
    assert starts.dtype == np.uint32 and rows.dtype == np.uint32
    assert starts.tolist() == bs and rows.tolist() == br
    check_group(starts, rows, keys, k)
    check_group(starts.view(np.int32), np.concatenate([rows, np.full(9, 77, np.uint32)]).view(np.int32), keys, k)   # device buffers: int32 bits, longer


def _pair_sets():
    rng = np.random.default_rng(12)
    yield [0], 4
    yield [0, 0], 4
    yield [0, 0, 0, 0], 32
    yield [0, 3], 4
    yield [0, 4], 4
    yield [0, 5], 4
    yield [0, 0, 0, 11, 11, 11, 12, 20, 20], 4
    yield [5, 5, 70, 70, 134, 199], 64                                   # a table that does not start at pair 0
    for G in (1, 4, 32):
        yield np.concatenate([[0], np.cumsum(rng.integers(0, 3 * G, 40) * (rng.random(40) < 0.6))]).tolist(), G


@pytest.mark.parametrize("case", range(11))
def test_work_items_match_brute_force(case):
    ps, G = list(_pair_sets())[case]
    total = brute_items(ps, G, 0)[0][-1]
    for max_items in sorted({0, max(total - 1, 0), total, total + 1, total + 300}):
        item_start, desc = work_items(np.array(ps, np.uint32), G, max_items)
        bi, bd = brute_items(ps, G, max_items)
        assert item_start.dtype == np.uint32 and desc.dtype == np.int32 and desc.shape == (max_items, 4)
        assert item_start.tolist() == bi and desc.tolist() == bd
        check_items(item_start, desc, ps, G, max_items)
        check_items(item_start.view(np.int32), np.concatenate([desc.reshape(-1), np.full(8, 9, np.int32)]), ps, G, max_items)


# ---- the checkers reject wrong answers ------------------------------------------------------------------------------------------------
def _answer():
    keys = np.array([1, 0, 1, 2, NONE, 1, 0, 2, 7, 2], np.uint32)      # k = 3: groups {1, 6}, {0, 2, 5}, {3, 7, 9}; rows 4 and 8 dropped
    starts, rows = group(keys, 3)
    assert starts.tolist() == [0, 2, 5, 8] and rows.tolist() == [1, 6, 0, 2, 5, 3, 7, 9]
    return keys, starts, rows


def test_check_group_rejects_rows_swapped_inside_a_group():
    keys, starts, rows = _answer()
    rows[[2, 3]] = rows[[3, 2]]            # the right members of key 1, not in ascending row order: an unstable scatter
    with pytest.raises(AssertionError, match=r"rows\[2\]"):
        check_group(starts, rows, keys, 3)


def test_check_group_rejects_rows_swapped_across_a_group_boundary():
    keys, starts, rows = _answer()
    rows[[4, 5]] = rows[[5, 4]]            # the last row of key 1 and the first of key 2: a cursor off by one
    with pytest.raises(AssertionError, match=r"rows\[4\]"):
        check_group(starts, rows, keys, 3)


@pytest.mark.parametrize("at", [0, 1, 2, 3])
@pytest.mark.parametrize("by", [1, -1])
def test_check_group_rejects_a_start_off_by_one(at, by):
    keys, starts, rows = _answer()
    starts = starts.astype(np.int64)
    starts[at] += by
    with pytest.raises(AssertionError, match=rf"starts\[{at}\]"):
        check_group(starts.astype(np.uint32), rows, keys, 3)


def test_check_group_rejects_a_kept_dropped_row_and_a_short_answer():
    keys, starts, rows = _answer()
    with pytest.raises(AssertionError):
        check_group(starts, np.concatenate([rows[:7], [8]]).astype(np.uint32), keys, 3)     # row 8 (key 7 >= k) in place of row 9
    with pytest.raises(AssertionError, match="rows holds"):
        check_group(starts, rows[:7], keys, 3)
    with pytest.raises(AssertionError, match="starts holds"):
        check_group(starts[:3], rows, keys, 3)
    check_group(starts, rows, keys, 3)


def _items(G=4):
    ps = np.array([0, 0, 2 * G + 3, 2 * G + 3, 3 * G + 3], np.uint32)      # partitions 0 and 2 empty; 1 holds 2G + 3 pairs, 3 holds G
    max_items = 7
    item_start, desc = work_items(ps, G, max_items)
    assert item_start.tolist() == [0, 0, 3, 3, 4]
    assert desc.tolist() == [[1, 0, G, 0], [1, G, G, 0], [1, 2 * G, 3, 0], [3, 2 * G + 3, G, 0]] + [[-1, 0, 0, 0]] * 3
    return ps, G, max_items, item_start, desc


def test_check_items_rejects_a_block_longer_than_G():
    ps, G, max_items, item_start, desc = _items()
    desc[1, 2] = G + 1
    with pytest.raises(AssertionError, match=r"desc\[1\]"):
        check_items(item_start, desc, ps, G, max_items)


def test_check_items_rejects_a_desc_on_the_preceding_empty_partition():
    ps, G, max_items, item_start, desc = _items()
    desc[3, 0] = 2                         # partition 2 is empty and shares partition 3's item_start
    with pytest.raises(AssertionError, match=r"desc\[3\]"):
        check_items(item_start, desc, ps, G, max_items)
    ps, G, max_items, item_start, desc = _items()
    desc[0, 0] = 0                         # likewise at the head of the table
    with pytest.raises(AssertionError, match=r"desc\[0\]"):
        check_items(item_start, desc, ps, G, max_items)


def test_check_items_rejects_a_missing_tail():
    ps, G, max_items, item_start, desc = _items()
    for slot in (4, 6):                    # the first and the last record past the item total
        wrong = desc.copy()
        wrong[slot] = [0x55555555, 0x55555555, 0x55555555, 0x55555555]      # never written: the buffer's fill is still there
        with pytest.raises(AssertionError, match=rf"desc\[{slot}\]"):
            check_items(item_start, wrong, ps, G, max_items)
    wrong = desc.copy()
    wrong[5, 3] = 1                        # the fourth word of a record is part of the contract too
    with pytest.raises(AssertionError, match=r"desc\[5\]"):
        check_items(item_start, wrong, ps, G, max_items)
    with pytest.raises(AssertionError, match="desc holds"):
        check_items(item_start, desc[:6], ps, G, max_items)


def test_check_items_rejects_a_wrong_item_start():
    ps, G, max_items, item_start, desc = _items()
    for at in range(5):
        wrong = item_start.copy()
        wrong[at] += 1
        with pytest.raises(AssertionError, match=rf"item_start\[{at}\]"):
            check_items(wrong, desc, ps, G, max_items)
    check_items(item_start, desc, ps, G, max_items)
