"""tests/index_update_spec.py pinned against independent formulations: what merge / remap / delete of an index must store."""
import numpy as np

import index_update_spec as S


def storage(seed, nlist=6, n=200, width=5, empty=(), id_base=0):
    return S.random_storage(np.random.default_rng(seed), nlist, n, width, empty=empty, id_base=id_base)


def test_merge_is_a_stable_sort_of_the_concatenation():
    srcs = [storage(1, n=200, empty=(2,)), storage(2, n=90, empty=(2, 4), id_base=1000), storage(3, n=0), storage(4, n=7, empty=(2,), id_base=5000)]
    offs, (ids, rows) = S.merge_storage([(o, [i, r]) for o, i, r in srcs])
    part = np.concatenate([S.part_ids(o) for o, _, _ in srcs])
    order = np.argsort(part, kind="stable")
    assert np.array_equal(ids, np.concatenate([i for _, i, _ in srcs])[order])
    assert np.array_equal(rows, np.concatenate([r for _, _, r in srcs])[order])
    assert np.array_equal(offs[1:], np.cumsum(np.bincount(part, minlength=6)))
    assert offs[2] == offs[3]                                   # a partition empty in every source stays an empty range
    one = S.merge_storage([(srcs[0][0], [srcs[0][1]])])
    assert np.array_equal(one[0], srcs[0][0]) and np.array_equal(one[1][0], srcs[0][1])


def test_remap_with_only_deletions_is_compaction_by_mask():
    offs, ids, rows = storage(5)
    gone = ids[::3]
    o2, i2, (r2,) = S.remap_storage(offs, ids, [rows], {int(g): None for g in gone})
    mask = ~np.isin(ids, gone)
    assert np.array_equal(i2, ids[mask]) and np.array_equal(r2, rows[mask])
    assert np.array_equal(o2[1:], np.cumsum(np.bincount(S.part_ids(offs)[mask], minlength=6)))


def test_swap_big_ids_absent_ids_and_whole_partitions():
    offs, ids, rows = storage(6)
    a, b = int(ids[3]), int(ids[150])
    o2, i2, (r2,) = S.remap_storage(offs, ids, [rows], {a: b, b: a})
    assert np.array_equal(o2, offs) and np.array_equal(r2, rows)
    assert i2[3] == b and i2[150] == a and np.array_equal(np.delete(i2, [3, 150]), np.delete(ids, [3, 150]))
    big = (1 << 40) + 17
    o3, i3, _ = S.remap_storage(offs, ids, [rows], {a: big, 10 ** 12: 5})          # 10^12 is no stored id: ignored
    assert i3[3] == big and i3.dtype == np.uint64 and np.array_equal(o3, offs) and 5 not in i3[[3]]
    p = 2
    whole = {int(i): None for i in ids[offs[p]:offs[p + 1]]}
    o4, i4, _ = S.remap_storage(offs, ids, [rows], whole)
    assert o4[p] == o4[p + 1] and o4[-1] == offs[-1] - (offs[p + 1] - offs[p])
    o5, i5, (r5,) = S.remap_storage(offs, ids, [rows], {int(i): None for i in ids})
    assert not o5.any() and i5.size == 0 and r5.shape == (0, 5)


def test_empty_mapping_is_the_identity():
    offs, ids, rows = storage(7)
    o2, i2, (r2,) = S.remap_storage(offs, ids, [rows], {})
    assert np.array_equal(o2, offs) and np.array_equal(i2, ids) and np.array_equal(r2, rows)
    old, new = S.mapping_arrays({5: None, 2: 9})
    assert old.tolist() == [2, 5] and new.tolist() == [9, S.DELETED]
