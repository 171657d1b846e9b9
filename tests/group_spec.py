"""What the library's grouping returns, in numpy: the stable group-by of row numbers by key (lance_amd/csrc/group.hip, stable_group) and
the work items a grouped scan cuts its pair table into (lance_amd/csrc/search_q.hip, qscan_items).  Both are deterministic integer
code, so the checkers compare exactly.  tests/test_group_spec.py holds the spec against a brute-force definition and shows that the
checkers reject wrong answers; tests/test_zz_gpu_grouping.py holds the kernels against the spec."""
import numpy as np

NONE = 0xFFFFFFFF      # LANCE_HIP_NONE


def _u32(a):
    """flat, and the uint32 bits of an int32 array (torch has no uint32 arithmetic: the device buffers travel as int32)"""
    a = np.asarray(a).reshape(-1)
    return a.view(np.uint32) if a.dtype == np.int32 else a


def group(keys, k):
    """keys: uint32 [n]; a key >= k (NONE among them) drops its row.
    -> (starts uint32 [k + 1], rows uint32 [starts[k]]): starts = the exclusive running sum of the rows per key with the total at [k],
    rows = the kept row numbers grouped by key, ascending inside a key."""
    keys = np.asarray(keys, dtype=np.uint32).reshape(-1)
    valid = np.flatnonzero(keys.astype(np.int64) < k)
    counts = np.bincount(keys[valid].astype(np.int64), minlength=k)
    starts = np.zeros(k + 1, np.int64)
    np.cumsum(counts, out=starts[1:])
    rows = valid[np.argsort(keys[valid], kind="stable")]
    return starts.astype(np.uint32), rows.astype(np.uint32)


def work_items(pair_starts, G, max_items):
    """pair_starts: uint32 [nvp + 1], non-decreasing.
    -> (item_start uint32 [nvp + 1], desc int32 [max_items][4]): item_start = the exclusive running sum of ceil(pairs of vp / G);
    desc[item] = {vp, pair_starts[vp] + G * g, min(G, pairs left), 0} for block g of partition vp, {-1, 0, 0, 0} from the item
    total on.  A max_items below the total cuts the list short."""
    ps = np.asarray(pair_starts, dtype=np.uint32).reshape(-1).astype(np.int64)
    counts = np.diff(ps)
    assert ps.size >= 1 and (counts >= 0).all() and G >= 1
    per = (counts + G - 1) // G
    item_start = np.zeros(ps.size, np.int64)
    np.cumsum(per, out=item_start[1:])
    total = int(item_start[-1])
    desc = np.zeros((max_items, 4), np.int64)
    desc[:, 0] = -1
    vp = np.repeat(np.arange(counts.size), per)
    g = np.arange(total) - item_start[vp]
    first = ps[vp] + G * g
    m = min(total, max_items)
    desc[:m, 0] = vp[:m]
    desc[:m, 1] = first[:m]
    desc[:m, 2] = np.minimum(G, ps[vp + 1] - first)[:m]
    return item_start.astype(np.uint32), desc.astype(np.int32)


def check_group(got_starts, got_rows, keys, k):
    """got_starts: at least k + 1 entries; got_rows: at least starts[k] entries (what lies behind is not compared)."""
    starts, rows = group(keys, k)
    got_starts, got_rows = _u32(got_starts), _u32(got_rows)
    assert got_starts.size >= k + 1, f"starts holds {got_starts.size} entries, k + 1 = {k + 1}"
    bad = np.flatnonzero(got_starts[:k + 1] != starts)
    assert bad.size == 0, f"starts[{bad[0]}] = {got_starts[bad[0]]}, expected {starts[bad[0]]} ({bad.size} entries differ; k = {k}, n = {np.size(keys)})"
    total = int(starts[k])
    assert got_rows.size >= total, f"rows holds {got_rows.size} entries, {total} rows are grouped"
    bad = np.flatnonzero(got_rows[:total] != rows)
    assert bad.size == 0, f"rows[{bad[0]}] = {got_rows[bad[0]]}, expected {rows[bad[0]]} ({bad.size} of {total} differ; k = {k}, n = {np.size(keys)})"


def check_items(got_item_start, got_desc, pair_starts, G, max_items):
    """got_item_start: at least nvp + 1 entries; got_desc: at least max_items records of four."""
    item_start, desc = work_items(pair_starts, G, max_items)
    nvp = item_start.size - 1
    gi = _u32(got_item_start)
    assert gi.size >= nvp + 1, f"item_start holds {gi.size} entries, nvp + 1 = {nvp + 1}"
    bad = np.flatnonzero(gi[:nvp + 1] != item_start)
    assert bad.size == 0, f"item_start[{bad[0]}] = {gi[bad[0]]}, expected {item_start[bad[0]]} ({bad.size} entries differ; nvp = {nvp}, G = {G})"
    gd = np.asarray(got_desc).reshape(-1)
    assert gd.size >= 4 * max_items, f"desc holds {gd.size // 4} records, max_items = {max_items}"
    gd = gd[:4 * max_items].reshape(max_items, 4)
    bad = np.flatnonzero((gd != desc).any(axis=1))
    assert bad.size == 0, (f"desc[{bad[0]}] = {gd[bad[0]].tolist()}, expected {desc[bad[0]].tolist()} "
                           f"({bad.size} of {max_items} differ; item total {int(item_start[-1])}, nvp = {nvp}, G = {G})")
