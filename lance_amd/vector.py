"""Host-side mirror of the reference's IVF_PQ build / query interface for the hot path.

Names, argument meaning and defaults follow the reference (citations relative to the
lancedb/lance tree):
  * create_index(..., "IVF_PQ", metric, num_partitions, num_sub_vectors, ivf_centroids=,
    pq_codebook=, sample_rate, max_iters)          python/python/lance/dataset.py:2517-2545
  * IvfBuildParams / PQBuildParams defaults        rust/lance-index/src/vector/ivf/builder.rs:62-78,
                                                   pq/builder.rs:48-58
  * build order: sample -> train IVF -> residuals -> train PQ -> transform all rows ->
    per-partition storage                          rust/lance/src/index/vector/builder.rs:236-254,377-466
  * nearest={"q", "k", "nprobes", "refine_factor"} python/src/dataset.rs:984-1095
  * KMeans(k, metric_type, max_iters, centroids).fit/.predict   python/python/lance/util.py:45-170

All computation happens in liblance_hip.so; this module only orchestrates.
"""
import time
from dataclasses import dataclass, field, replace
from typing import Optional

import numpy as np
import torch

from ._lib import EINVAL, METRICS, MULTIVEC_MAX_QUERY_VECTORS, NONE, ROW_DELETED, LanceHipError
from .engine import (DeviceFlatIndex, DeviceIndex, DeviceRqIndex, DeviceSqIndex, Engine, _dtype_name, _export_ids, check_multivector,
                     check_multivector_ann_sizes, to_device)

_engine = None


def default_engine():
    global _engine
    if _engine is None:
        _engine = Engine()
    return _engine


def _normalize_metric_type(metric):
    m = str(metric).lower()
    if m == "euclidean":
        m = "l2"
    if m not in ("l2", "cosine", "dot"):
        raise ValueError(f"Metric {metric} not supported.")
    return m


class KMeans:
    """lance.util.KMeans (python/python/lance/util.py:45-170) on the MI355X engine."""

    def __init__(self, k, metric_type="l2", max_iters=50, centroids=None, seed=0, engine=None):
        self.k = k
        self._metric_type = _normalize_metric_type(metric_type)
        self.max_iters = max_iters
        self.seed = seed
        self._engine = engine or default_engine()
        self._centroids = None if centroids is None else to_device(np.asarray(centroids, np.float32))
        self.loss = None
        self.iters = None

    def __repr__(self):
        return f"lance_amd.KMeans(k={self.k}, metric_type={self._metric_type})"

    @property
    def centroids(self):
        return None if self._centroids is None else self._centroids.cpu().numpy()

    @staticmethod
    def _check(data):
        if isinstance(data, torch.Tensor):
            if data.dim() != 2 or data.dtype != torch.float32:
                raise ValueError("Data must be a 2-D float32 array")
            return data
        data = np.asarray(data)
        if data.ndim != 2:
            raise ValueError(f"Numpy array must be a 2-D array, got {data.ndim}-D")
        if data.dtype != np.float32:
            raise ValueError(f"Numpy array must be float32 type, got: {data.dtype}")
        return data

    def fit(self, data):
        x = to_device(self._check(data))
        metric = self._metric_type
        if metric == "cosine":  # python/src/utils.rs _KMeans::fit -> KMeans::new_with_params normalises for cosine
            x = self._engine.normalize(x)
            metric = "l2"
        # _KMeans uses KMeansParams::new(...) (redos 1, no balance) and sample_rate 256 (python/src/utils.rs:75-109)
        n = x.shape[0]
        if n > 256 * self.k:
            x = x[: 256 * self.k]
        self._centroids, self.loss, self.iters = self._engine.kmeans_train(
            x, self.k, max_iters=self.max_iters, init=self._centroids, seed=self.seed, metric=metric)

    def predict(self, data):
        if self._centroids is None:
            raise ValueError("KMeans model is not trained")
        x = to_device(self._check(data))
        metric = self._metric_type
        if metric == "cosine":
            x = self._engine.normalize(x)
            metric = "l2"
        ids, _ = self._engine.assign(x, self._centroids, metric)
        return ids.cpu().numpy().view(np.uint32)


@dataclass
class IvfPqParams:
    num_partitions: int = 256
    num_sub_vectors: int = 16
    num_bits: int = 8
    metric: str = "l2"
    max_iters: int = 50          # IvfBuildParams::max_iters / PQBuildParams::max_iters
    sample_rate: int = 256       # both default to 256
    seed: int = 42


@dataclass
class BuildStats:
    seconds: dict = field(default_factory=dict)
    ivf_iters: int = 0
    pq_iters: Optional[np.ndarray] = None
    ivf_loss: float = 0.0
    ivf_training: str = "single"      # multi-GPU builds: "replicated" | "sharded" | "hierarchical" (lance_amd/dist.py)
    ivf_hierarchical: Optional[dict] = None      # hierarchical training spread over ranks: rounds, splits applied / thrown away

    @property
    def total(self):
        return sum(self.seconds.values())


def _mapping_arrays(mapping):
    """dict {old: new | None} or (old_ids, new_ids) with None / -1 for a deleted row -> (old u64, new u64) numpy arrays"""
    def ids(seq, allow_deleted):
        if isinstance(seq, torch.Tensor):
            seq = seq.detach().cpu().numpy()
        if isinstance(seq, np.ndarray) and seq.dtype.kind in "iu":
            return np.ascontiguousarray(seq.astype(np.int64) if seq.dtype.kind == "i" else seq.astype(np.uint64)).view(np.uint64).reshape(-1)
        out = np.empty(len(seq), np.uint64)
        for i, v in enumerate(seq):
            if v is None or int(v) == -1:
                if not allow_deleted:
                    raise ValueError("remap: an old id cannot be None / -1")
                out[i] = ROW_DELETED
            else:
                out[i] = int(v)
        return out
    if isinstance(mapping, dict):
        old, new = list(mapping.keys()), list(mapping.values())
    else:
        old, new = mapping
    old, new = ids(old, False), ids(new, True)
    if old.size != new.size:
        raise ValueError(f"remap: {old.size} old ids but {new.size} new ids")
    return old, new


# ---- partition split / join: which partition, if any (rust/lance/src/index/vector/builder.rs:1152-1176, :1343-1400) ---------------
MAX_PARTITION_SIZE_FACTOR = 4          # lance-index/src/lib.rs:52-53
MIN_PARTITION_SIZE_PERCENT = 25


def target_partition_size(index_type):
    """IndexType::target_partition_size (lance-index/src/lib.rs:284-295): the rows a partition of this index kind should hold"""
    sizes = {"IVF_FLAT": 4096, "IVF_PQ": 8192, "IVF_SQ": 8192}
    key = str(index_type).upper()
    if key not in sizes:
        raise ValueError(f"target_partition_size: index type {index_type} has no partition split / join (IVF_FLAT, IVF_PQ, IVF_SQ)")
    return sizes[key]


def should_split(sizes, target):
    """sizes: the rows of every partition, old and appended together -> the partition optimize_indices would split, or None: the one
    with the most rows among those with MORE than 4 * target; on equal sizes the lowest id (the reference keeps a candidate only
    on `>`).  Pure host code."""
    best, best_size = None, 0
    for p, size in enumerate(sizes):
        size = int(size)
        if size > MAX_PARTITION_SIZE_FACTOR * int(target) and size > best_size:
            best, best_size = p, size
    return best


def should_join(sizes, target):
    """sizes: the rows of every partition that SURVIVE the mapping of a remap (rows mapped to deleted do not count) -> the partition
    remap would join into its neighbours, or None: the one with the fewest rows among those with FEWER than 25 * target / 100
    (integer arithmetic); on equal sizes the lowest id; never when there is only one partition.  Pure host code."""
    sizes = list(sizes)
    if len(sizes) <= 1:
        return None
    best, best_size = None, 0
    for p, size in enumerate(sizes):
        size = int(size)
        if size < MIN_PARTITION_SIZE_PERCENT * int(target) // 100 and (best is None or size < best_size):
            best, best_size = p, size
    return best


class _IvfIndex:
    """An index wrapper: `_ix` is the device index it speaks for."""

    @property
    def centroids(self):
        return self._ix.centroids.cpu().numpy()


class _Maintenance(_IvfIndex):
    """append / remap / delete of an index wrapper (lance_hip_index_merge / _remap): every call returns a NEW index and leaves this one
    as it is -- both are resident until the caller drops one.  By default append and remap take the reference's no-split / no-join
    branch of optimize_indices and remap (rust/lance/src/index/vector/ivf.rs:355-560, builder.rs:256-359); with rebalance=True they
    go on as the reference does: append splits the largest over-full partition of the merged index, remap / delete join the smallest
    under-full partition before the mapping is applied (should_split / should_join above, split_partition / join_partition below:
    lance_hip_index_split / _join)."""
    _index_type = None        # "IVF_PQ" | "IVF_FLAT" | "IVF_SQ": selects target_partition_size
    _rows_offered = None      # rows handed to create_index / append so far: the next positional row id (None: opened from files, merged)

    def _wrap(self, dev_index, rows_offered):
        raise NotImplementedError

    def _delta(self, x_new, row_ids):
        raise NotImplementedError

    def export_rows(self):
        """the stored rows in stored order, row-major (DeviceIndex / DeviceFlatIndex / DeviceSqIndex.export_rows)"""
        return self._ix.export_rows()

    def _rewrap(self, dev_index):
        out = self._wrap(dev_index, self._rows_offered)
        out.params = replace(self.params, num_partitions=int(dev_index.centroids.shape[0]))
        return out

    def _target(self, size):
        return target_partition_size(self._index_type) if size is None else int(size)

    def split_partition(self, part, raw, centroids=None, seed=0):
        """The index with partition `part` split in two (split_partition_impl, builder.rs:1177-1340): c1 replaces its centroid, c2 becomes
        partition nlist; its rows and the rows of its up to 64 nearest neighbours are re-assigned on the GPU and the movers re-encoded
        with this index's own model.  raw [rows][d] float32, indexed by the stored row ids.  centroids: [c1, c2], or None to train them
        as the reference does -- k-means with k = 2, 50 iterations, on the partition's raw rows in ascending row id (normalised and
        trained in L2 for cosine); where the reference samples 512 rows at random, the first 512 in that order are taken."""
        ix = self._ix
        try:
            if centroids is None:
                centroids = self._train_split(int(part), raw, seed)
            return self._rewrap(ix.split(part, centroids, raw))
        except LanceHipError as e:
            if e.code == EINVAL:
                raise ValueError(str(e)) from e
            raise

    def join_partition(self, part, raw):
        """The index without partition `part` (join_partition_impl, builder.rs:1401-1530): every one of its rows goes to the nearest of
        its up to 64 neighbouring partitions and is re-encoded there; partition ids above `part` drop by one."""
        try:
            return self._rewrap(self._ix.join(part, raw))
        except LanceHipError as e:
            if e.code == EINVAL:
                raise ValueError(str(e)) from e
            raise

    def _train_split(self, part, raw, seed):
        ix = self._ix
        if raw is None:
            raise ValueError("split_partition: the raw vectors are required")
        if ix.data_dtype != torch.float32:
            raise ValueError(f"split_partition: f32 columns only in this version (the index holds {ix.data_dtype} vectors)")
        nlist = int(ix.centroids.shape[0])
        if not 0 <= part < nlist:
            raise ValueError(f"split_partition: partition {part} does not exist (nlist = {nlist})")
        offs, ids = _export_ids(ix.engine, ix.h, nlist)
        mine = np.sort(ids[int(offs[part]):int(offs[part + 1])])[:2 * 256]          # sample_rate 256 x k 2
        if mine.size < 2:
            raise ValueError(f"split_partition: partition {part} holds {mine.size} rows, a split needs at least 2")
        raw_t = to_device(raw, torch.float32)
        if int(mine.max()) >= raw_t.shape[0]:
            raise ValueError(f"split_partition: a stored row id is >= n_raw={raw_t.shape[0]} (the raw vectors do not cover the index)")
        rows = raw_t[to_device(mine.astype(np.int64))]
        metric = _normalize_metric_type(self.params.metric)
        if metric == "cosine":
            rows = ix.engine.normalize(rows)
        cent, _, _ = ix.engine.kmeans_train(rows, 2, max_iters=50, seed=seed, metric="l2" if metric == "cosine" else metric)
        return cent.to(torch.float32)

    def append(self, x_new, row_ids=None, raw=None, rebalance=False, target_partition_size=None, seed=0):
        """The index with the rows x_new added: they are transformed with THIS index's model (centroids, codebook, SQ bounds -- nothing is
        re-trained, ivf.rs:377-378) through the calls create_index makes, grouped into a delta index and merged behind the stored rows of
        every partition.  Non-finite rows are dropped.  row_ids: one id per row of x_new; None continues create_index's position
        convention (rows offered so far + i), which an index opened from files cannot do.  raw (IVF_PQ): the vectors for refine.
        rebalance=True (raw required: the vectors of the old AND the new rows, indexed by row id): after the merge, the partition
        should_split picks among the merged sizes -- at most one -- is split (split_partition with trained centroids, `seed`).
        target_partition_size: None = the index type's reference value.  An IVF_PQ result has raw attached for refine whether or
        not a partition was split."""
        if rebalance and raw is None:
            raise ValueError("append(rebalance=True): the raw vectors are required (old and new rows, indexed by row id)")
        x_new = to_device(x_new)
        if x_new.dim() != 2 or x_new.shape[1] != self._ix.centroids.shape[1]:
            raise ValueError(f"append: rows must be [n][{self._ix.centroids.shape[1]}], got {tuple(x_new.shape)}")
        n_new = x_new.shape[0]
        if row_ids is None:
            if self._rows_offered is None:
                raise ValueError("append: this index does not know how many rows it was built from (opened from files or merged): pass row_ids")
            rid = torch.arange(self._rows_offered, self._rows_offered + n_new, dtype=torch.int64, device=x_new.device)
        else:
            rid = to_device(_ids_u64(row_ids))
            if rid.numel() != n_new:
                raise ValueError(f"append: row_ids must hold one id per row ({n_new}), got {rid.numel()}")
        delta = self._delta(x_new, rid)
        try:
            merged = type(self._ix).merge([self._ix, delta], raw=raw)
        finally:
            delta.close()
        out = self._wrap(merged, None if self._rows_offered is None else self._rows_offered + n_new)
        if rebalance:
            offs, _ = _export_ids(merged.engine, merged.h, int(merged.centroids.shape[0]))
            part = should_split(np.diff(offs.astype(np.int64)), self._target(target_partition_size))
            if part is not None:
                try:
                    grown = out.split_partition(part, raw, seed=seed)
                finally:
                    merged.close()
                if isinstance(self, IvfPqIndex):
                    grown._ix.set_raw(raw)                      # as the merged index: the vectors stay attached for refine
                return grown
        return out

    def remap(self, mapping, raw=None, rebalance=False, target_partition_size=None):
        """The index after a compaction or a delete: mapping = dict {old id: new id | None} or a pair (old_ids, new_ids) with None / -1 for
        a deleted row.  Stored rows keep their order; a row whose id is not an old id stays as it is; all lookups are against the ids
        before the call (a swap swaps).  Duplicate old ids raise ValueError.
        rebalance=True (raw required, indexed by the ids stored NOW): the partition should_join picks among the sizes that survive the
        mapping -- at most one, rows mapped to deleted do not count -- is joined first, then the mapping is applied (the reference's
        order).  target_partition_size: None = the index type's reference value."""
        old, new = _mapping_arrays(mapping)
        if rebalance:
            if raw is None:
                raise ValueError("remap / delete(rebalance=True): the raw vectors are required (indexed by the stored row ids)")
            ix = self._ix
            offs, ids = _export_ids(ix.engine, ix.h, int(ix.centroids.shape[0]))
            gone = np.isin(ids, old[new == np.uint64(ROW_DELETED)])
            part_of = np.repeat(np.arange(offs.size - 1), np.diff(offs.astype(np.int64)))
            part = should_join(np.bincount(part_of[~gone], minlength=offs.size - 1), self._target(target_partition_size))
            if part is not None:
                joined = self.join_partition(part, raw)
                try:
                    return joined.remap((old, new), raw=raw if isinstance(self, IvfPqIndex) else None)
                finally:
                    joined._ix.close()
            if not isinstance(self, IvfPqIndex):
                raw = None                                      # (only IVF_PQ attaches raw vectors to the result, for refine)
        old_t, new_t = to_device(old), to_device(new)
        key = old_t ^ torch.iinfo(torch.int64).min          # signed order of the key = unsigned order of the id
        key, order = torch.sort(key)
        if key.numel() > 1 and bool((key[1:] == key[:-1]).any()):
            raise ValueError("remap: duplicate old ids in the mapping")
        kw = {"raw": raw} if raw is not None else {}
        return self._wrap(self._ix.remap(old_t[order], new_t[order], **kw), self._rows_offered)

    def delete(self, row_ids, raw=None, rebalance=False, target_partition_size=None):
        """remap with every given id mapped to deleted"""
        ids = np.unique(_ids_u64(row_ids))
        return self.remap((ids, np.full(ids.size, ROW_DELETED, np.uint64)), raw=raw, rebalance=rebalance, target_partition_size=target_partition_size)


def _ids_u64(row_ids):
    """row ids (numpy / torch / sequence, signed or unsigned) -> u64 numpy array"""
    if isinstance(row_ids, torch.Tensor):
        row_ids = row_ids.detach().cpu().numpy()
    a = np.asarray(row_ids)
    if a.dtype.kind == "i":
        return np.ascontiguousarray(a.astype(np.int64)).view(np.uint64).reshape(-1)
    return np.ascontiguousarray(a.astype(np.uint64)).reshape(-1)


def merge_indices(indices, raw=None):
    """Several indices over the same model -> one (the reference's merge of delta indices, `optimize_indices(num_indices_to_merge)`,
    builder.rs:742-756,849-935): for every partition the rows of indices[0] in stored order, then those of indices[1], ...  The
    sources are not modified.  ValueError (with the library's message) for mixed kinds or different models."""
    indices = list(indices)
    if not indices:
        raise ValueError("merge_indices: no index given")
    kinds = {type(ix) for ix in indices}
    if any(k.__name__ == "IvfRqIndex" for k in kinds):
        raise NotImplementedError("IVF_RQ: merge_indices is not supported (the reference's RabitQ storage has no append_batch): rebuild the index")
    if len(kinds) != 1 or not isinstance(indices[0], _Maintenance):
        raise ValueError(f"merge_indices: the indices must be of one kind, got {sorted(k.__name__ for k in kinds)}")
    try:
        merged = type(indices[0]._ix).merge([ix._ix for ix in indices], raw=raw)
    except LanceHipError as e:
        if e.code == EINVAL:
            raise ValueError(str(e)) from e
        raise
    return indices[0]._wrap(merged, None)


def _adaptive_nearest(run, q, d, k, nlist, nprobes, minimum_nprobes, maximum_nprobes, prefilter=None, shortcut=False):
    """Adaptive probing above any sub-index (Query::minimum_nprobes / maximum_nprobes; ANNIvfSubIndexExec initial_search +
    late_search, knn.rs:714-860), as IvfPqIndex.nearest documents it: every query searches its `minimum_nprobes` nearest
    partitions; while some query holds fewer than k rows and partitions are left, those queries alone are searched again with
    min(max, max(2 * n, n + 1)) partitions.  `nprobes=n` alone means minimum = maximum = n.
    run(queries, nprobes) -> (ids int64 [n, k] with -1 = missing, distances f32 [n, k]) on the device: what `nearest` would
    return for that many partitions, so a re-ranking search is judged after re-ranking.
    shortcut: late_search's early exit (knn.rs:741-779) applies -- the caller passes True for a prefilter without a refine
    factor or a range.  When the prefilter selects at most k rows, a query that has not found all of them gets the rest back
    at distance +inf in ascending row id order (SortExec's tie order) and no further partition is searched.
    -> (ids int64, distances f32) as numpy."""
    min_np = nprobes if minimum_nprobes is None else minimum_nprobes
    max_np = (min_np if minimum_nprobes is None else nlist) if maximum_nprobes is None else maximum_nprobes
    max_np = max(min(max_np, nlist), min(min_np, nlist))
    min_np = min(min_np, max_np)
    ids, dists = run(q, min_np)
    if max_np <= min_np:
        return ids.cpu().numpy(), dists.cpu().numpy()
    if shortcut and prefilter is not None:
        allow_np = np.ascontiguousarray(prefilter.cpu().numpy() if isinstance(prefilter, torch.Tensor) else prefilter, dtype=bool)
        mask_ids = np.flatnonzero(allow_np).astype(np.int64)
        if mask_ids.size <= k:
            ids_h, dists_h = ids.cpu().numpy().copy(), dists.cpu().numpy().copy()
            for qi in range(ids_h.shape[0]):
                found = ids_h[qi][ids_h[qi] != -1]
                if found.size < k and found.size < mask_ids.size:
                    rest = np.setdiff1d(mask_ids, found)
                    ids_h[qi, found.size:found.size + rest.size] = rest
                    dists_h[qi, found.size:found.size + rest.size] = np.inf
            return ids_h, dists_h
    qt = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q))
    qt = qt.reshape(-1, d)
    npb = min_np
    while npb < max_np:
        starved = torch.nonzero((ids == -1).any(dim=1)).reshape(-1)     # fewer than k rows found so far
        if starved.numel() == 0:
            break
        npb = min(max_np, max(npb * 2, npb + 1))
        si, sd = run(qt[starved.cpu()] if not qt.is_cuda else qt[starved], npb)
        ids[starved] = si
        dists[starved] = sd
    return ids.cpu().numpy(), dists.cpu().numpy()


def _refined_nearest(name, ix, q, k, nprobes, prefilter, refine_factor, distance_range, minimum_nprobes, maximum_nprobes):
    """`nearest` of the kinds that scan codes and re-rank on the raw column (name = "IVF_SQ" | "IVF_RQ") over the device index ix"""
    if distance_range is not None:
        raise NotImplementedError(f"{name}: distance_range is not supported by this engine")
    if refine_factor is not None:
        if refine_factor < 1:
            raise ValueError("Refine factor can not be zero")
        if ix._raw is None:
            raise NotImplementedError(f"{name}: refine_factor needs the raw vectors (re-ranking scores the candidates against the column): attach them "
                                      "with set_raw(x), or build with create_index(..., keep_raw=True)")

        def run(qq, npb):
            return ix.search(qq, k, npb, allow=prefilter, refine_factor=int(refine_factor))
    else:
        def run(qq, npb):
            return ix.search(qq, k, npb) if prefilter is None else ix.search(qq, k, npb, allow=prefilter)
    ids, dists = _adaptive_nearest(run, q, ix.centroids.shape[1], k, ix.centroids.shape[0], nprobes, minimum_nprobes, maximum_nprobes,
                                   prefilter=prefilter, shortcut=refine_factor is None)
    return ids.view(np.uint64), dists


def _masked_part_ids(allow, part, row_ids=None):
    """The partition ids `part` with -1 (LANCE_HIP_NONE: such rows are dropped by the create calls) for every row that `allow`
    (bool over row ids) does not select.  row_ids: the id of each row, None = its position."""
    allow_t = to_device(np.ascontiguousarray(allow, dtype=bool)) if not isinstance(allow, torch.Tensor) else allow.to(part.device)
    ids = torch.arange(part.numel(), device=part.device) if row_ids is None else row_ids
    inside = ids < allow_t.numel()
    sel = torch.zeros_like(inside)
    sel[inside] = allow_t[ids[inside]]
    return torch.where(sel, part, torch.full_like(part, -1))


def _element_type_name(ix):
    """the `dtype` argument of DeviceIndex.create for the element type of ix's queries and raw vectors"""
    return {torch.float16: "float16", torch.int8: "int8"}.get(ix.data_dtype, "float32")


class IvfPqIndex(_Maintenance):
    """An IVF_PQ index resident in HBM with the reference's query semantics."""
    _index_type = "IVF_PQ"

    def __init__(self, dev_index, params, stats=None, part_ids=None, codes=None):
        self._ix = dev_index
        self.params = params
        self.stats = stats
        self.part_ids = part_ids   # shuffle-buffer columns (device), kept for hand-off to Lance
        self.codes = codes

    @property
    def codebook(self):
        """numpy (M, 256, d/M) -- the `pq_codebook` artefact (dataset.py:2928-2954)"""
        return self._ix.codebook.cpu().numpy()

    def info(self):
        return self._ix.info()

    def export_storage(self):
        return self._ix.export()

    def _wrap(self, dev_index, rows_offered):
        out = IvfPqIndex(dev_index, self.params, self.stats)
        out._rows_offered = rows_offered
        return out

    def _delta(self, x_new, row_ids):
        ix = self._ix
        part, codes = _transform_rows(ix.engine, "IVF_PQ", self.params.metric, x_new, ix.centroids, codebook=ix.codebook)
        return DeviceIndex.create(ix.engine, ix.metric, ix.centroids, ix.codebook, part, codes, row_ids, dtype=_element_type_name(ix))

    def shuffle_buffers(self):
        """(row_id u64, __ivf_part_id u32, __pq_code u8[M]) as numpy -- the artefact the reference's
        `precomputed_shuffle_buffers` hand-off consumes (python/lance/vector.py:659-665).  An index without the retained columns
        (opened from files, merged, appended to, remapped) hands back its stored rows: real row ids, partition order."""
        if self.part_ids is None or self.codes is None:
            offs, codes, rid = self._ix.export_rows()
            return rid, np.repeat(np.arange(offs.size - 1, dtype=np.uint32), np.diff(offs.astype(np.int64))), codes
        part = self.part_ids.cpu().numpy().view(np.uint32)
        keep = part != NONE
        rid = np.arange(part.size, dtype=np.uint64)[keep]
        return rid, part[keep], self.codes.cpu().numpy()[keep]

    def nearest(self, q, k=10, nprobes=1, refine_factor=None, prefilter=None, distance_range=None, minimum_nprobes=None,
                maximum_nprobes=None):
        """-> (row ids int64 [nq,k] (-1 = missing), distances f32 [nq,k]) as numpy.
        prefilter: boolean array over row ids (True = row may be returned) -- `nearest=..., filter=..., prefilter=True`
        of the reference (scanner.rs prefilter -> FlatIndex::search's RowIdMask branch, flat/index.rs:129-165).  The mask is
        tested inside the scan kernels (lance_hip_ivfpq_search_filtered); no filtered copy of the index is built.
        distance_range: (lower, upper), either may be None -- rows with lower <= d < upper only (Query::lower_bound /
        upper_bound, flat/index.rs:98-113).
        minimum_nprobes / maximum_nprobes: adaptive probing (Query::minimum_nprobes / maximum_nprobes; ANNIvfSubIndexExec
        initial_search + late_search, knn.rs:714-860): every query searches its `minimum_nprobes` nearest partitions; a query
        that found fewer than k rows (a selective prefilter, tiny partitions) goes on through further partitions, nearest
        first, until it has k rows or `maximum_nprobes` (default: all) partitions were searched.  `nprobes=n` alone means
        minimum = maximum = n, as in pylance (python/src/dataset.rs:984-1020).  The reference extends the search one
        partition at a time from concurrently running tasks, so how far it overshoots depends on thread timing; here the
        extension is deterministic: the number of partitions doubles until the query is satisfied.  late_search's shortcut
        for prefilters that select at most k rows (the unfound selected rows come back at distance +inf) is reproduced for
        searches without a refine factor."""
        rf = 0 if refine_factor is None else refine_factor

        def run(qq, npb):
            if distance_range is not None:      # late_search extends range queries too (knn.rs:714-860)
                lo, hi = distance_range
                return self._ix.search_range(qq, k, npb, lo, hi, refine_factor=rf, allow=prefilter)
            if prefilter is None:
                return self._ix.search(qq, k, npb, rf)
            return self._ix.search_filtered(qq, k, npb, prefilter, rf)

        return _adaptive_nearest(run, q, self._ix.centroids.shape[1], k, self.params.num_partitions, nprobes, minimum_nprobes,
                                 maximum_nprobes, prefilter=prefilter, shortcut=(not rf and distance_range is None))

    def _storage_rows(self):
        """(part ids int32 [n], row-major codes u8 [n, code bytes], row ids int64 [n] | None) on the device, in an order
        whose stable grouping by partition is the stored order"""
        if self.part_ids is not None and self.codes is not None:
            return self.part_ids, self.codes, None
        if hasattr(self._ix, "export_rows"):            # no retained columns: the stored rows, row-major
            offs, codes, rid = self._ix.export_rows()
            lens = to_device(np.diff(offs.astype(np.int64)))
            part = torch.repeat_interleave(torch.arange(offs.size - 1, dtype=torch.int32, device=lens.device), lens)
            return part, to_device(codes), to_device(rid)
        offs, codes_t, rid = self._ix.export()          # a handle that only hands out the reference's layout: undo the per-partition
        n = len(rid)                                    # transpose with one gather (row r, byte j sits at off*cb + j*n_p + r - off)
        cb = codes_t.size // n if n else 1
        ct = to_device(codes_t)
        lens = to_device(np.diff(offs.astype(np.int64)))
        part = torch.repeat_interleave(torch.arange(offs.size - 1, dtype=torch.int32, device=ct.device), lens)
        start = to_device(offs[:-1].astype(np.int64))[part.long()]
        row = torch.arange(n, device=ct.device) - start
        src = (start * cb + row)[:, None] + torch.arange(cb, device=ct.device)[None, :] * lens[part.long()][:, None]
        return part, ct[src.reshape(-1)].view(n, cb), to_device(rid)

    def prefiltered(self, allow):
        """The index restricted to the rows whose id is selected by `allow` (bool over row ids).  Under a prefilter the
        reference visits a partition's rows in storage order, skips the unselected ones and feeds the rest to the same
        k-heap (flat/index.rs:129-165); for 8-bit PQ `distance(id)` sums the same table entries in the same order as
        `distance_all` (pq/storage.rs:893-960), so searching a compacted copy of the storage -- unselected rows dropped,
        order kept -- gives bit-identical results (tests/test_oracle_golden.py::test_prefilter_equals_compaction).  The
        compacted copy is built by lance_hip_index_create, which already drops rows without a partition.  One O(n) pass
        per distinct filter; queries sharing a filter should share the returned index."""
        from .engine import DeviceIndex
        if self.params.num_bits == 4:
            # 4-bit PQ: the reference scores FILTERED rows with the unquantised f32 table (pq/storage.rs:893-921), a different arithmetic
            # from its unfiltered fast-scan -- a compacted copy would be searched with the wrong one.  The masked kernels implement it
            # (lance_hip_ivfpq_search_filtered, search.hip pq4_masked_row): hand back a view that carries the mask into every search.
            return _MaskedIndexView(self, allow)
        part, codes, rid = self._storage_rows()
        masked = _masked_part_ids(allow, part, rid)
        ix = self._ix
        sub = DeviceIndex.create(ix.engine, ix.metric, ix.centroids, ix.codebook, masked, codes, rid, raw=ix._raw, dtype=_element_type_name(ix))
        return IvfPqIndex(sub, self.params, self.stats, masked, codes if rid is None else None)

    def search_device(self, q, k, nprobes, refine_factor=0, out=None, sync=True, engine=None):
        return self._ix.search(q, k, nprobes, refine_factor, out=out, sync=sync, engine=engine)

    def save(self, index_dir):
        """Writes `index.idx` + `auxiliary.idx` under index_dir -- the files IvfIndexBuilder::merge_partitions produces
        (rust/lance/src/index/vector/builder.rs:938-1079), loadable by `load_index` here (and laid out for the
        reference's IvfQuantizationStorage reader)."""
        self._ix.save(index_dir, None if self.stats is None else self.stats.ivf_loss)

    def to_arrow_artifacts(self, batch_size=10240):
        """-> (ivf_centroids RecordBatch, pq_codebook RecordBatch, iterator of shuffle-buffer RecordBatches): the three
        arguments `Dataset.create_index(..., ivf_centroids=, pq_codebook=, precomputed_shuffle_buffers=)` takes
        (python/python/lance/dataset.py:2780-2954, vector.py:659-665); see lance_amd/arrow_io.py."""
        from . import arrow_io
        rid, part, codes = self.shuffle_buffers()
        return (arrow_io.ivf_centroids_batch(self.centroids), arrow_io.pq_codebook_batch(self.codebook),
                arrow_io.shuffle_buffer_batches(rid, part, codes, batch_size))


class IvfFlatIndex(_Maintenance):
    """IVF_FLAT: IVF partitions over the raw vectors (exact distances inside the probed partitions)."""
    _index_type = "IVF_FLAT"

    def __init__(self, ix, params, stats, part_ids):
        self._ix = ix
        self.params = params
        self.stats = stats
        self.part_ids = part_ids

    def _wrap(self, dev_index, rows_offered):
        out = IvfFlatIndex(dev_index, self.params, self.stats, None)
        out._rows_offered = rows_offered
        return out

    def _delta(self, x_new, row_ids):
        ix = self._ix
        part, xs = _transform_rows(ix.engine, "IVF_FLAT", self.params.metric, x_new.to(ix.data_dtype), ix.centroids)
        return DeviceFlatIndex.create(ix.engine, ix.metric, ix.centroids, xs, part, row_ids)

    def search_device(self, q, k, nprobes):
        return self._ix.search(q, k, nprobes)

    def nearest(self, q, k=10, nprobes=1, prefilter=None, distance_range=None, minimum_nprobes=None, maximum_nprobes=None):
        """-> (row ids uint64 [nq,k] (2^64 - 1 = missing), distances f32 [nq,k]) as numpy.
        prefilter: boolean array over row ids; the mask is tested inside the scan kernels (no copy of the index).
        distance_range: (lower, upper), either may be None -- rows with lower <= d < upper only (Query::lower_bound /
        upper_bound, flat/index.rs:91-149), decided inside every probed partition on this index's exact distances
        (lance_hip_ivfflat_search_range); with a prefilter both are tested in the scan kernels.
        minimum_nprobes / maximum_nprobes: adaptive probing, as IvfPqIndex.nearest (_adaptive_nearest)."""
        if distance_range is not None:
            lo, hi = distance_range
            if lo is None and hi is None:       # (None, None): the range entry point with both ends open
                lo = float(np.finfo(np.float32).min)

            def run(qq, npb):
                return self._ix.search(qq, k, npb, allow=prefilter, lower=lo, upper=hi)
        else:
            def run(qq, npb):
                return self._ix.search(qq, k, npb) if prefilter is None else self._ix.search(qq, k, npb, allow=prefilter)
        cent = self._ix.centroids
        ids, dists = _adaptive_nearest(run, q, cent.shape[1], k, cent.shape[0], nprobes, minimum_nprobes, maximum_nprobes,
                                       prefilter=prefilter, shortcut=distance_range is None)
        return ids.view(np.uint64), dists

    def prefiltered(self, allow):
        """A compacted copy of the index restricted to the selected rows (kept for callers that reuse one filter for many
        batches; `nearest(prefilter=)` does not need it).  FlatIndex::search scores each selected row with the same distance
        function as the unfiltered scan (flat/storage.rs:345-402), so the compacted copy is exact."""
        from .engine import DeviceFlatIndex
        if self.part_ids is None or getattr(self, "_x", None) is None:
            raise NotImplementedError("prefilter needs the index's vectors and partition ids (an index built by create_index)")
        masked = _masked_part_ids(allow, self.part_ids)
        sub = DeviceFlatIndex.create(self._ix.engine, self._ix.metric, self._ix.centroids, self._x, masked)
        out = IvfFlatIndex(sub, self.params, self.stats, masked)
        out._x = self._x
        return out

    def save(self, index_dir):
        self._ix.save(index_dir, None if self.stats is None else self.stats.ivf_loss)


class IvfSqIndex(_Maintenance):
    """IVF_SQ: IVF partitions over 8-bit scalar-quantised codes (lance-index/src/vector/sq.rs, sq/storage.rs): IVF_FLAT's search
    over a quarter of its bytes, distances computed between codes."""
    _index_type = "IVF_SQ"

    def __init__(self, ix, params, stats, part_ids, codes=None):
        self._ix = ix
        self.params = params
        self.stats = stats
        self.part_ids = part_ids
        self._codes = codes

    @property
    def bounds(self):
        """the quantiser's Range<f64> as (start, end)"""
        return self._ix.bounds

    def _wrap(self, dev_index, rows_offered):
        out = IvfSqIndex(dev_index, self.params, self.stats, None)
        out._rows_offered = rows_offered
        return out

    def _delta(self, x_new, row_ids):
        ix = self._ix
        part, codes = _transform_rows(ix.engine, "IVF_SQ", self.params.metric, x_new.to(ix.data_dtype), ix.centroids, bounds=ix.bounds)
        return DeviceSqIndex.create(ix.engine, ix.metric, ix.centroids, codes, part, ix.bounds, row_ids)

    def search_device(self, q, k, nprobes, refine_factor=0):
        return self._ix.search(q, k, nprobes, refine_factor=refine_factor)

    def nearest(self, q, k=10, nprobes=1, prefilter=None, refine_factor=None, distance_range=None, minimum_nprobes=None,
                maximum_nprobes=None):
        """prefilter: boolean array over row ids; the mask is tested inside the scan kernels (no copy of the index).
        minimum_nprobes / maximum_nprobes: adaptive probing, as IvfPqIndex.nearest (_adaptive_nearest); with a refine_factor a
        query counts as satisfied by what re-ranking leaves it, and the shortcut for prefilters of at most k rows does not apply."""
        return _refined_nearest("IVF_SQ", self._ix, q, k, nprobes, prefilter, refine_factor, distance_range, minimum_nprobes, maximum_nprobes)

    def set_raw(self, raw):
        """attach the column (indexed by row id; the ORIGINAL rows) for nearest(..., refine_factor=)"""
        self._ix.set_raw(raw)

    def prefiltered(self, allow):
        """A compacted copy of the index restricted to the selected rows (for callers that reuse one filter for many batches;
        `nearest(prefilter=)` does not need it).  The selected rows keep their codes and their storage order, so the copy answers
        exactly as the prefilter branch of FlatIndex::search does (flat/index.rs:129-165)."""
        if self.part_ids is None or self._codes is None:
            raise NotImplementedError("prefilter needs the index's codes and partition ids (an index built by create_index with keep_raw)")
        masked = _masked_part_ids(allow, self.part_ids)
        sub = DeviceSqIndex.create(self._ix.engine, self._ix.metric, self._ix.centroids, self._codes, masked, self._ix.bounds)
        return IvfSqIndex(sub, self.params, self.stats, masked, self._codes)

    def save(self, index_dir):
        raise NotImplementedError("IVF_SQ index files are not supported (IVF_PQ and IVF_FLAT are)")


class IvfRqIndex(_IvfIndex):
    """IVF_RQ: IVF partitions over 1-bit RaBitQ codes (lance-index/src/vector/bq): d / 8 code bytes and two f32 factors per row, the
    residual rotated by a matrix that is part of the model.  Resident in HBM; nearest(refine_factor=) re-ranks k * refine_factor
    candidates (up to 768) on the raw vectors; no index files, distance ranges or maintenance (the reference's RabitQ storage has no
    append_batch either)."""

    def __init__(self, ix, params, stats, part_ids):
        self._ix = ix
        self.params = params
        self.stats = stats
        self.part_ids = part_ids

    @property
    def rotation(self):
        """the rotation P [d][d] float32 stored with the index (rotated = P @ residual)"""
        return self._ix.rotation.cpu().numpy()

    def search_device(self, q, k, nprobes, refine_factor=0):
        return self._ix.search(q, k, nprobes, refine_factor=refine_factor)

    def nearest(self, q, k=10, nprobes=1, prefilter=None, refine_factor=None, distance_range=None, minimum_nprobes=None,
                maximum_nprobes=None):
        """prefilter: boolean array over row ids; the mask is tested inside the scan kernels, and every selected row takes the f32
        distance (the reference's prefiltered FlatIndex::search never uses the quantised table).
        minimum_nprobes / maximum_nprobes: adaptive probing, as IvfPqIndex.nearest (_adaptive_nearest); with a refine_factor a
        query counts as satisfied by what re-ranking leaves it, and the shortcut for prefilters of at most k rows does not apply."""
        return _refined_nearest("IVF_RQ", self._ix, q, k, nprobes, prefilter, refine_factor, distance_range, minimum_nprobes, maximum_nprobes)

    def set_raw(self, raw):
        """attach the column (indexed by row id; the ORIGINAL rows) for nearest(..., refine_factor=)"""
        self._ix.set_raw(raw)

    def _unmaintained(self, what):
        raise NotImplementedError(f"IVF_RQ: {what} is not supported (the reference's RabitQ storage has no append_batch): rebuild the index")

    def append(self, *a, **kw):
        self._unmaintained("append")

    def remap(self, *a, **kw):
        self._unmaintained("remap")

    def delete(self, *a, **kw):
        self._unmaintained("delete")

    def split_partition(self, *a, **kw):
        self._unmaintained("split_partition")

    def join_partition(self, *a, **kw):
        self._unmaintained("join_partition")

    def save(self, index_dir):
        raise NotImplementedError("IVF_RQ index files are not supported (IVF_PQ and IVF_FLAT are)")

    def close(self):
        self._ix.close()


def rq_rotation_matrix(d, seed):
    """The default rotation of an IVF_RQ index: Q of the QR decomposition of a seeded Gaussian matrix, computed in float64 on the
    host and cast to float32.  (The reference draws its own random orthogonal matrix; its RNG stream is not reproduced -- the matrix
    is part of the model and is stored with the index, as the reference stores its own.)"""
    g = np.random.default_rng(seed).standard_normal((d, d))
    return np.ascontiguousarray(np.linalg.qr(g)[0].astype(np.float32))


def train_sq_bounds(x, params: IvfPqParams, engine=None):
    """load_or_build_quantizer for the scalar quantiser (rust/lance/src/index/vector/builder.rs:399-466, sq.rs:152-180): sample
    sample_rate * 2^num_bits rows, normalise (cosine), drop non-finite rows, fold the rest into fresh bounds.  There is no residual
    step (ScalarQuantizer::use_residual is false).  -> (start, end)"""
    eng = engine or default_engine()
    metric = _normalize_metric_type(params.metric)
    x = to_device(x)
    idx = pq_sample_indices(x.shape[0], params)
    sample = x if idx is None else x[torch.from_numpy(idx).to(x.device)]
    if metric == "cosine":
        sample = eng.normalize(sample)
    sample = sample[torch.isfinite(sample).all(dim=1)]
    return eng.sq_bounds(sample)


def load_index(index_dir, dtype=None, raw=None, engine=None):
    """Opens an index directory (`index.idx` + `auxiliary.idx`, written by the reference or by `save`) straight into
    HBM -> IvfPqIndex | IvfFlatIndex.  dtype: element type of the indexed column when it differs from the stored model
    tensors ("int8" columns keep an f32 model); raw: the column's vectors for refine, indexed by row id."""
    from . import index_file
    from .engine import DeviceFlatIndex, DeviceIndex
    eng = engine or default_engine()
    c = index_file.read_index_files(index_dir, with_rows=False)    # model + metadata only: the rows go files -> HBM natively
    params = IvfPqParams(num_partitions=c.centroids.shape[0], num_sub_vectors=c.num_sub_vectors, num_bits=c.nbits or 8,
                         metric=c.metric)
    stats = BuildStats(ivf_loss=c.loss if c.loss is not None else 0.0)
    if c.index_type == "IVF_PQ":
        return IvfPqIndex(DeviceIndex.load(eng, index_dir, dtype=dtype, raw=raw), params, stats)
    return IvfFlatIndex(DeviceFlatIndex.load(eng, index_dir, dtype=dtype), params, stats, None)


def _sample_rows(n, size, rng):
    """maybe_sample_training_data (rust/lance/src/index/vector/utils.rs:173): all rows when the
    table is small, else `size` distinct random rows (ascending)."""
    if n <= size:
        return None
    return np.sort(rng.choice(n, size=size, replace=False))


def train_ivf_centroids(x, params: IvfPqParams, engine=None, init=None):
    """build_ivf_model (rust/lance/src/index/vector/ivf.rs:1213-1272): sample num_partitions*sample_rate
    rows, normalise for cosine, drop non-finite rows, k-means with balance factor 1.0 (:1846-1871)."""
    eng = engine or default_engine()
    metric = _normalize_metric_type(params.metric)
    x = to_device(x)
    rng = np.random.default_rng(params.seed)
    idx = _sample_rows(x.shape[0], params.num_partitions * params.sample_rate, rng)
    sample = x if idx is None else x[torch.from_numpy(idx).to(x.device)]
    if metric == "cosine":
        sample = eng.normalize(sample)
    sample = sample[torch.isfinite(sample).all(dim=1)]
    kmetric = "l2" if metric == "cosine" else metric
    pool = _hier_engine_pool(eng) if (params.num_partitions > 256 and isinstance(sample, torch.Tensor) and sample.is_cuda) else None
    if pool and len(pool) > 1:
        # k > 256: the reference trains hierarchically (kmeans.rs:1027) -- thousands of small k-means, one after the other.  The splits the
        # reference is about to pop are computed side by side on several engine contexts of this GPU and applied in its order (the
        # multi-GPU trainer of lance_amd/dist.py on one rank): same centroids bit for bit, a fraction of the wall time.
        from . import dist as _ld
        f16 = sample.dtype == torch.float16
        cent = _ld.train_kmeans_hierarchical_sharded(eng, sample, params.num_partitions, max_iters=params.max_iters, balance_factor=1.0,
                                                     seed=params.seed, metric=kmetric, group=False, engines=pool)
        return (cent.to(torch.float16) if f16 else cent), 0.0, 0      # "Loss is not meaningful for hierarchical clustering" (kmeans.rs:1001)
    return eng.kmeans_train(sample, params.num_partitions, max_iters=params.max_iters, balance_factor=1.0, init=init,
                            seed=params.seed, metric=kmetric)


_HIER_POOLS = {}


def _hier_engine_pool(eng):
    """engine contexts (own HIP stream + scratch arena each) the hierarchical trainer's splits run on side by side; LANCE_HIP_HIER_CONTEXTS
    sets the count (default 8; 1 = the library's own sequential loop)"""
    import os
    want = int(os.environ.get("LANCE_HIP_HIER_CONTEXTS", "8"))
    if want <= 1 or not hasattr(eng, "device"):
        return None
    key = id(eng)
    if key not in _HIER_POOLS:
        from .engine import Engine
        _HIER_POOLS[key] = [eng] + [Engine(device=eng.device) for _ in range(want - 1)]
    return _HIER_POOLS[key]


def pq_sample_indices(n, params: IvfPqParams):
    """The rows the PQ codebook is trained on (maybe_sample_training_data, rust/lance/src/index/vector/utils.rs:173): a pure function of
    (n, params) -- create_index draws it on a host thread WHILE the IVF k-means runs on the device (2.7 ms of numpy at n = 1M that used to
    sit inside train_pq with the GPU idle)."""
    rng = np.random.default_rng(params.seed + 1)
    return _sample_rows(n, params.sample_rate * (1 << params.num_bits), rng)


_UNSET = object()


def train_pq_codebook(x, centroids, params: IvfPqParams, engine=None, sample_idx=_UNSET):
    """load_or_build_quantizer (rust/lance/src/index/vector/builder.rs:399-466): sample
    sample_rate * 2^nbits rows, normalise (cosine), drop non-finite, residual vs the IVF centroids
    (L2/cosine), then PQBuildParams::build (L2 k-means per sub-vector).  sample_idx: the result of pq_sample_indices when the
    caller already has it (None = all rows), or a concurrent.futures.Future of it."""
    eng = engine or default_engine()
    metric = _normalize_metric_type(params.metric)
    x = to_device(x)
    if sample_idx is _UNSET:
        idx = pq_sample_indices(x.shape[0], params)
    else:
        idx = sample_idx.result() if hasattr(sample_idx, "result") else sample_idx
    sample = x if idx is None else x[torch.from_numpy(idx).to(x.device)]
    if metric == "cosine":
        sample = eng.normalize(sample)
    sample = sample[torch.isfinite(sample).all(dim=1)]
    if metric in ("l2", "cosine"):
        part, _ = eng.assign(sample, centroids, "l2")
        sample = eng.residual(sample, centroids, part)
    return eng.pq_train(sample, params.num_sub_vectors, params.num_bits, params.max_iters, params.sample_rate, params.seed + 2)


def _transform_rows(eng, itype, metric, x, cent, codebook=None, bounds=None, timed=None):
    """The rows x through the IvfTransformer chain of an index kind with a GIVEN model -> (part ids, what the storage keeps: PQ codes,
    the rows as IVF_FLAT stores them, SQ codes).  One code path for create_index and for append (which brings the index's own model).
    timed(name, fn): create_index's clock."""
    if timed is None:
        timed = lambda name, fn: fn()
    if itype == "IVF_FLAT":
        if metric == "cosine":
            # IvfTransformer::new_flat (rust/lance-index/src/vector/ivf.rs:147-175): rows are normalised, assigned with L2 and
            # STORED normalised; the sub-index keeps the cosine distance function (ivf/v2.rs:405-411)
            if x.dtype not in (torch.float32, torch.float16):
                raise NotImplementedError("IVF_FLAT with the cosine metric needs float32 or float16 vectors (normalize_fsl accepts float arrays only)")
            xs = timed("normalize", lambda: eng.normalize(x))
            part, _ = timed("transform", lambda: eng.assign(xs, cent, "l2"))
        else:
            xs = x
            part, _ = timed("transform", lambda: eng.assign(x, cent, metric))
        return part, xs
    if itype == "IVF_SQ":
        # the transform chain of IVF_FLAT (normalise for cosine, assign in L2 / under dot) followed by SQTransformer
        def transform():
            xs = eng.normalize(x) if metric == "cosine" else x
            part, _ = eng.assign(xs, cent, "l2" if metric == "cosine" else metric)
            # KeepFiniteVectors runs ahead of the partition transform (ivf.rs new_ivf_transformer_with_quantizer): a row with a
            # NaN or an infinity has no partition under any metric
            part = torch.where(torch.isfinite(xs).all(dim=1), part, torch.full_like(part, -1))
            return part, eng.sq_encode(xs, bounds)
        return timed("transform", transform)
    part, codes, _ = timed("transform", lambda: eng.ivfpq_encode(x, cent, codebook, metric, want_loss=False))
    return part, codes


def create_index(x, index_type="IVF_PQ", metric="l2", num_partitions=256, num_sub_vectors=16, num_bits=None, max_iters=50,
                 sample_rate=256, ivf_centroids=None, pq_codebook=None, seed=42, keep_raw=True, engine=None, rq_rotation=None, _row_ids=None,
                 _sq_bounds=None):
    """Dataset.create_index(column, "IVF_PQ", ...) for a vector matrix resident (or copied) in HBM.
    num_bits: None = the index type's default (8 for IVF_PQ / IVF_SQ, 1 for IVF_RQ, as in the reference's build parameters).
    rq_rotation: IVF_RQ only (ignored otherwise) -- the [d][d] float32 rotation of the model; None: rq_rotation_matrix(d, seed).
    _row_ids: create_multivector_index's and VectorColumn.create_delta's -- the id stored with every row (several rows may share one);
    None: the row index.  With ids of their own the raw vectors are NOT attached (they are indexed by row id: the caller attaches the
    column) and the wrappers keep no per-row columns (prefiltered() refuses; nearest(prefilter=) needs none).
    _sq_bounds: IVF_SQ only, VectorColumn.create_delta's -- the quantiser's (start, end) of an earlier delta instead of training."""
    # ---- argument rules of Dataset.create_index (python/python/lance/dataset.py:2708-2960), checked before any device work
    if not isinstance(metric, str):
        raise ValueError(f"Metric {metric} not supported.")
    metric_n = _normalize_metric_type(metric)
    itype = str(index_type).upper()
    if itype not in ("IVF_PQ", "IVF_FLAT", "IVF_SQ", "IVF_RQ"):
        raise NotImplementedError(f"index_type {index_type}: IVF_PQ, IVF_FLAT, IVF_SQ and IVF_RQ are on this engine's hot path")
    if num_bits is None:
        num_bits = 1 if itype == "IVF_RQ" else 8
    if itype == "IVF_RQ":
        # RabitQuantizer (lance-index/src/vector/bq/builder.rs): one bit per dimension here, f32 columns, L2 and dot
        if num_bits != 1:
            raise ValueError(f"RabitQuantization: num_bits {num_bits} not supported (only 1 is)")
        if len(tuple(x.shape)) == 2 and (x.shape[1] % 8 != 0 or x.shape[1] == 0):
            raise ValueError(f"IVF_RQ: dimension {x.shape[1]} is not a multiple of 8 (one bit per dimension, packed into bytes)")
        if _dtype_name(x) not in ("float32", "float64"):
            raise NotImplementedError(f"IVF_RQ: unsupported data type: {_dtype_name(x)} (float32 columns are supported; float16 and int8 are not)")
        if metric_n == "cosine":
            raise NotImplementedError("IVF_RQ: metric cosine is not supported (which distance type the reference's loaded storage carries into "
                                      "q_factor is not established); use l2 or dot")
    if itype == "IVF_SQ":
        # ScalarQuantizer (lance-index/src/vector/sq.rs): 8 bits only (`// TODO: support SQ4`), float columns only
        if num_bits != 8:
            raise ValueError(f"ScalarQuantization: num_bits {num_bits} not supported (only 8 is)")
        if _dtype_name(x) not in ("float32", "float16"):
            raise NotImplementedError(f"SQ builder: unsupported data type: {_dtype_name(x)} (float16 and float32 columns are supported)")
    if isinstance(num_partitions, float):
        import warnings
        warnings.warn("num_partitions is float, converting to int")
        num_partitions = int(num_partitions)
    elif num_partitions is not None and not isinstance(num_partitions, (int, np.integer)):
        raise TypeError(f"num_partitions must be int, got {type(num_partitions)}")
    shape = tuple(x.shape)
    if len(shape) != 2:
        raise TypeError(f"Vector column must be a 2-D (rows, dimension) array, got shape {shape}")
    d = shape[1]
    if "PQ" in itype:
        if num_sub_vectors is None or num_partitions is None:
            raise ValueError("num_partitions and num_sub_vectors are required for IVF_PQ")
        if d % num_sub_vectors != 0:
            raise ValueError(f"dimension ({d}) must be divisible by num_sub_vectors ({num_sub_vectors})")
    if ivf_centroids is None and pq_codebook is not None:
        raise ValueError("ivf_centroids must be specified when pq_codebook is provided")
    as_np = lambda a: a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if ivf_centroids is not None:
        ivf_centroids = as_np(ivf_centroids)
        if ivf_centroids.ndim != 2 or ivf_centroids.shape[0] != num_partitions:
            raise ValueError(f"Ivf centroids must be 2D array: (clusters, dim), got {ivf_centroids.shape}")
        if ivf_centroids.dtype not in (np.float16, np.float32, np.float64):
            raise TypeError("IVF centroids must be floating number" + f"got {ivf_centroids.dtype}")
    if pq_codebook is not None:
        pq_codebook = as_np(pq_codebook)
        if pq_codebook.ndim != 3 or pq_codebook.shape[0] != num_sub_vectors or pq_codebook.shape[1] != (1 << num_bits):
            raise ValueError(f"PQ codebook must be 3D array: (sub_vectors, {1 << num_bits}, dim), got {pq_codebook.shape}")
        if pq_codebook.dtype not in (np.float16, np.float32, np.float64):
            raise TypeError("PQ codebook must be floating number" + f"got {pq_codebook.dtype}")
    eng = engine or default_engine()
    params = IvfPqParams(num_partitions, num_sub_vectors, num_bits, metric_n, max_iters, sample_rate, seed)
    x = to_device(x)
    n, d = x.shape
    if x.dtype == torch.int8 and params.metric == "cosine":
        raise NotImplementedError("int8 vectors with the cosine metric are not supported by this engine (use l2 or dot)")
    stats = BuildStats()

    def timed(name, fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        stats.seconds[name] = time.perf_counter() - t
        return out

    pq_idx = _UNSET
    pq_pool = None
    if itype == "IVF_PQ" and pq_codebook is None and ivf_centroids is None:
        # the PQ training sample depends on (n, params) only: drawn on a host thread while the IVF k-means occupies the device
        from concurrent.futures import ThreadPoolExecutor
        pq_pool = ThreadPoolExecutor(max_workers=1)
        pq_idx = pq_pool.submit(pq_sample_indices, n, params)
    if ivf_centroids is not None:
        cent = to_device(np.asarray(ivf_centroids, np.float32))
        if cent.shape != (num_partitions, d):
            raise ValueError(f"IVF centroids length mismatch: {tuple(cent.shape)} != {(num_partitions, d)}")
    else:
        try:
            cent, stats.ivf_loss, stats.ivf_iters = timed("train_ivf", lambda: train_ivf_centroids(x, params, eng))
        except BaseException:
            if pq_pool is not None:
                pq_pool.shutdown(wait=True)
            raise
    if itype == "IVF_FLAT":
        part, xs = _transform_rows(eng, itype, params.metric, x, cent, timed=timed)
        fx = timed("build_partitions", lambda: DeviceFlatIndex.create(eng, params.metric, cent, xs, part, _row_ids))
        out = IvfFlatIndex(fx, params, stats, part if _row_ids is None else None)
        out._x = xs if keep_raw and _row_ids is None else None     # the stored rows (borrowed): needed to re-partition under a prefilter
        out._rows_offered = n if _row_ids is None else None
        return out
    if itype == "IVF_RQ":
        rot = to_device(np.asarray(rq_rotation_matrix(d, seed) if rq_rotation is None else
                                   (rq_rotation.detach().cpu().numpy() if isinstance(rq_rotation, torch.Tensor) else rq_rotation), np.float32))
        if tuple(rot.shape) != (d, d):
            raise ValueError(f"rq_rotation must be [{d}][{d}], got shape {tuple(rot.shape)}")

        x = x.to(torch.float32)

        def transform():
            # KeepFiniteVectors, then PartitionTransformer::with_distance(true), then RQTransformer (ivf.rs:281-326)
            part, dvc = eng.assign(x, cent, params.metric)
            part = torch.where(torch.isfinite(x).all(dim=1), part, torch.full_like(part, -1))
            return part, dvc
        part, dvc = timed("transform", transform)
        codes, add, scale = timed("encode", lambda: eng.rq_encode(x, part, dvc, cent, rot, params.metric))
        rx = timed("build_partitions", lambda: DeviceRqIndex.create(eng, params.metric, cent, rot, codes, add, scale, part, row_ids=_row_ids))
        if keep_raw and _row_ids is None:
            rx.set_raw(x)
        out = IvfRqIndex(rx, params, stats, part if _row_ids is None else None)
        out._rows_offered = n if _row_ids is None else None
        return out
    if itype == "IVF_SQ":
        # the quantiser trains on its own sample of the column (train_sq_bounds)
        bounds = timed("train_sq", lambda: train_sq_bounds(x, params, eng)) if _sq_bounds is None else (float(_sq_bounds[0]), float(_sq_bounds[1]))
        part, codes = _transform_rows(eng, itype, params.metric, x, cent, bounds=bounds, timed=timed)
        sx = timed("build_partitions", lambda: DeviceSqIndex.create(eng, params.metric, cent.to(x.dtype), codes, part, bounds, _row_ids))
        if keep_raw and _row_ids is None:
            sx.set_raw(x)          # the ORIGINAL column (a cosine index encoded its normalised rows): refine scores against it
        out = IvfSqIndex(sx, params, stats, part if _row_ids is None else None, codes if keep_raw and _row_ids is None else None)
        out._rows_offered = n if _row_ids is None else None
        return out
    if num_bits not in (4, 8):
        raise ValueError(f"ProductQuantization: num_bits {num_bits} not supported")
    if pq_codebook is not None:
        cb = to_device(np.asarray(pq_codebook, np.float32).reshape(num_sub_vectors, 1 << num_bits, d // num_sub_vectors))
    else:
        try:
            cb, stats.pq_iters = timed("train_pq", lambda: train_pq_codebook(x, cent, params, eng, sample_idx=pq_idx))
        finally:
            if pq_pool is not None:
                pq_pool.shutdown(wait=True)
    part, codes = _transform_rows(eng, itype, params.metric, x, cent, codebook=cb, timed=timed)
    ix = timed("build_partitions", lambda: DeviceIndex.create(eng, params.metric, cent, cb, part, codes, _row_ids,
                                                              raw=x if keep_raw and _row_ids is None else None,
                                                              dtype="int8" if x.dtype == torch.int8 else None))
    # Index::prewarm (ivf/v2.rs:349-352): the search-side constants (matrix-core scan tables, the lossless u8 refine copy of an
    # integer-valued f32 column) are built here, inside the build's clock, instead of inside the first search
    timed("prewarm", ix.prewarm)
    out = IvfPqIndex(ix, params, stats, part, codes)
    out._rows_offered = n
    return out


class _MaskedIndexView:
    """`IvfPqIndex.prefiltered(allow)` of a 4-bit index: the same index, every search under the row-id mask (no copy)."""

    def __init__(self, index, allow):
        self._index, self._allow = index, allow
        self.params, self.stats = index.params, index.stats

    def nearest(self, q, k=10, nprobes=1, refine_factor=None, distance_range=None, **kw):
        return self._index.nearest(q, k=k, nprobes=nprobes, refine_factor=refine_factor, prefilter=self._allow, distance_range=distance_range, **kw)


def validate_vector_index(index, vectors, refine_factor=5, sample_size=None, pass_threshold=1.0, seed=0):
    """lance.util.validate_vector_index (python/python/lance/util.py:171-220): in-sample queries with k=1, nprobes=1 and
    a refine factor must come back at distance ~0 (|d| < 1e-6) for at least `pass_threshold` of the non-NaN vectors,
    else ValueError with the reference's message.  One batched device search instead of one query per row."""
    vecs = np.asarray(vectors.detach().cpu().numpy() if isinstance(vectors, torch.Tensor) else vectors)
    if sample_size is not None and sample_size < len(vecs):
        vecs = vecs[np.sort(np.random.default_rng(seed).choice(len(vecs), size=sample_size, replace=False))]
    ok = ~np.isnan(vecs.astype(np.float32)).any(axis=1)
    total = int(ok.sum())
    passes = 0
    if total:
        _, dist = index.nearest(vecs[ok], k=1, nprobes=1, refine_factor=refine_factor)
        passes = int((np.abs(dist[:, 0]) < 1e-6).sum())
    if total and passes / total < pass_threshold:
        raise ValueError(f"Vector index failed sanity check, only {passes}/{total} passed")
    return passes, total


def _flat_distance_range(distance_range):
    """distance_range of the flat scans -> {} or {"lower": .., "upper": ..}.  (None, None) is no range at all."""
    if distance_range is None:
        return {}
    lo, hi = distance_range
    if lo is None and hi is None:
        return {}
    return {"lower": lo, "upper": hi}


def flat_knn(x, q, k=10, metric="l2", engine=None, prefilter=None, distance_range=None):
    """Exhaustive KNN (`use_index=False`): (row ids, distances) sorted by (distance, row id).
    prefilter: boolean array over rows; the scan then covers the selected rows only, as the reference's filtered
    scan feeds KNNVectorDistanceExec (scanner.rs:3386-3411) -- row ids stay those of the full table.
    distance_range: (lower, upper), either may be None -- the k nearest rows with lower <= d < upper (Scanner::flat_knn's
    LanceFilterExec between the distance node and the sort, scanner.rs:3336-3412), d being the distance the un-ranged call returns,
    compared in the total order on f32 (NaN above +inf, the negative NaN of an L2 row with a NaN element below -inf, -0 below +0).
    A bound that is None is NOT TESTED: (lower, None) keeps +inf and NaN distances, (None, upper) keeps negative-NaN rows.  This
    differs from IvfFlatIndex.nearest, whose open ends are the largest finite f32 of either sign.  lower above upper is refused;
    lower == upper returns nothing; missing slots hold id -1 and distance +inf.  With a prefilter the selected rows are gathered
    and the ranged scan runs over them."""
    eng = engine or default_engine()
    rng = _flat_distance_range(distance_range)
    if prefilter is not None:
        xt = to_device(x)
        keep = torch.nonzero(to_device(np.ascontiguousarray(prefilter, dtype=bool)) if not isinstance(prefilter, torch.Tensor)
                             else prefilter.to(xt.device)).reshape(-1)
        return eng.flat_topk(xt[keep].contiguous(), q, k, _normalize_metric_type(metric), row_ids=keep, **rng)
    ids, dists = eng.flat_topk(x, q, k, _normalize_metric_type(metric), **rng)
    return ids, dists


def multivector_distance(values, offsets, q, metric="cosine", engine=None):
    """Distances of ONE multivector query q [nqv][d] to every row of a multivector column (Arrow List<FixedSizeList<T, d>>:
    values [total vectors][d] float32 / float16, offsets [n_rows + 1]; arrow_io.multivector_from_arrow gives both) -> [n_rows].
    distance = 1 - sum_i max_j (1 - dist(q_i, v_j)), multivec_distance (lance-linalg distance.rs:107-206)."""
    check_multivector(values, offsets, q, metric)
    return (engine or default_engine()).multivec_distance(values, offsets, q, metric)


def multivector_flat_knn(values, offsets, q, k=10, metric="cosine", engine=None, prefilter=None, row_ids=None, distance_range=None):
    """Exhaustive KNN of one multivector query over a multivector column: (row ids [k], distances [k]) sorted by (distance, row id)
    (the flat scan of a List column, lance-index flat.rs:129-133).  prefilter: boolean array over rows, as in flat_knn -- the scan
    covers the selected rows, the ids stay those of the full table (row_ids, or the row index).
    distance_range: (lower, upper) on the rows' multivector distances, with flat_knn's semantics (a None bound is not tested).
    q may be a list or tuple of B queries [nqv_b][d] (a batch, Engine.multivec_topk_batch): -> ([B][k], [B][k]), row b the answer of
    the single call for query b; a prefilter's sub-column is gathered once for the whole batch."""
    rng = _flat_distance_range(distance_range)
    batch = isinstance(q, (list, tuple))
    if batch:
        if len(q) < 1:
            raise ValueError("q holds no query: a batch has at least one")
        for qb in q:
            if len(getattr(qb, "shape", ())) != 2:
                raise ValueError(f"every query of a batch must be [nqv][d], got shape {tuple(getattr(qb, 'shape', ()))}")
            _, off = check_multivector(values, offsets, qb, metric, k)
        q_offsets = np.concatenate([[0], np.cumsum([int(qb.shape[0]) for qb in q])]).astype(np.int64)
        if all(isinstance(qb, torch.Tensor) for qb in q):
            q = torch.cat([qb.reshape(qb.shape[0], -1) for qb in q], 0)
        else:
            q = np.concatenate([qb.detach().cpu().numpy() if isinstance(qb, torch.Tensor) else np.asarray(qb) for qb in q], 0)
    else:
        _, off = check_multivector(values, offsets, q, metric, k)

    def topk(eng, v, o, rid):
        if batch:
            return eng.multivec_topk_batch(v, o, q, q_offsets, k, metric, row_ids=rid, **rng)
        return eng.multivec_topk(v, o, q, k, metric, row_ids=rid, **rng)

    n = off.size - 1
    mask = None
    if prefilter is not None:
        mask = prefilter.detach().cpu().numpy() if isinstance(prefilter, torch.Tensor) else np.asarray(prefilter)
        if mask.dtype != np.bool_ or mask.shape != (n,):
            raise ValueError(f"prefilter must be a boolean array over the {n} rows, got {mask.dtype} {mask.shape}")
    if row_ids is not None and int(row_ids.shape[0]) != n:
        raise ValueError(f"row_ids must hold one id per row ({n}), got {int(row_ids.shape[0])}")
    eng = engine or default_engine()
    if mask is None:
        return topk(eng, values, offsets, row_ids)
    # the selected rows' vectors, gathered on the device (plumbing): the scan sees a column of its own
    vt = values.to(to_device(off).device) if isinstance(values, torch.Tensor) else to_device(values)
    od = to_device(off)
    keep = torch.nonzero(to_device(mask)).reshape(-1)
    lens = (od[1:] - od[:-1])[keep]
    sub_off = torch.zeros(keep.numel() + 1, dtype=torch.int64, device=od.device)
    sub_off[1:] = torch.cumsum(lens, 0)
    total = int(sub_off[-1])
    src = torch.repeat_interleave(od[:-1][keep] - sub_off[:-1], lens) + torch.arange(total, device=od.device)
    rid = keep if row_ids is None else to_device(row_ids, torch.int64)[keep]
    return topk(eng, vt[src].contiguous(), sub_off.cpu().numpy(), rid)


class IvfPqMultivectorIndex:
    """An IVF_PQ index over the FLATTENED vectors of a multivector column (Arrow List<FixedSizeList<T, d>>), the row's id repeated once
    per vector (the reference's Flatten transformer, lance-index/src/vector/transform.rs:203-216), searched as the reference's second
    multivector path does (Scanner::multivec_ann, scanner.rs:3471-3552): one ANN search per query vector with k * overfetch candidates,
    the lists joined by row id and scored with XTR-style imputation (MultivectorScoringExec, knn.rs:1132-1329) on the device."""
    _index_type = "IVF_PQ"

    def __init__(self, dev_index, params, stats, values, offsets):
        self._ix = dev_index
        self.params = params
        self.stats = stats
        self._values = values          # the column, kept by reference (None: built with keep_raw=False) -- the re-rank reads it
        self._offsets = offsets        # int64 [n_rows + 1] on the device
        self.n_rows = int(offsets.numel()) - 1

    @property
    def centroids(self):
        return self._ix.centroids.cpu().numpy()

    @property
    def codebook(self):
        return self._ix.codebook.cpu().numpy()

    def info(self):
        return self._ix.info()

    def _queries(self, q):
        """one [nqv][d] array or a list of them -> (all vectors [sum nqv][d] on the device, q_offsets, the queries, batched?)"""
        d = self._ix.centroids.shape[1]
        batched = isinstance(q, (list, tuple))
        qs = list(q) if batched else [q]
        if not qs:
            raise ValueError("q holds no query")
        ts = []
        for one in qs:
            t = one if isinstance(one, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(one))
            if t.dim() != 2 or int(t.shape[1]) != d:
                raise ValueError(f"a multivector query must be [nqv][d] with d = {d}, the dimension of the column, got shape {tuple(t.shape)}")
            if int(t.shape[0]) < 1:
                raise ValueError("q holds no vector: a multivector query has at least one")
            if int(t.shape[0]) > MULTIVEC_MAX_QUERY_VECTORS:
                raise ValueError(f"q holds {int(t.shape[0])} vectors, above the limit of {MULTIVEC_MAX_QUERY_VECTORS} query vectors per query")
            ts.append(to_device(t, self._ix.data_dtype))
        off = np.zeros(len(ts) + 1, np.int64)
        off[1:] = np.cumsum([int(t.shape[0]) for t in ts])
        return torch.cat(ts, 0).contiguous(), off, ts, batched

    def _rerank(self, q, cand, k):
        """the exact multivector distance (the flat scan's kernel) of the candidate rows to the ORIGINAL query -> the best k"""
        eng = self._ix.engine
        cand = cand[cand >= 0]
        if cand.numel() == 0:
            dev = cand.device
            return torch.full((k,), -1, dtype=torch.int64, device=dev), torch.full((k,), float("inf"), dtype=torch.float32, device=dev)
        od = self._offsets
        lens = od[cand + 1] - od[cand]
        sub_off = torch.zeros(cand.numel() + 1, dtype=torch.int64, device=od.device)
        sub_off[1:] = torch.cumsum(lens, 0)
        total = int(sub_off[-1])
        src = torch.repeat_interleave(od[cand] - sub_off[:-1], lens) + torch.arange(total, device=od.device)
        return eng.multivec_topk(self._values[src].contiguous(), sub_off.cpu().numpy(), q, k, "cosine", row_ids=cand)

    def nearest(self, q, k=10, nprobes=1, refine_factor=None, prefilter=None, overfetch=10, distance_range=None, minimum_nprobes=None,
                maximum_nprobes=None):
        """q: one multivector query [nqv][d], or a list of them (a batch).  -> (row ids uint64 [k] (2^64 - 1 = missing), distances
        f32 [k]) as numpy, [B][k] for a batch, sorted by (distance, row id).
        overfetch: candidates per query vector = k * overfetch (the reference's LANCE_XTR_OVERFETCH, default 10).
        refine_factor: None -- the k best by the imputed score; n >= 1 -- the k * n best by that score are scored exactly
        (multivector_flat_knn's distance, the original query) and the best k returned (scanner.rs:2884-2904).
        prefilter: boolean array over the rows (True = the row may be returned), tested inside the scan kernels."""
        for name, val in (("distance_range", distance_range), ("minimum_nprobes", minimum_nprobes), ("maximum_nprobes", maximum_nprobes)):
            if val is not None:
                raise NotImplementedError(f"multivector index: {name} is not supported")
        k, overfetch = int(k), int(overfetch)
        if k < 1 or overfetch < 1:
            raise ValueError(f"k={k}, overfetch={overfetch}: both must be at least 1")
        if refine_factor is not None and int(refine_factor) < 1:
            raise ValueError("Refine factor cannot be zero")
        rf = 1 if refine_factor is None else int(refine_factor)
        check_multivector_ann_sizes(k * overfetch, k * rf)
        if refine_factor is not None and self._values is None:
            raise NotImplementedError("multivector index: refine_factor needs the column (re-ranking scores the candidate rows exactly): "
                                      "build with create_multivector_index(..., keep_raw=True)")
        if prefilter is not None:
            shape = tuple(prefilter.shape)
            if shape != (self.n_rows,) or str(prefilter.dtype).replace("torch.", "") != "bool":
                raise ValueError(f"prefilter must be a boolean array over the {self.n_rows} rows, got {prefilter.dtype} {shape}")
        qv, off, qs, batched = self._queries(q)
        ids, dists = self._ix.multivec_search(qv, off, k, nprobes, overfetch=overfetch, k_out=k * rf, allow=prefilter)
        if refine_factor is not None:
            out = [self._rerank(qs[b], ids[b], k) for b in range(len(qs))]
            ids, dists = torch.stack([o[0] for o in out]), torch.stack([o[1] for o in out])
        ids, dists = ids.cpu().numpy().view(np.uint64), dists.cpu().numpy()
        return (ids, dists) if batched else (ids[0], dists[0])

    def close(self):
        self._ix.close()


def create_multivector_index(values, offsets, metric="cosine", num_partitions=256, num_sub_vectors=16, num_bits=8, max_iters=50,
                             sample_rate=256, ivf_centroids=None, pq_codebook=None, seed=42, keep_raw=True, engine=None):
    """Dataset.create_index on a multivector column (values [total vectors][d] float32 / float16, offsets [n_rows + 1];
    arrow_io.multivector_from_arrow gives both): IVF_PQ over the flattened vectors through exactly the calls create_index makes, with
    row_ids = the row index repeated once per vector.  Rows without vectors are allowed (they can never be found).  Only the cosine
    metric, as in the reference (lance/src/index/vector.rs:328).  keep_raw: keep the column (by reference) for nearest(refine_factor=)."""
    if not isinstance(metric, str):
        raise ValueError(f"Metric {metric} not supported.")
    if _normalize_metric_type(metric) != "cosine":
        raise ValueError("multivector type supports only cosine distance")
    name = _dtype_name(values)
    if name not in ("float32", "float16"):
        raise ValueError(f"unsupported multivector element type {name}: the column must be float32 or float16")
    if len(values.shape) != 2 or int(values.shape[1]) < 1:
        raise ValueError(f"values must be the flattened [total vectors][d] child array, got shape {tuple(values.shape)}")
    if offsets is None:
        raise ValueError("the multivector column holds null rows: not supported")
    off = offsets.detach().cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets)
    if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu":
        raise ValueError("offsets must be a 1-D integer array of n_rows + 1 entries")
    off = np.ascontiguousarray(off.astype(np.int64))
    if off[0] != 0 or (np.diff(off) < 0).any() or off[-1] != int(values.shape[0]):
        raise ValueError(f"offsets must start at 0, never decrease and end at len(values) = {int(values.shape[0])}")
    # the argument rules, the training and the transform are create_index's own; only the storage differs (repeated row ids, no raw matrix)
    flat = create_index(values, "IVF_PQ", metric="cosine", num_partitions=num_partitions, num_sub_vectors=num_sub_vectors, num_bits=num_bits,
                        max_iters=max_iters, sample_rate=sample_rate, ivf_centroids=ivf_centroids, pq_codebook=pq_codebook, seed=seed,
                        keep_raw=False, engine=engine, _row_ids=np.repeat(np.arange(off.size - 1, dtype=np.int64), np.diff(off)))
    vt = None
    if keep_raw:
        vt = values.to(flat._ix.centroids.device) if isinstance(values, torch.Tensor) else to_device(values)
    out = IvfPqMultivectorIndex(flat._ix, flat.params, flat.stats, vt, to_device(off))
    return out


# ---- a column whose index is behind its rows: deltas + unindexed fragments ----------------------------------------------
TAKE_FLAT_KNN_MAX_CANDIDATES = 4096      # lance_hip_take_flat_knn: ca + cb


def _index_type_of(index):
    for cls, name in ((IvfPqIndex, "IVF_PQ"), (IvfFlatIndex, "IVF_FLAT"), (IvfSqIndex, "IVF_SQ"), (IvfRqIndex, "IVF_RQ")):
        if isinstance(index, cls):
            return name
    if isinstance(index, IvfPqMultivectorIndex):
        raise NotImplementedError("VectorColumn: multivector columns and their indices are not supported")
    raise TypeError(f"VectorColumn: {type(index).__name__} is not an index of this package")


class VectorColumn:
    """A vector column as a Lance dataset holds it after appends: the rows x [N][d] resident in HBM, split into fragments (consecutive
    row blocks), zero or more DELTA indices built with one model, each covering a set of fragments (IndexMetadata.fragment_bitmap), and
    whatever fragments no index covers yet.  The row id is the row index.  `nearest` is the reference's plan for such a column
    (Scanner::nearest, scanner.rs:2847-3030, 3336-3468); every method that changes the column returns a NEW column and leaves this one
    as it is.  x: numpy (copied to HBM once) or a torch tensor (kept by reference).  Multivector columns are refused."""

    def __init__(self, x, fragment_sizes=None, engine=None):
        if isinstance(x, (list, tuple)) or len(getattr(x, "shape", ())) != 2:
            raise NotImplementedError("VectorColumn: multivector columns are not supported (a [N][d] matrix is required); "
                                      "see create_multivector_index")
        self._engine = engine
        self._x = x if isinstance(x, torch.Tensor) else to_device(x)
        n = int(self._x.shape[0])
        sizes = [n] if fragment_sizes is None else [int(s) for s in fragment_sizes]
        if any(s < 0 for s in sizes) or sum(sizes) != n:
            raise ValueError(f"VectorColumn: fragment_sizes must be non-negative and sum to the {n} rows, got {sizes}")
        self._offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        self._deltas = ()          # ((index, frozenset of fragment ids), ...) in the order they were added

    # ---- what the column is made of ----
    @property
    def num_fragments(self):
        return int(self._offsets.size) - 1

    @property
    def deltas(self):
        """the delta indices, oldest first"""
        return [ix for ix, _ in self._deltas]

    def indexed_fragments(self):
        out = set()
        for _, frags in self._deltas:
            out |= frags
        return out

    def unindexed_fragments(self):
        covered = self.indexed_fragments()
        return [f for f in range(self.num_fragments) if f not in covered]

    def _runs(self, fragments):
        """contiguous runs of the given fragment ids -> [(first row, end row)], empty runs dropped"""
        runs, frags = [], sorted(fragments)
        i = 0
        while i < len(frags):
            j = i
            while j + 1 < len(frags) and frags[j + 1] == frags[j] + 1:
                j += 1
            r0, r1 = int(self._offsets[frags[i]]), int(self._offsets[frags[j] + 1])
            if r1 > r0:
                runs.append((r0, r1))
            i = j + 1
        return runs

    def _engine_or_default(self):
        return self._engine or default_engine()

    def _copy(self, deltas):
        out = VectorColumn.__new__(VectorColumn)
        out._engine, out._x, out._offsets, out._deltas = self._engine, self._x, self._offsets, tuple(deltas)
        return out

    def _check_fragments(self, fragments, what):
        frags = frozenset(int(f) for f in fragments)
        bad = sorted(f for f in frags if not 0 <= f < self.num_fragments)
        if bad:
            raise ValueError(f"{what}: fragments {bad} do not exist (the column has {self.num_fragments})")
        return frags

    # ---- maintenance ----
    def with_index(self, index, fragments):
        """The column with `index` as one more delta over the given fragment ids.  The index must store the column's row ids (the row
        index).  Refused: fragments another delta covers; a metric, element type, index type or dimension other than the first delta's."""
        itype = _index_type_of(index)
        frags = self._check_fragments(fragments, "with_index")
        both = sorted(frags & self.indexed_fragments())
        if both:
            raise ValueError(f"with_index: fragments {both} are covered by another delta (fragment bitmaps of deltas do not overlap)")
        d = int(index._ix.centroids.shape[1])
        if d != int(self._x.shape[1]):
            raise ValueError(f"with_index: the index has dimension {d}, the column {int(self._x.shape[1])}")
        if self._deltas:
            first = self._deltas[0][0]
            mine = (itype, _normalize_metric_type(index.params.metric), index._ix.data_dtype, d)
            theirs = (_index_type_of(first), _normalize_metric_type(first.params.metric), first._ix.data_dtype, int(first._ix.centroids.shape[1]))
            for name, a, b in zip(("index type", "metric", "element type", "dimension"), mine, theirs):
                if a != b:
                    raise ValueError(f"with_index: {name} {a} differs from the first delta's {b} (the deltas of a column share one model)")
        return self._copy(self._deltas + ((index, frags),))

    def _rows_of(self, fragments):
        runs = self._runs(fragments)
        if not runs:
            return None
        dev = self._x.device
        return torch.cat([torch.arange(r0, r1, dtype=torch.int64, device=dev) for r0, r1 in runs])

    def create_delta(self, fragments=None, **create_index_args):
        """The column with a new delta over the rows of `fragments` (default: every unindexed fragment), storing the column's row ids.
        With a delta already there its model is used -- centroids, and codebook / quantiser bounds / rotation: an index type, metric or
        size in create_index_args that differs from that delta's, or a model of the caller's, is refused -- otherwise create_index
        trains one from those rows with create_index_args.  keep_raw is not the caller's to give: the column itself is attached."""
        for name in ("keep_raw", "_row_ids", "_sq_bounds"):
            if name in create_index_args:
                raise ValueError(f"create_delta: {name} is set by the column (its row ids are stored and the column is attached)")
        frags = self._check_fragments(self.unindexed_fragments() if fragments is None else fragments, "create_delta")
        both = sorted(frags & self.indexed_fragments())
        if both:
            raise ValueError(f"create_delta: fragments {both} are covered by another delta")
        rows = self._rows_of(frags)
        if rows is None:
            raise ValueError("create_delta: no rows to index (no unindexed fragment holds a row)")
        args = dict(create_index_args)
        if self._deltas:
            first = self._deltas[0][0]
            itype, p = _index_type_of(first), first.params
            theirs = {"index_type": itype, "metric": _normalize_metric_type(p.metric), "num_partitions": int(first._ix.centroids.shape[0])}
            if itype == "IVF_PQ":
                theirs.update(num_sub_vectors=p.num_sub_vectors, num_bits=p.num_bits)
            for name, want in theirs.items():
                got = args.get(name)
                if name == "index_type" and got is not None:
                    got = str(got).upper()
                elif name == "metric" and got is not None:
                    got = _normalize_metric_type(got)
                if got is not None and got != want:
                    raise ValueError(f"create_delta: {name}={args[name]} differs from the first delta's {want} (the deltas of a column share one model)")
            for name in ("ivf_centroids", "pq_codebook", "rq_rotation"):
                if args.get(name) is not None:
                    raise ValueError(f"create_delta: {name} was given, but the column has a delta: its model is used")
            args.update(index_type=itype, metric=p.metric, num_partitions=int(first._ix.centroids.shape[0]), ivf_centroids=first.centroids)
            if itype == "IVF_PQ":
                args.update(num_sub_vectors=p.num_sub_vectors, num_bits=p.num_bits, pq_codebook=first.codebook)
            elif itype == "IVF_SQ":
                args.update(_sq_bounds=first.bounds)
            elif itype == "IVF_RQ":
                args.update(rq_rotation=first.rotation)
        args.setdefault("engine", self._engine)
        index = create_index(self._x[rows], _row_ids=rows, keep_raw=False, **args)
        if hasattr(index._ix, "set_raw"):
            index._ix.set_raw(self._x)         # indexed by row id: index.nearest(refine_factor=) of the delta alone works too
        return self.with_index(index, frags)

    def optimize(self):
        """The column with its unindexed fragments folded into the LAST delta by that index's `append` (its model, nothing re-trained).
        IVF_RQ has no append: it refuses with its own message -- use create_delta there."""
        tail = self.unindexed_fragments()
        if not self._deltas:
            raise ValueError("optimize: the column has no index to fold rows into (create_delta builds one)")
        last, frags = self._deltas[-1]
        rows = self._rows_of(tail)
        if rows is None:
            return self._copy(self._deltas[:-1] + ((last, frags | frozenset(tail)),))
        kw = {"raw": self._x} if isinstance(last, IvfPqIndex) else {}
        grown = last.append(self._x[rows], row_ids=rows, **kw)
        return self._copy(self._deltas[:-1] + ((grown, frags | frozenset(tail)),))

    # ---- the search plan ----
    def _ann(self, index, itype, q, keff, nprobes, prefilter, rng):
        """one delta's own search for keff rows, un-refined -> (ids int64, distances) on the device"""
        ix = index._ix
        if itype == "IVF_PQ":
            if rng:
                return ix.search_range(q, keff, nprobes, rng.get("lower"), rng.get("upper"), refine_factor=0, allow=prefilter)
            return ix.search(q, keff, nprobes, 0) if prefilter is None else ix.search_filtered(q, keff, nprobes, prefilter, 0)
        if itype == "IVF_FLAT":
            if rng:
                return ix.search(q, keff, nprobes, allow=prefilter, lower=rng.get("lower"), upper=rng.get("upper"))
            return ix.search(q, keff, nprobes) if prefilter is None else ix.search(q, keff, nprobes, allow=prefilter)
        return ix.search(q, keff, nprobes) if prefilter is None else ix.search(q, keff, nprobes, allow=prefilter)

    def _refines_on_this_column(self, index, itype):
        """True when the delta re-ranks inside its own search AND on this very column (the tensor attached to it is the column's storage):
        steps 2 and 3 of a single un-ranged delta are then that one search -- the same ids and distance bits as the search for keff
        rows followed by take_flat_knn (tests/test_zz_gpu_knn_combined.py compares the two), without the second kernel's pass"""
        raw = getattr(index._ix, "_raw", None)
        return (itype != "IVF_FLAT" and isinstance(raw, torch.Tensor) and raw.data_ptr() == self._x.data_ptr()
                and raw.dtype == self._x.dtype and tuple(raw.shape) == tuple(self._x.shape))

    def _ann_refined(self, index, itype, q, k, nprobes, prefilter, refine_factor):
        """the delta's own search with its refine: k rows by the exact distance out of k * refine_factor by the index's"""
        ix = index._ix
        if itype == "IVF_PQ":
            return ix.search(q, k, nprobes, refine_factor) if prefilter is None else ix.search_filtered(q, k, nprobes, prefilter, refine_factor)
        return ix.search(q, k, nprobes, allow=prefilter, refine_factor=refine_factor)

    def _tail_lists(self, eng, q, k, metric, prefilter, rng):
        """flat_knn(k) over every contiguous run of unindexed fragments, with the rows' ids, the prefilter and the bounds"""
        dev = self._x.device
        allow = None
        if prefilter is not None:
            allow = prefilter if isinstance(prefilter, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(prefilter, dtype=bool))
            allow = allow.to(dev)
        lists = []
        for r0, r1 in self._runs(self.unindexed_fragments()):
            rid = torch.arange(r0, r1, dtype=torch.int64, device=dev)
            if allow is not None:
                inside = rid[rid < allow.numel()]
                rid = inside[allow[inside]]
                if rid.numel() == 0:
                    continue
                xs = self._x[rid].contiguous()
            else:
                xs = self._x[r0:r1]
            lists.append(eng.flat_topk(xs, q, k, metric, row_ids=rid, **rng))
        return lists

    def _combine(self, eng, q, ids_a, lists, k, metric, rng):
        """take_flat_knn of list A with the tail lists, several per call up to the candidate limit, chained beyond it: the k best of
        (the k best of a part of the candidates) and the rest are the k best of all of them"""
        pend = []
        for bi, bd in lists:
            if pend and ids_a.shape[1] + sum(int(i.shape[1]) for i, _ in pend) + int(bi.shape[1]) > TAKE_FLAT_KNN_MAX_CANDIDATES:
                ids_a, _ = eng.take_flat_knn(self._x, q, ids_a, k, metric, ids_b=torch.cat([i for i, _ in pend], 1),
                                             dists_b=torch.cat([d for _, d in pend], 1), **rng)
                pend = []
            pend.append((bi, bd))
        if not pend:
            return eng.take_flat_knn(self._x, q, ids_a, k, metric, **rng)
        return eng.take_flat_knn(self._x, q, ids_a, k, metric, ids_b=torch.cat([i for i, _ in pend], 1),
                                 dists_b=torch.cat([d for _, d in pend], 1), **rng)

    def nearest(self, q, k=10, nprobes=1, refine_factor=None, prefilter=None, distance_range=None, fast_search=False, use_index=True,
                metric=None, minimum_nprobes=None, maximum_nprobes=None):
        """-> (row ids int64 [nq][k] (-1 = missing), distances f32 [nq][k]) as numpy: Scanner::nearest over the whole column.
        1. use_index=False, or no delta: flat_knn over the column with the prefilter and the range (scanner.rs:2912-2942).
        2. ANN over every delta for keff = k * (refine_factor or 1) rows -- each delta's own search takes the prefilter and, where the
           index type answers ranges (IVF_PQ, IVF_FLAT), the bounds, tested on the INDEX's distances inside the partitions --, the
           lists joined by (distance, row id) and cut to keff (lance_hip_merge_topk; one delta needs no merge).
        3. With a refine_factor: take_flat_knn over those keff ids, the bounds on the EXACT distances, fetch k.  (A single un-ranged
           IVF_PQ / IVF_SQ / IVF_RQ delta that has this very column attached for its own refine answers steps 2 and 3 in one search of
           its own: the same ids and distance bits, without the second pass.)
        4. fast_search=True, or no unindexed fragment: done.
        5. Otherwise flat_knn(k) over the unindexed fragments (their rows' ids, the prefilter, the bounds) and take_flat_knn of the
           list so far with that tail list: every distance exact, the bounds on them, the k best by (distance, row id); a row id in
           both lists comes back twice (the reference's UnionExec does not de-duplicate).
        So an un-refined ANN list comes back with EXACT distances when, and only when, the column holds unindexed rows: that is what
        the reference's knn_combined does.  With one delta, no unindexed rows and no range the answer is `index.nearest(...)`'s, bit
        for bit, with and without refine_factor.  With a range AND a refine_factor it differs from IvfPqIndex.nearest by design: the
        column filters the exact distances, as the scanner does; lance_hip_ivfpq_search_range does not.
        metric: of the flat scan when the column has no delta (default l2); with deltas it is theirs.
        Limits of the plan (the library refuses beyond them, with its own message): k <= 1024; keff = k * refine_factor <= 4096
        (take_flat_knn's candidates) and, with several deltas, deltas * keff <= 4096 (merge_topk's); each delta's own search is asked
        for keff rows and has its index type's limit on that -- these are not the limits of index.nearest, which re-ranks inside.
        Refused: minimum_nprobes / maximum_nprobes (how the reference's late search interacts across deltas is not established here);
        distance_range on IVF_SQ / IVF_RQ deltas (those indices' own message); refine_factor=0."""
        for name, val in (("minimum_nprobes", minimum_nprobes), ("maximum_nprobes", maximum_nprobes)):
            if val is not None:
                raise NotImplementedError(f"VectorColumn.nearest: {name} is not supported (adaptive probing across delta indices)")
        if refine_factor is not None and int(refine_factor) < 1:
            raise ValueError("Refine factor can not be zero")
        rng = _flat_distance_range(distance_range)
        k = int(k)
        searched = use_index and bool(self._deltas)
        if self._deltas:
            first = self._deltas[0][0]
            itype = _index_type_of(first)
            if metric is not None and _normalize_metric_type(metric) != _normalize_metric_type(first.params.metric):
                raise ValueError(f"VectorColumn.nearest: metric {metric} is not the deltas' ({first.params.metric})")
            metric = _normalize_metric_type(first.params.metric)
            if searched and rng and itype in ("IVF_SQ", "IVF_RQ"):
                raise NotImplementedError(f"{itype}: distance_range is not supported by this engine")
        else:
            metric = _normalize_metric_type("l2" if metric is None else metric)
        eng = self._engine_or_default()
        if not searched:
            ids, dists = flat_knn(self._x, q, k, metric, engine=eng, prefilter=prefilter, distance_range=distance_range)
            return ids.cpu().numpy(), dists.cpu().numpy()
        keff = k * (1 if refine_factor is None else int(refine_factor))
        tail = (not fast_search) and bool(self._runs(self.unindexed_fragments()))
        if refine_factor is not None and len(self._deltas) == 1 and not rng and self._refines_on_this_column(first, itype):
            # steps 2 and 3 in the delta's own pipeline: the same answer bit for bit, one pass less (measurement (a))
            ids, dists = self._ann_refined(first, itype, q, k, nprobes, prefilter, int(refine_factor))
        else:
            found = [self._ann(ix, itype, q, keff, nprobes, prefilter, rng) for ix, _ in self._deltas]
            if len(found) == 1:
                ids, dists = found[0]
            else:
                ids, dists = eng.merge_topk(torch.cat([i for i, _ in found], 1), torch.cat([d for _, d in found], 1), keff)
            if refine_factor is not None:
                ids, dists = eng.take_flat_knn(self._x, q, ids, k, metric, **rng)
        if tail:
            ids, dists = self._combine(eng, q, ids, self._tail_lists(eng, q, k, metric, prefilter, rng), k, metric, rng)
        return ids.cpu().numpy(), dists.cpu().numpy()
