"""Thin Python host layer over the C ABI: device memory and streams come from torch
(plumbing), every computation is a call into liblance_hip.so.
"""
import ctypes as C
import functools
import os

import numpy as np
import torch

from . import _lib
from ._lib import METRICS, check


def _dev():
    if not torch.cuda.is_available():
        raise RuntimeError("lance_amd needs an MI355X: no HIP device is visible and there is no CPU fallback")
    return torch.device("cuda", torch.cuda.current_device())


def to_device(a, dtype=None):
    """numpy / torch (cpu or cuda) -> contiguous cuda tensor"""
    if isinstance(a, torch.Tensor):
        t = a
    else:
        arr = np.ascontiguousarray(a)
        if arr.dtype == np.uint64:  # torch has limited uint64 support: move the bits
            t = torch.from_numpy(arr.view(np.int64))
        elif arr.dtype == np.uint32:
            t = torch.from_numpy(arr.view(np.int32))
        else:
            t = torch.from_numpy(arr)
    if dtype is not None and t.dtype != dtype:
        t = t.to(dtype)
    return t.to(_dev()).contiguous()


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _vec(a):
    """vector data -> (cuda tensor in its own element type, dtype code); float16 stays float16"""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dtype == torch.float16:
        return t.to(_dev()).contiguous(), _lib.F16
    if t.dtype == torch.int8:      # Int8 columns: data stays int8, the model (centroids, codebook) is float32
        return t.to(_dev()).contiguous(), _lib.I8
    return t.to(torch.float32).to(_dev()).contiguous(), _lib.F32


def _nbits(codebook):
    """num_bits from the codebook shape (M, 2^nbits, d/M)"""
    kc = int(codebook.shape[1])
    if kc not in (16, 256):
        raise ValueError(f"codebook must have 16 or 256 centroids per sub-vector, got {kc}")
    return 4 if kc == 16 else 8


def _like(a, ref):
    """data arrays (queries, raw vectors) are cast to the element type of the vectors"""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(ref.dtype).to(_dev()).contiguous()


def _model(a, ref):
    """model arrays (centroids, codebook) take the element type of the vectors, float32 for int8 vectors"""
    t = a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))
    return t.to(torch.float32 if ref.dtype == torch.int8 else ref.dtype).to(_dev()).contiguous()


def _dtype_name(a):
    return str(a.dtype).replace("torch.", "") if isinstance(a, torch.Tensor) else np.asarray(a).dtype.name


def check_multivector(values, offsets, q, metric, k=None):
    """Host-side validation of a multivector column (values [N][d], offsets [n_rows + 1]) and a multivector query q [nqv][d]; every
    problem is a ValueError raised before any device call.  -> (metric name, offsets as a contiguous int64 numpy array)"""
    m = str(metric).lower()
    if m == "euclidean":
        m = "l2"
    if m == "hamming":
        raise ValueError("metric hamming is not supported for multivector columns (uint8 / hamming columns are not in this library)")
    if m not in ("l2", "cosine", "dot"):
        raise ValueError(f"metric {metric} is not supported for multivector columns: l2, dot or cosine")
    name = _dtype_name(values)
    if name not in ("float32", "float16"):
        raise ValueError(f"unsupported multivector element type {name}: the column must be float32 or float16 "
                         "(int8 / uint8 columns have no arm in the reference's float path)")
    if len(values.shape) != 2 or int(values.shape[1]) < 1:
        raise ValueError(f"values must be the flattened [total vectors][d] child array, got shape {tuple(values.shape)}")
    d = int(values.shape[1])
    if len(q.shape) != 2 or int(q.shape[1]) != d:
        raise ValueError(f"q must be [nqv][d] with d = {d}, the dimension of the column, got shape {tuple(q.shape)}")
    nqv = int(q.shape[0])
    if nqv < 1:
        raise ValueError("q holds no vector: a multivector query has at least one")
    if nqv > _lib.MULTIVEC_MAX_QUERY_VECTORS:
        raise ValueError(f"q holds {nqv} vectors, above the limit of {_lib.MULTIVEC_MAX_QUERY_VECTORS} query vectors per call")
    off = offsets.detach().cpu().numpy() if isinstance(offsets, torch.Tensor) else np.asarray(offsets)
    if off.ndim != 1 or off.size < 1 or off.dtype.kind not in "iu":
        raise ValueError("offsets must be a 1-D integer array of n_rows + 1 entries")
    off = np.ascontiguousarray(off.astype(np.int64))
    if off[0] != 0:
        raise ValueError(f"offsets must start at 0, got {int(off[0])}")
    step = np.diff(off)
    if (step < 0).any():
        raise ValueError(f"offsets decrease at row {int(np.argmax(step < 0))}")
    if off[-1] != int(values.shape[0]):
        raise ValueError(f"offsets must end at len(values) = {int(values.shape[0])}, got {int(off[-1])}")
    if (step == 0).any():
        raise ValueError(f"row {int(np.argmax(step == 0))} is empty: every row of a multivector column must hold at least one vector")
    if k is not None and not 1 <= int(k) <= 1024:
        raise ValueError(f"k={k} not supported (1..1024)")
    return m, off


def check_query_offsets(q_offsets):
    """q_offsets [B + 1] of a batch of multivector queries (query b holds the vectors q_offsets[b] .. q_offsets[b + 1] - 1) -> a
    contiguous uint64 numpy array; every query holds 1 .. MULTIVEC_MAX_QUERY_VECTORS vectors"""
    off = np.ascontiguousarray(np.asarray(q_offsets.detach().cpu().numpy() if isinstance(q_offsets, torch.Tensor) else q_offsets).astype(np.int64))
    if off.ndim != 1 or off.size < 1 or off[0] != 0:
        raise ValueError("q_offsets must be a 1-D array of B + 1 entries starting at 0")
    nqv = np.diff(off)
    if (nqv < 1).any():
        raise ValueError(f"query {int(np.argmax(nqv < 1))} holds no vector: a multivector query has at least one")
    if (nqv > _lib.MULTIVEC_MAX_QUERY_VECTORS).any():
        b = int(np.argmax(nqv > _lib.MULTIVEC_MAX_QUERY_VECTORS))
        raise ValueError(f"query {b} holds {int(nqv[b])} vectors, above the limit of {_lib.MULTIVEC_MAX_QUERY_VECTORS} query vectors per query")
    return off.astype(np.uint64)


def check_multivector_ann_sizes(keff, k_out):
    if not 1 <= int(keff) <= _lib.MULTIVEC_ANN_MAX_KEFF:
        raise ValueError(f"keff = k * overfetch = {keff} candidates per query vector not supported (1..{_lib.MULTIVEC_ANN_MAX_KEFF})")
    if not 1 <= int(k_out) <= _lib.MULTIVEC_ANN_MAX_K_OUT:
        raise ValueError(f"k_out = k * refine_factor = {k_out} not supported (1..{_lib.MULTIVEC_ANN_MAX_K_OUT})")


_DT = {"float32": (torch.float32, 0), "float16": (torch.float16, 1), "int8": (torch.int8, 2)}

SQ_FRESH_BOUNDS = (float(np.finfo(np.float64).max), float(np.finfo(np.float64).min))     # ScalarQuantizer::new (sq.rs:43-55)


def _sq_column(a):
    """a column or query batch for the scalar quantiser -> (cuda tensor, dtype code); float32 and float16 only"""
    name = _dtype_name(a)
    if name not in ("float32", "float16"):
        raise ValueError(f"SQ builder: unsupported data type: {name} (float16 and float32 columns are supported)")
    return _vec(a)


def _rq_f32(a, what):
    """an array for the RaBitQ entry points -> contiguous float32 cuda tensor; other element types are refused"""
    name = _dtype_name(a)
    if name not in ("float32", "float64"):      # (float64 host arrays are narrowed, as everywhere in this package)
        raise NotImplementedError(f"IVF_RQ: {what} must be float32, got {name} (float16 and int8 columns are not supported)")
    return _vec(a)[0]


def _rq_check(metric, x, cent, rot):
    if metric == "cosine":
        raise NotImplementedError("IVF_RQ: metric cosine is not supported (which distance type the reference's loaded storage carries into "
                                  "q_factor is not established); use l2 or dot")
    if metric not in ("l2", "dot"):
        raise ValueError(f"IVF_RQ: metric {metric} not supported (l2 and dot are)")
    if x.dim() != 2:
        raise ValueError(f"rows must be [n][d], got shape {tuple(x.shape)}")
    d = x.shape[1]
    if d % 8 != 0 or d == 0:
        raise ValueError(f"IVF_RQ: dimension {d} is not a multiple of 8 (one bit per dimension, packed into bytes)")
    if d > _lib.RQ_MAX_DIM:
        raise ValueError(f"IVF_RQ: dimension {d} not supported (up to {_lib.RQ_MAX_DIM})")
    if cent is not None and (cent.dim() != 2 or cent.shape[1] != d):
        raise ValueError(f"centroids must be [nlist][{d}], got shape {tuple(cent.shape)}")
    if tuple(rot.shape) != (d, d):
        raise ValueError(f"rq_rotation must be [{d}][{d}], got shape {tuple(rot.shape)}")


def _on_engine_device(fn):
    """Every tensor a method allocates or moves must live on the GPU the context was created on (two Engines in one process
    may sit on different GPUs): run the method with that device current."""
    @functools.wraps(fn)
    def wrapper(self, *a, **kw):
        eng = self if isinstance(self, Engine) else getattr(self, "engine", None)
        if eng is None or not torch.cuda.is_available() or torch.cuda.current_device() == eng.device:
            return fn(self, *a, **kw)
        with torch.cuda.device(eng.device):
            return fn(self, *a, **kw)
    return wrapper


def _wrap_methods(cls, skip=()):
    """_on_engine_device around the public methods cls itself defines (private helpers run inside one of those)"""
    for name, fn in list(vars(cls).items()):
        if callable(fn) and not name.startswith("_") and name not in skip and not isinstance(fn, (classmethod, staticmethod)):
            setattr(cls, name, _on_engine_device(fn))
    return cls


class Engine:
    """One context (stream + scratch arena) on the current device."""

    def __init__(self, device=None, use_torch_stream=False):
        self.lib = _lib.load()
        if device is None:
            device = _dev().index
        self.device = device
        self.use_torch_stream = bool(use_torch_stream)
        stream = None
        if use_torch_stream:
            stream = C.c_void_p(torch.cuda.current_stream(device).cuda_stream)
        h = C.c_void_p()
        check(self.lib.lance_hip_ctx_create(device, stream, C.byref(h)))
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.lib.lance_hip_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def synchronize(self):
        check(self.lib.lance_hip_synchronize(self.h))

    # ---- building blocks ---------------------------------------------------------
    def normalize(self, x):
        """normalize_fsl (kernels.rs:141-186): float32 rows in f32 arithmetic; float16 rows stay float16 and are normalised in
        half-precision arithmetic, as do_normalize_fsl::<Float16Type> does"""
        t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        f16 = t.dtype == torch.float16
        x = t.to(_dev()).contiguous() if f16 else to_device(x, torch.float32)
        out = torch.empty_like(x)
        n, d = x.shape
        torch.cuda.synchronize()
        check(self.lib.lance_hip_normalize(self.h, _lib.F16 if f16 else _lib.F32, _ptr(x), n, d, _ptr(out)))
        return out

    def assign(self, x, centroids, metric="l2", bias=None):
        x, dt = _vec(x); centroids = _model(centroids, x)
        n, d = x.shape
        k = centroids.shape[0]
        ids = torch.empty(n, dtype=torch.int32, device=x.device)
        dists = torch.empty(n, dtype=torch.float32, device=x.device)
        b = None if bias is None else to_device(bias, torch.float32)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_assign(self.h, dt, METRICS[metric], _ptr(x), n, d, _ptr(centroids), k, _ptr(b),
                                        _ptr(ids), _ptr(dists)))
        return ids, dists

    def kmeans_train(self, x, k, max_iters=50, tol=1e-4, balance_factor=0.0, init=None, seed=0, metric="l2", hierarchical_k=16):
        """KMeans::new_with_params: flat Lloyd for k <= 256 (or hierarchical_k <= 1), hierarchical otherwise."""
        x, dt = _vec(x)
        n, d = x.shape
        mdt = torch.float32 if x.dtype == torch.int8 else x.dtype
        cent = torch.zeros((k, d), dtype=mdt, device=x.device)
        init_t = None if init is None else _model(init, x)
        loss = C.c_double(0); iters = C.c_uint32(0); kout = C.c_uint32(0)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_kmeans_train_ex(self.h, dt, METRICS[metric], _ptr(x), n, d, k, max_iters, tol,
                                                 balance_factor, hierarchical_k, _ptr(init_t), seed, _ptr(cent), C.byref(loss),
                                                 C.byref(iters), C.byref(kout)))
        return cent[: kout.value], loss.value, iters.value

    def kmeans_split(self, x, rows, k, max_iters=50, tol=1e-4, balance_factor_scaled=0.0, seed=0, metric="l2", f16_arith=False):
        """One split of the hierarchical trainer (lance_hip_kmeans_split): k-means with k centroids over the rows `rows` (ascending u32
        indices, None: all) of the device sample x (f32; an f16 / int8 sample is widened -- f16_arith: the values are binary16 and the
        M-step rounds like half::f16), then their membership.  No device-wide synchronisation: host threads run splits side by side.
        -> (centroids np.float32 [k, d], membership np.uint32 [len(rows)])"""
        f16 = bool(f16_arith)
        if not (isinstance(x, torch.Tensor) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()):
            x, dt0 = _vec(x)
            f16 = f16 or x.dtype == torch.float16
            x = x.float().contiguous()          # (callers that split many times widen once themselves and pass f16_arith)
        dt = _lib.F16 if f16 else _lib.F32
        n, d = x.shape
        r = None if rows is None else np.ascontiguousarray(rows, np.uint32)
        nr = n if r is None else len(r)
        cent = np.empty((k, d), np.float32)
        mem = np.empty(nr, np.uint32)
        check(self.lib.lance_hip_kmeans_split(self.h, dt, METRICS[metric], _ptr(x), n, d, None if r is None else r.ctypes.data_as(C.c_void_p), nr, k,
                                              max_iters, tol, float(balance_factor_scaled), seed, cent.ctypes.data_as(C.c_void_p),
                                              mem.ctypes.data_as(C.c_void_p)))
        return cent, mem

    def kmeans_estep_partial(self, x, centroids, metric="l2", bias=None):
        """-> (buf [k*d sums | k counts] f32, losses [k] f64, radius [k] f32) device tensors"""
        x = to_device(x, torch.float32); centroids = to_device(centroids, torch.float32)
        n, d = x.shape
        k = centroids.shape[0]
        buf = torch.empty(k * d + k, dtype=torch.float32, device=x.device)
        losses = torch.empty(k, dtype=torch.float64, device=x.device)
        radius = torch.empty(k, dtype=torch.float32, device=x.device)
        b = None if bias is None else to_device(bias, torch.float32)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_kmeans_estep_partial(self.h, _lib.F32, METRICS[metric], _ptr(x), n, d, _ptr(centroids), k,
                                                      _ptr(b), _ptr(buf), _ptr(losses), _ptr(radius), None))
        return buf, losses, radius

    def kmeans_finalize(self, buf, k, d):
        cent = torch.empty((k, d), dtype=torch.float32, device=buf.device)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_kmeans_finalize(self.h, _lib.F32, _ptr(buf), k, d, _ptr(cent)))
        return cent

    # ---- row-sharded Lloyd loop, enqueue-only (lance_hip_kmeans_shard_*): see lance_amd/dist.py -------------------------
    def kmeans_shard_begin(self, k, d, balance_factor_scaled, seed):
        """-> dict of the device buffers one sharded training run needs (state, bias, reduce buffers)"""
        dev = _dev()
        st = {"state": torch.zeros(128, dtype=torch.uint8, device=dev), "bias": torch.zeros(k, dtype=torch.float32, device=dev),
              "buf": torch.zeros(k * d + k, dtype=torch.float32, device=dev), "losses": torch.zeros(k, dtype=torch.float64, device=dev),
              "radius": torch.zeros(k, dtype=torch.float32, device=dev), "k": k, "d": d, "bfs": float(balance_factor_scaled)}
        check(self.lib.lance_hip_kmeans_shard_begin(self.h, k, st["bfs"], seed, _ptr(st["state"]), _ptr(st["bias"])))
        return st

    def kmeans_shard_estep(self, st, x_local, cent, metric="l2"):
        n = x_local.shape[0]
        check(self.lib.lance_hip_kmeans_shard_estep(self.h, METRICS[metric], _ptr(x_local) if n else None, n, st["d"], _ptr(cent), st["k"],
                                                    _ptr(st["bias"]) if st["bfs"] != 0 else None, _ptr(st["state"]), _ptr(st["buf"]),
                                                    _ptr(st["losses"]), _ptr(st["radius"])))

    def kmeans_shard_update(self, st, cent, n_total, tol, it):
        check(self.lib.lance_hip_kmeans_shard_update(self.h, _ptr(st["state"]), _ptr(st["buf"]), _ptr(st["losses"]), _ptr(st["radius"]),
                                                     _ptr(cent), _ptr(st["bias"]), st["k"], st["d"], n_total, st["bfs"], tol, it))

    def kmeans_shard_end(self, st):
        loss = C.c_double(0); iters = C.c_uint32(0); active = C.c_int(0)
        check(self.lib.lance_hip_kmeans_shard_end(self.h, _ptr(st["state"]), C.byref(loss), C.byref(iters), C.byref(active)))
        return loss.value, iters.value, bool(active.value)

    # ---- the sharded Lloyd loop with its collectives behind the C ABI (comm.cpp): for hosts without torch.distributed ----
    def comm_unique_id(self):
        """ncclGetUniqueId through the library: 128 bytes rank 0 ships to the other ranks"""
        buf = C.create_string_buffer(128)
        check(self.lib.lance_hip_comm_unique_id(buf))
        return buf.raw

    def comm_create(self, unique_id, nranks, rank):
        """ncclCommInitRank on this engine's device -> opaque communicator handle (comm_destroy releases it)"""
        h = C.c_void_p()
        check(self.lib.lance_hip_comm_create(self.h, C.create_string_buffer(bytes(unique_id), 128), nranks, rank, C.byref(h)))
        return h

    def comm_from_callback(self, fn, nranks, rank):
        """lance_hip_comm_from_callback: the sharded trainer's exchanges through a host transport.  fn(buf_ptr, count, dtype, op,
        stream_ptr) -> 0 reduces `count` elements (dtype 0 = f32, 1 = f64; op 0 = sum, 1 = max) at DEVICE address buf_ptr in place
        across the ranks.  The ctypes thunk is kept alive on the returned handle's engine."""
        def guarded(user, buf, count, dtype, op, stream):
            # an exception must reach the trainer as a failed exchange: ctypes would print the traceback and hand 0 ("reduced") to C,
            # and the ranks would go on with unreduced buffers
            try:
                return int(fn(buf, count, dtype, op, stream))
            except BaseException:
                import traceback
                traceback.print_exc()
                return 1
        thunk = _lib.ALLREDUCE_FN(guarded)
        h = C.c_void_p()
        check(self.lib.lance_hip_comm_from_callback(thunk, None, nranks, rank, C.byref(h)))
        if not hasattr(self, "_comm_thunks"):
            self._comm_thunks = {}
        self._comm_thunks[h.value] = thunk       # alive exactly as long as the communicator
        return h

    def comm_destroy(self, comm):
        self.lib.lance_hip_comm_destroy(comm)
        getattr(self, "_comm_thunks", {}).pop(getattr(comm, "value", comm), None)

    def kmeans_train_sharded(self, comm, x_local, init_centroids, n_total, max_iters=50, tol=1e-4, balance_factor=0.0, seed=0, metric="l2"):
        """lance_hip_kmeans_train_sharded: rows sharded over the ranks of `comm` (None: single process), one fused all-reduce per
        Lloyd iteration inside the library.  init_centroids: identical on every rank.  -> (centroids, loss, iterations)"""
        x, dt = _vec(x_local)                # the shard in the column's own element type (f16 / int8 are widened inside the library, once)
        cent = to_device(init_centroids, torch.float32).clone().contiguous()
        n, d = x.shape
        k = cent.shape[0]
        loss = C.c_double(0); iters = C.c_uint32(0)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_kmeans_train_sharded_x(self.h, comm, dt, METRICS[metric], _ptr(x), n, d, k, int(n_total), max_iters, tol, balance_factor,
                                                        seed, _ptr(cent), C.byref(loss), C.byref(iters)))
        return cent, loss.value, iters.value

    def pq_train(self, residuals, m, nbits=8, max_iters=50, sample_rate=256, seed=0):
        r, dt = _vec(residuals)
        n, d = r.shape
        cb = torch.empty((m, 1 << nbits, d // m), dtype=torch.float32 if r.dtype == torch.int8 else r.dtype, device=r.device)
        iters = np.zeros(m, np.uint32)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_pq_train(self.h, dt, _ptr(r), n, d, m, nbits, max_iters, sample_rate, seed, _ptr(cb),
                                          iters.ctypes.data_as(C.c_void_p)))
        return cb, iters

    def residual(self, x, centroids, part_ids):
        x, dt = _vec(x); centroids = _model(centroids, x)
        p = to_device(part_ids, torch.int32)
        out = torch.empty(x.shape, dtype=centroids.dtype, device=x.device)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_residual(self.h, dt, _ptr(x), x.shape[0], x.shape[1], _ptr(centroids), _ptr(p), _ptr(out)))
        return out

    def reassign_rows(self, metric, raw, row_ids, seg_offsets, seg_centroids, cand_ids, centroids2=None, part1=_lib.NONE, part2=_lib.NONE):
        """lance_hip_reassign_rows: where the visited rows of a partition split (centroids2 = [c1, c2], standing for the partitions
        part1 / part2) or join (centroids2 None) go.  row_ids [n] in visit order, in segments seg_offsets [C + 2] (segment 0: the chosen
        partition, segment s: candidate s - 1); seg_centroids [C + 1][d]: the old centroid, then the candidates'; cand_ids [C] in the
        result's numbering; raw [n_raw][d] float32, indexed by row id.  -> dest int32 [n] on the device (-1 = LANCE_HIP_NONE: stays)"""
        if _dtype_name(raw) not in ("float32", "float64"):
            raise ValueError(f"reassign_rows: raw vectors must be float32, got {_dtype_name(raw)} (float16 and int8 columns are not supported)")
        raw = _raw_column(raw, torch.float32)
        n_raw, d = raw.shape
        rid = to_device(row_ids, torch.int64).reshape(-1)
        seg = to_device(seg_offsets, torch.int32).reshape(-1)
        cent = to_device(seg_centroids, torch.float32).reshape(-1, d)
        cand = to_device(cand_ids, torch.int32).reshape(-1)
        ncand = cand.numel()
        if seg.numel() != ncand + 2 or cent.shape[0] != ncand + 1:
            raise ValueError(f"reassign_rows: {ncand} candidates need {ncand + 2} segment offsets and {ncand + 1} centroids, "
                             f"got {seg.numel()} and {cent.shape[0]}")
        c12 = None if centroids2 is None else to_device(centroids2, torch.float32).reshape(2, d)
        dest = torch.empty(rid.numel(), dtype=torch.int32, device=raw.device)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_reassign_rows(self.h, METRICS[metric], _lib.REASSIGN_JOIN if c12 is None else _lib.REASSIGN_SPLIT, _ptr(raw),
                                               n_raw, d, _ptr(rid), rid.numel(), _ptr(seg), _ptr(cent), _ptr(cand), ncand, _ptr(c12),
                                               int(part1), int(part2), _ptr(dest)))
        return dest

    def pq_encode(self, x, codebook, metric="l2"):
        x, dt = _vec(x); codebook = _model(codebook, x)
        n, d = x.shape
        m = codebook.shape[0]
        nb = _nbits(codebook)
        codes = torch.empty((n, m if nb == 8 else m // 2), dtype=torch.uint8, device=x.device)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_pq_encode(self.h, dt, METRICS[metric], _ptr(x), n, d, _ptr(codebook), m, nb, _ptr(codes)))
        return codes

    def ivfpq_encode(self, x, centroids, codebook, metric="l2", want_loss=True):
        """-> (partition ids, PQ codes, loss).  want_loss=False passes NULL for `loss_out_host`: the C side then skips copying the n
        assignment distances to the host and summing them there (0.5 ms per million rows; the index build does not use the figure)."""
        x, dt = _vec(x); centroids = _model(centroids, x)
        codebook = _model(codebook, x)
        n, d = x.shape
        m = codebook.shape[0]
        nb = _nbits(codebook)
        part = torch.empty(n, dtype=torch.int32, device=x.device)
        codes = torch.empty((n, m if nb == 8 else m // 2), dtype=torch.uint8, device=x.device)
        loss = C.c_double(0)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_ivfpq_encode(self.h, dt, METRICS[metric], _ptr(x), n, d, _ptr(centroids),
                                              centroids.shape[0], _ptr(codebook), m, nb, _ptr(part), _ptr(codes),
                                              C.byref(loss) if want_loss else None))
        return part, codes, (loss.value if want_loss else None)

    def find_partitions(self, q, centroids, nprobes, metric="l2"):
        centroids, dt = _vec(centroids)
        if isinstance(q, (torch.Tensor, np.ndarray)) and str(q.dtype).endswith("int8"):
            q, dt = _vec(q)                       # int8 queries against the f32 centroids of an Int8 column
            q = q.reshape(-1, centroids.shape[1])
        else:
            q = _like(q, centroids).reshape(-1, centroids.shape[1])
        nq, d = q.shape
        nlist = centroids.shape[0]
        nprobes = min(nprobes, nlist)
        ids = torch.empty((nq, nprobes), dtype=torch.int32, device=q.device)
        dists = torch.empty((nq, nprobes), dtype=torch.float32, device=q.device)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_find_partitions(self.h, dt, METRICS[metric], _ptr(q), nq, d, _ptr(centroids), nlist,
                                                 nprobes, _ptr(ids), _ptr(dists)))
        return ids, dists

    def pq_scan_topk(self, q_residual, codebook, codes_transposed, row_ids, k, metric="l2", lower=None, upper=None):
        cb, dt = _vec(codebook)
        q = _like(q_residual, cb).reshape(-1)
        ct = to_device(codes_transposed, torch.uint8)
        rid = to_device(row_ids, torch.int64)
        nb = _nbits(cb)
        m = cb.shape[0]
        n_p = ct.shape[1]
        out_i = torch.empty(k, dtype=torch.int64, device=q.device)
        out_d = torch.empty(k, dtype=torch.float32, device=q.device)
        cnt = C.c_uint32(0)
        has = lower is not None or upper is not None
        lo, hi = _range_f32(lower, upper)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_pq_scan_topk(self.h, dt, METRICS[metric], _ptr(q), q.numel(), _ptr(cb), m, nb, _ptr(ct),
                                              _ptr(rid), n_p, k, int(has), lo, hi, _ptr(out_i), _ptr(out_d), C.byref(cnt)))
        return out_i[:cnt.value], out_d[:cnt.value]

    def flat_topk(self, x, q, k, metric="l2", row_ids=None, lower=None, upper=None):
        """exhaustive KNN -> (ids [nq][k] int64, distances [nq][k]) sorted by (distance, row id); missing slots: id -1, distance +inf.
        lower / upper: distance range (lance_hip_flat_topk_range) -- the k nearest rows with lower <= d < upper in the total order
        on f32.  A bound that is None is NOT TESTED (IvfFlatIndex.nearest's open ends are the largest finite f32 instead): (lower,
        None) keeps +inf and NaN distances.  Both None: lance_hip_flat_topk, the call from before ranges existed."""
        rng = _flat_range_args(lower, upper)
        x, dt = _vec(x)
        q = _like(q, x).reshape(-1, x.shape[1])
        n, d = x.shape
        nq = q.shape[0]
        rid = None if row_ids is None else to_device(row_ids, torch.int64)
        ids = torch.empty((nq, k), dtype=torch.int64, device=x.device)
        dists = torch.empty((nq, k), dtype=torch.float32, device=x.device)
        torch.cuda.synchronize()
        if rng is None:
            check(self.lib.lance_hip_flat_topk(self.h, dt, METRICS[metric], _ptr(x), _ptr(rid), n, d, _ptr(q), nq, k,
                                               _ptr(ids), _ptr(dists)))
        else:
            check(self.lib.lance_hip_flat_topk_range(self.h, dt, METRICS[metric], _ptr(x), _ptr(rid), n, d, _ptr(q), nq, k, *rng,
                                                     _ptr(ids), _ptr(dists)))
        return ids, dists

    def multivec_distance(self, values, offsets, q, metric="cosine"):
        """multivec_distance (lance-linalg distance.rs:107-206) of the multivector query q [nqv][d] to every row of a multivector
        column: values [total vectors][d] (float32 / float16), offsets [n_rows + 1] -> [n_rows] float32"""
        m, off = check_multivector(values, offsets, q, metric)
        v, dt = _vec(values)
        qd = _like(q, v)
        od = to_device(off, torch.int64)
        n = off.size - 1
        dists = torch.empty(n, dtype=torch.float32, device=v.device)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_multivec_distance(self.h, dt, METRICS[m], _ptr(v), _ptr(od), n, v.shape[1], _ptr(qd), qd.shape[0],
                                                   _ptr(dists)))
        return dists

    def multivec_topk(self, values, offsets, q, k, metric="cosine", row_ids=None, lower=None, upper=None):
        """exhaustive KNN of one multivector query over a multivector column -> (ids [k] int64, distances [k]) sorted by
        (distance, row id); slots beyond the number of rows hold id -1 and distance +inf, as flat_topk's do.
        lower / upper: distance range on the rows' multivector distances, with flat_topk's semantics (a None bound is not tested)"""
        rng = _flat_range_args(lower, upper)
        m, off = check_multivector(values, offsets, q, metric, k)
        n = off.size - 1
        if row_ids is not None and int(row_ids.shape[0]) != n:
            raise ValueError(f"row_ids must hold one id per row ({n}), got {int(row_ids.shape[0])}")
        v, dt = _vec(values)
        qd = _like(q, v)
        od = to_device(off, torch.int64)
        rid = None if row_ids is None else to_device(row_ids, torch.int64)
        ids = torch.empty(k, dtype=torch.int64, device=v.device)
        dists = torch.empty(k, dtype=torch.float32, device=v.device)
        torch.cuda.synchronize()
        if rng is None:
            check(self.lib.lance_hip_flat_multivec_topk(self.h, dt, METRICS[m], _ptr(v), _ptr(od), _ptr(rid), n, v.shape[1], _ptr(qd),
                                                        qd.shape[0], k, _ptr(ids), _ptr(dists)))
        else:
            check(self.lib.lance_hip_flat_multivec_topk_range(self.h, dt, METRICS[m], _ptr(v), _ptr(od), _ptr(rid), n, v.shape[1], _ptr(qd),
                                                              qd.shape[0], k, *rng, _ptr(ids), _ptr(dists)))
        return ids, dists

    def multivec_topk_batch(self, values, offsets, q, q_offsets, k, metric="cosine", row_ids=None, lower=None, upper=None,
                            return_survivors=False):
        """exhaustive KNN of a BATCH of B multivector queries over a multivector column: q [sum nqv][d], the vectors of query b are
        rows q_offsets[b] .. q_offsets[b + 1] - 1 (the pair arrow_io.multivector_from_arrow returns for a List<FixedSizeList> array of
        queries) -> (ids [B][k] int64, distances [B][k]), row b bit for bit multivec_topk's answer for query b.  Cosine without a
        range, d <= 256: a MaxSim surrogate on the matrix cores filters the rows (lance_hip_flat_multivec_topk_batch); everything
        else runs the single-query scan per query inside the call.  return_survivors: also the rows evaluated exactly per query
        (int64 numpy [B]; n_rows where the exact scan answered the query)"""
        rng = _flat_range_args(lower, upper)
        qoff = check_query_offsets(q_offsets)
        B = qoff.size - 1
        if not 1 <= B <= 65535:
            raise ValueError(f"{B} queries: a batch holds 1..65535")
        if len(q.shape) != 2 or int(q.shape[0]) != int(qoff[-1]):
            raise ValueError(f"q must be [{int(qoff[-1])}][d], the vectors of all queries (q_offsets ends at {int(qoff[-1])}), got shape {tuple(q.shape)}")
        m = off = None
        for b in range(B):
            m, off = check_multivector(values, offsets, q[int(qoff[b]):int(qoff[b + 1])], metric, k)
        n = off.size - 1
        if row_ids is not None and int(row_ids.shape[0]) != n:
            raise ValueError(f"row_ids must hold one id per row ({n}), got {int(row_ids.shape[0])}")
        v, dt = _vec(values)
        qd = _like(q, v)
        od = to_device(off, torch.int64)
        rid = None if row_ids is None else to_device(row_ids, torch.int64)
        ids = torch.empty((B, k), dtype=torch.int64, device=v.device)
        dists = torch.empty((B, k), dtype=torch.float32, device=v.device)
        surv = np.zeros(B, dtype=np.uint32)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_flat_multivec_topk_batch(self.h, dt, METRICS[m], _ptr(v), _ptr(od), _ptr(rid), n, v.shape[1], _ptr(qd),
                                                          qoff.ctypes.data_as(C.c_void_p), B, k, *(rng or (0, 0.0, 0, 0.0)), _ptr(ids), _ptr(dists),
                                                          surv.ctypes.data_as(C.c_void_p)))
        return (ids, dists, surv.astype(np.int64)) if return_survivors else (ids, dists)

    def multivec_xtr_score(self, cand_ids, cand_dists, q_offsets, k_out):
        """The join and score stage of the multivector ANN search (lance_hip_multivec_xtr_score; MultivectorScoringExec,
        knn.rs:1132-1329) for a batch of B multivector queries: cand_ids / cand_dists [sum nqv][keff] hold one candidate list per
        query vector in (distance, row id) order (valid entries first, then id -1 / +inf), the lists of query b are rows
        q_offsets[b] .. q_offsets[b + 1] - 1.  -> (ids [B][k_out] int64 (-1 = none), distances [B][k_out]) sorted by (distance, row id)"""
        off = check_query_offsets(q_offsets)
        B = off.size - 1
        ci = to_device(cand_ids, torch.int64)
        cd = to_device(cand_dists, torch.float32)
        if ci.dim() != 2 or tuple(ci.shape) != tuple(cd.shape) or ci.shape[0] != int(off[-1]):
            raise ValueError(f"cand_ids / cand_dists must both be [{int(off[-1])}][keff] (one list per query vector), got "
                             f"{tuple(ci.shape)} and {tuple(cd.shape)}")
        keff = int(ci.shape[1])
        check_multivector_ann_sizes(keff, k_out)
        ids = torch.empty((B, k_out), dtype=torch.int64, device=ci.device)
        dists = torch.empty((B, k_out), dtype=torch.float32, device=ci.device)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_multivec_xtr_score(self.h, _ptr(ci), _ptr(cd), off.ctypes.data_as(C.c_void_p), B, keff, k_out, _ptr(ids),
                                                    _ptr(dists)))
        return ids, dists

    # ---- 8-bit scalar quantisation (lance-index/src/vector/sq.rs) -------------------------
    def sq_bounds(self, x, bounds=None):
        """ScalarQuantizer::update_bounds: folds the elements of x (float32 / float16) into `bounds` = (start, end) -- None: a fresh
        quantiser's (f64::MAX, f64::MIN) -- skipping NaN.  -> (start, end) as Python floats"""
        x, dt = _sq_column(x)
        b = (C.c_double * 2)(*(SQ_FRESH_BOUNDS if bounds is None else (float(bounds[0]), float(bounds[1]))))
        torch.cuda.synchronize()
        check(self.lib.lance_hip_sq_bounds(self.h, dt, _ptr(x), x.numel(), b))
        return float(b[0]), float(b[1])

    def sq_encode(self, x, bounds):
        """scale_to_u8: x [n][d] -> uint8 codes [n][d] under bounds = (start, end)"""
        x, dt = _sq_column(x)
        if x.dim() != 2:
            raise ValueError(f"x must be [n][d], got shape {tuple(x.shape)}")
        n, d = x.shape
        codes = torch.empty((n, d), dtype=torch.uint8, device=x.device)
        b = (C.c_double * 2)(float(bounds[0]), float(bounds[1]))
        torch.cuda.synchronize()
        check(self.lib.lance_hip_sq_encode(self.h, dt, _ptr(x), n, d, b, _ptr(codes)))
        return codes

    def sq_distance(self, codes, q, bounds, metric="l2"):
        """SQDistCalculator::distance_all for every query: codes [n][d] uint8, raw queries q [nq][d] (float32 / float16, encoded
        with the same bounds) -> [nq][n] float32"""
        q, dt = _sq_column(q)
        codes = to_device(codes, torch.uint8)
        n, d = codes.shape
        q = q.reshape(-1, d)
        dists = torch.empty((q.shape[0], n), dtype=torch.float32, device=codes.device)
        b = (C.c_double * 2)(float(bounds[0]), float(bounds[1]))
        torch.cuda.synchronize()
        check(self.lib.lance_hip_sq_distance(self.h, dt, METRICS[metric], _ptr(codes), n, d, _ptr(q), q.shape[0], b, _ptr(dists)))
        return dists

    # ---- 1-bit RaBitQ (lance-index/src/vector/bq) ------------------------------------------
    def rq_encode(self, x, part_ids, dist_v_c, centroids, rotation, metric="l2"):
        """RabitQuantizer::quantize + RQTransformer::transform: float32 rows x [n][d] with their partition ids and the distances the
        assignment reported (Engine.assign's two results), centroids [nlist][d], rotation P [d][d] -> (codes uint8 [n][d / 8],
        add float32 [n], scale float32 [n]).  Rows without a partition (id -1) get zeros."""
        x, cent, rot = _rq_f32(x, "x"), _rq_f32(centroids, "centroids"), _rq_f32(rotation, "rotation")
        _rq_check(metric, x, cent, rot)
        n, d = x.shape
        part = to_device(part_ids, torch.int32)
        dvc = to_device(dist_v_c, torch.float32)
        if part.numel() != n or dvc.numel() != n:
            raise ValueError(f"part_ids and dist_v_c must hold one entry per row ({n}), got {part.numel()} and {dvc.numel()}")
        codes = torch.empty((n, d // 8), dtype=torch.uint8, device=x.device)
        add = torch.empty(n, dtype=torch.float32, device=x.device)
        scale = torch.empty(n, dtype=torch.float32, device=x.device)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_rq_encode(self.h, METRICS[metric], _ptr(x), n, d, _ptr(part), _ptr(dvc), _ptr(cent), cent.shape[0], _ptr(rot),
                                           _ptr(codes), _ptr(add), _ptr(scale)))
        return codes, add, scale

    def rq_distance(self, codes, add, scale, qr, dist_q_c, rotation, metric="l2", quantised=True):
        """RabitDistCalculator over ONE partition's storage (codes [n][d / 8], add [n], scale [n], in storage order) against residual
        queries qr [nq][d] (q - centroid) with their dist_q_c [nq]: quantised=True is distance_all (rows below n - n % 32 through the
        u8 table, the rest in f32), False is distance(id) of every row (a prefiltered search) -> [nq][n] float32"""
        rot = _rq_f32(rotation, "rotation")
        d = rot.shape[0]
        qr = _rq_f32(qr, "qr").reshape(-1, d)
        _rq_check(metric, qr, None, rot)
        codes = to_device(codes, torch.uint8)
        add, scale, dqc = to_device(add, torch.float32), to_device(scale, torch.float32), to_device(dist_q_c, torch.float32)
        n = codes.shape[0]
        if codes.dim() != 2 or codes.shape[1] != d // 8 or add.numel() != n or scale.numel() != n or dqc.numel() != qr.shape[0]:
            raise ValueError(f"codes must be [n][{d // 8}] with add / scale [n] and dist_q_c [nq]")
        dists = torch.empty((qr.shape[0], n), dtype=torch.float32, device=qr.device)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_rq_distance(self.h, METRICS[metric], _ptr(codes), _ptr(add), _ptr(scale), n, d, _ptr(qr), _ptr(dqc), qr.shape[0],
                                             _ptr(rot), int(bool(quantised)), _ptr(dists)))
        return dists

    def search_stats(self):
        """queries of the last search replayed by the exact (heap-emulating) kernel"""
        n = C.c_uint32(0)
        check(self.lib.lance_hip_search_stats(self.h, C.byref(n)))
        return n.value

    # ---- timing hooks --------------------------------------------------------------
    def timing(self, on=True):
        check(self.lib.lance_hip_timing_enable(self.h, int(on)))

    def timing_query(self, kernel):
        ms = C.c_double(0); n = C.c_uint64(0)
        check(self.lib.lance_hip_timing_query(self.h, kernel.encode(), C.byref(ms), C.byref(n)))
        return ms.value, n.value


    def merge_topk(self, ids, dists, k, exact=None, keff=None):
        """(dist, rowid) merge of gathered candidate lists on the device (lance_hip_merge_topk): ids [nq, C] int64 (-1 = none),
        dists [nq, C]; with `exact` the keff best by PQ distance are re-ranked by the exact distances.  -> ([nq,k], [nq,k])"""
        ids = to_device(ids, torch.int64); dists = to_device(dists, torch.float32)
        ex = None if exact is None else to_device(exact, torch.float32)
        nq, c = ids.shape
        out_i = torch.empty((nq, k), dtype=torch.int64, device=ids.device)
        out_d = torch.empty((nq, k), dtype=torch.float32, device=ids.device)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_merge_topk(self.h, _ptr(ids), _ptr(dists), _ptr(ex), nq, c, keff if keff is not None else k, k,
                                            _ptr(out_i), _ptr(out_d)))
        return out_i, out_d

    def take_flat_knn(self, x, q, ids_a, k, metric="l2", ids_b=None, dists_b=None, lower=None, upper=None):
        """`take` + `flat_knn` over candidate lists (lance_hip_take_flat_knn; scanner.rs:2884-2904, 3336-3468): per query the rows
        ids_a [nq][ca] and ids_b [nq][cb] (int64, -1 = an empty slot; a row id is a row index of x [n][d]) are scored against the
        column with the query as given -- the distance flat_topk returns for that (row, query), bit for bit --, tested against
        lower <= d < upper (flat_topk's bounds: None is not tested) and the k best by (distance, row id) returned; nothing is
        de-duplicated.  dists_b: list B's distances as flat_topk returned them, taken as they are; None: its rows are scored
        too.  -> (ids [nq][k] int64, distances [nq][k]); missing slots: id -1, distance +inf.  ca + cb <= 4096, k <= 1024."""
        rng = _flat_range_args(lower, upper) or (0, 0.0, 0, 0.0)
        x, dt = _vec(x)
        n, d = x.shape
        q = _like(q, x).reshape(-1, d)
        nq = q.shape[0]
        a = to_device(ids_a, torch.int64).reshape(nq, -1)
        b = None if ids_b is None else to_device(ids_b, torch.int64).reshape(nq, -1)
        db = None
        if dists_b is not None:
            if b is None:
                raise ValueError("take_flat_knn: dists_b given without ids_b")
            db = to_device(dists_b, torch.float32).reshape(nq, -1)
            if db.shape != b.shape:
                raise ValueError(f"take_flat_knn: dists_b {tuple(db.shape)} does not match ids_b {tuple(b.shape)}")
        ids = torch.empty((nq, k), dtype=torch.int64, device=x.device)
        dists = torch.empty((nq, k), dtype=torch.float32, device=x.device)
        torch.cuda.synchronize()
        check(self.lib.lance_hip_take_flat_knn(self.h, dt, METRICS[metric], _ptr(x), n, d, _ptr(q), nq, _ptr(a), a.shape[1], _ptr(b),
                                               _ptr(db), 0 if b is None else b.shape[1], *rng, k, _ptr(ids), _ptr(dists)))
        return ids, dists

    def ubench(self, what):
        """in-process ceilings for bench.py (lance_hip_ubench): "lds4" / "lds8" / "lds16" lane-gathers per second,
        "copy" bytes per second, "valu" / "valu_pk" f32 wave-instructions per second"""
        r = C.c_double(0)
        codes = {"lds4": 0, "lds8": 1, "lds16": 2, "copy": 3, "valu": 4, "valu_pk": 5,
                 # round 3: code-major m-staggered u16x4 table (M = 16 / 32), today's layout with the integer accumulate, and the
                 # conflict-free ds_read_b64 stream (the LDS pipe's own ceiling)
                 "lds8_stagger16": 6, "lds8_stagger32": 7, "lds8_u16x4": 8, "lds8_linear": 9,
                 # round 6: dense 32x32x16 MFMA rate (flop per second), f16 / bf16 operands
                 "mfma_f16": 10, "mfma_bf16": 11}
        check(self.lib.lance_hip_ubench(self.h, codes[what], C.byref(r)))
        return r.value


_wrap_methods(Engine, skip=("close",))



def _torch_inputs_ready():
    """What a search call needs from torch before the engine's stream reads the batch: the work torch's CURRENT stream has queued (the
    conversion / move of the queries).  Not torch.cuda.synchronize(): a device-wide synchronise is not permitted while ANY stream of the
    process is capturing -- another host thread's repeated search being captured into a HIP graph -- and both threads then fail (the
    synchronising one in torch, the capturing one in the runtime; tests/test_zz_gpu_threads.py, gpurun r06zm).  The engines' streams are
    non-blocking: torch's stream has no implicit dependency on them."""
    torch.cuda.current_stream().synchronize()

# ---- index maintenance (lance_amd/csrc/index_update.hip): shared by the three handle classes -----------------------------------
def _merge_handles(engine, indices):
    """lance_hip_index_merge over the handles of `indices`, in that order -> a new handle"""
    arr = (C.c_void_p * max(1, len(indices)))(*[ix.h.value for ix in indices])
    h = C.c_void_p()
    torch.cuda.synchronize()
    check(engine.lib.lance_hip_index_merge(engine.h, arr, len(indices), C.byref(h)))
    return h


def _remap_handle(engine, handle, old_ids, new_ids):
    """lance_hip_index_remap: old_ids strictly ascending (as unsigned), new_ids with _lib.ROW_DELETED (-1 as int64) for a deleted row;
    both int64 bit patterns of the u64 ids -> a new handle"""
    old = to_device(old_ids, torch.int64).reshape(-1)
    new = to_device(new_ids, torch.int64).reshape(-1)
    if old.numel() != new.numel():
        raise ValueError(f"remap: {old.numel()} old ids but {new.numel()} new ids")
    h = C.c_void_p()
    torch.cuda.synchronize()
    check(engine.lib.lance_hip_index_remap(engine.h, handle, _ptr(old), _ptr(new), old.numel(), C.byref(h)))
    return h


def _export_ids(engine, handle, nlist):
    """lance_hip_index_export_rows without the payload -> (part_offsets u32[nlist + 1], row_ids u64[n]) in stored order"""
    n = C.c_uint64()
    check(engine.lib.lance_hip_index_info(handle, C.byref(n), None, None, None))
    offs = np.empty(nlist + 1, np.uint32)
    rid = np.empty(n.value, np.uint64)
    torch.cuda.synchronize()
    check(engine.lib.lance_hip_index_export_rows(engine.h, handle, offs.ctypes.data_as(C.c_void_p), None, None, rid.ctypes.data_as(C.c_void_p)))
    return offs, rid


def _rebalance_handle(engine, handle, centroids, part, raw, centroids2=None):
    """lance_hip_index_split (centroids2 = [c1, c2]) / lance_hip_index_join (centroids2 None) of partition `part` -> (a new handle, its
    centroid tensor: c1 in row `part` and c2 appended, or row `part` removed).  raw [n_raw][d] float32, indexed by the stored row ids."""
    if raw is None:
        raise ValueError("split / join: the raw vectors are required (rows are re-assigned and re-encoded from them)")
    if _dtype_name(raw) not in ("float32", "float64"):
        raise ValueError(f"split / join: raw vectors must be float32, got {_dtype_name(raw)} (float16 and int8 columns are not supported)")
    raw = _raw_column(raw, torch.float32)
    d = centroids.shape[1]
    if raw.shape[1] != d:
        raise ValueError(f"split / join: raw vectors must be [rows][{d}], got {tuple(raw.shape)}")
    part = int(part)
    h = C.c_void_p()
    torch.cuda.synchronize()
    if centroids2 is None:
        check(engine.lib.lance_hip_index_join(engine.h, handle, part, _ptr(raw), raw.shape[0], C.byref(h)))
        return h, torch.cat([centroids[:part], centroids[part + 1:]]).contiguous()
    c12 = to_device(centroids2, torch.float32).reshape(2, d)
    check(engine.lib.lance_hip_index_split(engine.h, handle, part, _ptr(c12), _ptr(raw), raw.shape[0], C.byref(h)))
    c = c12.to(centroids.dtype)
    return h, torch.cat([centroids[:part], c[:1], centroids[part + 1:], c[1:]]).contiguous()


def _export_rows(engine, handle, nlist, row_bytes, aux=False):
    """lance_hip_index_export_rows -> (part_offsets u32[nlist + 1], rows u8 [n, row_bytes], aux u32[n] | None, row_ids u64[n])"""
    n = C.c_uint64()
    check(engine.lib.lance_hip_index_info(handle, C.byref(n), None, None, None))
    n = n.value
    offs = np.empty(nlist + 1, np.uint32)
    rows = np.empty((n, row_bytes), np.uint8)
    xx = np.empty(n, np.uint32) if aux else None
    rid = np.empty(n, np.uint64)
    torch.cuda.synchronize()
    check(engine.lib.lance_hip_index_export_rows(engine.h, handle, offs.ctypes.data_as(C.c_void_p), rows.ctypes.data_as(C.c_void_p),
                                                 None if xx is None else xx.ctypes.data_as(C.c_void_p), rid.ctypes.data_as(C.c_void_p)))
    return offs, rows, xx, rid


def _raw_column(raw, dtype):
    t = raw if isinstance(raw, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(raw))
    t = t.to(dtype).to(_dev()).contiguous()
    if t.dim() != 2:
        raise ValueError(f"raw vectors must be [rows][d], got shape {tuple(t.shape)}")
    return t


def _allow_bytes(allow):
    """a prefilter (boolean array indexed by row id) -> uint8 device tensor; None stays None"""
    if allow is None:
        return None
    a = allow if isinstance(allow, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(allow, dtype=bool))
    return a.to(torch.uint8).to(_dev()).contiguous()


def _range_f32(lower, upper):
    """distance range -> (lo, hi) as the library takes them.  The bounds are f32 values in the reference (Query::lower_bound:
    Option<f32>): they are rounded before use, and an open end is the largest finite f32 of its sign."""
    lo = float(np.finfo(np.float32).min) if lower is None else float(np.float32(lower))
    hi = float(np.finfo(np.float32).max) if upper is None else float(np.float32(upper))
    return lo, hi


def _flat_range_args(lower, upper):
    """flat-scan distance range -> None (no range: the un-ranged entry point) or (has_lower, lower, has_upper, upper) as
    lance_hip_flat_topk_range takes them.  The bounds are rounded to f32 (Query::lower_bound: Option<f32>); an absent bound is
    absent -- not the largest finite f32, which is what _range_f32 gives the IVF entry points."""
    if lower is None and upper is None:
        return None
    lo = 0.0 if lower is None else float(np.float32(lower))
    hi = 0.0 if upper is None else float(np.float32(upper))
    return int(lower is not None), lo, int(upper is not None), hi


# ---- the index handles ---------------------------------------------------------------------------------------------------------------
# _DeviceHandle is what the four kinds share; _Maintainable adds merge / remap / split / join for the kinds whose storage can be appended
# to (IVF_RQ's cannot); _CodeIndex is the search of the two kinds that scan codes and re-rank on the raw column (IVF_SQ, IVF_RQ).  A new
# kind supplies its `create`, its table of search symbols and, to be maintainable, the `_ctor_args` hook.
class _DeviceHandle:
    """A device-resident index: the library handle `h`, the model tensors that must outlive it, the element type of queries and raw
    vectors, and the raw column when one is attached (borrowed by the handle, kept alive here)."""

    def __init__(self, engine, handle, metric, centroids, data_dtype):
        self.engine = engine
        self.h = handle
        self.metric = metric
        self.centroids = centroids
        self.data_dtype = data_dtype
        self._raw = None

    def _queries(self, q):
        """-> (q as the [nq][d] device tensor of the index's element type, the tensor it was made from: the same storage when the
        caller handed over a ready batch)"""
        t = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q))
        return t.to(self.data_dtype).to(_dev()).contiguous().reshape(-1, self.centroids.shape[1]), t

    @staticmethod
    def _outputs(q, k, out=None, rows=None):
        """-> (ids int64, dists f32), [rows or len(q)][k] each, beside q: the caller's `out` or fresh tensors"""
        if out is not None:
            return out
        rows = q.shape[0] if rows is None else rows
        return torch.empty((rows, k), dtype=torch.int64, device=q.device), torch.empty((rows, k), dtype=torch.float32, device=q.device)

    def _set_raw(self, t):
        self._raw = t
        check(self.engine.lib.lance_hip_index_set_raw(self.h, _ptr(t), t.shape[0]))

    def save(self, index_dir, loss=None):
        """HBM -> the file pair, in the layout merge_partitions writes (builder.rs:938-1079), through lance_hip_index_save."""
        torch.cuda.synchronize()
        check(self.engine.lib.lance_hip_index_save(self.engine.h, self.h, os.fspath(index_dir).encode(),
                                                   0 if loss is None else 1, 0.0 if loss is None else float(loss)))

    def close(self):
        if getattr(self, "h", None):
            self.engine.lib.lance_hip_index_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Maintainable:
    """merge / remap / split / join (lance_amd/csrc/index_update.hip): every call returns a NEW index of the same kind over the same
    model and leaves its sources as they are.  The class supplies _ctor_args(handle, centroids=None, raw=None): the constructor
    arguments of an index like this one over another handle, with other centroids and, where the kind attaches one, a raw column."""

    @classmethod
    def merge(cls, indices, raw=None):
        """For every partition the rows of indices[0], then those of indices[1], ... (lance_hip_index_merge) -> a new index; the
        sources must share the model bit for bit (centroids, codebook, quantiser bounds).  raw: the vectors for refine, indexed by
        row id, attached by IVF_PQ (the sources' attachments are not inherited); the other kinds accept and ignore it."""
        first = indices[0]
        return cls(*first._ctor_args(_merge_handles(first.engine, indices), raw=raw))

    def remap(self, old_ids, new_ids):
        """lance_hip_index_remap with a mapping already sorted by old id -> a new index"""
        return type(self)(*self._ctor_args(_remap_handle(self.engine, self.h, old_ids, new_ids)))

    def split(self, part, centroids2, raw):
        """lance_hip_index_split -> a new index with nlist + 1 partitions (c1 = centroids2[0] replaces centroid `part`, c2 is appended);
        no raw vectors attached"""
        return type(self)(*self._ctor_args(*_rebalance_handle(self.engine, self.h, self.centroids, part, raw, centroids2)))

    def join(self, part, raw):
        """lance_hip_index_join -> a new index without partition `part`: its rows go to their nearest neighbours"""
        return type(self)(*self._ctor_args(*_rebalance_handle(self.engine, self.h, self.centroids, part, raw)))


class DeviceFlatIndex(_Maintainable, _DeviceHandle):
    """Handle of a device-resident IVF_FLAT index (FlatIndex sub-index over the raw vectors of each partition)."""

    def _ctor_args(self, handle, centroids=None, raw=None):
        return self.engine, handle, self.metric, self.centroids if centroids is None else centroids, self.data_dtype

    @classmethod
    def create(cls, engine, metric, centroids, x, part_ids, row_ids=None):
        x, dt = _vec(x)
        cent = _model(centroids, x)
        part = to_device(part_ids, torch.int32)
        rid = None if row_ids is None else to_device(row_ids, torch.int64)
        n, d = x.shape
        h = C.c_void_p()
        torch.cuda.synchronize()
        check(engine.lib.lance_hip_ivfflat_create(engine.h, dt, METRICS[metric], d, _ptr(cent), cent.shape[0], _ptr(x), _ptr(part),
                                                  _ptr(rid), n, C.byref(h)))
        return cls(engine, h, metric, cent, x.dtype)

    @classmethod
    def load(cls, engine, index_dir, dtype=None):
        """IVF_FLAT index files -> HBM (lance_hip_index_load)."""
        from . import index_file
        c = index_file.read_index_files(index_dir, with_rows=False)
        if c.index_type != "IVF_FLAT":
            raise ValueError(f"{index_dir} holds an {c.index_type} index; use DeviceIndex.load")
        ddt, dt = _DT[dtype if dtype is not None else c.dtype]
        h = C.c_void_p()
        torch.cuda.synchronize()
        check(engine.lib.lance_hip_index_load(engine.h, os.fspath(index_dir).encode(), dt, C.byref(h)))
        return cls(engine, h, c.metric, to_device(c.centroids, torch.float16 if c.dtype == "float16" else torch.float32), ddt)

    def export_rows(self):
        """-> (part_offsets u32[nlist + 1], vectors f32 [n, d], row_ids u64[n]) in stored order"""
        nlist, d = self.centroids.shape
        offs, rows, _, rid = _export_rows(self.engine, self.h, nlist, 4 * d)
        return offs, rows.view(np.float32), rid

    def search(self, q, k, nprobes, allow=None, lower=None, upper=None):
        """allow: boolean array indexed by row id (a prefilter) -- tested inside the scan kernels
        (lance_hip_ivfflat_search_filtered), no filtered copy of the index.
        lower / upper: distance range -- only rows with lower <= d < upper enter the per-partition heaps (flat/index.rs:91-149),
        alone or combined with `allow` (lance_hip_ivfflat_search_range whenever either bound is given)."""
        q, _ = self._queries(q)
        ids, dists = self._outputs(q, k)
        a = _allow_bytes(allow)
        lib, args = self.engine.lib, (self.engine.h, self.h, _ptr(q), q.shape[0], k, nprobes)
        torch.cuda.synchronize()
        if lower is not None or upper is not None:
            check(lib.lance_hip_ivfflat_search_range(*args, _ptr(a), 0 if a is None else a.numel(), *_range_f32(lower, upper),
                                                     _ptr(ids), _ptr(dists)))
        elif a is not None:
            check(lib.lance_hip_ivfflat_search_filtered(*args, _ptr(a), a.numel(), _ptr(ids), _ptr(dists)))
        else:
            check(lib.lance_hip_ivfflat_search(*args, _ptr(ids), _ptr(dists)))
        return ids, dists


class _CodeIndex(_DeviceHandle):
    """The two kinds that scan quantised codes and can re-rank on the raw column: IVF_SQ and IVF_RQ."""
    _SEARCH = None      # the library's (search, search_filtered, search_refine) of the kind

    def set_raw(self, raw):
        """the column for refine_factor searches, indexed by row id, in the element type of the queries (borrowed by the handle,
        kept alive here).  For a cosine index: the ORIGINAL rows, not the normalised ones the codes were made from"""
        self._set_raw(_raw_column(raw, self.data_dtype))

    def search(self, q, k, nprobes, allow=None, refine_factor=0):
        """allow: boolean array indexed by row id (a prefilter), tested inside the scan kernels (search_filtered); for IVF_RQ every
        selected row then takes the f32 distance, as the reference's prefiltered FlatIndex::search does.
        refine_factor > 0: the k * refine_factor best by the quantised distance are re-scored against the raw vectors (set_raw) with
        the query as given and the k best by the exact distance are returned (search_refine)"""
        plain, filtered, refine = (getattr(self.engine.lib, name) for name in self._SEARCH)
        q, _ = self._queries(q)
        ids, dists = self._outputs(q, k)
        a = _allow_bytes(allow)
        args = (self.engine.h, self.h, _ptr(q), q.shape[0], k, nprobes)
        torch.cuda.synchronize()
        if refine_factor:
            check(refine(*args, refine_factor, _ptr(a), 0 if a is None else a.numel(), _ptr(ids), _ptr(dists)))
        elif a is not None:
            check(filtered(*args, _ptr(a), a.numel(), _ptr(ids), _ptr(dists)))
        else:
            check(plain(*args, _ptr(ids), _ptr(dists)))
        return ids, dists


class DeviceRqIndex(_CodeIndex):
    """Handle of a device-resident IVF_RQ index (FlatIndex sub-index over the 1-bit RaBitQ codes and factors of each partition)."""
    _SEARCH = ("lance_hip_ivfrq_search", "lance_hip_ivfrq_search_filtered", "lance_hip_ivfrq_search_refine")

    def __init__(self, engine, handle, metric, centroids, rotation):
        super().__init__(engine, handle, metric, centroids, torch.float32)
        self.rotation = rotation

    @classmethod
    def create(cls, engine, metric, centroids, rotation, codes, add, scale, part_ids, row_ids=None):
        """centroids [nlist][d] and rotation [d][d] float32; codes [n][d / 8] uint8, add / scale [n] float32 (Engine.rq_encode of the
        rows); part_ids [n] (-1 = dropped)"""
        cent, rot = _rq_f32(centroids, "centroids"), _rq_f32(rotation, "rotation")
        _rq_check(metric, cent, cent, rot)
        d = cent.shape[1]
        codes = to_device(codes, torch.uint8)
        add, scale = to_device(add, torch.float32), to_device(scale, torch.float32)
        part = to_device(part_ids, torch.int32)
        rid = None if row_ids is None else to_device(row_ids, torch.int64)
        n = codes.shape[0]
        if codes.dim() != 2 or codes.shape[1] != d // 8 or add.numel() != n or scale.numel() != n or part.numel() != n:
            raise ValueError(f"codes must be [n][{d // 8}] with add / scale / part_ids [n]")
        h = C.c_void_p()
        torch.cuda.synchronize()
        check(engine.lib.lance_hip_ivfrq_create(engine.h, METRICS[metric], d, _ptr(cent), cent.shape[0], _ptr(rot), _ptr(codes), _ptr(add),
                                                _ptr(scale), _ptr(part), _ptr(rid), n, C.byref(h)))
        return cls(engine, h, metric, cent, rot)

    def _queries(self, q):
        return _rq_f32(q, "queries").reshape(-1, self.centroids.shape[1]), q

    def save(self, index_dir, loss=None):
        raise NotImplementedError("IVF_RQ index files are not supported (IVF_PQ and IVF_FLAT are)")


class DeviceSqIndex(_Maintainable, _CodeIndex):
    """Handle of a device-resident IVF_SQ index (FlatIndex sub-index over the 8-bit scalar-quantised codes of each partition)."""
    _SEARCH = ("lance_hip_ivfsq_search", "lance_hip_ivfsq_search_filtered", "lance_hip_ivfsq_search_refine")

    def __init__(self, engine, handle, metric, centroids, data_dtype, bounds):
        super().__init__(engine, handle, metric, centroids, data_dtype)
        self.bounds = bounds

    def _ctor_args(self, handle, centroids=None, raw=None):
        return self.engine, handle, self.metric, self.centroids if centroids is None else centroids, self.data_dtype, self.bounds

    @classmethod
    def create(cls, engine, metric, centroids, codes, part_ids, bounds, row_ids=None):
        """centroids: float32 / float16 (the element type of the column and of the queries); codes [n][d] uint8 (Engine.sq_encode of
        the rows -- the NORMALISED rows for cosine); part_ids [n] (NONE = dropped)"""
        cent, dt = _sq_column(centroids)
        codes = to_device(codes, torch.uint8)
        part = to_device(part_ids, torch.int32)
        rid = None if row_ids is None else to_device(row_ids, torch.int64)
        n, d = codes.shape
        b = (C.c_double * 2)(float(bounds[0]), float(bounds[1]))
        h = C.c_void_p()
        torch.cuda.synchronize()
        check(engine.lib.lance_hip_ivfsq_create(engine.h, dt, METRICS[metric], d, _ptr(cent), cent.shape[0], _ptr(codes), _ptr(part),
                                                _ptr(rid), n, b, C.byref(h)))
        return cls(engine, h, metric, cent, cent.dtype, (float(bounds[0]), float(bounds[1])))

    def export_rows(self):
        """-> (part_offsets u32[nlist + 1], codes u8 [n, d], sums of squared codes u32[n], row_ids u64[n]) in stored order"""
        nlist, d = self.centroids.shape
        return _export_rows(self.engine, self.h, nlist, d, aux=True)

    def save(self, index_dir, loss=None):
        raise NotImplementedError("IVF_SQ index files are not supported (IVF_PQ and IVF_FLAT are)")


class DeviceIndex(_Maintainable, _DeviceHandle):
    """Handle of a device-resident IVF_PQ index (lance_hip_index)."""

    def __init__(self, engine, handle, metric, centroids, codebook, raw=None, data_dtype=None):
        super().__init__(engine, handle, metric, centroids, data_dtype if data_dtype is not None else centroids.dtype)
        self.codebook = codebook
        if raw is not None:
            self.set_raw(raw)

    def _ctor_args(self, handle, centroids=None, raw=None):
        return self.engine, handle, self.metric, self.centroids if centroids is None else centroids, self.codebook, raw, self.data_dtype

    @classmethod
    def create(cls, engine, metric, centroids, codebook, part_ids, codes, row_ids=None, raw=None, dtype=None):
        cent, dt = _vec(centroids); cb = _like(codebook, cent)
        ddt = cent.dtype
        if dtype is not None:
            ddt, dt = _DT[dtype]
        part = to_device(part_ids, torch.int32); codes = to_device(codes, torch.uint8)
        rid = None if row_ids is None else to_device(row_ids, torch.int64)
        n = part.numel()
        nlist, d = cent.shape
        m = cb.shape[0]
        h = C.c_void_p()
        torch.cuda.synchronize()
        check(engine.lib.lance_hip_index_create(engine.h, dt, METRICS[metric], d, _ptr(cent), nlist, _ptr(cb), m, _nbits(cb),
                                                _ptr(part), _ptr(codes), _ptr(rid), n, C.byref(h)))
        return cls(engine, h, metric, cent, cb, raw, ddt)

    @classmethod
    def from_storage(cls, engine, metric, centroids, codebook, part_offsets, codes, row_ids, transposed=True, raw=None, dtype=None):
        cent, dt = _vec(centroids); cb = _like(codebook, cent)
        ddt = cent.dtype
        if dtype is not None:
            ddt, dt = _DT[dtype]
        offs = np.ascontiguousarray(part_offsets, np.uint32)
        codes = to_device(np.ascontiguousarray(codes, np.uint8).reshape(-1), torch.uint8)
        rid = to_device(row_ids, torch.int64)
        nlist, d = cent.shape
        m = cb.shape[0]
        n = rid.numel()
        h = C.c_void_p()
        torch.cuda.synchronize()
        check(engine.lib.lance_hip_index_from_storage(engine.h, dt, METRICS[metric], d, _ptr(cent), nlist, _ptr(cb), m, _nbits(cb),
                                                      offs.ctypes.data_as(C.c_void_p), _ptr(codes), int(transposed), _ptr(rid), n,
                                                      C.byref(h)))
        return cls(engine, h, metric, cent, cb, raw, ddt)

    @classmethod
    def load(cls, engine, index_dir, dtype=None, raw=None, lists=None):
        """`<index_dir>/index.idx` + `auxiliary.idx` (an IVF_PQ index the reference wrote, or `save`) -> HBM, through
        lance_hip_index_load.  dtype: element type of the indexed column ("float32" | "float16" | "int8"); default = the
        element type of the stored tensors.  lists = (world, rank): only the IVF lists p with p % world == rank."""
        from . import index_file
        c = index_file.read_index_files(index_dir, with_rows=False)
        if c.index_type != "IVF_PQ":
            raise ValueError(f"{index_dir} holds an {c.index_type} index; use DeviceFlatIndex.load")
        ddt, dt = _DT[dtype if dtype is not None else c.dtype]
        mdt = torch.float16 if c.dtype == "float16" else torch.float32
        h = C.c_void_p()
        torch.cuda.synchronize()
        mod, rem = (1, 0) if lists is None else (int(lists[0]), int(lists[1]))
        check(engine.lib.lance_hip_index_load_lists(engine.h, os.fspath(index_dir).encode(), dt, mod, rem, C.byref(h)))
        return cls(engine, h, c.metric, to_device(c.centroids, mdt), to_device(c.codebook, mdt), raw, ddt)

    def remap(self, old_ids, new_ids, raw=None):
        """as the other kinds' remap; raw: the vectors for refine, attached to the new index"""
        out = super().remap(old_ids, new_ids)
        if raw is not None:
            out.set_raw(raw)
        return out

    def export_rows(self):
        """-> (part_offsets u32[nlist + 1], codes u8 [n, code bytes] row-major, row_ids u64[n]) in stored order"""
        m = self.codebook.shape[0]
        offs, rows, _, rid = _export_rows(self.engine, self.h, self.centroids.shape[0], m if _nbits(self.codebook) == 8 else m // 2)
        return offs, rows, rid

    def set_raw(self, raw):
        t = raw if isinstance(raw, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(raw))
        self._set_raw(t.to(self.data_dtype).to(_dev()).contiguous())         # (any shape: the library takes the row count)

    def prewarm(self):
        """Index::prewarm (ivf/v2.rs:349-352, dataset.py prewarm_index): build the per-index search constants now."""
        check(self.engine.lib.lance_hip_index_prewarm(self.engine.h, self.h))

    def info(self):
        n = C.c_uint64(); nlist = C.c_uint32(); m = C.c_uint32(); d = C.c_uint32()
        check(self.engine.lib.lance_hip_index_info(self.h, C.byref(n), C.byref(nlist), C.byref(m), C.byref(d)))
        return {"n": n.value, "nlist": nlist.value, "m": m.value, "d": d.value}

    def export(self):
        """-> (part_offsets u32[nlist+1], codes_transposed u8 (per-partition [m][n_p] blocks), row_ids u64[n])"""
        inf = self.info()
        offs = np.empty(inf["nlist"] + 1, np.uint32)
        mb = inf["m"] if _nbits(self.codebook) == 8 else inf["m"] // 2
        codes = np.empty(inf["n"] * mb, np.uint8)
        rid = np.empty(inf["n"], np.uint64)
        check(self.engine.lib.lance_hip_index_export(self.engine.h, self.h, offs.ctypes.data_as(C.c_void_p),
                                                     codes.ctypes.data_as(C.c_void_p), rid.ctypes.data_as(C.c_void_p)))
        return offs, codes, rid

    def part_offsets(self):
        """-> part_offsets u32[nlist+1] alone (no copy of the codes or row ids to the host: at a billion rows those are 40 GB)"""
        inf = self.info()
        offs = np.empty(inf["nlist"] + 1, np.uint32)
        check(self.engine.lib.lance_hip_index_export(self.engine.h, self.h, offs.ctypes.data_as(C.c_void_p), None, None))
        return offs

    MAX_PAIRS_PER_CALL = 1_500_000      # (query, probe) pairs per library call of a synchronous search (256 survivor slots x 8 B each)

    def search(self, q, k, nprobes, refine_factor=0, out=None, sync=True, engine=None):
        """engine: another Engine (own stream + scratch arena) on the same GPU to run this batch on -- the index is read-only
        during searches, so batches enqueued through different engines overlap on the device (sync=False)."""
        q, t = self._queries(q)
        nq = q.shape[0]
        ids, dists = self._outputs(q, k, out)
        eng = engine if engine is not None else self.engine
        fn = eng.lib.lance_hip_ivfpq_search if sync else eng.lib.lance_hip_ivfpq_search_async
        if sync and nq > 1 and nq * max(1, nprobes) > self.MAX_PAIRS_PER_CALL:
            # a batch whose survivor segments would not fit the library's 2 GiB scratch limit leaves the batched kernels for the
            # query-major ones (correct, many times slower): queries are independent, so the batch goes through in slices
            step = max(1, self.MAX_PAIRS_PER_CALL // max(1, nprobes))
            _torch_inputs_ready()
            for a in range(0, nq, step):
                b = min(nq, a + step)
                check(fn(eng.h, self.h, _ptr(q[a:b]), b - a, k, nprobes, refine_factor, _ptr(ids[a:b]), _ptr(dists[a:b])))
            return ids, dists
        if sync or (not eng.use_torch_stream and (q.data_ptr() != t.data_ptr() or out is None)):
            # asynchronous: only when the batch was converted / moved / allocated by torch kernels on torch's stream -- they must
            # finish before the engine's own stream reads them.  reshape() always makes a new tensor OBJECT, so the test is on the
            # storage: a caller that hands over ready device tensors of the index's element type (and `out`) pays nothing
            _torch_inputs_ready()
        check(fn(eng.h, self.h, _ptr(q), nq, k, nprobes, refine_factor, _ptr(ids), _ptr(dists)))
        return ids, dists

    def search_filtered(self, q, k, nprobes, allow, refine_factor=0, out=None):
        """Search under a row-id prefilter (lance_hip_ivfpq_search_filtered): `allow` = boolean array indexed by row id.  The
        mask is tested inside the scan kernels; no filtered copy of the index is built.  out = (ids, dists) device tensors to
        write into (a caller that keeps its query / output buffers gets the captured-graph path from its second call)."""
        q, _ = self._queries(q)
        a = _allow_bytes(allow)
        ids, dists = self._outputs(q, k, out)
        _torch_inputs_ready()
        check(self.engine.lib.lance_hip_ivfpq_search_filtered(self.engine.h, self.h, _ptr(q), q.shape[0], k, nprobes, refine_factor, _ptr(a),
                                                              a.numel(), _ptr(ids), _ptr(dists)))
        return ids, dists

    def multivec_search(self, q, q_offsets, k, nprobes, overfetch=10, k_out=None, allow=None):
        """ANN search of a multivector column through THIS index over its flattened vectors (row ids repeated per vector), for a
        batch of B multivector queries: q [sum nqv][d], the vectors of query b are rows q_offsets[b] .. q_offsets[b + 1] - 1.  One
        IVF_PQ search of all query vectors with k = k * overfetch, then the join by row id (lance_hip_ivfpq_multivec_search).
        allow: boolean array indexed by row id (the prefilter).  -> (ids [B][k_out] int64 (-1 = none), distances [B][k_out]),
        k_out = k by default"""
        off = check_query_offsets(q_offsets)
        B = off.size - 1
        k_out = int(k if k_out is None else k_out)
        if int(k) < 1 or int(overfetch) < 1:
            raise ValueError(f"k={k}, overfetch={overfetch}: both must be at least 1")
        check_multivector_ann_sizes(int(k) * int(overfetch), k_out)
        q, _ = self._queries(q)
        if q.shape[0] != int(off[-1]):
            raise ValueError(f"q holds {q.shape[0]} vectors, q_offsets end at {int(off[-1])}")
        a = _allow_bytes(allow)
        ids, dists = self._outputs(q, k_out, rows=B)
        _torch_inputs_ready()
        check(self.engine.lib.lance_hip_ivfpq_multivec_search(self.engine.h, self.h, _ptr(q), off.ctypes.data_as(C.c_void_p), B, int(k),
                                                              min(int(nprobes), self.centroids.shape[0]), int(overfetch), k_out, _ptr(a),
                                                              0 if a is None else a.numel(), _ptr(ids), _ptr(dists)))
        return ids, dists

    def search_candidates(self, q, keff, nprobes, exact=True, engine=None):
        """ONE scan -> (ids [nq, keff] int64 (-1 = none), PQ distances, exact distances or None): the keff nearest rows by PQ distance in
        (dist, rowid) order and, aligned with them, each one's exact distance to the query (lance_hip_ivfpq_search_candidates) -- the
        local half of a list-sharded search with refine (lance_amd/dist.py: search_list_sharded)."""
        eng = engine or self.engine
        q, _ = self._queries(q)
        ids, pq = self._outputs(q, keff)
        ex = torch.empty_like(pq) if exact else None
        _torch_inputs_ready()
        check(eng.lib.lance_hip_ivfpq_search_candidates(eng.h, self.h, _ptr(q), q.shape[0], keff, min(nprobes, self.centroids.shape[0]),
                                                        _ptr(ids), _ptr(pq), _ptr(ex)))
        return ids, pq, ex

    def search_range(self, q, k, nprobes, lower=None, upper=None, refine_factor=0, allow=None, out=None):
        """Distance-range query: only rows with lower <= d < upper (ADC distance) enter the per-partition heaps.  With a
        refine factor the reference also filters the exact distances before the final fetch (scanner.rs:3334-3377): all
        k * refine_factor candidates come back re-ranked from the device and the range is applied to them here.
        allow: boolean array indexed by row id -- the range combined with a row-id prefilter, tested inside the scan
        kernels (lance_hip_ivfpq_search_filtered_range; flat/index.rs:131-149)."""
        lo, hi = _range_f32(lower, upper)
        if refine_factor and refine_factor > 0:
            keff = k * refine_factor
            ci, cd = self.search_range(q, keff, nprobes, lower, upper, refine_factor=-1, allow=allow)       # -1: re-rank, keep all
            ok = (ci >= 0) & (cd >= lo) & (cd < hi)
            # first k in-range entries of every row, order kept (the device returned them sorted by (distance, row id))
            rank = torch.cumsum(ok.to(torch.int64), dim=1) - 1
            ids = torch.full((ci.shape[0], k), -1, dtype=torch.int64, device=ci.device)
            dists = torch.full((ci.shape[0], k), float("inf"), dtype=torch.float32, device=ci.device)
            take = ok & (rank < k)
            rows = torch.arange(ci.shape[0], device=ci.device).unsqueeze(1).expand_as(ci)
            ids[rows[take], rank[take]] = ci[take]
            dists[rows[take], rank[take]] = cd[take]
            return ids, dists
        q, _ = self._queries(q)
        ids, dists = self._outputs(q, k, out)
        a = _allow_bytes(allow)
        args = (self.engine.h, self.h, _ptr(q), q.shape[0], k, nprobes, 1 if refine_factor == -1 else 0)
        _torch_inputs_ready()
        if a is not None:
            check(self.engine.lib.lance_hip_ivfpq_search_filtered_range(*args, _ptr(a), a.numel(), lo, hi, _ptr(ids), _ptr(dists)))
        else:
            check(self.engine.lib.lance_hip_ivfpq_search_range(*args, lo, hi, _ptr(ids), _ptr(dists)))
        return ids, dists


_wrap_methods(_DeviceHandle, skip=("close",))       # (_wrap_methods sees a class's own methods only: the bases are wrapped here)
_wrap_methods(_Maintainable)
_wrap_methods(_CodeIndex)
_wrap_methods(DeviceFlatIndex)
_wrap_methods(DeviceSqIndex, skip=("save",))
_wrap_methods(DeviceRqIndex, skip=("save",))
_wrap_methods(DeviceIndex)
