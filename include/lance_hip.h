/*
 * lance_hip.h -- C ABI of liblance_hip.so: the MI355X (gfx950) engine for Lance's
 * IVF-PQ hot path (k-means training, PQ codebook learning/encoding, flat and IVF-PQ
 * distance scans with top-k).
 *
 * This is the drop-in boundary: a Rust `extern "C"` block (or JNI / ctypes) binds
 * exactly these symbols; INTEGRATION.md shows the reference-side call sites.
 * Every entry point cites the reference interface it replaces (paths relative to the
 * lancedb/lance tree).
 *
 * Conventions
 *   - Plain C types only.  All data pointers are DEVICE pointers (HBM) unless the
 *     parameter name ends in `_host`; buffers are caller-owned, row-major, and no
 *     allocation crosses the ABI except opaque handles.  lance_hip_malloc/free/memcpy
 *     are provided so a host without its own HIP binding can stage data.
 *   - Alignment: a data pointer needs the alignment of its ELEMENT and no more (4 bytes for f32 /
 *     u32 / f32 outputs, 2 for f16, 1 for int8 and code bytes, 8 for u64 row ids): a slice of an
 *     Arrow FixedSizeList column that starts at any row is a valid argument, inputs and outputs
 *     alike.  16-byte alignment only selects faster kernels (vector loads, the matrix-core
 *     routes); an operand off that grid is served by kernels that read element by element, with
 *     the same bits in every result ("Pointer alignment"; tests/test_zz_gpu_unaligned.py).
 *     One entry point refuses instead of falling back: lance_hip_rq_distance with d % 128 == 0
 *     (code rows of whole 16-byte words) answers LANCE_HIP_EINVAL unless `codes` is 16-byte aligned.
 *   - Return 0 on success, a negative LANCE_HIP_E* code on failure; the message is
 *     available from lance_hip_last_error() (thread-local).  Never throws or aborts.
 *   - Work is issued on the context's stream; calls return after the stream has been
 *     synchronised unless stated otherwise.
 *   - Threads (the reference calls these paths from rayon / tokio worker threads,
 *     rust/lance/src/index/vector/ivf/v2.rs:232-306): every entry point is re-entrant.  A
 *     context is a stream + scratch arena; its entry points hold a per-context lock, so
 *     threads sharing one context take turns, and threads with a context each overlap on
 *     the device.  An index is read-only during searches and may be searched through any
 *     number of contexts at once (tests/test_zz_gpu_threads.py); building / destroying it
 *     while it is being searched is the caller's error.  lance_hip_last_error() is
 *     thread-local.  A context's own stream is non-blocking (no implicit ordering against the
 *     legacy default stream).  While one thread's repeated search is being captured into a HIP
 *     graph (its second call with the same arguments), a DEVICE-WIDE synchronise from another
 *     thread (hipDeviceSynchronize, torch.cuda.synchronize()) is refused by the runtime and
 *     invalidates that capture: the library then runs the batch on the plain path, but the
 *     synchronising thread sees the runtime's error.  Hosts that search from several threads
 *     wait on streams or events, not on the device (lance_amd/engine.py does), or set
 *     LANCE_HIP_GRAPH=0.
 *   - "No partition" (all-NaN row; kmeans.rs:1447-1486) is id 0xFFFFFFFF.
 *   - Results are bit-identical to the reference CPU path for ids / codes / distances
 *     (see DESIGN.md for the exact statement and the two documented tie rules).
 */
#ifndef LANCE_HIP_H
#define LANCE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LANCE_HIP_OK 0
#define LANCE_HIP_EINVAL -1    /* bad argument */
#define LANCE_HIP_ERUNTIME -2  /* HIP runtime error */
#define LANCE_HIP_ENOTSUP -3   /* combination not implemented */
#define LANCE_HIP_ENOMEM -4
#define LANCE_HIP_EIO -5       /* file cannot be opened / read / written */

#define LANCE_HIP_NONE 0xFFFFFFFFu

/* lance_linalg::distance::DistanceType (distance.rs:36).  Cosine is handled the way
 * the reference index does: normalise, then L2 (lance-index ivf.rs:198-205).        */
enum { LANCE_HIP_L2 = 0, LANCE_HIP_COSINE = 1, LANCE_HIP_DOT = 2 };
/* element type of vectors / centroids / codebook.
 * LANCE_HIP_I8: the DATA operands (vectors x, queries q, raw vectors for refine) are int8 and are widened to
 * f32 exactly, as the reference does for Int8 columns (kmeans.rs:1216-1224 convert_to_floating_point,
 * l2.rs:253-260); the MODEL operands (centroids, codebook, init centroids, residual query, every output) are f32. */
enum { LANCE_HIP_F32 = 0, LANCE_HIP_F16 = 1, LANCE_HIP_I8 = 2 };

typedef struct lance_hip_ctx lance_hip_ctx;
typedef struct lance_hip_index lance_hip_index;

/* ---- context ------------------------------------------------------------------ */
/* stream == NULL: the context creates and owns a stream; otherwise it borrows the
 * caller's hipStream_t (e.g. torch's current stream).                               */
int lance_hip_ctx_create(int device_id, void *stream, lance_hip_ctx **out);
void lance_hip_ctx_destroy(lance_hip_ctx *ctx);
const char *lance_hip_last_error(void);
const char *lance_hip_version(void);
int lance_hip_synchronize(lance_hip_ctx *ctx);

int lance_hip_malloc(lance_hip_ctx *ctx, size_t bytes, void **out);
int lance_hip_free(lance_hip_ctx *ctx, void *ptr);
int lance_hip_memcpy_h2d(lance_hip_ctx *ctx, void *dst, const void *src_host, size_t bytes);
int lance_hip_memcpy_d2h(lance_hip_ctx *ctx, void *dst_host, const void *src, size_t bytes);

/* ---- a4: normalize_fsl (lance-linalg kernels.rs:141-146,172-211) ---------------- */
int lance_hip_normalize(lance_hip_ctx *ctx, int dtype, const void *x, uint64_t n, uint32_t d, void *out);

/* ---- a5/a6/a9: argmin over centroids ------------------------------------------- */
/* KMeansAlgoFloat::compute_membership_and_dist (lance-index kmeans.rs:317-369),
 * compute_partitions_arrow_array (:1187-1246), compute_partition (:1350-1369) with
 * argmin_value_float[_with_bias] (lance-linalg kernels.rs:79-111).
 * bias: k floats added before the comparison (un-biased distance returned) or NULL.
 * ids: n (LANCE_HIP_NONE = None); dists: n or NULL.                                  */
int lance_hip_assign(lance_hip_ctx *ctx, int dtype, int metric, const void *x, uint64_t n, uint32_t d,
                     const void *centroids, uint32_t k, const float *bias, uint32_t *ids, float *dists);

/* ---- a7/a8: KMeans::train_kmeans (kmeans.rs:610-719) ---------------------------- */
/* Lloyd iterations on exactly the n rows given (the caller applies the sample_rate*k
 * slice of kmeans.rs:1328-1340; the k*512 cap of :623-627 is applied here).
 * balance_factor is the caller's value (1.0 for IVF, ivf.rs:1859); it is divided by n
 * as train_kmeans does (:1344).  init_centroids: k*d or NULL (random rows from `seed`,
 * kmeans_random_init :149-170).  Given the same inputs, init and seed the centroids,
 * loss and iteration count are bit-identical to the reference algorithm (M-step sums
 * are accumulated per centroid in row order, :371-446).  As in the reference, k > 256
 * takes the hierarchical path (see lance_hip_kmeans_train_ex).                          */
int lance_hip_kmeans_train(lance_hip_ctx *ctx, int dtype, int metric, const void *x, uint64_t n, uint32_t d,
                           uint32_t k, uint32_t max_iters, double tol, float balance_factor,
                           const void *init_centroids, uint64_t seed, void *centroids_out,
                           double *loss_out_host, uint32_t *iters_out_host);

/* KMeans::new_with_params (kmeans.rs:1008-1073) with every KMeansParams field: k > 256 and
 * hierarchical_k > 1 selects train_hierarchical_kmeans (:746-1003; init centroids unused, loss 0,
 * *k_out_host = clusters produced, normally k).  lance_hip_kmeans_train == hierarchical_k 16.  */
int lance_hip_kmeans_train_ex(lance_hip_ctx *ctx, int dtype, int metric, const void *x, uint64_t n, uint32_t d,
                              uint32_t k, uint32_t max_iters, double tol, float balance_factor,
                              uint32_t hierarchical_k, const void *init_centroids, uint64_t seed,
                              void *centroids_out, double *loss_out_host, uint32_t *iters_out_host,
                              uint32_t *k_out_host);

/* Building blocks of one Lloyd iteration, for a host that owns the loop (multi-GPU:
 * one process per GPU, rows sharded, one all-reduce per iteration).
 * estep_partial assigns the LOCAL rows and accumulates, per centroid and in local row
 * order: buf = [k*d sums | k counts] as f32 (one all-reduce(sum) buffer), and optionally
 * losses[k] (f64, all-reduce sum) and radius[k] (f32, all-reduce max) -- the inputs of
 * compute_cluster_sizes / compute_balance_loss (kmeans.rs:210-237).                     */
int lance_hip_kmeans_estep_partial(lance_hip_ctx *ctx, int dtype, int metric, const void *x, uint64_t n,
                                   uint32_t d, const void *centroids, uint32_t k, const float *bias,
                                   float *buf /* k*d + k */, double *losses /* k or NULL */,
                                   float *radius /* k or NULL */, double *loss_out_host);
/* finalize: centroids = sums * (1/count) for count > 0 (kmeans.rs:410-418). */
int lance_hip_kmeans_finalize(lance_hip_ctx *ctx, int dtype, const float *buf, uint32_t k, uint32_t d,
                              void *centroids_out);

/* One split of the hierarchical trainer -- train_hierarchical_kmeans, kmeans.rs:746-1003: k-means with k centroids over the rows
 * `rows_host` (n_rows indices into x, ascending; NULL = all rows: the first level) of the training sample x [n][d] (device, f32 values;
 * dtype = the COLUMN's type: LANCE_HIP_F16 says the values are binary16-representable -- widened once by the caller -- and the M-step
 * rounds like half::f16, as the single-GPU trainer of an f16 column does), then the membership of those rows
 * (kmeans.rs:866-905).  balance_factor_scaled is the factor ALREADY divided by the sample size (train_kmeans :1344 divides once, by the
 * whole sample, and every split inherits it); seed = the run's seed (the trainer uses seed + number of k-means runs so far).  Outputs on
 * the host: centroids [k][d] f32, membership [n_rows] (LANCE_HIP_NONE: no centroid).
 * This is the unit of work of the multi-GPU hierarchical trainer (lance_amd/dist.py train_kmeans_hierarchical_sharded, SURVEY 8(e);
 * BASELINE config 5: nlist 65,536): every rank holds the sample, the splits of the largest clusters are computed on different ranks at
 * the same time and applied in the reference's order -- the result is the single-GPU trainer's bit for bit.                         */
int lance_hip_kmeans_split(lance_hip_ctx *ctx, int dtype, int metric, const float *x, uint64_t n, uint32_t d, const uint32_t *rows_host,
                           uint64_t n_rows, uint32_t k, uint32_t max_iters, double tol, float balance_factor_scaled, uint64_t seed,
                           float *centroids_out_host, uint32_t *membership_out_host);

/* Row-sharded Lloyd iteration WITHOUT host round trips (multi-GPU build).  Per iteration the caller enqueues, on
 * the stream the context was created on (e.g. torch's current stream, so that RCCL collectives are ordered with it):
 *   shard_estep  -- local E-step + local partials: buf = [k*d sums | k counts] (f32), losses [k] (f64), radius [k] (f32);
 *   all-reduce SUM of buf and of losses, all-reduce MAX of radius (the caller's collective library);
 *   shard_update -- on the reduced numbers: centroids = sums / counts, loss, balance-factor update, convergence test,
 *                   empty-cluster split (RNG seeded identically on every rank), bias of the next iteration.
 * `state` is an opaque device block of LANCE_HIP_KMEANS_SHARD_STATE_BYTES bytes; `bias` k device floats.  Once the run has
 * converged the state turns inactive: further estep / update calls leave every buffer untouched.  shard_end synchronises and
 * reports (loss, iterations, still active).  Reference loop: KMeans::train_kmeans, kmeans.rs:610-719.                     */
#define LANCE_HIP_KMEANS_SHARD_STATE_BYTES 128
/* The k row indices kmeans_random_init draws (kmeans.rs:149-170: k distinct rows; here the engine's seeded reservoir so that
 * seeded runs are reproducible -- the reference seeds from the OS).  Host-only helper for callers that gather the initial
 * centroids themselves (the sharded trainer: rank 0 draws from its rows and broadcasts).                                */
int lance_hip_kmeans_init_indices(uint64_t n, uint32_t k, uint64_t seed, uint64_t *out_host);
int lance_hip_kmeans_shard_begin(lance_hip_ctx *ctx, uint32_t k, float balance_factor_scaled, uint64_t seed, void *state, float *bias);
int lance_hip_kmeans_shard_estep(lance_hip_ctx *ctx, int metric, const float *x, uint64_t n, uint32_t d, const float *centroids, uint32_t k,
                                 const float *bias, const void *state, float *buf, double *losses, float *radius);
/* the same E-step on a shard in the column's own element type (dtype: f32 / f16 / int8 -- widened exactly inside; VERDICT r05: the f32-only
 * entry points made the host widen f16 / int8 shards) */
int lance_hip_kmeans_shard_estep_x(lance_hip_ctx *ctx, int dtype, int metric, const void *x, uint64_t n, uint32_t d, const float *centroids, uint32_t k,
                                   const float *bias, const void *state, float *buf, double *losses, float *radius);
int lance_hip_kmeans_shard_update(lance_hip_ctx *ctx, void *state, const float *buf, const double *losses, const float *radius,
                                  float *centroids, float *bias, uint32_t k, uint32_t d, uint64_t n_total, float balance_factor_scaled,
                                  double tol, uint32_t it);
int lance_hip_kmeans_shard_end(lance_hip_ctx *ctx, const void *state, double *loss_host, uint32_t *iters_host, int *active_host);

/* ---- the same loop with its collectives behind the ABI (RCCL over xGMI) ----------------------------------------
 * For hosts without torch.distributed.  One process per GPU; rank 0 draws an id (lance_hip_comm_unique_id, 128 bytes = an
 * ncclUniqueId), ships it to the other ranks by whatever channel the host has, every rank calls lance_hip_comm_create on its own
 * context -- or lance_hip_comm_adopt wraps an ncclComm_t the host already owns (it stays the host's to destroy).
 * lance_hip_kmeans_train_sharded runs KMeans::train_kmeans (kmeans.rs:610-719) over rows sharded across the ranks: per Lloyd
 * iteration a local E-step + partial sums, ONE ncclAllReduce(sum) of the fused f32 buffer [k*d sums | k counts] (129 KiB at
 * nlist 256, d 128), one of the k f64 losses and one max-reduce of the k radii, then the update kernel -- all enqueued on the
 * context's stream; the host reads the state every 8 iterations.  `centroids` holds the initial centroids (identical on every
 * rank: e.g. rank 0's kmeans_random_init rows, broadcast by the host) and receives the trained ones (identical on every rank).
 * comm == NULL: single process, no collective.  balance_factor is the unscaled parameter (divided by n_total as train_kmeans does).
 * Each rank adds its rows in row order and the partials arrive in rank order: against the single-GPU trainer the centroids are bit for
 * bit the same on one rank and wherever the sums are exact (integer-valued rows), and differ by f32 summation order otherwise; among
 * clusters that tie for largest the update takes the smallest id (the reference: the one whose last member comes first), which shows
 * only when such a tie happens while the adjusted balance factor binds.  An RCCL the process already maps answers; otherwise librccl.so.1 is loaded on first use.
 * Whatever can fail on one rank only (its row count, scratch, the f32 copy of an f16 / int8 shard, its first E-step) is exchanged as one
 * status word before the first all-reduce of the loop: every rank returns.                                                          */
typedef struct lance_hip_comm lance_hip_comm;
int lance_hip_comm_unique_id(char *id_out_host /* 128 bytes */);
int lance_hip_comm_create(lance_hip_ctx *ctx, const char *id_host /* 128 bytes */, int nranks, int rank, lance_hip_comm **out);
int lance_hip_comm_adopt(void *nccl_comm, int nranks, int rank, lance_hip_comm **out);
/* A host with its own transport (MPI, gloo, ...) hands over an in-place all-reduce instead of an RCCL communicator: `buf` is a DEVICE
 * pointer holding `count` elements (LANCE_HIP_COMM_F32 / _F64), `op` LANCE_HIP_COMM_SUM / _MAX, `stream` the hipStream_t the producing
 * kernels were enqueued on and the consuming ones will be (the callback must order itself against it -- e.g. synchronise it, reduce
 * through host memory, copy back -- and return 0, or non-zero to abort the training on this rank).  lance_hip_kmeans_train_sharded
 * issues the same exchanges through it as through RCCL (rust/lance-index/src/vector/kmeans.rs:610-719: the rayon reduction's place). */
enum { LANCE_HIP_COMM_F32 = 0, LANCE_HIP_COMM_F64 = 1 };
enum { LANCE_HIP_COMM_SUM = 0, LANCE_HIP_COMM_MAX = 1 };
typedef int (*lance_hip_allreduce_fn)(void *user, void *buf, uint64_t count, int dtype, int op, void *stream);
int lance_hip_comm_from_callback(lance_hip_allreduce_fn fn, void *user, int nranks, int rank, lance_hip_comm **out);
void lance_hip_comm_destroy(lance_hip_comm *comm);
int lance_hip_kmeans_train_sharded(lance_hip_ctx *ctx, lance_hip_comm *comm, int metric, const float *x_local, uint64_t n_local, uint32_t d,
                                   uint32_t k, uint64_t n_total, uint32_t max_iters, double tol, float balance_factor, uint64_t seed,
                                   float *centroids, double *loss_out_host, uint32_t *iters_out_host);

/* ... and on a shard in the column's own element type (f32 / f16 / int8; the shard is widened once, inside, for the whole loop) */
int lance_hip_kmeans_train_sharded_x(lance_hip_ctx *ctx, lance_hip_comm *comm, int dtype, int metric, const void *x_local, uint64_t n_local, uint32_t d,
                                     uint32_t k, uint64_t n_total, uint32_t max_iters, double tol, float balance_factor, uint64_t seed,
                                     float *centroids, double *loss_out_host, uint32_t *iters_out_host);

/* ---- a11: PQBuildParams::build_from_fsl (pq/builder.rs:89-157) ------------------- */
/* M independent k-means (k = 2^nbits, L2, no balance) over the sub-vector columns of
 * `residuals`; sub-quantiser m uses seed + m.  codebook_out: [m][2^nbits][d/m].      */
int lance_hip_pq_train(lance_hip_ctx *ctx, int dtype, const void *residuals, uint64_t n, uint32_t d,
                       uint32_t m, uint32_t nbits, uint32_t max_iters, uint32_t sample_rate, uint64_t seed,
                       void *codebook_out, uint32_t *iters_out_host /* m or NULL */);

/* ---- a10: do_compute_residual (residual.rs:58-102) ------------------------------- */
int lance_hip_residual(lance_hip_ctx *ctx, int dtype, const void *x, uint64_t n, uint32_t d,
                       const void *centroids, const uint32_t *part_ids, void *out);

/* ---- a12: ProductQuantizer::transform_impl (pq.rs:116-191) ----------------------- */
/* codes: [n][m] (nbits = 8) or [n][m/2] (nbits = 4).  `metric` is the QUANTIZER's distance type (pq.rs:143): a quantizer
 * produced by an index build is always an L2 one (lance/src/index/vector/builder.rs:456), whatever the index metric. */
int lance_hip_pq_encode(lance_hip_ctx *ctx, int dtype, int metric, const void *x, uint64_t n, uint32_t d,
                        const void *codebook, uint32_t m, uint32_t nbits, uint8_t *codes);

/* ---- a9+a10+a12: the IvfTransformer chain for one batch (lance-index ivf.rs:188-236;
 * precedent: one_pass_assign_ivf_pq_on_accelerator, python/lance/vector.py:607-755) --- */
/* [cosine: normalise] -> assign -> residual (L2/cosine) -> PQ encode.  Emits the
 * shuffle-buffer columns (__ivf_part_id u32, __pq_code u8[m]).  Non-finite rows get
 * part id LANCE_HIP_NONE (KeepFiniteVectors, utils.rs:263-286).  `metric` is the INDEX metric: it selects the
 * partition assignment (dot indices assign by dot product and take no residual); the PQ step always encodes with the
 * L2-nearest codeword, as the reference's build does (builder.rs:456 + pq.rs:143,165).   */
int lance_hip_ivfpq_encode(lance_hip_ctx *ctx, int dtype, int metric, const void *x, uint64_t n, uint32_t d,
                           const void *centroids, uint32_t nlist, const void *codebook, uint32_t m,
                           uint32_t nbits, uint32_t *part_ids, uint8_t *codes, double *loss_out_host);

/* ---- a13 + builder.rs:685-846: per-partition storage ------------------------------ */
/* Builds a device-resident index from the shuffle-buffer columns: rows are grouped by
 * partition in ascending input order (stable), rows with part id NONE are dropped.
 * row_ids: n u64 labels or NULL (row i gets id i).  The index keeps its own copies.   */
int lance_hip_index_create(lance_hip_ctx *ctx, int dtype, int metric, uint32_t d, const void *centroids,
                           uint32_t nlist, const void *codebook, uint32_t m, uint32_t nbits,
                           const uint32_t *part_ids, const uint8_t *codes, const uint64_t *row_ids, uint64_t n,
                           lance_hip_index **out);
/* Same, from the reference's on-disk/storage layout (pq/storage.rs:183-290): rows
 * already grouped by partition (part_offsets_host[nlist+1]) and each partition's codes
 * transposed to [m][n_p] (transposed != 0) or row-major.                              */
int lance_hip_index_from_storage(lance_hip_ctx *ctx, int dtype, int metric, uint32_t d, const void *centroids,
                                 uint32_t nlist, const void *codebook, uint32_t m, uint32_t nbits,
                                 const uint32_t *part_offsets_host, const uint8_t *codes, int transposed,
                                 const uint64_t *row_ids, uint64_t n, lance_hip_index **out);
void lance_hip_index_destroy(lance_hip_index *idx);
/* Optional raw vectors for refine (scanner.rs:2884-2904 `take` + flat_knn): x[n_raw][d],
 * indexed by row id (row id r -> x[r]); the element type is the handle's dtype (IVF_PQ,
 * IVF_SQ: the column's; IVF_RQ: f32).  IVF_SQ and IVF_RQ handles take them too (for
 * lance_hip_ivfsq_search_refine / lance_hip_ivfrq_search_refine); for a cosine IVF_SQ index
 * they are the ORIGINAL rows, not the normalised ones.  Borrowed, must outlive the index and must not
 * change while attached: the engine may keep a lossless compact copy of it (an f32 column
 * whose every element is an integer in [0, 255] is read as bytes by the refine kernel) and
 * captured searches hold its address.  After changing the contents call set_raw again
 * (same pointer allowed): it drops the copy and invalidates the captured searches.       */
int lance_hip_index_set_raw(lance_hip_index *idx, const void *x, uint64_t n_raw);
/* Index::prewarm (rust/lance/src/index/vector/ivf/v2.rs:349-352, python dataset.py:2991 prewarm_index): builds NOW, on ctx's
 * stream, the per-index search constants the first search would otherwise build (the matrix-core scan's f16 codebook and row norms;
 * the lossless u8 refine copy of an integer-valued f32 raw column).  Optional: results never depend on it, only the first search's
 * latency does.  Synchronises the stream.                                                                                        */
int lance_hip_index_prewarm(lance_hip_ctx *ctx, lance_hip_index *idx);
int lance_hip_index_info(const lance_hip_index *idx, uint64_t *n_rows, uint32_t *nlist, uint32_t *m, uint32_t *d);
/* Copies out the storage layout (host pointers, any may be NULL): part_offsets[nlist+1],
 * codes transposed per partition (the reference layout), row ids in partition order. */
int lance_hip_index_export(lance_hip_ctx *ctx, const lance_hip_index *idx, uint32_t *part_offsets_host,
                           uint8_t *codes_transposed_host, uint64_t *row_ids_host);

/* ---- index maintenance: append / merge, remap / delete, row-major read side ------------------------------------------------
 * optimize_indices (rust/lance/src/index/vector/ivf.rs:355-560; builder.rs:685-935 take_partition_batches + StorageBuilder::build)
 * and remap (builder.rs:256-359, pq/storage.rs:499-560, quantizer.rs:244-280) for IVF_PQ (8- and 4-bit), IVF_FLAT and IVF_SQ
 * handles.  A source is never modified: every call returns a NEW handle (own copy of the model, no raw vectors attached -- see
 * lance_hip_index_set_raw), destroyed with lance_hip_index_destroy.  The rows move HBM -> HBM; until the caller destroys the
 * sources, sources and result are resident together.  These calls neither split a partition (builder.rs:1152-1176) nor join one
 * (:1343-1400): lance_hip_index_split / lance_hip_index_join below do, on the handle a merge returns / ahead of a remap.          */
/* new_ids[i] of lance_hip_index_remap: the row is deleted.  (The same value marks a missing result id in the search outputs.) */
#define LANCE_HIP_ROW_DELETED 0xFFFFFFFFFFFFFFFFull
/* For every partition: the rows of srcs[0] in stored order, then those of srcs[1], ...  1 <= n_srcs <= 64.  The sources must agree
 * on kind, metric, dtype, d, nlist, m, nbits and (IVF_SQ) bounds, and carry bitwise equal centroids and codebook: otherwise
 * LANCE_HIP_EINVAL, the message naming the first field that differs.  Fewer than 2^32 rows in all.                                */
int lance_hip_index_merge(lance_hip_ctx *ctx, const lance_hip_index *const *srcs, uint32_t n_srcs, lance_hip_index **out);
/* old_ids / new_ids: n_map DEVICE words each, old_ids strictly ascending (checked; LANCE_HIP_EINVAL otherwise).  For every stored
 * row, in stored order: id == old_ids[i] -> the row is kept with id new_ids[i], or dropped when new_ids[i] == LANCE_HIP_ROW_DELETED;
 * id not among old_ids -> kept unchanged.  Every lookup is against the ids BEFORE the call (a mapping that swaps two ids swaps
 * them).  n_map == 0: an equal copy.                                                                                              */
int lance_hip_index_remap(lance_hip_ctx *ctx, const lance_hip_index *src, const uint64_t *old_ids, const uint64_t *new_ids,
                          uint64_t n_map, lance_hip_index **out);
/* The stored rows of any index kind in stored order, row-major and unpadded (HOST pointers, any may be NULL): part_offsets
 * [nlist + 1]; rows = code bytes per row (IVF_PQ: m, or m / 2 for 4-bit), d f32 (IVF_FLAT) or d code bytes (IVF_SQ); aux = the
 * per-row sums of squared codes (IVF_SQ only, ignored otherwise); row ids.  lance_hip_index_export keeps the reference's
 * transposed layout.                                                                                                              */
int lance_hip_index_export_rows(lance_hip_ctx *ctx, const lance_hip_index *idx, uint32_t *part_offsets_host, void *rows_host,
                                uint32_t *aux_host, uint64_t *row_ids_host);

/* ---- partition split / join: the decision (split_partition_impl, join_partition_impl, reassign_vectors; builder.rs:1152-1814) ----
 * Where every visited row goes, in one launch.  All pointers are DEVICE pointers.  The visited rows row_ids[n] come in n_cand + 1
 * segments, seg_offsets[n_cand + 2] (seg_offsets[0] = 0, seg_offsets[n_cand + 1] = n): segment 0 holds the rows of the chosen
 * partition P, segment s >= 1 the rows of candidate s - 1.  seg_centroids [n_cand + 1][d]: P's old centroid c0, then the candidates'
 * centroids in candidate order.  cand_ids[n_cand]: the candidates' partition ids in the numbering of the RESULT.  n_cand <= 64
 * (REASSIGN_RANGE).  A row's vector is raw[row id] (f32, [n_raw][d]); distances are the index metric's, bit for bit the reference's.
 * LANCE_HIP_REASSIGN_SPLIT: centroids2 [2][d] = c1, c2, standing for the partitions part1 and part2.  With d0 / d1 / d2 the distances
 *   FROM the row's own old centroid / c1 / c2 TO the row: a row of P with d0 <= d1 && d0 <= d2 takes the first minimum (f32::total_cmp)
 *   of its distances (from the row) to the candidates and goes to that candidate when min <= d1 && min <= d2; every other row of P,
 *   and every such row when n_cand == 0, goes to part1 when d1 <= d2, else to part2.  A row of a candidate stays where it is
 *   (dest = LANCE_HIP_NONE) when d0 <= d1 && d0 <= d2, else it goes to part1 / part2 the same way.
 * LANCE_HIP_REASSIGN_JOIN: every row of segment 0 goes to the candidate at the first minimum distance (n_cand >= 1; centroids2, part1
 *   and part2 are ignored); rows of other segments get LANCE_HIP_NONE.
 * A row id >= n_raw is never read: the call returns LANCE_HIP_EINVAL (that row's dest is LANCE_HIP_NONE).  Synchronises the stream. */
#define LANCE_HIP_REASSIGN_SPLIT 0
#define LANCE_HIP_REASSIGN_JOIN 1
int lance_hip_reassign_rows(lance_hip_ctx *ctx, int metric, int mode, const float *raw, uint64_t n_raw, uint32_t d,
                            const uint64_t *row_ids, uint64_t n, const uint32_t *seg_offsets, const float *seg_centroids,
                            const uint32_t *cand_ids, uint32_t n_cand, const float *centroids2, uint32_t part1, uint32_t part2,
                            uint32_t *dest);

/* ---- partition split / join: the index (optimize_indices' split_partition_impl, remap's join_partition_impl) ---------------------
 * Like merge / remap: the source is never written; the result is a NEW handle with nlist + 1 (split) or nlist - 1 (join) partitions,
 * its own model copy with the new centroid array, rebuilt offsets, no raw vectors attached.  IVF_PQ (8- and 4-bit), IVF_FLAT and
 * IVF_SQ handles over f32 columns; L2, cosine and dot.  raw [n_raw][d] f32 (device), indexed by the stored row ids: a VISITED row's id
 * >= n_raw is LANCE_HIP_EINVAL and nothing is built (rows of partitions outside the candidate range are never read from raw and are
 * not checked).  Candidates: the nearest min(65, nlist) centroids of the partition's centroid by
 * (distance in f32::total_cmp order, partition id), without the partition itself, at most 64.  Rows are visited partition by partition
 * (the chosen one, then -- split only -- the candidates in that order), in ascending row id, and decided by lance_hip_reassign_rows.
 * Storage: in every partition the surviving rows keep their stored order and bytes; the arriving rows follow in visit order, re-encoded
 * through the index's own chain with the partition id given (normalise for cosine; IVF_PQ: residual against the new partition's
 * centroid unless dot, PQ encode; IVF_SQ: the code under the stored bounds).  Nothing is trained here.
 * split: centroids2 [2][d] f32 (device) = c1, c2; c1 replaces centroid `part`, c2 becomes partition nlist.  Every row of `part` moves:
 *   the result holds every row exactly once (the reference as written would keep a stale copy of the old rows).
 *   LANCE_HIP_EINVAL: part >= nlist, fewer than 2 rows in `part`, nlist + 1 > 65536, an f16 / int8 or IVF_RQ handle.
 * join: partition `part` is removed, its rows go to the nearest candidate, partition ids above `part` drop by one.
 *   LANCE_HIP_EINVAL: part >= nlist, nlist == 1, an f16 / int8 or IVF_RQ handle.                                                    */
int lance_hip_index_split(lance_hip_ctx *ctx, const lance_hip_index *src, uint32_t part, const float *centroids2, const float *raw,
                          uint64_t n_raw, lance_hip_index **out);
int lance_hip_index_join(lance_hip_ctx *ctx, const lance_hip_index *src, uint32_t part, const float *raw, uint64_t n_raw,
                         lance_hip_index **out);

/* ---- a14: IvfModel::find_partitions (ivf/storage.rs:107-119, kmeans.rs:1134-1158) -- */
/* Batched.  Ascending by distance; equal distances ordered by partition id (the
 * reference's partial sort is unstable, so any order of equals is a valid outcome).
 * part_ids / dists: [nq][nprobes].  Cosine: q must already be normalised.
 * nlist <= 65536; with more than 8192 partitions nprobes <= 256.                        */
int lance_hip_find_partitions(lance_hip_ctx *ctx, int dtype, int metric, const void *q, uint32_t nq, uint32_t d,
                              const void *centroids, uint32_t nlist, uint32_t nprobes, uint32_t *part_ids,
                              float *dists);

/* ---- a16+a17+a19: one partition (PQDistCalculator::new + distance_all, pq/storage.rs:
 * 854-960; FlatIndex::search, flat/index.rs:82-177) --------------------------------- */
/* q_residual: [d] already residualised (v2.rs:316-332).  codes_transposed: [m][n_p].
 * has_range: keep only lower <= dist < upper.  out_*: capacity k; *out_n_host = count;
 * output is sorted by (dist, row id).                                                 */
int lance_hip_pq_scan_topk(lance_hip_ctx *ctx, int dtype, int metric, const void *q_residual, uint32_t d,
                           const void *codebook, uint32_t m, uint32_t nbits, const uint8_t *codes_transposed,
                           const uint64_t *row_ids, uint64_t n_p, uint32_t k, int has_range, float lower,
                           float upper, uint64_t *out_ids, float *out_dists, uint32_t *out_n_host);

/* ---- a14..a21 batched: the ANN query (knn.rs:359-1075, v2.rs:455-505, scanner.rs:
 * 3440-3468, refine :2884-2904) -------------------------------------------------------- */
/* q: [nq][d] raw queries (cosine: normalised internally, knn.rs:495-498).  nprobes =
 * minimum_nprobes = maximum_nprobes.  refine_factor 0 = None (no refine); rf >= 1 = Some(rf):
 * k*rf candidates re-ranked with exact distances on the raw vectors.  ids/dists: [nq][k],
 * missing results are id UINT64_MAX / dist +inf.                                      */
int lance_hip_ivfpq_search(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq,
                           uint32_t k, uint32_t nprobes, uint32_t refine_factor, uint64_t *ids, float *dists);
/* Same, but only enqueues on the stream (no synchronisation, no host reads): for
 * callers that time or pipeline batches.  Scratch is owned by the context.           */
int lance_hip_ivfpq_search_async(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq,
                                 uint32_t k, uint32_t nprobes, uint32_t refine_factor, uint64_t *ids,
                                 float *dists);

/* Distance-range query (`nearest={..., "distance_range": (lower, upper)}`; Query::lower_bound / upper_bound): inside
 * every probed partition only rows with lower <= d < upper enter the k-heap (FlatIndex::search, flat/index.rs:98-113),
 * d being the ADC distance (after the dot offset).  An open end is -FLT_MAX / FLT_MAX as in the reference
 * (`unwrap_or(f32::MIN)` / `unwrap_or(f32::MAX)`).  refine_factor as in lance_hip_ivfpq_search: the k * refine_factor
 * candidates that passed the ADC range are re-ranked by exact distance -- the exact distances are NOT filtered here; a
 * caller reproducing the reference plan (scanner.rs:3334-3377 filters them before the final fetch) asks for all
 * candidates (k = k * rf, refine_factor = 1) and applies the range to the returned exact distances.                 */
int lance_hip_ivfpq_search_range(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                                 uint32_t nprobes, uint32_t refine_factor, float lower, float upper, uint64_t *ids,
                                 float *dists);

/* One scan, two distances per candidate -- the local half of a LIST-SHARDED multi-GPU search with refine (search is
 * embarrassingly parallel over IVF lists; scanner.rs:2884-2904 re-ranks the k * refine_factor best by PQ distance with exact
 * distances): ids / pq_dists [nq][keff] = the keff nearest rows of this index by PQ distance in (dist, rowid) order (~0 / +inf
 * beyond the found ones), exactly lance_hip_ivfpq_search(k = keff, refine_factor = 0); exact_dists [nq][keff] (may be NULL) = each
 * candidate's exact distance to the query in the index's metric, the refine kernels' arithmetic, in the SAME order.  The ranks
 * all-gather the three arrays and lance_hip_merge_topk picks the global keff by PQ distance and orders them by the exact one.
 * (Round 5 obtained the exact distances from a second scan with refine_factor = 1 and aligned the two lists with sorts.)          */
int lance_hip_ivfpq_search_candidates(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t keff,
                                      uint32_t nprobes, uint64_t *ids, float *pq_dists, float *exact_dists);

/* The same search under a row-id prefilter (`nearest=..., filter=..., prefilter=True`: scanner.rs -> DatasetPreFilter ->
 * FlatIndex::search's RowIdMask branch, flat/index.rs:129-165).  allow_by_rowid[r] != 0 <=> row id r may be returned; rows
 * whose id is >= n_allow are filtered out.  The mask is applied INSIDE the scan kernels (one bit per stored row, tested
 * before a row can become a candidate, bound pass included): no per-filter copy of the index.  The result is identical
 * to the reference's per-row distance(id) loop.  4-bit PQ: the reference scores filtered rows with the UNQUANTISED f32
 * table, byte-wise terms (pq/storage.rs:893-921) -- a different arithmetic from its own unfiltered fast-scan -- and so do
 * the 4-bit scan kernel and its exact replay here when a mask is given (search.hip pq4_masked_row).                     */
int lance_hip_ivfpq_search_filtered(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                                    uint32_t nprobes, uint32_t refine_factor, const uint8_t *allow_by_rowid, uint64_t n_allow,
                                    uint64_t *ids, float *dists);

/* Prefilter and distance range together: FlatIndex::search's RowIdMask branch with lower / upper bounds
 * (flat/index.rs:131-149: selected rows only, each scored with distance(id), kept when lower <= d < upper). */
int lance_hip_ivfpq_search_filtered_range(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                                          uint32_t nprobes, uint32_t refine_factor, const uint8_t *allow_by_rowid, uint64_t n_allow,
                                          float lower, float upper, uint64_t *ids, float *dists);

/* Number of queries of the most recent search on this context that had to be replayed by the exact
 * (heap-emulating) kernel -- ties at a partition's k-th distance, or candidate-buffer overflow.      */
int lance_hip_search_stats(lance_hip_ctx *ctx, uint32_t *n_exact_replays_host);

/* ---- a20+a21: flat KNN (flat.rs:95-148, l2.rs:245-266, scanner.rs:3386-3411) ------- */
/* Exhaustive scan of x[n][d] for nq queries; result sorted by (dist, row id).
 * row_ids NULL -> row index.                                                          */
int lance_hip_flat_topk(lance_hip_ctx *ctx, int dtype, int metric, const void *x, const uint64_t *row_ids,
                        uint64_t n, uint32_t d, const void *q, uint32_t nq, uint32_t k, uint64_t *ids,
                        float *dists);
/* The same scan under a distance range (Scanner::flat_knn's LanceFilterExec(_distance >= lower AND _distance < upper) between
 * KNNVectorDistanceExec and SortExec.fetch(k), scanner.rs:3336-3412): the k smallest IN-RANGE rows, not the in-range part of the k
 * smallest.  A row is in range iff lower <= d < upper in the TOTAL order on f32 (IEEE 754 totalOrder: -NaN < -inf < .. < -0 < +0 < ..
 * < +inf < +NaN), d being the distance lance_hip_flat_topk returns for that (row, query), bit for bit.  has_lower / has_upper == 0:
 * that bound is NOT TESTED (the value is ignored) -- unlike lance_hip_ivfflat_search_range, whose open ends are -FLT_MAX / FLT_MAX:
 * (lower, none) keeps +inf and positive-NaN distances, (none, upper) keeps the negative NaN of an L2 row with a NaN element.
 * lower above upper: LANCE_HIP_EINVAL; lower == upper: nothing.  Missing slots: id UINT64_MAX, distance +inf.  Same limits on k,
 * dtypes and metrics as lance_hip_flat_topk, which is this entry with both bounds absent.                                        */
int lance_hip_flat_topk_range(lance_hip_ctx *ctx, int dtype, int metric, const void *x, const uint64_t *row_ids,
                              uint64_t n, uint32_t d, const void *q, uint32_t nq, uint32_t k, int has_lower, float lower,
                              int has_upper, float upper, uint64_t *ids, float *dists);

/* ---- flat KNN over a MULTIVECTOR column (Arrow List<FixedSizeList<T, d>>: one bag of vectors per row) ------------------
 * values  [offsets[n_rows]][d]: the flattened child array, LANCE_HIP_F32 or LANCE_HIP_F16 (int8 / uint8 columns: LANCE_HIP_EINVAL);
 * offsets [n_rows + 1], device, 64-bit, non-decreasing; row r holds the vectors offsets[r] .. offsets[r + 1] - 1;
 * q       [nqv][d] in the column's element type, 1 <= nqv <= LANCE_HIP_MULTIVEC_MAX_QUERY_VECTORS.
 * distance(row) = 1 - sum_i max_j (1 - dist(q_i, v_j)): the max by f32::total_cmp, the sum sequential in query-vector order,
 * dist = l2 | 1 - dot | cosine.  A zero-length row is an error (LANCE_HIP_EINVAL; the reference unwraps a None there), reported
 * after the scan: the outputs are then undefined.  Any d >= 1; k <= 1024; slots beyond n_rows: id UINT64_MAX, distance +inf.   */
#define LANCE_HIP_MULTIVEC_MAX_QUERY_VECTORS 256
/* multivec_distance (lance-linalg distance.rs:107-206): dists[n_rows] */
int lance_hip_multivec_distance(lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                                uint64_t n_rows, uint32_t d, const void *q, uint32_t nqv, float *dists);
/* flat KNN over a multivector column (flat.rs:129-133 + SortExec(dist, rowid).fetch(k)); row_ids NULL -> row index */
int lance_hip_flat_multivec_topk(lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                                 const uint64_t *row_ids, uint64_t n_rows, uint32_t d, const void *q, uint32_t nqv,
                                 uint32_t k, uint64_t *ids, float *dists);
/* ... under a distance range: the semantics of lance_hip_flat_topk_range on the rows' multivector distances */
int lance_hip_flat_multivec_topk_range(lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                                       const uint64_t *row_ids, uint64_t n_rows, uint32_t d, const void *q, uint32_t nqv,
                                       uint32_t k, int has_lower, float lower, int has_upper, float upper, uint64_t *ids,
                                       float *dists);

/* ... for a batch of n_queries multivector queries: q [q_offsets[n_queries]][d] in the column's element type (device), query b holds
 * the vectors q_offsets[b] .. q_offsets[b + 1] - 1 (q_offsets: HOST, as lance_hip_multivec_xtr_score takes them; 1..256 vectors per
 * query, 1..65535 queries).  ids / dists [n_queries][k]: bit for bit what lance_hip_flat_multivec_topk[_range] returns per query.
 * Cosine without a range, d <= 256: a MaxSim surrogate on the matrix cores filters the rows and only the survivors are evaluated
 * exactly (multivec_batch.hip); everything else is the single-query scan, query by query, inside the call.  survivors (host
 * uint32 [n_queries], or NULL): the rows evaluated exactly for each query, n_rows where the exact scan answered it. */
int lance_hip_flat_multivec_topk_batch(lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                                       const uint64_t *row_ids, uint64_t n_rows, uint32_t d, const void *q, const uint64_t *q_offsets,
                                       uint32_t n_queries, uint32_t k, int has_lower, float lower, int has_upper, float upper,
                                       uint64_t *ids, float *dists, uint32_t *survivors);

/* ---- multivector ANN: per-query-vector candidate lists joined by row id and scored with XTR-style imputation ----------
 * (Scanner::multivec_ann, scanner.rs:3471-3552; MultivectorScoringExec, knn.rs:1132-1329).  The index is an ordinary IVF_PQ index
 * over the FLATTENED vectors of the column whose row_ids repeat the row's id once per vector; one ANN search per query vector
 * gives a candidate list of keff = k * overfetch pairs in (dist, rowid) order.  For a multivector query of nqv vectors, every
 * operation one f32 rounding, lists taken in query-vector order j = 0 .. nqv - 1:
 *   min_sim_j = 1 - (distance of the list's last entry), 0 for an empty list;  sim_j(r) = 1 - dist of r's FIRST entry in list j
 *   missed_j  = ((0 + min_sim_0) + min_sim_1) + ... + min_sim_{j-1}
 *   s(r)      = sim_{j0}(r) + missed_{j0}, j0 = r's first list;  then for j = j0 + 1 .. nqv - 1: s += r in list j ? sim_j(r) : min_sim_j
 *   distance  = (float)nqv - s
 * and the k_out smallest by (distance in total order, row id) come back; slots beyond the joined rows: id UINT64_MAX, +inf.
 * (The reference joins the lists in stream-arrival order; order 0 .. nqv - 1 is one of those and is this library's definition.)
 * Limits, each refused with LANCE_HIP_EINVAL: 1 <= nqv <= LANCE_HIP_MULTIVEC_MAX_QUERY_VECTORS per query,
 * 1 <= keff <= LANCE_HIP_MULTIVEC_ANN_MAX_KEFF, 1 <= k_out <= LANCE_HIP_MULTIVEC_ANN_MAX_K_OUT.                                  */
#define LANCE_HIP_MULTIVEC_ANN_MAX_KEFF 4096
#define LANCE_HIP_MULTIVEC_ANN_MAX_K_OUT 1024
/* The join and score stage alone, for a batch of B multivector queries: cand_ids / cand_dists [q_offsets[B]][keff] (device) hold
 * one list per query vector -- valid entries first, then id UINT64_MAX / +inf --, the lists of query b are rows
 * q_offsets[b] .. q_offsets[b + 1] - 1; q_offsets [B + 1] is a HOST array starting at 0.  ids / dists [B][k_out] (device).  Any
 * index type's lists will do.                                                                                                  */
int lance_hip_multivec_xtr_score(lance_hip_ctx *ctx, const uint64_t *cand_ids, const float *cand_dists,
                                 const uint64_t *q_offsets, uint32_t B, uint32_t keff, uint32_t k_out, uint64_t *ids,
                                 float *dists);
/* One IVF_PQ search of all q_offsets[B] query vectors (q [q_offsets[B]][d] in the index's element type, device) with
 * k = keff = k * overfetch and no refine, into the context's scratch, then the stage above.  allow_by_rowid / n_allow as in
 * lance_hip_ivfpq_search_filtered (NULL: no prefilter).                                                                        */
int lance_hip_ivfpq_multivec_search(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, const uint64_t *q_offsets,
                                    uint32_t B, uint32_t k, uint32_t nprobes, uint32_t overfetch, uint32_t k_out,
                                    const uint8_t *allow_by_rowid, uint64_t n_allow, uint64_t *ids, float *dists);

/* ---- N4: IVF_FLAT (FlatIndex sub-index over raw vectors: flat/index.rs:82-177, flat/storage.rs:345-402) ------ */
/* Builds the per-partition FlatFloatStorage on the device: x[n][d] (dtype elements, widened exactly to f32) is
 * gathered into partition order (stable, rows with part id LANCE_HIP_NONE dropped).  L2, Dot and Cosine (f32 and f16 columns;
 * an int8 column under cosine is refused).
 * Cosine (IvfTransformer::new_flat, ivf.rs:147-175): the caller passes the rows ALREADY NORMALISED (lance_hip_normalize) with
 * part ids assigned in L2 -- the reference stores the normalised rows too; lance_hip_ivfflat_search normalises the query
 * key (knn.rs:498), finds the partitions in L2 (ivf/v2.rs:455-465) and scores rows with cosine_distance (ivf/v2.rs:405-411).
 * The handle is destroyed with lance_hip_index_destroy.                                               */
int lance_hip_ivfflat_create(lance_hip_ctx *ctx, int dtype, int metric, uint32_t d, const void *centroids,
                             uint32_t nlist, const void *x, const uint32_t *part_ids, const uint64_t *row_ids,
                             uint64_t n, lance_hip_index **out);
/* find_partitions + exact scan of the nprobes partitions + SortExec(dist, rowid).fetch(k); k <= 128.
 * When one partition holds more than k rows at or below a tied k-th distance, the survivors are those FlatIndex's
 * BinaryHeap keeps (such queries are replayed through a heap with std's push/pop, as in the IVF_PQ path). */
int lance_hip_ivfflat_search(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                             uint32_t nprobes, uint64_t *ids, float *dists);
/* IVF_FLAT under a row-id prefilter (FlatIndex::search's RowIdMask branch, flat/index.rs:129-165): allow_by_rowid[r] != 0
 * <=> row id r may be returned.  The mask is tested inside the scan kernels (bound pass, main pass, exact replay) -- the
 * selected rows are scored by the same distance function, so no filtered copy of the index is needed.      */
int lance_hip_ivfflat_search_filtered(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                                      uint32_t nprobes, const uint8_t *allow_by_rowid, uint64_t n_allow, uint64_t *ids, float *dists);
/* IVF_FLAT distance-range query (Query::lower_bound / upper_bound; FlatIndex::search, flat/index.rs:91-149): inside every
 * probed partition only rows with lower <= d < upper are offered to the partition's k-heap, d being the distance the index's
 * metric produces -- exact on this index type, so "every row within radius r" is decided on true distances.  The comparison
 * is OrderedFloat's total order (a NaN distance lies above every bound and is never in range; -0.0 sorts below +0.0, and no
 * metric here produces -0.0); an open end is -FLT_MAX / FLT_MAX (the reference's unwrap_or(f32::MIN) / unwrap_or(f32::MAX)).
 * lower > upper is refused, lower == upper returns nothing.  The range is tested inside the scan kernels (bound pass, main
 * pass, exact replay); k as in lance_hip_ivfflat_search.
 * allow_by_rowid may be NULL (n_allow ignored): range alone; otherwise FlatIndex::search's RowIdMask branch with bounds
 * (flat/index.rs:131-149).                                                                                                 */
int lance_hip_ivfflat_search_range(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                                   uint32_t nprobes, const uint8_t *allow_by_rowid, uint64_t n_allow,
                                   float lower, float upper, uint64_t *ids, float *dists);

/* ---- N6: 1-bit RaBitQ and IVF_RQ (lance-index/src/vector/bq/{builder,transform,storage}.rs, ivf.rs:281-326) ------------ */
/* f32 columns, metric LANCE_HIP_L2 or LANCE_HIP_DOT (Cosine is refused), num_bits = 1, d a multiple of 8 up to
 * LANCE_HIP_RQ_MAX_DIM.  rotation is the model's [d][d] f32 matrix P (row j is the j-th rotated axis), a DEVICE pointer like every
 * other array here.  A code row is d / 8 bytes: bit j % 8 of byte j / 8 is set iff the sign bit of dot(P[j], v - c) is clear. */
#define LANCE_HIP_RQ_MAX_DIM 2048
/* RabitQuantizer::quantize + RQTransformer::transform (bq/builder.rs, bq/transform.rs:95-208) for rows x[n][d] already assigned:
 * part_ids[n] (LANCE_HIP_NONE: the row gets zero codes and factors), dist_v_c[n] the distance the assignment reported
 * (PartitionTransformer::with_distance), centroids[nlist][d].  Out: codes[n][d / 8], add[n], scale[n] (ADD_FACTORS / SCALE_FACTORS).
 * The rotation is summed in the order of lance_linalg::distance::dot and the code / residual inner product sequentially: the
 * reference runs a BLAS GEMM there, so codes may differ from its own where a rotated component is within rounding of zero. */
int lance_hip_rq_encode(lance_hip_ctx *ctx, int metric, const float *x, uint64_t n, uint32_t d, const uint32_t *part_ids,
                        const float *dist_v_c, const float *centroids, uint32_t nlist, const float *rotation, uint8_t *codes,
                        float *add, float *scale);
/* RabitQuantizationStorage::dist_calculator + RabitDistCalculator (bq/storage.rs:296-369, 409-445) over ONE partition's storage:
 * codes[n][d / 8], add[n], scale[n] in storage order against nq residual queries qr[nq][d] (q - centroid) with their dist_q_c[nq].
 * quantised != 0: distance_all (rows below n - n % 32 through the u8 table with saturating u16 sums, the rest in f32);
 * quantised == 0: distance(id) of every row (what a prefiltered search computes).  dists[nq][n]; nq <= 65535. */
int lance_hip_rq_distance(lance_hip_ctx *ctx, int metric, const uint8_t *codes, const float *add, const float *scale, uint64_t n,
                          uint32_t d, const float *qr, const float *dist_q_c, uint32_t nq, const float *rotation, int quantised,
                          float *dists);
/* Per-partition RabitQuantizationStorage on the device (bq/storage.rs; IvfTransformer::with_rq ivf.rs:281-326): codes / add / scale
 * are gathered into partition order (stable; rows with part id LANCE_HIP_NONE dropped); row_ids NULL -> row index.  The handle
 * keeps its own copy of centroids and rotation; it is destroyed with lance_hip_index_destroy; every IVF_PQ / IVF_FLAT / IVF_SQ
 * entry point, lance_hip_index_save and the maintenance entries (merge / remap / export_rows) refuse it.                       */
int lance_hip_ivfrq_create(lance_hip_ctx *ctx, int metric, uint32_t d, const float *centroids, uint32_t nlist, const float *rotation,
                           const uint8_t *codes, const float *add, const float *scale, const uint32_t *part_ids,
                           const uint64_t *row_ids, uint64_t n, lance_hip_index **out);
/* find_partitions + preprocess_query (ivf/v2.rs:316-332: residual query and dist_q_c per probed partition) + FlatIndex::search over
 * the partition's RabitQ storage (flat/index.rs:82-126: distance_all, a max-heap of k, rows in storage order) +
 * SortExec(dist, rowid).fetch(k); k <= 128.  Queries whose answer depends on the heap's handling of ties are replayed through it. */
int lance_hip_ivfrq_search(lance_hip_ctx *ctx, const lance_hip_index *idx, const float *q, uint32_t nq, uint32_t k,
                           uint32_t nprobes, uint64_t *ids, float *dists);
/* The same under a row-id prefilter (flat/index.rs:129-165: distance(id) of every selected row -- the f32 table, never the
 * quantised one), tested inside the scan and the replay kernel; k <= 128. */
int lance_hip_ivfrq_search_filtered(lance_hip_ctx *ctx, const lance_hip_index *idx, const float *q, uint32_t nq, uint32_t k,
                                    uint32_t nprobes, const uint8_t *allow_by_rowid, uint64_t n_allow, uint64_t *ids, float *dists);

/* ---- re-ranking for IVF_SQ and IVF_RQ (scanner.rs:2884-2904: the ANN node is asked for k * refine_factor rows, knn.rs:642, the rows
 * are taken by row id and re-scored by flat_knn in the index's metric with the original query) ------------------------------------
 * keff = k * refine_factor, 1 <= keff <= LANCE_HIP_SQRQ_MAX_CANDIDATES; refine_factor = 0 is refused (scanner.rs:2869).  First the
 * search of that index type with k = keff: a heap of keff per probed partition, the (dist, rowid) merge with fetch keff, the same
 * arithmetic branches, prefilter branch (allow_by_rowid != NULL) and tie replay as lance_hip_ivf{sq,rq}_search[_filtered] -- through
 * the same kernels up to keff = 128, through their wide-capacity counterparts beyond.  Then the keff row ids are scored against the
 * raw vectors (lance_hip_index_set_raw; without them: LANCE_HIP_EINVAL) with the ORIGINAL query -- for a cosine IVF_SQ index not the
 * normalised copy the quantiser sees, for an f16 index widened --, ordered by (exact dist, rowid), and the first k are returned;
 * missing slots are id ~0 and distance +inf.  A stored row id >= n_raw is an error (LANCE_HIP_EINVAL), never ranked.           */
#define LANCE_HIP_SQRQ_MAX_CANDIDATES 768
int lance_hip_ivfsq_search_refine(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                                  uint32_t nprobes, uint32_t refine_factor, const uint8_t *allow_by_rowid /* NULL = none */,
                                  uint64_t n_allow, uint64_t *ids, float *dists);
int lance_hip_ivfrq_search_refine(lance_hip_ctx *ctx, const lance_hip_index *idx, const float *q, uint32_t nq, uint32_t k,
                                  uint32_t nprobes, uint32_t refine_factor, const uint8_t *allow_by_rowid /* NULL = none */,
                                  uint64_t n_allow, uint64_t *ids, float *dists);

/* ---- N5: 8-bit scalar quantisation and IVF_SQ (lance-index/src/vector/sq.rs, sq/storage.rs, sq/builder.rs) ------------ */
/* Columns are LANCE_HIP_F32 or LANCE_HIP_F16 (an int8 column is refused: the reference's SQ builder takes float arrays only; f64
 * columns are not in this library).  1 <= d <= LANCE_HIP_SQ_MAX_DIM; only num_bits = 8 exists (sq.rs `// TODO: support SQ4`).
 * bounds_host is the quantiser's Range<f64> as double[2] = {start, end} in HOST memory.                              */
#define LANCE_HIP_SQ_MAX_DIM 16384
/* ScalarQuantizer::update_bounds (sq.rs:67-89): folds the `count` elements of x into bounds_host, start.min(v) .. end.max(v)
 * after widening to f64; NaN elements are skipped (f64::min / max).  A fresh quantiser starts at {DBL_MAX, -DBL_MAX}
 * (sq.rs:43-55); folding a second array into the result is the same fold (retrain).  The sign of a zero bound is unspecified. */
int lance_hip_sq_bounds(lance_hip_ctx *ctx, int dtype, const void *x, uint64_t count, double *bounds_host);
/* scale_to_u8 (sq.rs:263-277): codes[n][d] = ((f64(v) - start) * 255.0 / (end - start)) as u8 -- truncated toward zero,
 * saturated to 0..255, NaN -> 0; start == end: every code is 0.                                                      */
int lance_hip_sq_encode(lance_hip_ctx *ctx, int dtype, const void *x, uint64_t n, uint32_t d, const double *bounds_host,
                        uint8_t *codes);
/* SQDistCalculator::distance_all (sq/storage.rs:398-468) for nq raw queries q[nq][d] (dtype elements, encoded with the same
 * bounds) against codes[n][d]: dists[nq][n] = (dist0 * r * r) / 65025 in f32, r = (end - start) as f32, dist0 = the u32 sum of
 * squared code differences as f32 (L2 and Cosine: l2_distance_uint_scalar, l2.rs:44-49) or 1 - the u32 sum of code products
 * as f32 (Dot: dot.rs:152-161).  The query is taken as given (a cosine caller normalises it first).  Finite bounds; nq <= 65535. */
int lance_hip_sq_distance(lance_hip_ctx *ctx, int dtype, int metric, const uint8_t *codes, uint64_t n, uint32_t d,
                          const void *q, uint32_t nq, const double *bounds_host, float *dists);
/* Per-partition ScalarQuantizationStorage on the device (sq/builder.rs, sq/storage.rs): codes[n][d] are gathered into partition
 * order (stable; rows with part id LANCE_HIP_NONE dropped); row_ids NULL -> row index.  dtype is the element type of centroids
 * and queries.  Cosine: the caller encoded NORMALISED rows and assigned them in L2, as for lance_hip_ivfflat_create.  The handle
 * is destroyed with lance_hip_index_destroy; every IVF_PQ / IVF_FLAT entry point and lance_hip_index_save refuse it.            */
int lance_hip_ivfsq_create(lance_hip_ctx *ctx, int dtype, int metric, uint32_t d, const void *centroids, uint32_t nlist,
                           const uint8_t *codes, const uint32_t *part_ids, const uint64_t *row_ids, uint64_t n,
                           const double *bounds_host, lance_hip_index **out);
/* find_partitions + FlatIndex::search over every probed partition's SQ storage (flat/index.rs:82-177: a max-heap of k on the
 * scaled f32 distance, rows in storage order) + SortExec(dist, rowid).fetch(k); k <= 128.  Queries whose answer depends on the
 * heap's handling of ties are replayed through it (counted by lance_hip_search_stats).                                      */
int lance_hip_ivfsq_search(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                           uint32_t nprobes, uint64_t *ids, float *dists);
/* The same under a row-id prefilter (flat/index.rs:129-165), tested inside the scan and the replay kernel. */
int lance_hip_ivfsq_search_filtered(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                                    uint32_t nprobes, const uint8_t *allow_by_rowid, uint64_t n_allow, uint64_t *ids, float *dists);

/* ---- a22 / 8(f) N3: index files (lance/src/index/vector/builder.rs:938-1079 merge_partitions) ---------------------- */
/* The `index.idx` + `auxiliary.idx` pair of an IVF_PQ / IVF_FLAT index directory, Lance file format 2.0 (the
 * FileWriter default, lance-file/src/writer.rs:553-561).  Host-side: nothing here needs a GPU except load/save, and every
 * pointer of the view below is a HOST pointer (the exception to this header's device-pointer convention).
 * Readers replaced: IvfQuantizationStorage::try_new (lance-index/src/vector/storage.rs:182-243),
 * ProductQuantizationMetadata (pq/storage.rs:52-144), IvfModel <-> pb (ivf/storage.rs:181-244).                    */
enum { LANCE_HIP_IVF_PQ = 0, LANCE_HIP_IVF_FLAT = 1 };
typedef struct lance_hip_index_file lance_hip_index_file;
typedef struct lance_hip_index_file_view {
  int index_type;               /* LANCE_HIP_IVF_PQ / LANCE_HIP_IVF_FLAT */
  int metric;
  int dtype;                    /* element type of the stored tensors / flat vectors: LANCE_HIP_F32 or LANCE_HIP_F16 */
  uint32_t d, nlist, m, nbits;  /* m = nbits = 0 for IVF_FLAT */
  uint64_t n_rows;
  int transposed;               /* codes are [code bytes][n_p] inside each partition (pq/storage.rs:430-449) */
  int has_loss;
  double loss;
  const float *centroids;       /* [nlist][d], widened to f32 */
  const float *codebook;        /* [m][2^nbits][d/m] f32 (pq/builder.rs:139-154 layout); NULL for IVF_FLAT */
  const uint32_t *part_offsets; /* [nlist+1] row offsets */
  const uint64_t *row_ids;      /* [n_rows], partition order */
  const uint8_t *codes;         /* IVF_PQ: n_rows * (nbits == 4 ? m/2 : m) bytes */
  const void *vectors;          /* IVF_FLAT: [n_rows][d] of dtype */
} lance_hip_index_file_view;
/* Maps and validates both files; the view's pointers stay valid until close.  Files written by Lance <= 0.27 (PQ
 * codebook inline in the schema metadata) are read too, and so is the legacy single-file layout of Lance <= 0.21
 * (`index.idx` only: pb Index behind a 16-byte footer; lance/src/index/vector/ivf.rs IVFIndex::try_new, pq.rs
 * PQIndex::load) -- its codes come back row-major (transposed = 0).  Other index types are refused.             */
int lance_hip_index_file_open(const char *index_dir, lance_hip_index_file **out);
int lance_hip_index_file_get(const lance_hip_index_file *f, lance_hip_index_file_view *view);
void lance_hip_index_file_close(lance_hip_index_file *f);
/* Writes the pair (creating index_dir if needed) in the layout merge_partitions produces: global buffers
 * (pb IVF, pb Tensor codebook) ahead of the pages, 64-byte aligned buffers, transposed codes.                      */
int lance_hip_index_file_write(const char *index_dir, const lance_hip_index_file_view *view);
/* Files -> device-resident index.  dtype is the indexed column's element type (F32 / F16 / I8).                   */
int lance_hip_index_load(lance_hip_ctx *ctx, const char *index_dir, int dtype, lance_hip_index **out);
/* The same for one list shard of a multi-GPU search: only the IVF lists p with p % list_mod == list_rem are
 * copied to this GPU, the others are left empty; centroids and codebook are complete, row ids are the stored ones.   */
int lance_hip_index_load_lists(lance_hip_ctx *ctx, const char *index_dir, int dtype, uint32_t list_mod, uint32_t list_rem,
                               lance_hip_index **out);
/* Device-resident index -> files.  loss is the k-means loss recorded in index.idx (has_loss = 0 to omit).        */
int lance_hip_index_save(lance_hip_ctx *ctx, const lance_hip_index *idx, const char *index_dir, int has_loss, double loss);
/* One top-level fixed-width column (scalar or fixed-size list, uncompressed, no nulls) of a format-2.0 Lance file,
 * e.g. the vector column of a data file.  dst NULL: only reports rows / bytes per row.                           */
int lance_hip_file_read_column(const char *path, const char *column, void *dst, uint64_t dst_bytes, uint64_t *rows,
                               uint32_t *row_bytes);

/* Shuffle buffers -- the artefact the reference's `precomputed_shuffle_buffers` hand-off carries: rows of (row_id u64,
 * __ivf_part_id u32, __pq_code FSL<u8>[code_bytes]), un-transposed (python/lance/vector.py:659-665; read back by
 * IvfIndexBuilder::shuffle_dataset, lance/src/index/vector/builder.rs:509-546).  One Lance v2.0 FILE, written with the same
 * page encodings the reference's FileWriter uses; rows with part id LANCE_HIP_NONE are dropped; row_ids NULL = row numbers.
 * HOST pointers.  (Wrapping the file in a dataset directory -- manifest, version files -- stays with the caller's pylance:
 * the storage engine is outside this library's scope.)                                                           */
int lance_hip_shuffle_buffer_write(const char *path, const uint64_t *row_ids, const uint32_t *part_ids, const uint8_t *codes,
                                   uint64_t n, uint32_t code_bytes, uint64_t *rows_written);

/* ---- multi-GPU: merge of per-shard candidate lists (list-sharded search) -------------------------------- */
/* SortExec([_distance asc, _rowid asc]).with_fetch(k) (lance scanner.rs:3440-3468) over `c` candidates per query gathered
 * from the list shards: ids [nq][c] (int64, -1 = none), dists [nq][c].  With exact_dists != NULL (refine, scanner.rs:2884-
 * 2904) the keff best by (dists, id) are re-ranked by (exact_dists, id) before the fetch.  Outputs [nq][k] (-1 / +inf pad). */
int lance_hip_merge_topk(lance_hip_ctx *ctx, const int64_t *ids, const float *dists, const float *exact_dists, uint32_t nq,
                         uint32_t c, uint32_t keff, uint32_t k, int64_t *out_ids, float *out_dists);

/* ---- combined search: `take` + `flat_knn` over candidate lists ------------------------------------- */
/* The stage that joins an ANN list with the flat KNN of the rows no index covers yet (Scanner::nearest, scanner.rs:2847-3030;
 * knn_combined / flat_knn, scanner.rs:3336-3468: UnionExec of the two lists, every distance recomputed from the column, the range
 * filter on those distances, SortExec(_distance, _rowid).fetch(k)) -- and, with list B absent, the refine (scanner.rs:2884-2904).
 * Per query the candidates are the ca slots of ids_a [nq][ca] and the cb slots of ids_b [nq][cb] (UINT64_MAX = an empty slot; ids_b /
 * dists_b may be NULL with cb = 0).  No de-duplication: a row id present twice is returned twice.  Every candidate of list A is
 * scored against x[id] (x [n_rows][d], the row id is the row index) with the query as given: the distance lance_hip_flat_topk
 * returns for that (row, query), bit for bit (f32 / f16 / int8 columns, L2 / dot / cosine; int8 cosine: LANCE_HIP_EINVAL).  List B
 * is what lance_hip_flat_topk[_range] returned for the unindexed rows: with dists_b its distances are taken as they are (they
 * are those bits already), with dists_b NULL its rows are scored like list A's.  Bounds as in lance_hip_flat_topk_range, on the
 * exact distances: the total order on f32, an absent bound is not tested, lower above upper is LANCE_HIP_EINVAL, lower == upper
 * returns nothing.  The survivors are ordered by (distance, row id) and the first k written; missing slots: id UINT64_MAX,
 * distance +inf.  A candidate id >= n_rows is never read: the call returns LANCE_HIP_EINVAL after the stream is drained (outputs
 * undefined).  Limits: 1 <= k <= 1024, 1 <= ca + cb <= 4096.  q in the column's element type; device pointers.              */
int lance_hip_take_flat_knn(lance_hip_ctx *ctx, int dtype, int metric, const void *x, uint64_t n_rows, uint32_t d, const void *q,
                            uint32_t nq, const uint64_t *ids_a, uint32_t ca, const uint64_t *ids_b, const float *dists_b,
                            uint32_t cb, int has_lower, float lower, int has_upper, float upper, uint32_t k, uint64_t *out_ids,
                            float *out_dists);

/* ---- measurement hooks (bench.py): per-kernel HIP-event timing on the ctx stream --- */
/* When enabled, each internal launch of the named hot kernels is bracketed by events;
 * query returns accumulated milliseconds and launch count, then resets.              */
int lance_hip_timing_enable(lance_hip_ctx *ctx, int on);
int lance_hip_timing_query(lance_hip_ctx *ctx, const char *kernel, double *ms_total, uint64_t *launches);
/* Ceilings measured in-process for bench.py's roofline denominators (no reference counterpart; SURVEY 8(d) asks for
 * peaks "re-measured on the box").  what: 0 / 1 / 2 = random LDS gathers of 4 / 8 / 16-byte PQ-LUT entries, result in
 * lane-gathers per second; 3 = device copy, bytes (read + written) per second; 4 / 5 = v_add_f32 / v_pk_add_f32
 * wave-instructions per second; 6-9 = LDS table-layout variants (lane-gathers per second); 10 / 11 = dense
 * v_mfma_f32_32x32x16_f16 / _bf16 issue rate in flop per second (round 6: the MFMA roofline's measured peak).          */
int lance_hip_ubench(lance_hip_ctx *ctx, int what, double *result);

#ifdef __cplusplus
}
#endif
#endif /* LANCE_HIP_H */
