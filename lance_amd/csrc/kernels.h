// kernels.h -- internal launcher prototypes shared by the translation units.
#pragma once
#include <stdint.h>
#include <string.h>

#include "common.h"
#include "search_plan.h"

namespace lh {

// One operand per lane (rows of x), the other staged in LDS (centroids).
// Batched views: batch b reads columns [b*x_batch_off, +d) of x (row stride ldx) against
// centroid block cent + b*cent_batch_stride -- this is how the M PQ sub-quantisers run
// in one launch (pq/builder.rs:109-138, pq.rs:146-166).
struct PairwiseArgs {
  const void *x_native = nullptr;   // optional: the rows in the column's own element type (x_dtype); kernels that can read it
  int x_dtype = 0;                  // natively (mfma_assign.hip) then never touch `x` (which may be NULL)
  const float *x = nullptr;
  bool lanes32 = false;             // dot products in the 32-lane order of f16 columns (dot_scalar::<f16, f32, 32>, dot.rs:91-102);
                                    // set by the callers only when the operands are widened f16 values, metric = dot and d > 16
  int64_t n = 0;
  int64_t ldx = 0;
  int x_batch_off = 0;
  const float *cent = nullptr;
  int k = 0;
  int64_t cent_batch_stride = 0;
  const float *bias = nullptr;
  int64_t bias_batch_stride = 0;
  uint32_t *ids = nullptr;
  float *dists = nullptr;
  int64_t out_batch_stride = 0;
  uint8_t *codes = nullptr;  // codes[row*codes_ld + b] = id (0 if none), pq.rs:165
  int codes_ld = 0;
  float *matrix = nullptr;  // MODE 1: [b][n][k]
  const uint8_t *active = nullptr;
  bool x_aligned = false;
  bool cent_aligned = false;
  bool check_finite = false;  // MODE 0: rows with a non-finite element get id NONE
  // long UNIT-LENGTH rows (cosine indices: the normalise kernel writes them): the rows once more as a binary16 plane scaled by 2^14, row stride
  // x_plane_dp (d rounded up to 32, zero padded), and an upper bound of their squared norms (NaN for a row that has none) -- the K-tiled
  // coarse quantiser then runs one f16 product instead of three bf16 ones (mfma_assign.hip: ma_top3_wide_kernel<.., F16>)
  const uint16_t *x_plane16 = nullptr;
  const float *x_plane_n2 = nullptr;
  int x_plane_dp = 0;
  float *part_vb = nullptr;   // k-split partials (set by the launcher)
  float *part_v = nullptr;
  uint32_t *part_idx = nullptr;
};

// PQ sub-quantiser argmin (k = 256, sub-dimension 4 / 8 / 16, L2) on the matrix cores with exact re-check (pq_mfma.hip)
// its argument block
struct PqmArgs {
  PairwiseArgs p;
  // encode mode (fused residual + PQ encode, encode_fused.hip's contract): rows are read from `xn` in the column's own element
  // type (row stride p.ldx elements), row r's operand is xn[r] - rcent[rpart[r]] (rounded to f16 for Float16 columns,
  // residual.rs:96); rows without a partition encode the zero vector.  rcent == NULL: no residual (dot metric).
  const void *xn = nullptr;
  const float *rcent = nullptr;
  const uint32_t *rpart = nullptr;
  int round_f16 = 0;
  uint32_t *fb_cnt;      // [batches] undecided rows per sub-quantiser
  uint32_t *fb_items;    // [batches][n] their row numbers
  int batches;
};
bool pq_mfma_supported(const PairwiseArgs &p, int d, int metric, int batches);
int launch_pq_mfma(lance_hip_ctx *ctx, const PairwiseArgs &p, int d, int batches);
bool pq_mfma_encode_supported(int dtype, int d, int m, int nbits, const void *x, const float *cent, const float *codebook, int64_t n);
int launch_pq_mfma_encode(lance_hip_ctx *ctx, int dtype, const void *x, int64_t n, int d, const float *cent, const uint32_t *part_ids,
                          int residual, const float *codebook, int m, uint8_t *codes);

// flat scan v2: per-query candidate pools + threshold pairs (flat.hip)
struct FlatPool {
  const float *x;       // rows as f32 (NULL when the fixed-dimension kernels read the column in its own element type)
  const void *x_native = nullptr;   // the column itself: f32 / f16 / int8 rows, widened per element in registers
  int x_dtype = 0;                  // LANCE_HIP_F32 / F16 / I8
  const uint64_t *row_ids;
  int64_t r0, r1;       // rows of this epoch
  const float *q;       // queries of this chunk
  int nq, k, cap;
  uint32_t *tkey;       // [nq]
  uint64_t *trid;       // [nq]
  uint32_t *cnt;        // [nq]
  uint32_t *pkeys;      // [nq][cap]
  uint64_t *prids;      // [nq][cap]
  uint32_t *overflow;   // [1]
  const float *row_sy = nullptr;   // cosine: sqrt(y_norm) per row   (cosine.rs:143-175)
  const float *q_norm = nullptr;   // cosine: norm_l2(query)
  // distance range.  The upper bound is not carried: it is the threshold every query STARTS from (flat_pool_reset_kernel).
  // has_lower picks the LOWER instantiation of the scan kernels, which append a cell only when key >= lo_key (the total order on f32,
  // order_key); without a lower bound there is NO test, and the kernels are the ones from before ranges existed.
  int has_lower = 0;
  uint32_t lo_key = 0;
  uint32_t *qfill = nullptr;       // [1] LOWER on the matrix cores: the eval kernels leave the fullest queue's count of the epoch (atomicMax)
};
constexpr int FLAT_MC_QUEUE_CAP = 2048;      // rows a query's queue holds per epoch of the matrix-core filters (flat_mfma.hip, flat_mfma_wide.hip)

// a call's distance range as order keys (exact.cuh order_key, on the host): in range <=> (!has_lower || key >= lo_key) && (!has_upper || key < hi_key)
struct FlatRange {
  bool has_lower = false, has_upper = false;
  uint32_t lo_key = 0, hi_key = 0xFFFFFFFFu;
  bool any() const { return has_lower || has_upper; }
  bool empty() const { return (has_upper && hi_key == 0) || (has_lower && has_upper && lo_key >= hi_key); }
  // the threshold pair every query starts from: the largest pair still under the upper bound
  uint32_t start_key() const { return has_upper ? hi_key - 1 : 0xFFFFFFFFu; }
};
// f32::total_cmp order key of a bound on the host: exact.cuh order_key, whose __float_as_uint is device code
inline uint32_t host_order_key(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float key_to_float_host(uint32_t k) {
  const uint32_t b = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  memcpy(&f, &b, 4);
  return f;
}
inline FlatRange flat_range(int has_lower, float lower, int has_upper, float upper) {
  FlatRange r;
  r.has_lower = has_lower != 0; r.has_upper = has_upper != 0;
  if (r.has_lower) r.lo_key = host_order_key(lower);
  if (r.has_upper) r.hi_key = host_order_key(upper);
  return r;
}

int launch_wide_filter(lance_hip_ctx *ctx, const FlatPool &fp, int d, int metric);   // wide.hip, any d
// search.hip: prefilter by row id -> one bit per storage position (scratch "search.allow_bits")
int build_allow_bits(lance_hip_ctx *ctx, const uint64_t *row_ids, uint64_t n, const uint8_t *allow_by_rowid, uint64_t n_allow, const uint32_t **bits_out);
// bf16x3 MFMA surrogate + exact re-check for query batches (flat_mfma.hip)
bool flat_mfma_supported(int metric, int d, int nq, const void *x, const float *q);
int flat_mfma_prepare(lance_hip_ctx *ctx, const float *q, int nq, int d, const uint16_t **qhi, const uint16_t **qlo, const float **qn);
int launch_flat_filter_mfma(lance_hip_ctx *ctx, const FlatPool &e, int d, int metric, const uint16_t *qhi, const uint16_t *qlo, const float *qn);
// K-tiled bf16 MFMA surrogate + exact re-check for query batches against LONG f32 rows, L2 / dot / cosine (flat_mfma_wide.hip)
bool flat_mfma_wide_supported(int metric, int d, int nq, int64_t n, const float *x, const float *q);
int flat_mfma_wide_prepare_rows(lance_hip_ctx *ctx, const float *x, int64_t n, int d, const uint16_t **xb, const float **xn2);
int flat_mfma_wide_prepare_queries(lance_hip_ctx *ctx, const float *q, int nq, int d, const uint16_t **qb, const float **qn2);
int launch_flat_filter_mfma_wide(lance_hip_ctx *ctx, const FlatPool &e, int d, int metric, const uint16_t *xb, const float *xn2, const uint16_t *qb,
                                 const float *qn2);

int launch_assign(lance_hip_ctx *ctx, const PairwiseArgs &p, int d, int metric, int batches);
bool assign_reads_native(PairwiseArgs p, int d, int batches);
// residual + PQ encode in one kernel, rows read in the column's own element type (encode_fused.hip)
bool encode_fused_supported(int dtype, int d, int m, int nbits, const void *x, const float *cent, const float *codebook, const uint8_t *codes);
int launch_encode_fused(lance_hip_ctx *ctx, int dtype, const void *x, int64_t n, int d, const float *cent, const uint32_t *part_ids,
                        int residual, const float *codebook, int m, uint8_t *codes);
// the whole transform in one pass over the rows: coarse assign + exact re-check + residual + PQ encode (xform_fused.hip)
bool xform_fused_supported(int dtype, int metric, int d, int m, int nbits, int64_t n, int nlist, const void *x, const float *cent,
                           const float *codebook, uint8_t *codes, bool lanes32);
int launch_xform_fused(lance_hip_ctx *ctx, int dtype, int metric, const void *x, int64_t n, int d, const float *cent, int nlist,
                       const float *codebook, int m, uint32_t *part_ids, float *dists, uint8_t *codes, bool round_f16);
// long rows (d > 128): residual + PQ encode of 128-column blocks on the same machinery, after the K-tiled coarse quantiser (xform_fused.hip)
bool xform_tail_supported(int d, int m, int nbits, int64_t n, const float *x, const float *cent, const float *codebook);
int launch_xform_tail(lance_hip_ctx *ctx, const float *x, int64_t n, int d, const float *cent, const uint32_t *part_ids, int residual, bool round_f16,
                      const float *codebook, int m, uint8_t *codes);
// the codebook training's E-step (all sub-quantisers, one launch) on the transform's PQ phase (xform_fused.hip); the undecided items go to pq_mfma_fix_kernel
bool xform_pqtrain_supported(const PairwiseArgs &p, int sd, int batches);
int launch_xform_pqtrain(lance_hip_ctx *ctx, const PairwiseArgs &p, int sd, int batches, uint32_t *fb_cnt, uint32_t *fb_items);
// f32 rows of d <= 128: sweep + exact re-check in one kernel (phases 1-3 of the transform kernel, with the k-means bias); same outputs as launch_assign
bool xform_assign_supported(const PairwiseArgs &p, int d, int metric, int batches);
int launch_xform_assign(lance_hip_ctx *ctx, const PairwiseArgs &p, int d, int metric);
// find_partitions over thousands of lists: the transform kernel's sweep with per-group keys (xform_fused.hip; select: coarse_select_kernel, mfma_assign.hip)
// cpl_ready / maxbits_ready: the centroid planes and their maxima built earlier by xform_coarse_planes (an index's constants), or NULL
int launch_xform_sweep_groups(lance_hip_ctx *ctx, int metric, const float *q, uint32_t nq, int d, const float *cent, uint32_t nlist, uint32_t *maxbits,
                              float *gkey, int ng, float *e2, const uint16_t *cpl_ready = nullptr, const uint32_t *maxbits_ready = nullptr);
size_t xform_coarse_planes_elems(uint32_t nlist, int d);      // bf16 elements of the planes
int xform_coarse_planes(lance_hip_ctx *ctx, int metric, const float *cent, uint32_t nlist, int d, uint16_t *cpl, uint32_t *maxbits /* zeroed */);
bool coarse_groups_shape(int d, uint32_t nlist);             // mfma_assign.hip: find_partitions takes the per-group keys for this shape
// bf16x3 MFMA candidates + exact re-check (mfma_assign.hip); same outputs as launch_assign
bool mfma_assign_supported(const PairwiseArgs &p, int d, int batches);
int launch_assign_mfma(lance_hip_ctx *ctx, const PairwiseArgs &p, int d, int metric);
int launch_dist_matrix(lance_hip_ctx *ctx, const PairwiseArgs &p, int d, int metric, int batches);

int stable_group(lance_hip_ctx *ctx, const uint32_t *ids, int64_t n, int64_t id_stride, int k, int batches,
                 uint32_t *starts, uint32_t *sorted_rows, int64_t out_stride, const uint8_t *active);

// f16_arith: T = f16 -- x / cent hold f16-representable values and the M-step rounds like half::f16
int kmeans_train_batched(lance_hip_ctx *ctx, int metric, const float *x, int64_t n, int64_t ldx, int x_batch_off, int d,
                         int k, int B, uint32_t max_iters, double tol, float balance_factor_scaled, bool have_init,
                         const uint64_t *seeds, float *cent, double *loss_out, uint32_t *iters_out, bool f16_arith = false);

int kmeans_train_hierarchical(lance_hip_ctx *ctx, int metric, const float *x, int64_t n, int d, int target_k, uint32_t max_iters,
                              double tol, float bf_scaled, int hierarchical_k, uint64_t seed, float *cent_out, uint32_t *n_out,
                              bool f16_arith = false);
// element-type plumbing (dtype.hip)
int check_dtype(int dtype, const char *what);
int model_dtype(int dtype);   // f32 for int8 data, else the data type itself
int as_f32(lance_hip_ctx *ctx, int dtype, const void *p, size_t count, const char *slot, const float **out);
int widen_into(lance_hip_ctx *ctx, int dtype, const void *p, size_t count, float *dst);
int from_f32(lance_hip_ctx *ctx, int dtype, const float *src, void *dst, size_t count);
int launch_residual(lance_hip_ctx *ctx, const float *x, int64_t n, int d, const float *cent, const uint32_t *part_ids, float *out, bool f16);


// search_pm.hip: a plan (search_plan.h) with route ROUTE_PAIR_SCAN or ROUTE_QUANTISED; the launchers below follow plan.bound / plan.main
int ivfpq_scan_merge_pm(lance_hip_ctx *ctx, const lance_hip_index *ix, const IvfpqPlan &plan, const float *qs, uint32_t nq, const uint32_t *probes,
                        uint32_t nprobes, uint32_t keff, uint32_t k, bool do_refine, uint64_t *ids, float *dists,
                        uint64_t *cand_rid, uint32_t *cand_cnt, uint32_t *flags, const uint32_t *allow);
int find_partitions_f32(lance_hip_ctx *ctx, int metric, const float *qf, uint32_t nq, uint32_t d, const float *cf, uint32_t nlist,
                        uint32_t nprobes, uint32_t *part_ids, float *dists, bool lanes32);   // search.hip
// flat_small.hip: exhaustive KNN for one to four queries in a single streaming pass (*done = false: mass ties, take the batch path)
bool flat_small_supported(int metric, int dtype, uint32_t d, uint32_t nq, uint32_t k, uint64_t n);
int flat_topk_small(lance_hip_ctx *ctx, int metric, int dtype, const void *x, const uint64_t *row_ids, uint64_t n, uint32_t d, const float *q,
                    uint32_t nq, uint32_t k, const FlatRange &rg, uint64_t *ids, float *dists, bool *done);
// mfma_assign.hip: the coarse quantiser at query time on the matrix cores (surrogate matrix + exact re-check of the candidates)
bool coarse_mfma_supported(int metric, int d, uint32_t nq, uint32_t nlist, uint32_t nprobes, bool lanes32, const float *q, const float *cent);
// fewer lists than the per-group route takes: sweep + select in one kernel (coarse_fused_kernel), which needs no [nq][nlist] matrix.  Its centroid
// constants (ma_prep_kernel's planes, |c|^2 over nlist ^ 64 floats, maxima) are built per call or once per index (index.h CqConst)
struct CoarseFusedConst {
  const uint16_t *chi, *clo;   // [nlist][d] bf16 planes
  const float *cn;             // [coarse_fused_cn_elems(nlist)]
  const uint32_t *maxbits;     // [4] words, [0] = max |c|^2 as float bits
};
bool coarse_fused_shape(int d, uint32_t nlist);
size_t coarse_fused_cn_elems(uint32_t nlist);
int coarse_fused_planes(lance_hip_ctx *ctx, const float *cent, uint32_t nlist, int d, uint16_t *chi, uint16_t *clo, float *cn, uint32_t *maxbits /* zeroed */);
int find_partitions_mfma(lance_hip_ctx *ctx, int metric, const float *q, uint32_t nq, int d, const float *cent, uint32_t nlist, uint32_t nprobes,
                         float *matrix, uint32_t *part_ids, float *dists, const uint16_t *cpl_ready = nullptr, const uint32_t *maxbits_ready = nullptr,
                         const CoarseFusedConst *fused_ready = nullptr);
int launch_normalize(lance_hip_ctx *ctx, const float *x, int64_t n, int d, float *out, bool f16);   // f16: half-precision arithmetic on f32 containers
// the same, and the normalised rows once more as a binary16 plane x 2^14 (stride dp = d rounded up to 32) + the squared-norm bound per row
int launch_normalize_planes(lance_hip_ctx *ctx, const float *x, int64_t n, int d, float *out, bool f16, uint16_t *plane16, int dp, float *n2);

// quantised 4-query filter scan + exact re-evaluation (search_q.hip), driven by ivfpq_scan_merge_pm
int qscan_index_constants(lance_hip_ctx *ctx, lance_hip_index *ix);
// build.hip: an empty IVF_PQ handle with src's codebook and the centroid array given (f32, device)
int index_alloc_like_pq_centroids(lance_hip_ctx *ctx, const lance_hip_index *src, const float *centroids, uint32_t nlist, lance_hip_index **out);
// index_update.hip: the pieces of merge / remap that split / join (rebalance.hip) are built from
enum { IU_PQ = 0, IU_FLAT = 1, IU_SQ = 2 };
int iu_kind(const lance_hip_index *ix);
uint32_t iu_lists(const lance_hip_index *ix);
uint32_t iu_stride(const lance_hip_index *ix);
const uint8_t *iu_payload(const lance_hip_index *ix);
uint8_t *iu_payload(lance_hip_index *ix);
int iu_check_handle(const lance_hip_ctx *ctx, const lance_hip_index *ix, const char *what);
int iu_malloc(void **out, size_t bytes);
int iu_new_like(lance_hip_ctx *ctx, const lance_hip_index *src, const float *centroids, uint32_t lists, lance_hip_index **out);
int iu_alloc_rows(lance_hip_index *ix, uint64_t n);
int iu_copy(lance_hip_ctx *ctx, const void *src, void *dst, uint64_t n_rows, int64_t src_stride, int64_t dst_stride, int row_bytes,
            const uint32_t *perm, const uint32_t *src_offs, const uint32_t *dst_base, uint32_t nlist);
int iu_finish_layout(lance_hip_ctx *ctx, lance_hip_index *ix, const lance_hip_index *src, const std::vector<uint32_t> &offs);
// sq.hip: the per-row sums of squared codes of padded SQ rows [n][ld]
int sq_row_sums(lance_hip_ctx *ctx, const uint8_t *codes, uint64_t n, uint32_t ld, uint32_t *out);
constexpr int QSCAN_SEG_CAP = 256;   // survivors kept per (query, probe)
struct SelectOut;
// search_qt.hip: M = 48 / 64 / 96 (table tiled over the sub-quantisers); class-B queries of those shapes go to the rescan kernel
int qscan_classb_to_rescan(lance_hip_ctx *ctx, const uint32_t *tbound, uint32_t nq, uint32_t nprobes, uint32_t *seg_cnt, uint32_t *qovf);
int qscan_nearest_keys(lance_hip_ctx *ctx, const uint32_t *probes, uint32_t nq, uint32_t nprobes, uint32_t *keys, uint32_t nb = 1);
// G = queries per work item of the main pass; items = false: item_start4 / desc4 stay unwritten (only qscan_launch reads them)
int qscan_group(lance_hip_ctx *ctx, const uint32_t *probes, uint32_t nq, uint32_t nprobes, int nlist, const uint32_t *tglobal,
                uint32_t *keys, uint32_t *tbound, uint32_t *pair_starts, uint32_t *pair_idx, uint32_t *item_start4, int4 *desc4,
                uint32_t max_items4, int G = 4, int dot = 0, bool items = true);
int qbound_launch(lance_hip_ctx *ctx, const lance_hip_index *ix, const float *qs, uint32_t nq, uint32_t keff, const uint32_t *pair_starts0,
                  const uint32_t *pair_idx0, uint32_t *item_start, int4 *desc, uint32_t max_items, uint32_t *tglobal, const uint32_t *allow);
int qscan_launch(lance_hip_ctx *ctx, const lance_hip_index *ix, const float *qs, uint32_t nq, uint32_t nprobes, const uint32_t *pair_idx,
                 const uint32_t *item_start4, const int4 *desc4, uint32_t max_items4, const uint32_t *tbound, uint32_t *seg_cnt,
                 uint32_t *seg_pos, uint32_t *qovf, const uint32_t *allow, const uint32_t *probes, const IvfpqPlan &plan);
// search_qt.hip: per-query tables + per-row bias instead of a table per (query, partition) (M = 48 / 64 / 96; LANCE_HIP_QPT)
int qbound_pt_launch(lance_hip_ctx *ctx, const lance_hip_index *ix, const float *qs, uint32_t nq, uint32_t nprobes, uint32_t keff,
                     const uint32_t *probes, const uint32_t *pair_starts0, const uint32_t *pair_idx0, uint32_t *item_start, int4 *desc,
                     uint32_t max_items, uint32_t *tglobal, const uint32_t *allow);
int qmerge_launch(lance_hip_ctx *ctx, const lance_hip_index *ix, const float *qs, uint32_t nq, const uint32_t *probes, uint32_t nprobes,
                  const uint32_t *tbound, uint32_t *tglobal, const uint32_t *seg_cnt, const uint32_t *seg_pos, const uint32_t *qovf,
                  uint32_t *pool_key, uint32_t *pool_pos, uint32_t *pool_cnt, int pool_cap, const SelectOut &o, const uint32_t *allow,
                  PlanMain main, const uint32_t *qslack = nullptr, const float *seg_val = nullptr, const float *seg_scale = nullptr);
// search_ms.hip: the filter scan as a [rows x d] x [d x queries] product per partition on the matrix cores (8-bit PQ, d = 64 / 128, M = 16 / 32)
PlanMsState mscan_state(const lance_hip_index *ix);
int mscan_prepare(lance_hip_ctx *ctx, lance_hip_index *ix);   // builds lance_hip_index::ms once (allocates and synchronises: never during a capture)
int mscan_launch(lance_hip_ctx *ctx, const lance_hip_index *ix, const float *qs, uint32_t nq, uint32_t nprobes, const uint32_t *probes,
                 const uint32_t *pair_starts, const uint32_t *pair_idx, const uint32_t *tbound, uint32_t *seg_cnt, uint32_t *seg_pos,
                 uint32_t *qovf, const uint32_t *allow, uint32_t **qslack_out, float **seg_val_out, float **seg_scale_out);
void mscan_cut_params(int *cut_shift, uint32_t *cut_slack);
int msbound_launch(lance_hip_ctx *ctx, const lance_hip_index *ix, const float *qs, uint32_t nq, uint32_t keff, const uint32_t *pair_starts0,
                   const uint32_t *pair_idx0, uint32_t *item_start, int4 *desc, uint32_t max_items, uint32_t *tglobal, const uint32_t *allow,
                   uint32_t nb = 1);   // search_ms.hip: the bound pass of a plan with bound == BOUND_MATRIX
int qscan_items(lance_hip_ctx *ctx, const uint32_t *pair_starts, int nvp, int G, uint32_t *item_start, int4 *desc, uint32_t max_items);   // search_q.hip: work items of G grouped pairs
// search.hip: the exact re-ranking shared by every index type with a refine_factor.  cand_rid [nq][keff]: a query's valid ids are a prefix
// (empty slots ~0), launch_cand_count counts them; launch_refine scores them against the index's raw vectors in its metric with the ORIGINAL
// query (widened to f32) -- refine_pair_kernel / refine_u8_kernel / refine_rows_u8_kernel / refine_kernel by dtype, metric and d --, orders by (dist, rowid) and
// writes the first k; a row id >= n_raw sets FLAG_BADROW in flags [nq] (zeroed by the caller), which check_flags (synchronises) reports
int launch_cand_count(lance_hip_ctx *ctx, const uint64_t *ids, uint32_t nq, uint32_t keff, uint32_t *cnt);
int launch_refine(lance_hip_ctx *ctx, const lance_hip_index *ix, const float *q, uint32_t nq, int d, const uint64_t *cand_rid, const uint32_t *cand_cnt,
                  uint32_t keff, uint32_t k, uint64_t *ids, float *dists, uint32_t *flags, float *cand_exact);
int check_flags(lance_hip_ctx *ctx, const uint32_t *flags, uint32_t nq, const char *badrow_msg = nullptr);   // badrow_msg: what to report for FLAG_BADROW instead of the set_raw message
const uint8_t *raw_compact_prepare(lance_hip_ctx *ctx, const lance_hip_index *ix);   // search.hip: lossless u8 refine copy (index.h), or nullptr

}  // namespace lh
