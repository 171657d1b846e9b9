// rebalance.hip -- the decision of a partition split / join: where every visited row goes.
//
//   split_partition_impl / reassign_vectors   rust/lance/src/index/vector/builder.rs:1152-1340, :1532-1786
//   join_partition_impl                       builder.rs:1343-1530
//   select_reassign_candidates_impl           builder.rs:1788-1814 (REASSIGN_RANGE = 64)
// One launch over the visited rows.  The rows come in segments: segment 0 holds the rows of the chosen partition P, segment s >= 1
// those of candidate s - 1 (a neighbour of P).  Every decision is a chain of `<=` between f32 distances, so every distance is computed
// by exact.cuh's functions in the reference's order, with the reference's `from` / `to` roles (cosine rounds differently by role):
//   d0 = dist(own old centroid -> row), d1 = dist(c1 -> row), d2 = dist(c2 -> row);  candidates: dist(row -> candidate centroid).
// Split: a row of P with d0 <= d1 && d0 <= d2 looks for the first minimum (f32::total_cmp) among the candidates and goes there when
// min <= d1 && min <= d2; every other row of P goes to P (d1 <= d2) or to the appended partition.  A row of a candidate stays
// (LANCE_HIP_NONE) when d0 <= d1 && d0 <= d2, otherwise it goes to P or the appended partition the same way.  Without candidates
// (nlist == 1) the reference would unwrap an empty minimum; here such a row goes by d1 <= d2.
// Join: every row of segment 0 goes to the candidate with the first minimum distance.
//
// Layout: a workgroup of 256 lanes takes RB_TILE = 32 rows at a time.  The rows are gathered by id ONCE into LDS and serve all of their
// up to 67 distances; the table of up to 67 centroids (c0, the candidates, c1, c2) is staged once per workgroup.  Rows of the table are
// d | 1 words apart: lanes of a wave read the same row element (broadcast) and different table rows, which then fall into different
// banks.  A lane computes one (row, centroid) distance start to end -- dist_exact_rt's 16 accumulators are per lane, no partial sums
// cross lanes, so no new summation order exists.  When table and tile do not fit into 64 KiB (rb_lds_bytes), both are read through
// L2 in place, by the same code.  No atomics: the flag word only ever receives the value 1.
#include <algorithm>

#include <cstring>
#include <vector>

#include "common.h"
#include "exact.cuh"
#include "index.h"
#include "kernels.h"

namespace lh {

// ---- device code (tests/test_rebalance_kernels_cpu.py runs this text on the CPU)
constexpr uint32_t RB_NONE = 0xFFFFFFFFu;      // LANCE_HIP_NONE
constexpr int RB_TILE = 32;                    // rows per workgroup pass
constexpr int RB_MAX_CAND = 64;                // REASSIGN_RANGE
// the small per-workgroup arrays at the head of the LDS block, in words
constexpr int RB_W_TNORM = 0;                                // [68]     |table row| (cosine: the `from` norm of a centroid)
constexpr int RB_W_RNORM = RB_W_TNORM + 68;                  // [32]     |row| (cosine: the `from` norm of a row)
constexpr int RB_W_D3 = RB_W_RNORM + RB_TILE;                // [32][3]  d0, d1, d2
constexpr int RB_W_SEG = RB_W_D3 + 3 * RB_TILE;              // [32]     segment of the row
constexpr int RB_W_STATE = RB_W_SEG + RB_TILE;               // [32]     1: the row exists and its id is in range
constexpr int RB_W_NEED = RB_W_STATE + RB_TILE;              // [32]     1: the row ranks the candidates
constexpr int RB_W_CD = RB_W_NEED + RB_TILE;                 // [32][64] order_key of the row's distance to every candidate
constexpr int RB_W_HEAD = RB_W_CD + RB_TILE * RB_MAX_CAND;   // 2340 words; a multiple of 4

struct RbArgs {
  const float *raw;            // [n_raw][d]
  uint64_t n_raw;
  const uint64_t *ids;         // [n] visited rows, in visit order
  int64_t n;
  const uint32_t *seg_offs;    // [n_cand + 2]: segment s is ids[seg_offs[s] .. seg_offs[s + 1])
  const float *seg_cent;       // [n_cand + 1][d]: c0, then the candidates' centroids
  const uint32_t *cand_ids;    // [n_cand] destination ids (new numbering)
  const float *c12;            // [2][d]: c1, c2 (split)
  uint32_t *dest;              // [n]
  uint32_t *flag;              // |= 1: a row id >= n_raw
  int d, n_cand, join, lds;
  uint32_t part1, part2;       // the destinations that c1 / c2 stand for
};

extern __shared__ __attribute__((aligned(16))) char smem[];

template <int METRIC>
__device__ __forceinline__ float rb_dist(const float *from, float from_norm, const float *to, int d) {
  if constexpr (METRIC == METRIC_COSINE) return cosine_exact_rt<float>(from, from_norm, to, d);
  else return finish_metric<METRIC>(dist_exact_rt<METRIC, float>(from, to, d));
}

// LDS: table and row tile staged (the operands of every distance are LDS addresses at compile time: ds_read, not flat loads);
// otherwise both are read in place
template <int METRIC, bool LDS>
__global__ __launch_bounds__(256) void rb_reassign_kernel(RbArgs a) {
  uint32_t *wu = reinterpret_cast<uint32_t *>(smem);
  float *wf = reinterpret_cast<float *>(smem);
  const int t = (int)threadIdx.x, d = a.d, C = a.n_cand;
  const int S = a.join ? C + 1 : C + 3;      // table rows: c0, candidates (, c1, c2)
  const int ld = LDS ? (d | 1) : d;
  float *tab_l = wf + RB_W_HEAD, *rows_l = tab_l + (LDS ? S * ld : 0);
  // table row j: 0 = c0, 1 .. C = the candidates, C + 1 = c1, C + 2 = c2
  auto tab = [&](int j) -> const float * {
    if constexpr (LDS) return tab_l + j * ld;
    return j <= C ? a.seg_cent + (int64_t)j * d : a.c12 + (int64_t)(j - C - 1) * d;
  };
  if constexpr (LDS) {
    for (int e = t; e < S * d; e += 256) {
      const int j = e / d, c = e - j * d;
      tab_l[j * ld + c] = j <= C ? a.seg_cent[(int64_t)j * d + c] : a.c12[(int64_t)(j - C - 1) * d + c];
    }
    __syncthreads();
  }
  if (METRIC == METRIC_COSINE && t < S) wf[RB_W_TNORM + t] = norm_l2_rt<float>(tab(t), d);
  for (int64_t i0 = (int64_t)blockIdx.x * RB_TILE; i0 < a.n; i0 += (int64_t)gridDim.x * RB_TILE) {
    if (t < RB_TILE) {
      const int64_t i = i0 + t;
      uint32_t ok = 0, seg = 0;
      if (i < a.n) {
        ok = a.ids[i] < a.n_raw;
        if (!ok) { *a.flag = 1u; a.dest[i] = RB_NONE; }
        int lo = 0, hi = C + 1;      // largest s with seg_offs[s] <= i
        while (hi - lo > 0) {
          const int mid = (lo + hi + 1) >> 1;
          if ((int64_t)a.seg_offs[mid] <= i) lo = mid; else hi = mid - 1;
        }
        seg = (uint32_t)lo;
      }
      wu[RB_W_STATE + t] = ok;
      wu[RB_W_SEG + t] = seg;
    }
    __syncthreads();
    auto row = [&](int r) -> const float * {
      if constexpr (LDS) return rows_l + r * ld;
      else return a.raw + a.ids[i0 + r] * (uint64_t)d;
    };
    if constexpr (LDS) {
      for (int e = t; e < RB_TILE * d; e += 256) {
        const int r = e / d, c = e - r * d;
        if (wu[RB_W_STATE + r]) rows_l[r * ld + c] = a.raw[a.ids[i0 + r] * (uint64_t)d + c];
      }
      __syncthreads();
    }
    // d0, d1, d2 (split) and the row's own norm (cosine)
    if (t < RB_TILE * 4) {
      const int r = t >> 2, s = t & 3;
      if (wu[RB_W_STATE + r]) {
        if (s == 3) {
          if (METRIC == METRIC_COSINE) wf[RB_W_RNORM + r] = norm_l2_rt<float>(row(r), d);
        } else if (!a.join) {
          const int j = s == 0 ? (int)wu[RB_W_SEG + r] : C + s;
          wf[RB_W_D3 + 3 * r + s] = rb_dist<METRIC>(tab(j), wf[RB_W_TNORM + j], row(r), d);
        }
      }
    }
    __syncthreads();
    if (t < RB_TILE) {
      uint32_t need = 0;
      if (wu[RB_W_STATE + t] && wu[RB_W_SEG + t] == 0 && C > 0) {
        need = 1u;
        if (!a.join) {
          const float d0 = wf[RB_W_D3 + 3 * t], d1 = wf[RB_W_D3 + 3 * t + 1], d2 = wf[RB_W_D3 + 3 * t + 2];
          need = (uint32_t)(d0 <= d1 && d0 <= d2);
        }
      }
      wu[RB_W_NEED + t] = need;
    }
    __syncthreads();
    for (int w = t; w < RB_TILE * C; w += 256) {
      const int r = w / C, j = w - r * C;
      if (wu[RB_W_NEED + r]) wu[RB_W_CD + r * RB_MAX_CAND + j] = order_key(rb_dist<METRIC>(row(r), wf[RB_W_RNORM + r], tab(1 + j), d));
    }
    __syncthreads();
    if (t < RB_TILE && wu[RB_W_STATE + t]) {
      const uint32_t seg = wu[RB_W_SEG + t];
      float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f;
      if (!a.join) { d0 = wf[RB_W_D3 + 3 * t]; d1 = wf[RB_W_D3 + 3 * t + 1]; d2 = wf[RB_W_D3 + 3 * t + 2]; }
      uint32_t dst = RB_NONE;
      if (wu[RB_W_NEED + t]) {
        uint32_t best = wu[RB_W_CD + t * RB_MAX_CAND];
        int bj = 0;
        for (int j = 1; j < C; ++j) {
          const uint32_t k = wu[RB_W_CD + t * RB_MAX_CAND + j];
          if (k < best) { best = k; bj = j; }
        }
        const float mn = key_to_float(best);
        if (a.join || (mn <= d1 && mn <= d2)) dst = a.cand_ids[bj];
        else dst = d1 <= d2 ? a.part1 : a.part2;
      } else if (!a.join) {
        if (seg == 0 || !(d0 <= d1 && d0 <= d2)) dst = d1 <= d2 ? a.part1 : a.part2;
      }
      a.dest[i0 + t] = dst;
    }
    __syncthreads();
  }
}

// ---- host side

// bytes of LDS the staged route needs; the staged route is taken when this fits into 64 KiB
static int64_t rb_lds_bytes(int d, int n_cand, int join) {
  const int64_t S = join ? n_cand + 1 : n_cand + 3;
  return 4 * ((int64_t)RB_W_HEAD + (S + RB_TILE) * (int64_t)(d | 1));
}

}  // namespace lh

using namespace lh;

extern "C" int lance_hip_reassign_rows(lance_hip_ctx *ctx, int metric, int mode, const float *raw, uint64_t n_raw, uint32_t d,
                                       const uint64_t *row_ids, uint64_t n, const uint32_t *seg_offsets, const float *seg_centroids,
                                       const uint32_t *cand_ids, uint32_t n_cand, const float *centroids2, uint32_t part1, uint32_t part2,
                                       uint32_t *dest) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx, "reassign_rows: NULL context");
  LH_REQUIRE(metric == LANCE_HIP_L2 || metric == LANCE_HIP_COSINE || metric == LANCE_HIP_DOT, "reassign_rows: metric %d not supported", metric);
  LH_REQUIRE(mode == LANCE_HIP_REASSIGN_SPLIT || mode == LANCE_HIP_REASSIGN_JOIN, "reassign_rows: mode %d not supported (0 split, 1 join)", mode);
  LH_REQUIRE(d >= 1 && d <= 16384, "reassign_rows: d=%u not supported (1..16384)", d);
  LH_REQUIRE(n_cand <= (uint32_t)RB_MAX_CAND, "reassign_rows: %u candidates, at most %d (the reference's REASSIGN_RANGE)", n_cand, RB_MAX_CAND);
  LH_REQUIRE(n < (1ull << 32), "reassign_rows: %llu rows: row offsets are 32-bit in this version", (unsigned long long)n);
  const bool join = mode == LANCE_HIP_REASSIGN_JOIN;
  LH_REQUIRE(!join || n_cand >= 1, "reassign_rows: a join needs at least one candidate partition (nlist == 1 has none)");
  LH_REQUIRE(join || centroids2, "reassign_rows: a split needs the two new centroids");
  if (n == 0) return LANCE_HIP_OK;
  LH_REQUIRE(raw && row_ids && seg_offsets && seg_centroids && dest && (n_cand == 0 || cand_ids), "reassign_rows: NULL argument");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  uint32_t *flag = ctx->scratch_t<uint32_t>("rebalance.flag", 4);
  if (!flag) return LANCE_HIP_ENOMEM;
  LH_CHECK_HIP(lh::memset_async(flag, 0, 16, ctx->stream));
  RbArgs a;
  a.raw = raw; a.n_raw = n_raw; a.ids = row_ids; a.n = (int64_t)n; a.seg_offs = seg_offsets; a.seg_cent = seg_centroids; a.cand_ids = cand_ids;
  a.c12 = centroids2; a.dest = dest; a.flag = flag; a.d = (int)d; a.n_cand = (int)n_cand; a.join = join ? 1 : 0;
  a.part1 = part1; a.part2 = part2;
  const int64_t staged = rb_lds_bytes((int)d, (int)n_cand, a.join);
  a.lds = staged <= 65536 ? 1 : 0;
  const size_t lds = a.lds ? (size_t)staged : (size_t)RB_W_HEAD * 4;
  // a workgroup stages the table once and then walks tiles: no more workgroups than keep every CU busy twice over
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(cdiv(n, RB_TILE), 2ull * (uint64_t)ctx->num_cus));
  {
    ScopedTimer t(ctx, a.lds ? "rebalance_reassign" : "rebalance_reassign_global");
    auto launch = [&](auto kernel) { hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds, ctx->stream, a); };
    if (metric == LANCE_HIP_L2) a.lds ? launch(rb_reassign_kernel<METRIC_L2, true>) : launch(rb_reassign_kernel<METRIC_L2, false>);
    else if (metric == LANCE_HIP_COSINE) a.lds ? launch(rb_reassign_kernel<METRIC_COSINE, true>) : launch(rb_reassign_kernel<METRIC_COSINE, false>);
    else a.lds ? launch(rb_reassign_kernel<METRIC_DOT, true>) : launch(rb_reassign_kernel<METRIC_DOT, false>);
    LH_CHECK_HIP(hipGetLastError());
  }
  uint32_t fh = 0;
  LH_CHECK_HIP(hipMemcpyAsync(&fh, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  LH_REQUIRE(fh == 0, "reassign_rows: a row id is >= n_raw=%llu (the raw vectors do not cover the index)", (unsigned long long)n_raw);
  return LANCE_HIP_OK;
}

// ---- split / join of a handle ------------------------------------------------------------------------------------------------------
// The reference's split_partition_impl / join_partition_impl as ONE new handle (the source is never written): candidates from the
// distances of c0 to every centroid, the visit order (P, then the candidates, ascending row id inside each), the decision kernel above,
// and the storage -- in every partition the surviving rows in stored order (moved, never re-encoded), then the arriving rows in visit
// order, re-encoded through the index's own chain with the partition id GIVEN.  Two stable groupings give both orders: one over all
// stored rows keyed by "partition in the new numbering, or none when the row leaves", one over the visited rows keyed by dest.
// Only small mirrors cross to the host: the nlist centroid distances, the candidate list and the offsets.
namespace lh {

__device__ __forceinline__ uint32_t rb_partition_of(const uint32_t *__restrict__ offs, int nlist, uint32_t row) {
  int lo = 0, hi = nlist;      // largest p in [0, nlist) with offs[p] <= row
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (offs[mid] <= row) lo = mid; else hi = mid;
  }
  return (uint32_t)lo;
}

// out[j] = dist(from = centroid `part`, to = centroid j): what select_reassign_candidates_impl sorts
template <int METRIC>
__global__ __launch_bounds__(256) void rb_centroid_dist_kernel(const float *__restrict__ cent, int nlist, int d, int part, float *__restrict__ out) {
  const int j = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (j >= nlist) return;
  const float *c0 = cent + (int64_t)part * d;
  const float n0 = METRIC == METRIC_COSINE ? norm_l2_rt<float>(c0, d) : 0.0f;
  out[j] = rb_dist<METRIC>(c0, n0, cent + (int64_t)j * d, d);
}

// The visit order: visited slot seg_offs[s] + (rank of the row's id among the ids of its partition) takes the row.  A lane counts the
// smaller ids of its own partition (equal ids: the earlier stored row first) -- n_p reads per row, all lanes of a wave on one address.
// That is n_p^2 reads per partition: fine at a few times the target size (DESIGN.md 4c.1 has the figure), seconds for a partition of a
// million rows -- a key sort of (segment, id) is the follow-up that bounds it.
__global__ __launch_bounds__(256) void rb_visit_kernel(const uint64_t *__restrict__ row_ids, const uint32_t *__restrict__ seg_offs,
                                                       const uint32_t *__restrict__ seg_start, int nseg, int64_t n_vis,
                                                       uint64_t *__restrict__ vis_ids, uint32_t *__restrict__ vis_pos) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_vis; i += (int64_t)gridDim.x * 256) {
    const uint32_t s = rb_partition_of(seg_offs, nseg, (uint32_t)i);
    const uint32_t local = (uint32_t)i - seg_offs[s], len = seg_offs[s + 1] - seg_offs[s], base = seg_start[s];
    const uint64_t id = row_ids[base + local];
    uint32_t rank = 0;
    for (uint32_t j = 0; j < len; ++j) {
      const uint64_t other = row_ids[base + j];
      rank += (other < id || (other == id && j < local)) ? 1u : 0u;
    }
    vis_ids[seg_offs[s] + rank] = id;
    vis_pos[seg_offs[s] + rank] = base + local;
  }
}

// key of every stored row: its partition in the new numbering; none for the rows of `part` (they all leave)
__global__ __launch_bounds__(256) void rb_keys_kernel(const uint32_t *__restrict__ offs, int nlist, int64_t n, uint32_t part, int join,
                                                      uint32_t *__restrict__ keys) {
  for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x; r < n; r += (int64_t)gridDim.x * 256) {
    const uint32_t p = rb_partition_of(offs, nlist, (uint32_t)r);
    keys[r] = p == part ? RB_NONE : ((join && p > part) ? p - 1 : p);
  }
}

// ... and none for the rows of a candidate that move (visited slots from `first` on)
__global__ __launch_bounds__(256) void rb_keys_moved_kernel(const uint32_t *__restrict__ dest, const uint32_t *__restrict__ vis_pos, int64_t first,
                                                            int64_t n_vis, uint32_t *__restrict__ keys) {
  for (int64_t i = first + (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_vis; i += (int64_t)gridDim.x * 256)
    if (dest[i] != RB_NONE) keys[vis_pos[i]] = RB_NONE;
}

// the arriving rows in grouped order: raw vector, row id and (given) partition id of arrival i
__global__ __launch_bounds__(256) void rb_gather_kernel(const float *__restrict__ raw, const uint64_t *__restrict__ vis_ids,
                                                        const uint32_t *__restrict__ perm, const uint32_t *__restrict__ arr_offs, int nlist,
                                                        int64_t n_arr, int d, float *__restrict__ x, uint64_t *__restrict__ ids,
                                                        uint32_t *__restrict__ part) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n_arr * d; g += (int64_t)gridDim.x * 256) {
    const int64_t i = g / d;
    const int c = (int)(g - i * d);
    const uint64_t id = vis_ids[perm[i]];
    x[g] = raw[id * (uint64_t)d + c];
    if (c == 0) {
      ids[i] = id;
      part[i] = rb_partition_of(arr_offs, nlist, (uint32_t)i);
    }
  }
}

// SQ codes [n][d] -> the handle's padded rows [n][ld]
__global__ __launch_bounds__(256) void rb_pad_kernel(const uint8_t *__restrict__ codes, int64_t n, int d, int ld, uint8_t *__restrict__ out) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n * ld; g += (int64_t)gridDim.x * 256) {
    const int64_t i = g / ld;
    const int c = (int)(g - i * ld);
    out[g] = c < d ? codes[i * d + c] : (uint8_t)0;
  }
}

static unsigned rb_grid(uint64_t items) { return grid_stride_blocks(items, 256, 65536); }
static uint32_t rb_order_key(float f) {
  uint32_t b;
  memcpy(&b, &f, 4);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

// the arriving rows x [n][d] (raw vectors, grouped) through the index's own transform chain with the partition id given -> what the
// handle stores per row (`*enc`, rows `*enc_stride` bytes apart) and, for IVF_SQ, the sums of squared codes
static int rb_encode(lance_hip_ctx *ctx, const lance_hip_index *ix, float *x, uint64_t n, const uint32_t *part, const uint8_t **enc,
                     int64_t *enc_stride, const uint32_t **xx) {
  const uint32_t d = ix->d;
  const int kind = iu_kind(ix);
  *xx = nullptr;
  if (ix->metric == LANCE_HIP_COSINE) {      // NormalizeTransformer ahead of everything else
    float *xn = ctx->scratch_t<float>("rebalance.norm", (size_t)n * d);
    if (!xn) return LANCE_HIP_ENOMEM;
    LH_TRY(lance_hip_normalize(ctx, LANCE_HIP_F32, x, n, d, xn));
    x = xn;
  }
  if (kind == IU_FLAT) {
    *enc = reinterpret_cast<const uint8_t *>(x); *enc_stride = (int64_t)d * 4;
    return LANCE_HIP_OK;
  }
  if (kind == IU_SQ) {
    uint8_t *codes = ctx->scratch_t<uint8_t>("rebalance.sqcodes", (size_t)n * d);
    uint8_t *padded = ctx->scratch_t<uint8_t>("rebalance.sqpad", (size_t)n * ix->sq_ld + (size_t)n * 4);
    if (!codes || !padded) return LANCE_HIP_ENOMEM;
    const double bounds[2] = {ix->sq_lo, ix->sq_hi};
    LH_TRY(lance_hip_sq_encode(ctx, LANCE_HIP_F32, x, n, d, bounds, codes));
    hipLaunchKernelGGL(rb_pad_kernel, dim3(rb_grid(n * ix->sq_ld)), dim3(256), 0, ctx->stream, codes, (int64_t)n, (int)d, (int)ix->sq_ld, padded);
    LH_CHECK_HIP(hipGetLastError());
    uint32_t *sums = reinterpret_cast<uint32_t *>(padded + (size_t)n * ix->sq_ld);      // (sq_ld is a multiple of 16: aligned)
    LH_TRY(sq_row_sums(ctx, padded, n, ix->sq_ld, sums));
    *enc = padded; *enc_stride = ix->sq_ld; *xx = sums;
    return LANCE_HIP_OK;
  }
  const float *enc_in = x;
  if (ix->metric != LANCE_HIP_DOT) {         // residual against the NEW partition's centroid (ix carries the new centroid array)
    float *res = ctx->scratch_t<float>("rebalance.residual", (size_t)n * d);
    if (!res) return LANCE_HIP_ENOMEM;
    LH_TRY(lance_hip_residual(ctx, LANCE_HIP_F32, x, n, d, ix->centroids, part, res));
    enc_in = res;
  }
  uint8_t *codes = ctx->scratch_t<uint8_t>("rebalance.pqcodes", (size_t)n * ix->code_bytes());
  if (!codes) return LANCE_HIP_ENOMEM;
  // the quantiser encodes with its own distance type, L2, whatever the index metric (see lance_hip_ivfpq_encode)
  LH_TRY(lance_hip_pq_encode(ctx, LANCE_HIP_F32, LANCE_HIP_L2, enc_in, n, d, ix->codebook, ix->m, ix->nbits, codes));
  *enc = codes; *enc_stride = ix->code_bytes();
  return LANCE_HIP_OK;
}

// c12 NULL: join
static int rb_rebalance(lance_hip_ctx *ctx, const lance_hip_index *src, uint32_t part, const float *c12, const float *raw, uint64_t n_raw,
                        lance_hip_index **out) {
  const bool join = c12 == nullptr;
  const uint32_t lists = iu_lists(src), d = src->d, stride = iu_stride(src);
  const uint32_t lists_new = join ? lists - 1 : lists + 1;
  const uint64_t n = src->n;
  const std::vector<uint32_t> &so = src->part_offsets_h;
  // ---- the candidates: the nearest min(65, nlist) centroids of c0 by (distance in total order, id), without P, at most 64
  float *cdist = ctx->scratch_t<float>("rebalance.cdist", lists);
  if (!cdist) return LANCE_HIP_ENOMEM;
  {
    const dim3 grid((unsigned)cdiv(lists, 256));
    if (src->metric == LANCE_HIP_L2) hipLaunchKernelGGL(rb_centroid_dist_kernel<METRIC_L2>, grid, dim3(256), 0, ctx->stream, src->centroids, (int)lists, (int)d, (int)part, cdist);
    else if (src->metric == LANCE_HIP_COSINE) hipLaunchKernelGGL(rb_centroid_dist_kernel<METRIC_COSINE>, grid, dim3(256), 0, ctx->stream, src->centroids, (int)lists, (int)d, (int)part, cdist);
    else hipLaunchKernelGGL(rb_centroid_dist_kernel<METRIC_DOT>, grid, dim3(256), 0, ctx->stream, src->centroids, (int)lists, (int)d, (int)part, cdist);
    LH_CHECK_HIP(hipGetLastError());
  }
  std::vector<float> cdh(lists);
  LH_CHECK_HIP(hipMemcpyAsync(cdh.data(), cdist, (size_t)lists * 4, hipMemcpyDeviceToHost, ctx->stream));
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  std::vector<uint32_t> order(lists);
  for (uint32_t p = 0; p < lists; ++p) order[p] = p;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    const uint32_t ka = rb_order_key(cdh[a]), kb = rb_order_key(cdh[b]);
    return ka != kb ? ka < kb : a < b;
  });
  const uint32_t range = std::min<uint32_t>((uint32_t)RB_MAX_CAND + 1, lists);
  std::vector<uint32_t> cands;
  for (uint32_t i = 0; i < range && cands.size() + 1 < range; ++i)
    if (order[i] != part) cands.push_back(order[i]);
  const uint32_t C = (uint32_t)cands.size();
  // ---- the visited rows: P, then (split) the candidates
  // small[]: seg_offs [C + 2] | seg_start [C + 1] | cand ids in the new numbering [C] | table rows [C + 1]
  std::vector<uint32_t> small((size_t)4 * C + 4, 0);
  uint32_t *seg = small.data(), *start = seg + C + 2, *cnew = start + C + 1, *tab = cnew + C;
  for (uint32_t s = 0; s <= C; ++s) {
    const uint32_t p = s == 0 ? part : cands[s - 1];
    start[s] = so[p];
    seg[s + 1] = seg[s] + ((s == 0 || !join) ? so[p + 1] - so[p] : 0u);
    tab[s] = p;
    if (s > 0) cnew[s - 1] = (join && p > part) ? p - 1 : p;
  }
  const uint64_t n_vis = seg[C + 1];
  uint32_t *small_d = ctx->scratch_t<uint32_t>("rebalance.small", small.size());
  float *seg_cent = ctx->scratch_t<float>("rebalance.segcent", (size_t)(C + 1) * d);
  uint64_t *vis_ids = ctx->scratch_t<uint64_t>("rebalance.visids", (size_t)(n_vis ? n_vis : 1));
  uint32_t *vis_pos = ctx->scratch_t<uint32_t>("rebalance.vispos", (size_t)(n_vis ? n_vis : 1));
  uint32_t *dest = ctx->scratch_t<uint32_t>("rebalance.dest", (size_t)(n_vis ? n_vis : 1));
  if (!small_d || !seg_cent || !vis_ids || !vis_pos || !dest) return LANCE_HIP_ENOMEM;
  const uint32_t *seg_d = small_d, *start_d = small_d + C + 2, *cnew_d = start_d + C + 1, *tab_d = cnew_d + C;
  LH_CHECK_HIP(hipMemcpyAsync(small_d, small.data(), small.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  LH_TRY(iu_copy(ctx, src->centroids, seg_cent, C + 1, (int64_t)d * 4, (int64_t)d * 4, (int)d * 4, tab_d, nullptr, nullptr, lists));
  if (n_vis > 0) {
    ScopedTimer t(ctx, "rebalance_visit");
    hipLaunchKernelGGL(rb_visit_kernel, dim3(rb_grid(n_vis)), dim3(256), 0, ctx->stream, src->row_ids, seg_d, start_d, (int)(C + 1), (int64_t)n_vis,
                       vis_ids, vis_pos);
    LH_CHECK_HIP(hipGetLastError());
  }
  LH_TRY(lance_hip_reassign_rows(ctx, src->metric, join ? LANCE_HIP_REASSIGN_JOIN : LANCE_HIP_REASSIGN_SPLIT, raw, n_raw, d, vis_ids, n_vis, seg_d,
                                 seg_cent, cnew_d, C, c12, part, lists, dest));      // (synchronises; a stored id >= n_raw ends the call here)
  // ---- who stays, who arrives: two stable groupings
  uint32_t *keys = ctx->scratch_t<uint32_t>("index_update.keys", (size_t)(n ? n : 1));
  uint32_t *perm_s = ctx->scratch_t<uint32_t>("index.perm", (size_t)(n ? n : 1));
  uint32_t *perm_a = ctx->scratch_t<uint32_t>("rebalance.perm", (size_t)(n_vis ? n_vis : 1));
  uint32_t *offs_d = ctx->scratch_t<uint32_t>("rebalance.offs", (size_t)4 * (lists_new + 1));      // survivors | arrivals | base of either
  if (!keys || !perm_s || !perm_a || !offs_d) return LANCE_HIP_ENOMEM;
  uint32_t *surv_d = offs_d, *arr_d = offs_d + lists_new + 1, *base_d = arr_d + lists_new + 1;
  if (n > 0) {
    hipLaunchKernelGGL(rb_keys_kernel, dim3(rb_grid(n)), dim3(256), 0, ctx->stream, src->part_offsets, (int)lists, (int64_t)n, part, join ? 1 : 0, keys);
    if (!join && n_vis > seg[1])
      hipLaunchKernelGGL(rb_keys_moved_kernel, dim3(rb_grid(n_vis - seg[1])), dim3(256), 0, ctx->stream, dest, vis_pos, (int64_t)seg[1], (int64_t)n_vis, keys);
    LH_CHECK_HIP(hipGetLastError());
  }
  LH_TRY(stable_group(ctx, keys, (int64_t)n, (int64_t)n, (int)lists_new, 1, surv_d, perm_s, (int64_t)n, nullptr));
  LH_TRY(stable_group(ctx, dest, (int64_t)n_vis, (int64_t)n_vis, (int)lists_new, 1, arr_d, perm_a, (int64_t)n_vis, nullptr));
  std::vector<uint32_t> sa((size_t)2 * (lists_new + 1));
  LH_CHECK_HIP(hipMemcpyAsync(sa.data(), offs_d, sa.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  const uint32_t *sh = sa.data(), *ah = sa.data() + lists_new + 1;
  const uint64_t n_s = sh[lists_new], n_a = ah[lists_new];
  LH_REQUIRE(sh[0] == 0 && ah[0] == 0 && n_s + n_a == n, "index split / join: grouping kept %llu + %llu of %llu rows", (unsigned long long)n_s,
             (unsigned long long)n_a, (unsigned long long)n);
  std::vector<uint32_t> offs(lists_new + 1, 0), base((size_t)2 * lists_new);
  for (uint32_t p = 0; p < lists_new; ++p) {
    base[p] = offs[p];
    base[lists_new + p] = offs[p] + (sh[p + 1] - sh[p]);
    offs[p + 1] = base[lists_new + p] + (ah[p + 1] - ah[p]);
  }
  LH_CHECK_HIP(hipMemcpyAsync(base_d, base.data(), base.size() * 4, hipMemcpyHostToDevice, ctx->stream));
  // ---- the new handle: its centroid array first
  float *cent_new = ctx->scratch_t<float>("rebalance.cent", (size_t)lists_new * d);
  if (!cent_new) return LANCE_HIP_ENOMEM;
  const size_t rowb = (size_t)d * 4;
  if (join) {      // row P leaves
    if (part > 0) LH_CHECK_HIP(hipMemcpyAsync(cent_new, src->centroids, part * rowb, hipMemcpyDeviceToDevice, ctx->stream));
    if (part + 1 < lists) LH_CHECK_HIP(hipMemcpyAsync(cent_new + (size_t)part * d, src->centroids + (size_t)(part + 1) * d, (lists - part - 1) * rowb, hipMemcpyDeviceToDevice, ctx->stream));
  } else {         // c1 replaces row P, c2 is appended
    LH_CHECK_HIP(hipMemcpyAsync(cent_new, src->centroids, lists * rowb, hipMemcpyDeviceToDevice, ctx->stream));
    LH_CHECK_HIP(hipMemcpyAsync(cent_new + (size_t)part * d, c12, rowb, hipMemcpyDeviceToDevice, ctx->stream));
    LH_CHECK_HIP(hipMemcpyAsync(cent_new + (size_t)lists * d, c12 + d, rowb, hipMemcpyDeviceToDevice, ctx->stream));
  }
  lance_hip_index *ix = nullptr;
  LH_TRY(iu_new_like(ctx, src, cent_new, lists_new, &ix));
  auto body = [&]() -> int {
    LH_TRY(iu_alloc_rows(ix, n));
    // survivors: grouped row r is stored row perm_s[r]; it goes behind the survivors before it in its partition
    LH_TRY(iu_copy(ctx, iu_payload(src), iu_payload(ix), n_s, stride, stride, (int)stride, perm_s, surv_d, base_d, lists_new));
    LH_TRY(iu_copy(ctx, src->row_ids, ix->row_ids, n_s, 8, 8, 8, perm_s, surv_d, base_d, lists_new));
    if (ix->sq) LH_TRY(iu_copy(ctx, src->sq_xx, const_cast<uint32_t *>(ix->sq_xx), n_s, 4, 4, 4, perm_s, surv_d, base_d, lists_new));
    if (n_a > 0) {
      float *x = ctx->scratch_t<float>("rebalance.x", (size_t)n_a * d);
      uint64_t *ids_a = ctx->scratch_t<uint64_t>("rebalance.ids", (size_t)n_a);
      uint32_t *part_a = ctx->scratch_t<uint32_t>("rebalance.part", (size_t)n_a);
      if (!x || !ids_a || !part_a) return LANCE_HIP_ENOMEM;
      hipLaunchKernelGGL(rb_gather_kernel, dim3(rb_grid(n_a * d)), dim3(256), 0, ctx->stream, raw, vis_ids, perm_a, arr_d, (int)lists_new, (int64_t)n_a,
                         (int)d, x, ids_a, part_a);
      LH_CHECK_HIP(hipGetLastError());
      const uint8_t *enc = nullptr;
      const uint32_t *xx = nullptr;
      int64_t enc_stride = 0;
      LH_TRY(rb_encode(ctx, ix, x, n_a, part_a, &enc, &enc_stride, &xx));
      const int row_bytes = (int)std::min<int64_t>(enc_stride, stride);
      LH_TRY(iu_copy(ctx, enc, iu_payload(ix), n_a, enc_stride, stride, row_bytes, nullptr, arr_d, base_d + lists_new, lists_new));
      LH_TRY(iu_copy(ctx, ids_a, ix->row_ids, n_a, 8, 8, 8, nullptr, arr_d, base_d + lists_new, lists_new));
      if (ix->sq) LH_TRY(iu_copy(ctx, xx, const_cast<uint32_t *>(ix->sq_xx), n_a, 4, 4, 4, nullptr, arr_d, base_d + lists_new, lists_new));
    }
    const bool finite = ix->model_finite;      // (an IVF_PQ handle has judged its own new model)
    LH_TRY(iu_finish_layout(ctx, ix, src, offs));
    if (iu_kind(src) == IU_PQ) ix->model_finite = finite;
    return LANCE_HIP_OK;
  };
  const int r = body();
  if (r != LANCE_HIP_OK) { delete ix; return r; }
  *out = ix;
  return LANCE_HIP_OK;
}

static int rb_check(lance_hip_ctx *ctx, const lance_hip_index *src, uint32_t part, const float *raw, lance_hip_index **out, const char *what) {
  LH_REQUIRE(ctx && out, "%s: NULL argument", what);
  LH_TRY(iu_check_handle(ctx, src, what));
  LH_REQUIRE(src->dtype == LANCE_HIP_F32, "%s: f32 columns only in this version (the handle holds %s vectors)", what,
             src->dtype == LANCE_HIP_F16 ? "f16" : "int8");
  LH_REQUIRE(part < iu_lists(src), "%s: partition %u does not exist (nlist = %u)", what, part, iu_lists(src));
  LH_REQUIRE(raw, "%s: the raw vectors are needed (rows are re-assigned and re-encoded from them)", what);
  return LANCE_HIP_OK;
}

}  // namespace lh

extern "C" int lance_hip_index_split(lance_hip_ctx *ctx, const lance_hip_index *src, uint32_t part, const float *centroids2, const float *raw,
                                     uint64_t n_raw, lance_hip_index **out) {
  lh::CtxLock _ctx_lock(ctx);
  LH_TRY(rb_check(ctx, src, part, raw, out, "index_split"));
  LH_REQUIRE(centroids2, "index_split: the two new centroids are needed");
  const uint32_t rows = src->part_offsets_h[part + 1] - src->part_offsets_h[part];
  LH_REQUIRE(rows >= 2, "index_split: partition %u holds %u rows, a split needs at least 2", part, rows);
  LH_REQUIRE(iu_lists(src) + 1 <= 65536, "index_split: nlist + 1 = %u exceeds the 65536 partitions a handle holds", iu_lists(src) + 1);
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  return rb_rebalance(ctx, src, part, centroids2, raw, n_raw, out);
}

extern "C" int lance_hip_index_join(lance_hip_ctx *ctx, const lance_hip_index *src, uint32_t part, const float *raw, uint64_t n_raw,
                                    lance_hip_index **out) {
  lh::CtxLock _ctx_lock(ctx);
  LH_TRY(rb_check(ctx, src, part, raw, out, "index_join"));
  LH_REQUIRE(iu_lists(src) > 1, "index_join: nlist == 1: the only partition has no neighbour to join");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  return rb_rebalance(ctx, src, part, nullptr, raw, n_raw, out);
}
