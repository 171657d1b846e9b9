// flat_mfma_f16.hip -- batched flat scan of a FLOAT16 column on the f16 matrix cores: the column and the query batch are read as they
// are stored (no f32 copy, no bf16 plane, no conversion between HBM and the matrix pipe), v_mfma_f32_32x32x16_f16 filters the
// (query, row) pairs, and the few that can beat a query's threshold are recomputed in the reference's arithmetic from the same f16 rows.
//
//   half::f16 distance functions     l2.rs:57-91,128-159 (l2_scalar::<f16, f32, 16>), dot.rs:91-102 (dot_scalar::<f16, f32, 32>),
//                                    cosine.rs:171-179 (cosine_scalar), norm_l2.rs:60-85             (the exact arithmetic kept)
//   final SortExec / pool selection  scanner.rs:3386-3411                                           (flat.hip: select kernel)
//
// Before this file an f16 column under dot / cosine was widened to f32 on every call (as_f32: 2 bytes read, 4 written per element) and
// scanned pair by pair on the VALU (flat_scan_generic_kernel<.., H32>); under L2 outside the fixed dimensions it was widened and then
// rounded to a bf16 plane (flat_mfma_wide.hip) -- three passes over HBM and a 0.84 % margin on rows that were exact in half precision.
//
// Kernels (driven by flat_topk_f16 in flat.hip: flat_topk_v2's epoch loop, pool and repair):
//   fh_norms_kernel    one pass per call over the column, and one per chunk over the queries: |v|^2 summed in f32 from the f16 elements
//                      (a 16-lane group per vector, 16-byte loads), O(n) floats of scratch.  A vector the filter must not judge gets
//                      the SENTINEL (NaN) instead: an inf / NaN element, more than 2^-11 of its norm in subnormal elements (below), and under
//                      cosine a zero vector (0 / 0: the exact arithmetic's NaN decides, whatever its sign).
//   fh_filter_kernel   a workgroup of four waves (2 x 2) owns 128 rows x 128 queries and walks d in stages of 64 elements:
//                      global -> registers (16-byte loads of the caller's column and query batch, the next stage in flight under the
//                      matrix work) -> LDS (rows of 64 + 8 halves: 144-byte stride, conflict-free ds_read_b128) ->
//                      v_mfma_f32_32x32x16_f16, queries down the accumulator registers and rows across the lanes.  Tails never touch
//                      memory: elements past d (d % 8 == 0, so a 16-byte piece is inside or outside), rows past the epoch and query
//                      slots past the chunk are zeros written to LDS.  Epilogue: one fused multiply-add per pair against the lane's row
//                      constant and the query's threshold term, folded into a running minimum; only a lane whose minimum passes (or
//                      whose row carries the sentinel) looks for its pairs and appends the row to those queries' queues
//                      (FLAT_MC_QUEUE_CAP entries; an overflow raises the pool-overflow flag and flat.hip's repair loop rescans).
//                      The one-dimensional grid is ordered XCD-aware as in flat_mfma_wide.hip: the query tiles of a row tile run
//                      back to back on one XCD, so the row tile comes from HBM once.
//                      gfx950, -O3 (-Rpass-analysis=kernel-resource-usage): 144 VGPRs (64 of them the accumulators), 0 AGPRs, no
//                      scratch, 37,632 bytes of LDS: three waves per SIMD by registers, four workgroups per CU by LDS.
//   fh_eval_kernel     one workgroup per query, a lane per queued row: the f16 row is read natively and scored with the function the
//                      route before this one used -- L2 dist_exact_rt<L2, __half, 16, SWAP>, dot the 32-lane order, cosine
//                      cosine_scalar32_rt -- then the pool's (key, row id) test and entry, as in every other filter.
//   fh_exact_kernel    the exact any-dimension filter for the first epoch (FLAT_CAP / 2 rows, which gives every query a threshold)
//                      and the repair: lanes own queries, a workgroup walks a slice of rows, the same three functions on the f16 rows.
//
// Margin.  An f16 x f16 product is exact in f32 (11 x 11 significant bits), so the surrogate p~ of x.q errs only by
//   (a) the f32 accumulation of d products: <= d 2^-23 |x||q|  (the project's convention: twice the textbook bound, whatever the pipe
//       rounds inside);
//   (f) f16 SUBNORMAL inputs, should the matrix pipe flush them (not established for gfx950; search_ms.hip assumes it does).  The
//       products that then go missing are those of x's subnormal elements S_x and of q's, at most sx |q| + sq |x| by Cauchy-Schwarz with
//       sx = the norm of x's subnormal elements.  fh_norms_kernel sums sx^2 beside |x|^2 and hands out the sentinel when
//       sx > 2^-11 |x|, so for every judged pair (f) <= 2^-10 |x||q|.  2^-11 is what a unit-norm row needs: each subnormal element is
//       below 2^-14, so 64 of them stay under it however large they are, and a normalised 768-d embedding has one or two (its elements
//       fall under 2^-14 about once per row).  A bound of d 2^-23, this file's first version, made 0.4 % of such a column's rows
//       sentinel rows: every query queued them all, the queues overflowed and the repair scanned the column with the exact kernel
//       (profiles/flat_f16_mc.json, note).  A term of 2^-14 per element, as search_ms.hip carries, would be 3.4e-3 |x||q| at d = 768.
//       Right under both behaviours: if nothing is flushed, nothing is missing.
// The other terms:
//   (n) this file's norm sums, any order of d non-negative exact squares: <= d 2^-24 relative, each;
//   (r) the reference's own f32 evaluation against the real value: <= (d + 4) 2^-24 -- of the distance under L2 (one rounding of the
//       difference, one of the square, the sums), of |x||q| for its dot product, of 1 for each of the two norms under cosine;
//   (t) the test's own arithmetic, at most six roundings of quantities <= 1 + |x|^2 + |q|^2: 2^-19 covers it with room.
// With N = |x|^2 + |q|^2 >= 2 |x||q| and true L2 distance <= 2 N:
//   L2      the reference's value >= N~ - 2 p~ - [ (a) + (f) + (n) + 2 (r) ] N       test  N~ (1 - E) - 2 p~ <= T
//   dot     its 1 - x.q     >= 1 - p~ - [ (a) + (f) + (r) ] N / 2, and f32 values of 1 - x.q closer than an ulp of 1 tie (2^-22, the
//           wide filter's term, doubled for this test's own roundings near 1)         test  1 - p~ - E N~ / 2 - 2^-21 <= T
//   cosine  its 1 - x.q / (|x||q|) >= 1 - p~ / (|x|~ |q|~) - [ (a) + (f) + (n) + 2 (r) + 2^-21 ]   test  (1 - E - T) |q|~ |x|~ - p~ <= 0
//   E = ((5 d + 8) 2^-24 + 2^-10 + 2^-19) (1 + 2^-9)   -- d 2^-23 + d 2^-24 + 2 (d + 4) 2^-24, (f), (t); the last factor for N~ against N --
// computed on the host from d, per call (fh_margin): 1.2e-3 at d = 768, 2.2e-3 at d = 4096, against the bf16 route's fixed 8.4e-3.
// It is derived, not tuned.  No finite f16 input overflows an f32 norm or product at d <= 4096 (4096 x 65504^2 = 1.8e13) and no square
// of a nonzero f16 is an f32 denormal (>= 2^-48), so the only other special cases are an inf or NaN element -- a norm that is not
// finite -- and the sentinel takes them.  A filter only widens: a pair that passes is decided by the exact arithmetic.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "exact.cuh"
#include "grid.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace lh {

typedef _Float16 fh_f16x8 __attribute__((ext_vector_type(8)));
typedef float fh_f32x16 __attribute__((ext_vector_type(16)));

constexpr int FH_KT = 64;             // elements of d per stage
constexpr int FH_LS = FH_KT + 8;      // LDS row stride in halves: 144 bytes
constexpr int FH_TM = 128, FH_TN = 128;      // rows x queries of a workgroup tile
constexpr int FH_EX_ROWS = 8;         // rows a workgroup of fh_exact_kernel walks

static float fh_margin(int d) { return ((5.0f * (float)d + 8.0f) * 5.9604645e-8f + 9.765625e-4f + 1.9073486e-6f) * (1.0f + 0.001953125f); }

// |v|^2 of every vector (rows of the column, or the queries of a chunk), or the sentinel NaN (header).  One 16-lane group per vector,
// 16-byte loads; the grid strides over groups of four vectors (grid.h).  sub_r2 = (2^-11)^2.
__global__ __launch_bounds__(256) void fh_norms_kernel(const __half *__restrict__ v, int64_t n, int d, float sub_r2, int zero_is_odd,
                                                       float *__restrict__ out) {
  const int lane = threadIdx.x & 63, i = lane & 15;
  for (int64_t r0 = ((int64_t)blockIdx.x * 256 + (threadIdx.x & ~63)) >> 4; r0 < n; r0 += (int64_t)gridDim.x * 16) {
    const int64_t row = r0 + (lane >> 4);
    float s = 0.0f, ssub = 0.0f;
    if (row < n) {
      const uint4 *src = reinterpret_cast<const uint4 *>(v + row * d);
      for (int pc = i; pc < d / 8; pc += 16) {
        const uint4 u = src[pc];
        const uint32_t w[4] = {u.x, u.y, u.z, u.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint16_t h = (uint16_t)(w[e >> 1] >> (16 * (e & 1)));
          const float f = __half2float(__ushort_as_half(h));
          const float sq = f * f;
          s += sq;
          if ((h & 0x7C00u) == 0) ssub += sq;      // exponent field 0: a subnormal (or a zero, which adds nothing)
        }
      }
    }
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) { s += __shfl_xor(s, o, 64); ssub += __shfl_xor(ssub, o, 64); }
    if (row < n && i == 0) {
      const bool odd = !(s < INFINITY) || ssub > sub_r2 * s || (zero_is_odd && s == 0.0f);
      out[row] = odd ? __uint_as_float(0x7FC00000u) : s;
    }
  }
}

// norm_l2_impl::<f16, f32, 32> of every query (the x_norm of cosine_scalar), from the widened copy the exact functions read
__global__ __launch_bounds__(64) void fh_qnorm32_kernel(const float *__restrict__ q, int nq, int d, float *__restrict__ out) {
  const int qi = blockIdx.x * 64 + threadIdx.x;
  if (qi < nq) out[qi] = norm_l2_rt<float, 32>(q + (int64_t)qi * d, d);
}

struct FhArgs {
  FlatPool p;                  // p.x_native: the f16 column; p.q: the chunk's queries widened to f32 (the exact functions' operand)
  const __half *qh;            // [nq][d] the chunk's queries as the caller stored them (the matrix operand)
  const float *xn2;            // [n] |x|^2 or the sentinel (ALL rows of the call: indexed by absolute row)
  const float *qn2;            // [nq] |q|^2 or the sentinel
  uint32_t *scnt;              // [nq] queued rows of this epoch
  uint32_t *squeue;            // [nq][FLAT_MC_QUEUE_CAP] rows (relative to p.r0) whose surrogate distance passed
  int d;
  float E;                     // fh_margin(d)
  uint32_t nqt, nrt;           // query tiles, row tiles
};

template <int METRIC>
__device__ __forceinline__ float fh_side(float tq, float xk, float dot) {
  if constexpr (METRIC == METRIC_COSINE) return __builtin_fmaf(tq, xk, -dot);      // (1 - E - T) |q| |x| - p~
  else if constexpr (METRIC == METRIC_DOT) return (xk - tq) - dot;                 // 1 - E |x|^2 / 2 - (T + E |q|^2 / 2 + 2^-21) - p~
  else return __builtin_fmaf(-2.0f, dot, xk - tq);                                 // |x|^2 (1 - E) - (T - |q|^2 (1 - E)) - 2 p~
}

template <int METRIC>
__global__ __launch_bounds__(256, 2) void fh_filter_kernel(FhArgs a) {
  __shared__ __attribute__((aligned(16))) _Float16 Xs[FH_TM * FH_LS];
  __shared__ __attribute__((aligned(16))) _Float16 Qs[FH_TN * FH_LS];
  __shared__ __attribute__((aligned(16))) float tqs[FH_TN];
  const FlatPool &p = a.p;
  const int d = a.d;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, g = lane >> 5;
  const int wr = wave >> 1, wq = wave & 1;
  // XCD-aware tile order (flat_mfma_wide.hip): block b = 8 i + x takes row tile 8 (i / nqt) + x and query tile i % nqt
  const uint32_t xi = blockIdx.x >> 3, xc = blockIdx.x & 7u;
  const uint32_t rt = (xi / a.nqt) * 8u + xc;
  if (rt >= a.nrt) return;      // (the grid is padded to whole groups of eight row tiles)
  const int q0 = (int)(xi % a.nqt) * FH_TN;
  const int64_t row0 = p.r0 + (int64_t)rt * FH_TM;

  // per-query threshold term; NaN = the query takes every row (its sentinel, or a threshold that is a NaN)
  int q_odd = 0;
  if (threadIdx.x < FH_TN) {
    const int qi = q0 + threadIdx.x;
    float t;
    if (qi < p.nq) {
      const uint32_t tk = p.tkey[qi];
      const float T = tk >= 0xFF800000u ? INFINITY : key_to_float(tk);      // no threshold yet: every row is a candidate
      const float qn = a.qn2[qi];
      if constexpr (METRIC == METRIC_COSINE) t = (1.0f - a.E - T) * sqrtf(qn);
      else if constexpr (METRIC == METRIC_DOT) t = T + 0.5f * a.E * qn + 4.7683716e-7f;
      else t = T - (qn - a.E * qn);
      q_odd = t != t;
    } else {
      t = METRIC == METRIC_COSINE ? INFINITY : -INFINITY;      // padded query: nothing passes (and the queue test checks qi < nq)
    }
    tqs[threadIdx.x] = t;
  }

  // staging: thread (r, h) moves half a stage (32 elements = four 16-byte pieces) of row r and of query r
  const int sr = threadIdx.x >> 1, sh = threadIdx.x & 1;
  const bool xrow_ok = row0 + sr < p.r1, qrow_ok = q0 + sr < p.nq;
  const __half *xsrc = static_cast<const __half *>(p.x_native) + (row0 + sr) * (int64_t)d + sh * 32;
  const __half *qsrc = a.qh + (int64_t)(q0 + sr) * d + sh * 32;
  uint4 px[4], pq[4];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool in = k0 + sh * 32 + u * 8 < d;      // d % 8 == 0: a 16-byte piece is inside or outside
      px[u] = (xrow_ok && in) ? *reinterpret_cast<const uint4 *>(xsrc + k0 + u * 8) : make_uint4(0, 0, 0, 0);
      pq[u] = (qrow_ok && in) ? *reinterpret_cast<const uint4 *>(qsrc + k0 + u * 8) : make_uint4(0, 0, 0, 0);
    }
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      *reinterpret_cast<uint4 *>(&Xs[sr * FH_LS + sh * 32 + u * 8]) = px[u];
      *reinterpret_cast<uint4 *>(&Qs[sr * FH_LS + sh * 32 + u * 8]) = pq[u];
    }
  };

  fh_f32x16 acc[2][2];
#pragma unroll
  for (int bi = 0; bi < 2; ++bi)
#pragma unroll
    for (int bj = 0; bj < 2; ++bj)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[bi][bj][v] = 0.0f;

  fetch(0);
  store();
  const bool tile_qodd = __syncthreads_or(q_odd) != 0;      // some query of the tile takes every row: all lanes walk the pairs
  for (int k0 = 0; k0 < d; k0 += FH_KT) {
    const bool more = k0 + FH_KT < d;
    if (more) fetch(k0 + FH_KT);
#pragma unroll
    for (int s = 0; s < FH_KT / 16; ++s) {
      fh_f16x8 aq[2], bx[2];
#pragma unroll
      for (int b = 0; b < 2; ++b) aq[b] = *reinterpret_cast<const fh_f16x8 *>(&Qs[(wq * 64 + b * 32 + j) * FH_LS + s * 16 + g * 8]);
#pragma unroll
      for (int b = 0; b < 2; ++b) bx[b] = *reinterpret_cast<const fh_f16x8 *>(&Xs[(wr * 64 + b * 32 + j) * FH_LS + s * 16 + g * 8]);
#pragma unroll
      for (int bi = 0; bi < 2; ++bi)
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(aq[bj], bx[bi], acc[bi][bj], 0, 0, 0);
    }
    __syncthreads();      // every wave has read this stage
    if (more) store();
    __syncthreads();
  }

  // epilogue: lane (j, g) of block (bi, bj) holds row j of the row block against the queries (v & 3) + 8 (v >> 2) + 4 g of the query block
#pragma unroll
  for (int bi = 0; bi < 2; ++bi) {
    const int64_t row = row0 + wr * 64 + bi * 32 + j;
    const bool rvalid = row < p.r1;
    float xk = 0.0f;        // per-row constant of the test; NaN = the sentinel: every query takes the row
    if (rvalid) {
      const float n2 = a.xn2[row];
      if constexpr (METRIC == METRIC_COSINE) xk = sqrtf(n2);
      else if constexpr (METRIC == METRIC_DOT) xk = 1.0f - 0.5f * a.E * n2;
      else xk = n2 - a.E * n2;
    }
    const bool odd = xk != xk;
    float mn = INFINITY;
#pragma unroll
    for (int bj = 0; bj < 2; ++bj) {
      const float *tqb = tqs + wq * 64 + bj * 32 + 4 * g;
#pragma unroll
      for (int vq = 0; vq < 4; ++vq) {
        const f4 t4 = *reinterpret_cast<const f4 *>(tqb + 8 * vq);
#pragma unroll
        for (int e = 0; e < 4; ++e) mn = __builtin_fminf(mn, fh_side<METRIC>(t4[e], xk, acc[bi][bj][4 * vq + e]));      // (a NaN is ignored here and fails `<=` below)
      }
    }
    if ((mn <= 0.0f || odd || tile_qodd) && rvalid) {      // rare per lane: find the pairs, queue the row for each of their queries
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) {
        const float *tqb = tqs + wq * 64 + bj * 32 + 4 * g;
#pragma unroll
        for (int vq = 0; vq < 4; ++vq) {
          const f4 t4 = *reinterpret_cast<const f4 *>(tqb + 8 * vq);
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int qi = q0 + wq * 64 + bj * 32 + 8 * vq + 4 * g + e;
            const bool pass = qi < p.nq && (odd || t4[e] != t4[e] || fh_side<METRIC>(t4[e], xk, acc[bi][bj][4 * vq + e]) <= 0.0f);
            if (pass) {
              const uint32_t pos = atomicAdd(&a.scnt[qi], 1u);
              if (pos < (uint32_t)FLAT_MC_QUEUE_CAP) a.squeue[(int64_t)qi * FLAT_MC_QUEUE_CAP + pos] = (uint32_t)(row - p.r0);
            }
          }
        }
      }
    }
  }
}

// the reference's value of one (query, f16 row) pair: the functions the route before this one applied to the widened copy
template <int METRIC>
__device__ __forceinline__ float fh_exact_value(const float *__restrict__ qv, float qnorm, const __half *__restrict__ xr, int d) {
  if constexpr (METRIC == METRIC_COSINE) return cosine_scalar32_rt<__half>(qv, qnorm, xr, d);
  else if constexpr (METRIC == METRIC_DOT) return finish_metric<METRIC_DOT>(dist_exact_rt<METRIC_DOT, __half, 32>(qv, xr, d));
  else return dist_exact_rt<METRIC_L2, __half, 16, true>(qv, xr, d);      // (row - q: exact.cuh SWAP)
}

__device__ __forceinline__ void fh_pool_append(const FlatPool &p, int qi, uint32_t key, uint64_t rid, uint32_t tk, uint64_t tr) {
  if (key < tk || (key == tk && rid <= tr)) {
    const uint32_t pos = atomicAdd(&p.cnt[qi], 1u);
    if (pos < (uint32_t)p.cap) {
      p.pkeys[(int64_t)qi * p.cap + pos] = key;
      p.prids[(int64_t)qi * p.cap + pos] = rid;
    }
  }
}

// exact evaluation of the queued (query, row) pairs: one workgroup per query, one lane per queued row
template <int METRIC>
__global__ __launch_bounds__(256) void fh_eval_kernel(FhArgs a) {
  const FlatPool &p = a.p;
  const int d = a.d;
  const int qi = blockIdx.x;
  const uint32_t raw = a.scnt[qi];
  if (raw == 0) return;
  if (raw > (uint32_t)FLAT_MC_QUEUE_CAP && threadIdx.x == 0) atomicOr(p.overflow, 1u);   // rows were lost: the caller's repair loop rescans
  const int c = (int)min(raw, (uint32_t)FLAT_MC_QUEUE_CAP);
  const uint32_t tk = p.tkey[qi];
  const uint64_t tr = p.trid[qi];
  const float *qv = p.q + (int64_t)qi * d;
  const float qnorm = METRIC == METRIC_COSINE ? p.q_norm[qi] : 0.0f;
  const __half *xh = static_cast<const __half *>(p.x_native);
  for (int i = threadIdx.x; i < c; i += 256) {
    const int64_t row = p.r0 + (int64_t)a.squeue[(int64_t)qi * FLAT_MC_QUEUE_CAP + i];
    const uint64_t rid = p.row_ids ? p.row_ids[row] : (uint64_t)row;
    fh_pool_append(p, qi, order_key(fh_exact_value<METRIC>(qv, qnorm, xh + row * d, d)), rid, tk, tr);
  }
}

// exact filter, any dimension: lanes own queries, workgroup (bx, by) walks rows [r0 + 8 bx, + 8) for queries [256 by, + 256).  The row
// address is wave-uniform; it is not fast and does not have to be (2048 rows per chunk, and the repair).
template <int METRIC>
__global__ __launch_bounds__(256) void fh_exact_kernel(FlatPool p, int d) {
  const int qi = blockIdx.y * 256 + threadIdx.x;
  if (qi >= p.nq) return;
  const uint32_t tk = p.tkey[qi];
  const uint64_t tr = p.trid[qi];
  const float *qv = p.q + (int64_t)qi * d;
  const float qnorm = METRIC == METRIC_COSINE ? p.q_norm[qi] : 0.0f;
  const __half *xh = static_cast<const __half *>(p.x_native);
  const int64_t rb = p.r0 + (int64_t)blockIdx.x * FH_EX_ROWS;
  const int64_t re = min(p.r1, rb + FH_EX_ROWS);
  for (int64_t row = rb; row < re; ++row) {
    const uint64_t rid = p.row_ids ? p.row_ids[row] : (uint64_t)row;
    fh_pool_append(p, qi, order_key(fh_exact_value<METRIC>(qv, qnorm, xh + row * d, d)), rid, tk, tr);
  }
}

// Taken for f16 columns, L2 / dot / cosine, k <= 128, d % 8 == 0 in 8 .. 4096, query chunks of at least 128 (the wide filter's figure,
// taken over and not measured for this kernel), 16-byte aligned operands, no lower bound (an upper bound is only the start key).  L2 at a
// fixed dimension keeps the native fixed-dimension route.  LANCE_HIP_NO_MFMA / LANCE_HIP_NO_FLAT_F16_MC: the routes from before this file.
bool flat_mfma_f16_supported(int dtype, int metric, int d, int k, int nq, int64_t n, const void *x, const void *q, const FlatRange &rg) {
  static const bool off = getenv("LANCE_HIP_NO_MFMA") != nullptr || getenv("LANCE_HIP_NO_FLAT_F16_MC") != nullptr;
  if (off || dtype != LANCE_HIP_F16 || (metric != LANCE_HIP_L2 && metric != LANCE_HIP_DOT && metric != LANCE_HIP_COSINE)) return false;
  if (k > 128 || nq < 128 || d % 8 != 0 || d < 8 || d > 4096 || rg.has_lower) return false;
  if (metric == LANCE_HIP_L2 && (d == 8 || d == 16 || d == 32 || d == 64 || d == 96 || d == 128)) return false;
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(q)) & 15) != 0) return false;
  // the grids over ALL rows in one epoch: the repair's exact filter, and the matrix-core filter
  if (!grid_fits(cdiv((uint64_t)std::max<int64_t>(n, 1), (uint64_t)FH_EX_ROWS), 256)) return false;
  const uint64_t nqt = cdiv((uint64_t)std::min(nq, 2048), (uint64_t)FH_TN);
  return grid_fits(cdiv(cdiv((uint64_t)std::max<int64_t>(n, 1), (uint64_t)FH_TM), 8) * 8 * nqt, 256);
}

static void fh_launch_norms(lance_hip_ctx *ctx, const void *v, int64_t n, int d, int metric, float *out) {
  hipLaunchKernelGGL(fh_norms_kernel, dim3(grid_stride_blocks((uint64_t)n * 16)), dim3(256), 0, ctx->stream, static_cast<const __half *>(v), n, d,
                     2.3841858e-7f, metric == METRIC_COSINE ? 1 : 0, out);
}

// once per flat_topk call: |x|^2 (or the sentinel) of ALL rows
int flat_mfma_f16_prepare_rows(lance_hip_ctx *ctx, const void *x, int64_t n, int d, int metric, const float **xn2_out) {
  float *xn2 = ctx->scratch_t<float>("fh.xn2", (size_t)std::max<int64_t>(n, 1));
  if (!xn2) return LANCE_HIP_ENOMEM;
  if (n > 0) fh_launch_norms(ctx, x, n, d, metric, xn2);
  *xn2_out = xn2;
  return LANCE_HIP_OK;
}

// once per query chunk: |q|^2 (or the sentinel) from the caller's f16 queries; cosine: the reference's x_norm from their widened copy
int flat_mfma_f16_prepare_queries(lance_hip_ctx *ctx, const void *qh, const float *qf, int nq, int d, int metric, const float **qn2_out,
                                  const float **qnorm_out) {
  float *qn2 = ctx->scratch_t<float>("fh.qn2", (size_t)nq);
  float *qnorm = ctx->scratch_t<float>("fh.qnorm", (size_t)nq);
  if (!qn2 || !qnorm) return LANCE_HIP_ENOMEM;
  fh_launch_norms(ctx, qh, nq, d, metric, qn2);
  if (metric == METRIC_COSINE) hipLaunchKernelGGL(fh_qnorm32_kernel, dim3(cdiv(nq, 64)), dim3(64), 0, ctx->stream, qf, nq, d, qnorm);
  *qn2_out = qn2; *qnorm_out = metric == METRIC_COSINE ? qnorm : nullptr;
  return LANCE_HIP_OK;
}

// the exact filter over rows [e.r0, e.r1): the first epoch and the repair
int launch_flat_f16_exact(lance_hip_ctx *ctx, const FlatPool &e, int d, int metric) {
  const int64_t rows = e.r1 - e.r0;
  if (rows <= 0 || e.nq <= 0) return LANCE_HIP_OK;
  LH_REQUIRE(metric != METRIC_COSINE || e.q_norm, "flat scan (f16 matrix cores): cosine needs the query norms");
  const dim3 grid((unsigned)cdiv((uint64_t)rows, (uint64_t)FH_EX_ROWS), (unsigned)cdiv(e.nq, 256), 1);
  if (metric == METRIC_COSINE) hipLaunchKernelGGL((fh_exact_kernel<METRIC_COSINE>), grid, dim3(256), 0, ctx->stream, e, d);
  else if (metric == METRIC_DOT) hipLaunchKernelGGL((fh_exact_kernel<METRIC_DOT>), grid, dim3(256), 0, ctx->stream, e, d);
  else hipLaunchKernelGGL((fh_exact_kernel<METRIC_L2>), grid, dim3(256), 0, ctx->stream, e, d);
  LH_CHECK_HIP(hipGetLastError());
  return LANCE_HIP_OK;
}

// one matrix-core epoch (rows [e.r0, e.r1) against the chunk's queries) -- every threshold must already be set
int launch_flat_filter_mfma_f16(lance_hip_ctx *ctx, const FlatPool &e, int d, int metric, const void *qh, const float *xn2, const float *qn2) {
  FhArgs a;
  a.p = e; a.qh = static_cast<const __half *>(qh); a.xn2 = xn2; a.qn2 = qn2; a.d = d; a.E = fh_margin(d);
  const int64_t rows = e.r1 - e.r0;
  if (rows <= 0 || e.nq <= 0) return LANCE_HIP_OK;
  LH_REQUIRE(rows < (1ll << 32), "flat scan: an epoch of %lld rows does not fit the 32-bit row queue", (long long)rows);
  LH_REQUIRE(metric != METRIC_COSINE || e.q_norm, "flat scan (f16 matrix cores): cosine needs the query norms");
  a.scnt = ctx->scratch_t<uint32_t>("fh.scnt", (size_t)e.nq);
  a.squeue = ctx->scratch_t<uint32_t>("fh.squeue", (size_t)e.nq * FLAT_MC_QUEUE_CAP);
  if (!a.scnt || !a.squeue) return LANCE_HIP_ENOMEM;
  LH_CHECK_HIP(lh::memset_async(a.scnt, 0, (size_t)e.nq * 4, ctx->stream));
  a.nqt = (uint32_t)cdiv((uint64_t)e.nq, (uint64_t)FH_TN);
  a.nrt = (uint32_t)cdiv((uint64_t)rows, (uint64_t)FH_TM);
  const uint64_t nblocks = cdiv((uint64_t)a.nrt, 8) * 8 * a.nqt;
  LH_REQUIRE(grid_fits(nblocks, 256), "flat scan: an epoch of %lld rows x %d queries exceeds the grid of the f16 matrix-core filter",
             (long long)rows, e.nq);
  const dim3 grid((unsigned)nblocks, 1, 1);
  ScopedTimer t(ctx, "flat_mfma_f16");
  if (metric == METRIC_COSINE) {
    hipLaunchKernelGGL((fh_filter_kernel<METRIC_COSINE>), grid, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL((fh_eval_kernel<METRIC_COSINE>), dim3(e.nq), dim3(256), 0, ctx->stream, a);
  } else if (metric == METRIC_DOT) {
    hipLaunchKernelGGL((fh_filter_kernel<METRIC_DOT>), grid, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL((fh_eval_kernel<METRIC_DOT>), dim3(e.nq), dim3(256), 0, ctx->stream, a);
  } else {
    hipLaunchKernelGGL((fh_filter_kernel<METRIC_L2>), grid, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL((fh_eval_kernel<METRIC_L2>), dim3(e.nq), dim3(256), 0, ctx->stream, a);
  }
  LH_CHECK_HIP(hipGetLastError());
  if (ctx->timing) {      // measurement runs: rows queued by this epoch, read back through "count:flat_mfma_f16_queued" (scripts/flat_f16_probe.py)
    std::vector<uint32_t> h((size_t)e.nq);
    LH_CHECK_HIP(hipMemcpyAsync(h.data(), a.scnt, (size_t)e.nq * 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    uint64_t sum = 0;
    for (uint32_t v : h) sum += v;
    ctx->stage_counts["flat_mfma_f16_queued"] += sum;
  }
  return LANCE_HIP_OK;
}

}  // namespace lh
