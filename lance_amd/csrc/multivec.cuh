// multivec.cuh -- what the multivector scans share: the constants, the pair distance in the reference's arithmetic, the row's
// sequential sum and the tile staging of multivec.hip (its header has the layout), used unchanged by multivec_batch.hip.
#pragma once
#include "common.h"
#include "exact.cuh"
#include "kernels.h"

#pragma clang fp contract(off)

namespace lh {

constexpr int MV_WAVES = 4;                                   // rows in flight per workgroup
constexpr int MV_MAX_NQV = LANCE_HIP_MULTIVEC_MAX_QUERY_VECTORS;
constexpr int MV_PASSES = MV_MAX_NQV / 64;
constexpr int MV_TILE_FLOATS = 4096;                          // per wave (16 KiB): two workgroups per CU
constexpr int MV_TILE_VECS = 64;                              // at most this many vectors per tile
constexpr int MV_SEL = 2048;                                  // candidates one selection block sorts
constexpr size_t MV_LDS_LIMIT = 160 * 1024;

// the variants of the pair distance: which of exact.cuh's functions a (metric, column type) takes
enum { MV_L2 = 0, MV_DOT = 1, MV_COS = 2, MV_DOT_H = 3, MV_COS_H = 4 };

__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// distance of one (query vector, row vector) pair, run-time dimension; TB = float (LDS tile) or the column's own type (untiled)
// L2 takes the difference as v - q, not q - v: the square is the same bit for bit, and a NaN element of the ROW then reaches the sum
// with its own sign, as on the reference's CPU -- as the subtrahend it would come back negated, sort as the MINIMUM of the row's
// similarities and the row would score as if the vector were not there (a NaN in the QUERY makes every distance NaN on either side;
// its sign is not pinned).  The register kernels get there by holding -q and adding (dist_exact's packed-add form).
template <int V, typename TB>
__device__ __forceinline__ float mv_pair_rt(const float *__restrict__ qv, float qn, const TB *__restrict__ y, int d) {
  if constexpr (V == MV_L2) return dist_exact_rt<METRIC_L2, TB, 16, true>(qv, y, d);      // (v - q)^2
  else if constexpr (V == MV_DOT) return finish_metric<METRIC_DOT>(dist_exact_rt<METRIC_DOT, TB>(qv, y, d));
  else if constexpr (V == MV_DOT_H) return finish_metric<METRIC_DOT>(dist_exact_rt<METRIC_DOT, TB, 32>(qv, y, d));
  else if constexpr (V == MV_COS) return cosine_exact_rt<TB>(qv, qn, y, d);
  else return cosine_scalar32_rt<TB>(qv, qn, y, d);
}

// lane 0 of the wave: the sequential sum of the maxima and the row's distance
__device__ __forceinline__ float mv_finish(const uint32_t *best, int nqv) {
  float s = 0.0f;
  for (int i = 0; i < nqv; ++i) s = s + key_to_float(best[i]);
  return one_minus(s);
}

template <typename TV>
__device__ __forceinline__ void mv_stage(float *tile, const TV *__restrict__ src, int nt, int d, int stride, int vec4, int lane) {
  if (vec4) {
    const int dq = d >> 2;
    for (int i = lane; i < nt * dq; i += 64) {
      const int v = i / dq, e = i - v * dq;
      *reinterpret_cast<f4 *>(tile + v * stride + 4 * e) = load4(src + (int64_t)i * 4);
    }
  } else {
    for (int i = lane; i < nt * d; i += 64) {
      const int v = i / d, e = i - v * d;
      tile[v * stride + e] = ld_elem(src, i);
    }
  }
}

// multivec.hip: the single-query exact scan and selection (lance_hip_flat_multivec_topk[_range]); multivec_batch.hip answers with it
// every query its filter does not serve
int mv_check_args(const char *what, lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                  uint64_t n_rows, uint32_t d, const void *q, uint32_t nqv);
int mv_topk_impl(const char *what, lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                 const uint64_t *row_ids, uint64_t n_rows, uint32_t d, const void *q, uint32_t nqv, uint32_t k, const FlatRange &rg,
                 uint64_t *ids, float *dists);

}  // namespace lh
