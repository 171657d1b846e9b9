// multivec.hip -- exhaustive KNN over a MULTIVECTOR column (Arrow List<FixedSizeList<T, d>>: one bag of vectors per row;
// late interaction, ColBERT / ColPali).
//
//   multivec_distance / multivec_distance_impl   lance-linalg distance.rs:107-206
//   flat scan of a List column                   lance-index flat.rs:129-133, lance scanner.rs:982-1000
//   SortExec(dist asc, rowid asc).fetch(k)       lance/src/dataset/scanner.rs:3386-3406
//
// For a query of nqv vectors q_i and a row of L vectors v_j:
//   sim(i, j) = 1 - dist(q_i, v_j)     dist = l2 | 1 - dot | cosine (x = the query vector), exact.cuh's orders
//   best_i    = max_j sim(i, j)        by f32::total_cmp: a key max (order_key) -- the positive NaN is the maximum, fmaxf would drop it
//   s         = ((0 + best_0) + best_1) + ...   sequentially, in query-vector order
//   distance  = 1 - s
//
// Layout.  One WAVE per row (document), four rows in flight per workgroup, waves stride over the rows.  The lanes of a wave are
// split into 64 / QP sub-slices of QP lanes, QP = the power of two >= min(nqv, 64): lane (sub, qi) owns query vector qi and the
// row's vectors j = sub, sub + 64/QP, ...  The row's vectors stream through a wave-private LDS tile (widened to f32 as they are
// staged, padded row stride) that the lanes of a sub-slice read with one address (broadcast).  Every lane keeps a running key max
// in a register; the sub-slices are folded with lane shuffles (a max: order-free), the nqv maxima go to LDS and lane 0 adds them in
// order.  nqv > 64 runs passes of 64 query vectors over each staged tile, the maxima of every pass stay in registers until the one
// sequential sum.  No atomics, nothing but the [n_rows] distances is written to memory.
//
// The top-k is a (distance key, row id) sort: blocks of 2048 candidates are sorted in LDS and keep their k best, repeated until one
// block is left.  (key, row id) is a total order, so the answer equals the reference's SortExec, ties included.
// Distance ranges (lance_hip_flat_multivec_topk_range): the first selection round loads a row whose distance key lies
// outside lower <= d < upper as the empty sentinel; the scan itself does not change.
#include <algorithm>

#include "common.h"
#include "exact.cuh"
#include "kernels.h"
#include "multivec.cuh"

#pragma clang fp contract(off)

namespace lh {

struct MvArgs {
  const void *values;        // [offsets[n_rows]][d] in the column's element type
  const uint64_t *offsets;   // [n_rows + 1]
  uint64_t n_rows;
  int d;
  int stride;                // tile row stride in floats (a multiple of 4, d rounded up plus one quad)
  int tv;                    // vectors per tile
  int tile_floats;           // per wave
  int vec4;                  // rows can be staged four elements at a time (d % 4 == 0, 16-byte aligned base)
  const float *q;            // [nqv][d], widened
  const float *qnorm;        // [nqv] (cosine)
  int nqv;
  int qp_log2;               // log2 of the lanes per sub-slice
  float *dists;              // [n_rows]
  uint32_t *flag;            // bit 0: a zero-length row, bit 1: decreasing offsets
};

// Any dimension, any nqv <= MV_MAX_NQV: the query vectors are read through the cache per pair (flat.hip's generic kernel).
// TILED = false (rows too long for LDS): the row's vectors are read where they are, in their own element type.
template <int V, typename TV, bool TILED>
__global__ __launch_bounds__(64 * MV_WAVES) void mv_scan_generic_kernel(MvArgs p) {
  extern __shared__ __attribute__((aligned(16))) char mv_smem[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float *tile = reinterpret_cast<float *>(mv_smem) + (size_t)wave * p.tile_floats;
  uint32_t *best = reinterpret_cast<uint32_t *>(reinterpret_cast<float *>(mv_smem) + (size_t)MV_WAVES * p.tile_floats) + wave * MV_MAX_NQV;
  const int qp = 1 << p.qp_log2, qi = lane & (qp - 1), sub = lane >> p.qp_log2, nsub = 64 >> p.qp_log2;
  const TV *vals = static_cast<const TV *>(p.values);
  for (uint64_t r = (uint64_t)blockIdx.x * MV_WAVES + wave; r < p.n_rows; r += (uint64_t)gridDim.x * MV_WAVES) {
    const uint64_t o0 = p.offsets[r], o1 = p.offsets[r + 1];
    if (o1 <= o0) {                                   // refused by the host once the flag is read; never scored
      if (lane == 0) { atomicOr(p.flag, o1 < o0 ? 2u : 1u); p.dists[r] = __uint_as_float(0x7FC00000u); }
      continue;
    }
    const uint64_t len = o1 - o0;
    uint32_t bk[MV_PASSES];
#pragma unroll
    for (int ps = 0; ps < MV_PASSES; ++ps) bk[ps] = 0u;
    const uint64_t step = TILED ? (uint64_t)p.tv : len;
    for (uint64_t t0 = 0; t0 < len; t0 += step) {
      const int nt = (int)(len - t0 < step ? len - t0 : step);         // TILED: <= MV_TILE_VECS
      const TV *src = vals + (o0 + t0) * (uint64_t)p.d;
      if constexpr (TILED) {
        wave_sync();
        mv_stage<TV>(tile, src, nt, p.d, p.stride, p.vec4, lane);
        wave_sync();
      }
#pragma unroll
      for (int ps = 0; ps < MV_PASSES; ++ps) {
        const int q = ps * 64 + qi;
        if (ps * 64 < p.nqv && q < p.nqv) {
          const float *qv = p.q + (int64_t)q * p.d;
          const float qn = (V == MV_COS || V == MV_COS_H) ? p.qnorm[q] : 0.0f;
          if constexpr (TILED) {
            for (int j = sub; j < nt; j += nsub) bk[ps] = max(bk[ps], order_key(one_minus(mv_pair_rt<V, float>(qv, qn, tile + j * p.stride, p.d))));
          } else {
            // nt may exceed 2^31 only for rows no device holds; the loop index is 64-bit all the same
            for (uint64_t j = sub; j < len; j += nsub) bk[ps] = max(bk[ps], order_key(one_minus(mv_pair_rt<V, TV>(qv, qn, src + j * (uint64_t)p.d, p.d))));
          }
        }
      }
    }
#pragma unroll
    for (int ps = 0; ps < MV_PASSES; ++ps) {
      uint32_t b = bk[ps];
      for (int off = qp; off < 64; off <<= 1) b = max(b, (uint32_t)__shfl_xor((int)b, off));
      const int q = ps * 64 + qi;
      if (sub == 0 && q < p.nqv) best[q] = b;
    }
    wave_sync();
    if (lane == 0) p.dists[r] = mv_finish(best, p.nqv);
    wave_sync();
  }
}

// Fixed dimension, nqv <= 64: the lane's query vector lives in VGPRs for the whole kernel.  L2 / dot take dist_exact (L2 with the
// query negated once, flat.hip's packed-add form).  Cosine: the half of the formula that depends on the row's vector alone
// (sqrt of its squared norm) is computed once per staged vector, a lane per vector, and kept beside the tile; the pair then costs the
// products with the query only (cosine_exact_fixed; f16 columns: the 32-lane dot of cosine_scalar32_rt).
template <int D, int V, typename TV>
__global__ __launch_bounds__(64 * MV_WAVES, 2) void mv_scan_fixed_kernel(MvArgs p) {      // two waves per SIMD: the LDS admits two workgroups per CU
  extern __shared__ __attribute__((aligned(16))) char mv_smem[];
  constexpr bool COS = V == MV_COS || V == MV_COS_H;
  constexpr bool NEG = V == MV_L2;                  // the lane holds -q: (-q) + v = v - q
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  float *tile = reinterpret_cast<float *>(mv_smem) + (size_t)wave * p.tile_floats;
  uint32_t *best = reinterpret_cast<uint32_t *>(reinterpret_cast<float *>(mv_smem) + (size_t)MV_WAVES * p.tile_floats) + wave * MV_MAX_NQV;
  float *ysq = reinterpret_cast<float *>(mv_smem) + (size_t)MV_WAVES * (p.tile_floats + MV_MAX_NQV) + wave * MV_TILE_VECS;
  const int qp = 1 << p.qp_log2, qi = lane & (qp - 1), sub = lane >> p.qp_log2, nsub = 64 >> p.qp_log2;
  const bool active = qi < p.nqv;
  const float *qsrc = p.q + (int64_t)(active ? qi : 0) * D;
  RegVec<D> a;
#pragma unroll
  for (int i = 0; i < RegVec<D>::Q * 4; ++i) a.q[i >> 2][i & 3] = i < D ? (NEG ? -qsrc[i] : qsrc[i]) : 0.0f;
  float qn = 0.0f;
  if constexpr (COS) qn = p.qnorm[active ? qi : 0];
  const TV *vals = static_cast<const TV *>(p.values);
  for (uint64_t r = (uint64_t)blockIdx.x * MV_WAVES + wave; r < p.n_rows; r += (uint64_t)gridDim.x * MV_WAVES) {
    const uint64_t o0 = p.offsets[r], o1 = p.offsets[r + 1];
    if (o1 <= o0) {
      if (lane == 0) { atomicOr(p.flag, o1 < o0 ? 2u : 1u); p.dists[r] = __uint_as_float(0x7FC00000u); }
      continue;
    }
    const uint64_t len = o1 - o0;
    uint32_t bk = 0u;
    for (uint64_t t0 = 0; t0 < len; t0 += (uint64_t)p.tv) {
      const int nt = (int)(len - t0 < (uint64_t)p.tv ? len - t0 : (uint64_t)p.tv);
      wave_sync();
      mv_stage<TV>(tile, vals + (o0 + t0) * (uint64_t)D, nt, D, p.stride, p.vec4, lane);
      wave_sync();
      if constexpr (COS) {
        if (lane < nt) {       // nt <= MV_TILE_VECS = 64
          const float *y = tile + lane * p.stride;
          ysq[lane] = V == MV_COS ? cosine_exact_ysqrt<D>(y) : sqrtf(dist_exact_rt<METRIC_DOT, float, 32>(y, y, D));
        }
        wave_sync();
      }
      if (active) {
#pragma unroll 1
        for (int j = sub; j < nt; j += nsub) {
          const float *y = tile + j * p.stride;
          float v;
          if constexpr (V == MV_L2) v = dist_exact<D, METRIC_L2, true>(a, y);
          else if constexpr (V == MV_DOT) v = finish_metric<METRIC_DOT>(dist_exact<D, METRIC_DOT>(a, y));
          else if constexpr (V == MV_DOT_H) v = finish_metric<METRIC_DOT>(dist_exact<D, METRIC_DOT, false, 32>(a, y));
          else if constexpr (V == MV_COS) v = cosine_exact_fixed<D>(a, qn, y, ysq[j]);
          else { const float xy = dist_exact<D, METRIC_DOT, false, 32>(a, y); v = cosine_finish(xy, xy / (qn * ysq[j])); }
          bk = max(bk, order_key(one_minus(v)));
        }
      }
    }
    for (int off = qp; off < 64; off <<= 1) bk = max(bk, (uint32_t)__shfl_xor((int)bk, off));
    if (sub == 0 && active) best[qi] = bk;
    wave_sync();
    if (lane == 0) p.dists[r] = mv_finish(best, p.nqv);
    wave_sync();
  }
}

template <bool H32>
__global__ __launch_bounds__(64) void mv_qnorm_kernel(const float *__restrict__ q, int nqv, int d, float *__restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < nqv) out[i] = H32 ? norm_l2_rt<float, 32>(q + (int64_t)i * d, d) : norm_l2_rt<float>(q + (int64_t)i * d, d);
}

// One block sorts MV_SEL candidates by (key, row id) and keeps the k best (k <= MV_SEL / 2).  First round: the candidates are the
// rows (dists, row_ids or the row index); later rounds: the survivors of the round before.  The last round (one block) writes the answer.
// RANGE (distance ranges), first round only: a row whose distance key lies outside lo_key <= key <= hi_last loads as the
// empty sentinel -- a row that is not there; absent bounds are 0 / ~0, which test nothing.  RANGE = false is the kernel from before.
template <bool RANGE>
__global__ __launch_bounds__(256) void mv_select_kernel(const float *__restrict__ dists, const uint64_t *__restrict__ row_ids,
                                                        const uint32_t *__restrict__ in_keys, const uint64_t *__restrict__ in_rids,
                                                        uint64_t n_in, int k, uint32_t *__restrict__ out_keys, uint64_t *__restrict__ out_rids,
                                                        uint64_t *__restrict__ ids, float *__restrict__ out_dists, uint32_t lo_key, uint32_t hi_last) {
  __shared__ uint64_t rid[MV_SEL];
  __shared__ uint32_t key[MV_SEL];
  const uint64_t base = (uint64_t)blockIdx.x * MV_SEL;
  for (int i = threadIdx.x; i < MV_SEL; i += 256) {
    const uint64_t g = base + i;
    uint32_t kk = 0xFFFFFFFFu;
    uint64_t rr = ~0ull;
    if (g < n_in) {
      if (dists) {
        kk = order_key(dists[g]); rr = row_ids ? row_ids[g] : g;
        if constexpr (RANGE) {
          if (kk < lo_key || kk > hi_last) { kk = 0xFFFFFFFFu; rr = ~0ull; }
        }
      }
      else { kk = in_keys[g]; rr = in_rids[g]; }
    }
    key[i] = kk; rid[i] = rr;
  }
  __syncthreads();
  for (int k2 = 2; k2 <= MV_SEL; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < MV_SEL / 2; i += 256) {
        const int ix = 2 * j * (i / j) + (i % j);
        const int px = ix + j;
        const bool up = (ix & k2) == 0;
        const uint32_t kx = key[ix], ky = key[px];
        const uint64_t rx = rid[ix], ry = rid[px];
        const bool gt = kx > ky || (kx == ky && rx > ry);
        if (gt == up) { key[ix] = ky; key[px] = kx; rid[ix] = ry; rid[px] = rx; }
      }
      __syncthreads();
    }
  }
  for (int i = threadIdx.x; i < k; i += 256) {
    if (ids) {
      ids[i] = rid[i];
      out_dists[i] = rid[i] != ~0ull ? key_to_float(key[i]) : INFINITY;
    } else {
      out_keys[(uint64_t)blockIdx.x * k + i] = key[i];
      out_rids[(uint64_t)blockIdx.x * k + i] = rid[i];
    }
  }
}

static bool mv_fixed_dim(uint32_t d) { return d == 8 || d == 16 || d == 32 || d == 64 || d == 96 || d == 128; }

template <int V, typename TV>
static void mv_launch(lance_hip_ctx *ctx, const MvArgs &a, bool tiled, bool fixed, unsigned grid, size_t lds) {
  const dim3 g(grid), b(64 * MV_WAVES);
  if (!tiled) { hipLaunchKernelGGL((mv_scan_generic_kernel<V, TV, false>), g, b, lds, ctx->stream, a); return; }
  switch (fixed ? a.d : 0) {
    case 8: hipLaunchKernelGGL((mv_scan_fixed_kernel<8, V, TV>), g, b, lds, ctx->stream, a); break;
    case 16: hipLaunchKernelGGL((mv_scan_fixed_kernel<16, V, TV>), g, b, lds, ctx->stream, a); break;
    case 32: hipLaunchKernelGGL((mv_scan_fixed_kernel<32, V, TV>), g, b, lds, ctx->stream, a); break;
    case 64: hipLaunchKernelGGL((mv_scan_fixed_kernel<64, V, TV>), g, b, lds, ctx->stream, a); break;
    case 96: hipLaunchKernelGGL((mv_scan_fixed_kernel<96, V, TV>), g, b, lds, ctx->stream, a); break;
    case 128: hipLaunchKernelGGL((mv_scan_fixed_kernel<128, V, TV>), g, b, lds, ctx->stream, a); break;
    default: hipLaunchKernelGGL((mv_scan_generic_kernel<V, TV, true>), g, b, lds, ctx->stream, a);
  }
}

int mv_check_args(const char *what, lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                         uint64_t n_rows, uint32_t d, const void *q, uint32_t nqv) {
  LH_REQUIRE(ctx && offsets && q && (n_rows == 0 || values), "%s: NULL argument", what);
  LH_REQUIRE(dtype == LANCE_HIP_F32 || dtype == LANCE_HIP_F16,
             "%s: unsupported element type %d: multivector columns are float32 (0) or float16 (1); int8 / uint8 (hamming) columns are not supported", what, dtype);
  LH_REQUIRE(metric == LANCE_HIP_L2 || metric == LANCE_HIP_DOT || metric == LANCE_HIP_COSINE, "%s: bad metric %d (l2 = 0, cosine = 1, dot = 2)", what, metric);
  LH_REQUIRE(d >= 1 && d <= 0x7FFFFFF0u / 64, "%s: dimension %u out of range", what, d);
  LH_REQUIRE(nqv >= 1 && nqv <= (uint32_t)MV_MAX_NQV, "%s: %u query vectors: a multivector query holds 1..%d vectors", what, nqv, MV_MAX_NQV);
  return LANCE_HIP_OK;
}

// enqueues the scan: dists[n_rows]; the flag word is zeroed in front of it
static int mv_scan(lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets, uint64_t n_rows, uint32_t d,
                   const void *q, uint32_t nqv, float *dists, uint32_t **flag_out) {
  MvArgs a;
  const bool f16 = dtype == LANCE_HIP_F16;
  const bool cos = metric == LANCE_HIP_COSINE;
  a.values = values; a.offsets = offsets; a.n_rows = n_rows; a.d = (int)d; a.nqv = (int)nqv; a.dists = dists;
  LH_TRY(as_f32(ctx, dtype, q, (size_t)nqv * d, "mv.q", &a.q));
  a.flag = ctx->scratch_t<uint32_t>("mv.flag", 1);
  float *qn = ctx->scratch_t<float>("mv.qnorm", MV_MAX_NQV);
  if (!a.flag || !qn) return LANCE_HIP_ENOMEM;
  a.qnorm = qn;
  *flag_out = a.flag;
  LH_CHECK_HIP(lh::memset_async(a.flag, 0, 4, ctx->stream));
  if (n_rows == 0) return LANCE_HIP_OK;
  if (cos) {
    if (f16) hipLaunchKernelGGL(mv_qnorm_kernel<true>, dim3(cdiv(nqv, 64)), dim3(64), 0, ctx->stream, a.q, (int)nqv, (int)d, qn);
    else hipLaunchKernelGGL(mv_qnorm_kernel<false>, dim3(cdiv(nqv, 64)), dim3(64), 0, ctx->stream, a.q, (int)nqv, (int)d, qn);
  }
  a.qp_log2 = 0;
  while ((1u << a.qp_log2) < std::min<uint32_t>(nqv, 64)) ++a.qp_log2;
  a.stride = (int)((d + 3) / 4 * 4 + 4);
  a.vec4 = d % 4 == 0 && (reinterpret_cast<uintptr_t>(values) & 15) == 0;
  const size_t best_bytes = (size_t)MV_WAVES * (MV_MAX_NQV + MV_TILE_VECS) * 4;     // the maxima, and the fixed cosine kernels' per-vector norms
  bool tiled = (size_t)MV_WAVES * a.stride * 4 + best_bytes <= MV_LDS_LIMIT;
  if (tiled) {
    a.tv = std::max(1, std::min(MV_TILE_VECS, MV_TILE_FLOATS / a.stride));
    a.tile_floats = a.tv * a.stride;
  } else {
    a.tv = 0; a.tile_floats = 0;
  }
  const size_t lds = (size_t)MV_WAVES * a.tile_floats * 4 + best_bytes;
  const bool fixed = tiled && mv_fixed_dim(d) && nqv <= 64 && a.vec4;
  const unsigned grid = (unsigned)std::min<uint64_t>(cdiv(n_rows, MV_WAVES), (uint64_t)ctx->num_cus * 4);
  {
    ScopedTimer t(ctx, "multivec_scan");
    if (metric == LANCE_HIP_L2) {
      if (f16) mv_launch<MV_L2, __half>(ctx, a, tiled, fixed, grid, lds);
      else mv_launch<MV_L2, float>(ctx, a, tiled, fixed, grid, lds);
    } else if (metric == LANCE_HIP_DOT) {
      if (f16) mv_launch<MV_DOT_H, __half>(ctx, a, tiled, fixed, grid, lds);
      else mv_launch<MV_DOT, float>(ctx, a, tiled, fixed, grid, lds);
    } else {
      if (f16) mv_launch<MV_COS_H, __half>(ctx, a, tiled, fixed, grid, lds);
      else mv_launch<MV_COS, float>(ctx, a, tiled, fixed, grid, lds);
    }
  }
  LH_CHECK_HIP(hipGetLastError());
  return LANCE_HIP_OK;
}

// waits for the stream and turns the scan's flag word into the call's return code
static int mv_finish_call(lance_hip_ctx *ctx, const char *what, const uint32_t *flag) {
  uint32_t f = 0;
  LH_CHECK_HIP(hipMemcpyAsync(&f, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  LH_REQUIRE((f & 2u) == 0, "%s: offsets decrease", what);
  LH_REQUIRE((f & 1u) == 0, "%s: a row holds no vector (zero-length rows are refused: the reference unwraps a None there)", what);
  return LANCE_HIP_OK;
}

}  // namespace lh

using namespace lh;

extern "C" int lance_hip_multivec_distance(lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                                           uint64_t n_rows, uint32_t d, const void *q, uint32_t nqv, float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  LH_TRY(mv_check_args("multivec_distance", ctx, dtype, metric, values, offsets, n_rows, d, q, nqv));
  LH_REQUIRE(n_rows == 0 || dists, "multivec_distance: NULL argument");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  uint32_t *flag = nullptr;
  LH_TRY(mv_scan(ctx, dtype, metric, values, offsets, n_rows, d, q, nqv, dists, &flag));
  return mv_finish_call(ctx, "multivec_distance", flag);
}

// lance_hip_flat_multivec_topk and lance_hip_flat_multivec_topk_range: the scan writes every row's distance, the range is applied
// where the first selection round loads them (mv_select_kernel<true>); an empty range still scans, so that a malformed column is refused
int lh::mv_topk_impl(const char *what, lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                        const uint64_t *row_ids, uint64_t n_rows, uint32_t d, const void *q, uint32_t nqv, uint32_t k, const FlatRange &rg,
                        uint64_t *ids, float *dists) {
  LH_TRY(mv_check_args(what, ctx, dtype, metric, values, offsets, n_rows, d, q, nqv));
  LH_REQUIRE(ids && dists, "%s: NULL argument", what);
  LH_REQUIRE(k > 0 && k <= (uint32_t)MV_SEL / 2, "%s: k=%u not supported (1..%d)", what, k, MV_SEL / 2);
  LH_REQUIRE(!(rg.has_lower && rg.has_upper) || rg.lo_key <= rg.hi_key, "%s: lower bound %g is above the upper bound %g", what,
             (double)key_to_float_host(rg.lo_key), (double)key_to_float_host(rg.hi_key));
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  // in range <=> lo <= key <= hi_last; an empty range (lower == upper, or an upper bound under every key) is lo > hi_last
  const uint32_t sel_lo = rg.empty() ? 1u : (rg.has_lower ? rg.lo_key : 0u), sel_hi = rg.empty() ? 0u : rg.start_key();
  const uint64_t nb0 = std::max<uint64_t>(1, cdiv(n_rows, MV_SEL));
  float *rd = ctx->scratch_t<float>("mv.dists", std::max<uint64_t>(1, n_rows));
  uint32_t *sk[2] = {nullptr, nullptr};
  uint64_t *sr[2] = {nullptr, nullptr};
  if (!rd) return LANCE_HIP_ENOMEM;
  if (nb0 > 1) {
    sk[0] = ctx->scratch_t<uint32_t>("mv.selk0", nb0 * k);
    sr[0] = ctx->scratch_t<uint64_t>("mv.selr0", nb0 * k);
    sk[1] = ctx->scratch_t<uint32_t>("mv.selk1", cdiv(nb0 * k, MV_SEL) * k);
    sr[1] = ctx->scratch_t<uint64_t>("mv.selr1", cdiv(nb0 * k, MV_SEL) * k);
    if (!sk[0] || !sr[0] || !sk[1] || !sr[1]) return LANCE_HIP_ENOMEM;
  }
  uint32_t *flag = nullptr;
  LH_TRY(mv_scan(ctx, dtype, metric, values, offsets, n_rows, d, q, nqv, rd, &flag));
  {
    ScopedTimer t(ctx, "multivec_select");
    uint64_t n_in = n_rows;
    int cur = -1;                                        // -1: the candidates are the rows
    for (;;) {
      const uint64_t nb = std::max<uint64_t>(1, cdiv(n_in, MV_SEL));
      const bool last = nb == 1;
      const int nxt = cur == 0 ? 1 : 0;
      if (rg.any() && cur < 0)
        hipLaunchKernelGGL(mv_select_kernel<true>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, rd, row_ids, nullptr, nullptr, n_in, (int)k,
                           last ? nullptr : sk[nxt], last ? nullptr : sr[nxt], last ? ids : nullptr, last ? dists : nullptr, sel_lo, sel_hi);
      else
        hipLaunchKernelGGL(mv_select_kernel<false>, dim3((unsigned)nb), dim3(256), 0, ctx->stream, cur < 0 ? rd : nullptr, cur < 0 ? row_ids : nullptr,
                           cur < 0 ? nullptr : sk[cur], cur < 0 ? nullptr : sr[cur], n_in, (int)k, last ? nullptr : sk[nxt],
                           last ? nullptr : sr[nxt], last ? ids : nullptr, last ? dists : nullptr, 0u, 0xFFFFFFFFu);
      if (last) break;
      n_in = nb * k;
      cur = nxt;
    }
  }
  LH_CHECK_HIP(hipGetLastError());
  return mv_finish_call(ctx, what, flag);
}

extern "C" int lance_hip_flat_multivec_topk(lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                                            const uint64_t *row_ids, uint64_t n_rows, uint32_t d, const void *q, uint32_t nqv,
                                            uint32_t k, uint64_t *ids, float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  return mv_topk_impl("flat_multivec_topk", ctx, dtype, metric, values, offsets, row_ids, n_rows, d, q, nqv, k, FlatRange{}, ids, dists);
}

extern "C" int lance_hip_flat_multivec_topk_range(lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                                                  const uint64_t *row_ids, uint64_t n_rows, uint32_t d, const void *q, uint32_t nqv,
                                                  uint32_t k, int has_lower, float lower, int has_upper, float upper, uint64_t *ids,
                                                  float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  return mv_topk_impl("flat_multivec_topk_range", ctx, dtype, metric, values, offsets, row_ids, n_rows, d, q, nqv, k,
                      flat_range(has_lower, lower, has_upper, upper), ids, dists);
}
