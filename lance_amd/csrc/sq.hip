// sq.hip -- 8-bit scalar quantisation (SQ) and the IVF_SQ index: bounds, encode, distances, search.
//
//   ScalarQuantizer::update_bounds / scale_to_u8 / inverse_scalar_dist   lance-index/src/vector/sq.rs:43-89, 263-287
//   SQDistCalculator::distance / distance_all                            sq/storage.rs:398-468
//   l2_distance_uint_scalar, impl Dot for u8                             lance-linalg l2.rs:44-49, dot.rs:152-161
//   FlatIndex::search (the sub-index of IVF_SQ)                          flat/index.rs:82-177
//   SortExec(dist, rowid).fetch(k)                                       lance/src/dataset/scanner.rs:3440-3468
//
// Everything that decides a result is exact: the encoder is three f64 operations per element (subtract, multiply, divide -- each
// correctly rounded, never contracted), the distance of a row is a u32 sum over the codes (order-free), converted once to f32
// and rescaled by one f32 multiply and one f32 divide.  So the kernels below reproduce the reference bit for bit without a
// surrogate pass.
//
// L2 between codes is computed as sum(x^2) + sum(q^2) - 2 sum(x q) in u32: the reference's sum of squared |x - q| is the same
// integer, the three terms stay below 2^32 up to d = 16384 (2 d 255^2 < 2^32 needs d <= 33025), and the packed 4 x u8 dot
// product (v_dot4_u32_u8) serves both metrics: one instruction per 4 codes with sum(x^2) stored per row at build time.
//
// Search (pair_cand.cuh, shared with IVF_RQ; this file supplies the row distance): one workgroup per (query, probed partition) keeps
// that pair's k best (key, storage position) -- key = order_key of the SCALED f32 distance, the value the reference's heap compares
// (two integer sums above 2^24 may round to one float and tie).  A pair is ambiguous when a row tied with its k-th key had to be left
// out; a query is flagged when an ambiguous pair's k-th key is not above the k-th key of the merged candidates, and flagged queries
// are replayed through std BinaryHeap's push / pop in storage order (the IVF_FLAT replay with the SQ distance).  The final order is
// (dist, rowid).  k here is keff = k * refine_factor under a refine_factor: up to 128 in a 512-entry buffer, up to 768 in a wide one.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include <hip/hip_fp16.h>

#include "common.h"
#include "exact.cuh"
#include "index.h"
#include "kernels.h"
#include "search_common.cuh"
#include "pair_cand.cuh"

#pragma clang fp contract(off)

namespace lh {

constexpr uint32_t SQ_MAX_DIM = LANCE_HIP_SQ_MAX_DIM;
constexpr int SQ_MAX_K = 128;

__device__ __forceinline__ double sq_widen(float v) { return (double)v; }
__device__ __forceinline__ double sq_widen(__half v) { return (double)__half2float(v); }    // f16 -> f32 -> f64: both exact

// ---- bounds: fold min / max of a column into f64 partials (Range<f64> fold of update_bounds; f64::min / max skip NaN) --------
template <typename T>
__global__ __launch_bounds__(256) void sq_bounds_kernel(const T *__restrict__ x, int64_t count, double *__restrict__ partials) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double *red = reinterpret_cast<double *>(smem);      // [4 waves][2]
  double lo = 1.7976931348623157e308, hi = -1.7976931348623157e308;    // f64::MAX .. f64::MIN
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    const double v = sq_widen(x[i]);
    if (v == v) { lo = v < lo ? v : lo; hi = v > hi ? v : hi; }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double l2 = __shfl_xor(lo, o, 64), h2 = __shfl_xor(hi, o, 64);
    lo = l2 < lo ? l2 : lo; hi = h2 > hi ? h2 : hi;
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { red[2 * wave] = lo; red[2 * wave + 1] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int w = 1; w < 4; ++w) { lo = red[2 * w] < lo ? red[2 * w] : lo; hi = red[2 * w + 1] > hi ? red[2 * w + 1] : hi; }
    partials[2 * blockIdx.x] = lo; partials[2 * blockIdx.x + 1] = hi;
  }
}

// ---- encode: scale_to_u8 (sq.rs:263-277) -------------------------------------------------------------------------------------
// (v - start) * 255.0 / range, three separately rounded f64 operations, then Rust's `as u8`: truncation toward zero, saturation
// to 0..255, NaN -> 0 -- written out, no conversion instruction sees an out-of-range value.
__device__ __forceinline__ uint8_t sq_code(double v, double lo, double range) {
  const double t = __ddiv_rn(__dmul_rn(__dsub_rn(v, lo), 255.0), range);
  if (!(t > 0.0)) return 0;          // NaN, zero and everything negative (truncation takes (-1, 0) to 0 as well)
  if (t >= 255.0) return 255;
  return (uint8_t)(int)t;            // 0 < t < 255: the conversion truncates
}

// out[row * ldo + col]; degenerate (start == end): every code is 0
template <typename T>
__global__ __launch_bounds__(256) void sq_encode_kernel(const T *__restrict__ x, int64_t count, int d, int64_t ldo, double lo, double range,
                                                        int degenerate, uint8_t *__restrict__ out) {
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < count; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / d;
    const int col = (int)(i - row * d);
    out[row * ldo + col] = degenerate ? (uint8_t)0 : sq_code(sq_widen(x[i]), lo, range);
  }
}

// ---- integer sums ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t sq_udot4(uint32_t a, uint32_t b, uint32_t c) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(a, b, c, false);     // v_dot4_u32_u8
#else
  return c + (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u) + (a >> 24) * (b >> 24);
#endif
}

// sum(x q) over one row of nv 16-byte words (row and query zero-padded to the word)
__device__ __forceinline__ uint32_t sq_row_xq(const uint4 *__restrict__ row, const uint4 *__restrict__ qs, int nv) {
  uint32_t acc = 0;
  for (int c = 0; c < nv; ++c) {
    const uint4 v = row[c], q = qs[c];
    acc = sq_udot4(v.x, q.x, acc); acc = sq_udot4(v.y, q.y, acc); acc = sq_udot4(v.z, q.z, acc); acc = sq_udot4(v.w, q.w, acc);
  }
  return acc;
}

// inverse_scalar_dist (sq.rs:279-287) of the integer distance: dot_distance = 1.0 - sum as f32 (dot.rs:152-161)
__device__ __forceinline__ float sq_finish(int dot, uint32_t s, float r2) {
  const float d0 = dot ? __fsub_rn(1.0f, (float)s) : (float)s;
  return __fdiv_rn(__fmul_rn(d0, r2), 65025.0f);
}
__device__ __forceinline__ uint32_t sq_sum(int dot, uint32_t xq, uint32_t xx, uint32_t qq) { return dot ? xq : xx + qq - 2u * xq; }

// per-row sum of squared codes over padded rows [n][ld]
__global__ __launch_bounds__(256) void sq_norms_kernel(const uint8_t *__restrict__ codes, int64_t n, int ld, uint32_t *__restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const uint4 *r = reinterpret_cast<const uint4 *>(codes + row * ld);
  out[row] = sq_row_xq(r, r, ld / 16);
}

// distance_all in its testable form: [nq][n] distances of encoded queries (padded, [nq][ldq]) against a caller's code matrix [n][d]
// (tightly packed).  Rows are read 16 bytes per lane when d is a multiple of 16 and the matrix is aligned; otherwise word by word
// with the tail bytes masked -- never past the row.
template <bool WIDE>
__global__ __launch_bounds__(256) void sq_distance_kernel(const uint8_t *__restrict__ codes, int64_t n, int d, const uint8_t *__restrict__ qcodes,
                                                          int ldq, int dot, float r2, float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4 *qs = reinterpret_cast<uint4 *>(smem);
  const int q = blockIdx.y;
  const int nv = ldq / 16;
  for (int i = threadIdx.x; i < nv; i += 256) qs[i] = reinterpret_cast<const uint4 *>(qcodes + (int64_t)q * ldq)[i];
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (row >= n) return;
  const uint8_t *r = codes + row * d;
  uint32_t xq = 0, xx = 0, qq = 0;
  if constexpr (WIDE) {
    const uint4 *rv = reinterpret_cast<const uint4 *>(r);
    xq = sq_row_xq(rv, qs, nv);
    if (!dot) { xx = sq_row_xq(rv, rv, nv); qq = sq_row_xq(qs, qs, nv); }
  } else {
    const uint32_t *qw = reinterpret_cast<const uint32_t *>(qs);
    for (int c = 0; c < d; c += 4) {
      uint32_t w = 0;
#pragma unroll
      for (int b = 0; b < 4; ++b)
        if (c + b < d) w |= (uint32_t)r[c + b] << (8 * b);
      const uint32_t y = qw[c >> 2];
      xq = sq_udot4(w, y, xq);
      if (!dot) { xx = sq_udot4(w, w, xx); qq = sq_udot4(y, y, qq); }
    }
  }
  out[(int64_t)q * n + row] = sq_finish(dot, sq_sum(dot, xq, xx, qq), r2);
}

// codes [n][d] -> partition order with padded rows [n_out][ld]; one thread per output byte
__global__ __launch_bounds__(256) void sq_gather_kernel(const uint8_t *__restrict__ codes, const uint64_t *__restrict__ row_ids,
                                                        const uint32_t *__restrict__ perm, int64_t n_out, int d, int ld,
                                                        uint8_t *__restrict__ out, uint64_t *__restrict__ rid_out) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n_out * ld; g += (int64_t)gridDim.x * 256) {      // (grid.h: n_out * ld reaches 2^32)
    const int64_t s = g / ld;
    const int c = (int)(g - s * ld);
    const uint32_t r = perm[s];
    out[g] = c < d ? codes[(int64_t)r * d + c] : (uint8_t)0;
    if (c == 0) rid_out[s] = row_ids ? row_ids[r] : (uint64_t)r;
  }
}

// ---- IVF_SQ search (pair_cand.cuh with the SQ row distance) -----------------------------------------------------------------------
struct SqArgs {
  const uint8_t *codes;          // [n][ld] partition-ordered, zero-padded rows
  const uint32_t *xx;            // [n] sum of squared codes
  const uint8_t *qcodes;         // [nq][ld]
  const uint32_t *qq;            // [nq] sum of squared query codes
  int ld, dot;
  float r2;                      // ((end - start) as f32)^2
  CandLists w;
};

// dynamic LDS (sq_scan_lds): [ld] query codes | [w.cap] u64 entries | CandCtl
__global__ __launch_bounds__(256) void sq_scan_kernel(SqArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint4 *qs = reinterpret_cast<uint4 *>(smem);
  uint64_t *e = reinterpret_cast<uint64_t *>(smem + a.ld);
  CandCtl *ctl = reinterpret_cast<CandCtl *>(e + a.w.cap);
  const int pair = blockIdx.x;
  const int qi = pair / a.w.nprobes;
  const uint32_t part = a.w.probes[pair];
  const uint32_t r0 = a.w.part_offsets[part], r1 = a.w.part_offsets[part + 1];
  const int nv = a.ld / 16;
  for (int i = threadIdx.x; i < nv; i += 256) qs[i] = reinterpret_cast<const uint4 *>(a.qcodes + (int64_t)qi * a.ld)[i];
  if (threadIdx.x == 0) { ctl->cnt = 0; ctl->thr = 0xFFFFFFFFu; ctl->amb_key = 0; ctl->amb = 0; }
  __syncthreads();
  const uint32_t qq = a.qq[qi];
  cand_scan_pair(a.w, pair, r0, r1, e, ctl, [&](uint32_t row) {
    const uint32_t xq = sq_row_xq(reinterpret_cast<const uint4 *>(a.codes + (int64_t)row * a.ld), qs, nv);
    return order_key(sq_finish(a.dot, sq_sum(a.dot, xq, a.xx[row], qq), a.r2));
  });
}

struct SqDist {
  const SqArgs &a;
  const uint4 *qs;
  uint32_t qq;
  __device__ __forceinline__ void partition(int, uint32_t) {}
  __device__ __forceinline__ uint32_t key(uint32_t off, int row, int) const {
    const uint32_t xq = sq_row_xq(reinterpret_cast<const uint4 *>(a.codes + (int64_t)(off + row) * a.ld), qs, a.ld / 16);
    return order_key(sq_finish(a.dot, sq_sum(a.dot, xq, a.xx[off + row], qq), a.r2));
  }
};

// the heap replay of a flagged query (the IVF_FLAT replay with the SQ distance).  Dynamic LDS (sq_replay_lds): [ld] query codes | replay area
__global__ __launch_bounds__(64) void sq_exact_kernel(SqArgs a, uint64_t *__restrict__ out_ids, float *__restrict__ out_dists) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int qi = blockIdx.x;
  if (!a.w.flags[qi]) return;
  uint4 *qs = reinterpret_cast<uint4 *>(smem);
  const int nv = a.ld / 16;
  for (int i = threadIdx.x; i < nv; i += 64) qs[i] = reinterpret_cast<const uint4 *>(a.qcodes + (int64_t)qi * a.ld)[i];
  __syncthreads();
  SqDist dist = {a, qs, a.qq[qi]};
  cand_replay_query(a.w, qi, smem + a.ld, dist, out_ids, out_dists);
}

// launch sizes: capacity 512 up to CAND_NARROW_K (ld + 4096 + 16 bytes), the largest that fits above
static inline int sq_scan_cap(uint32_t ld, int k) { return cand_scan_cap(k, (size_t)ld + sizeof(CandCtl)); }
static inline size_t sq_scan_lds(uint32_t ld, int cap) { return (size_t)ld + (size_t)cap * 8 + sizeof(CandCtl); }
static inline size_t sq_replay_lds(uint32_t ld, int k) { return (size_t)ld + cand_replay_bytes(k); }

// ---- host side ---------------------------------------------------------------------------------------------------------------
static int sq_check_column(int dtype, uint32_t d, const char *what) {
  LH_REQUIRE(dtype == LANCE_HIP_F32 || dtype == LANCE_HIP_F16, "%s: SQ builder: unsupported data type: element type %d (f32 = 0 and f16 = 1 are supported)",
             what, dtype);
  LH_REQUIRE(d >= 1 && d <= SQ_MAX_DIM, "%s: d=%u not supported (1..%u)", what, d, SQ_MAX_DIM);
  return LANCE_HIP_OK;
}

static int sq_check_bounds(const double *bounds_host, const char *what) {
  LH_REQUIRE(bounds_host, "%s: NULL bounds", what);
  LH_REQUIRE(std::isfinite(bounds_host[0]) && std::isfinite(bounds_host[1]) && bounds_host[0] <= bounds_host[1],
             "%s: bounds %g..%g are not a finite, ordered range (fold a column with lance_hip_sq_bounds first)", what, bounds_host[0], bounds_host[1]);
  return LANCE_HIP_OK;
}

static float sq_r2(double lo, double hi) {
  const float r = (float)(hi - lo);     // `(bounds.end - bounds.start) as f32`, then range.powi(2)
  return r * r;
}

static unsigned sq_grid(uint64_t count) { return grid_stride_blocks(count, 256, 2048); }

// rows of `dtype` elements -> codes out[row * ldo + col]
static int sq_encode_launch(lance_hip_ctx *ctx, int dtype, const void *x, uint64_t n, uint32_t d, double lo, double hi, int64_t ldo, uint8_t *out) {
  const uint64_t count = n * d;
  if (count == 0) return LANCE_HIP_OK;
  const int degenerate = lo == hi;
  const double range = hi - lo;
  if (dtype == LANCE_HIP_F16)
    hipLaunchKernelGGL(sq_encode_kernel<__half>, dim3(sq_grid(count)), dim3(256), 0, ctx->stream, static_cast<const __half *>(x), (int64_t)count, (int)d,
                       ldo, lo, range, degenerate, out);
  else
    hipLaunchKernelGGL(sq_encode_kernel<float>, dim3(sq_grid(count)), dim3(256), 0, ctx->stream, static_cast<const float *>(x), (int64_t)count, (int)d,
                       ldo, lo, range, degenerate, out);
  LH_CHECK_HIP(hipGetLastError());
  return LANCE_HIP_OK;
}

// pair_cand.cuh: the merge step of IVF_SQ and IVF_RQ, at the capacity of w.k
int cand_merge_lists(lance_hip_ctx *ctx, const CandLists &w, uint32_t nq, uint64_t *ids, float *dists, const char *timer) {
  {
    ScopedTimer t(ctx, timer);
    if (w.k <= CAND_NARROW_K)
      hipLaunchKernelGGL((cand_merge_kernel<CAND_MERGE_NARROW, CAND_NARROW_K>), dim3(nq), dim3(256), cand_merge_bytes(CAND_MERGE_NARROW), ctx->stream, w, ids, dists);
    else
      hipLaunchKernelGGL((cand_merge_kernel<CAND_MERGE_WIDE, CAND_MAX_K>), dim3(nq), dim3(256), cand_merge_bytes(CAND_MERGE_WIDE), ctx->stream, w, ids, dists);
  }
  LH_CHECK_HIP(hipGetLastError());
  return LANCE_HIP_OK;
}

}  // namespace lh

using namespace lh;

extern "C" int lance_hip_sq_bounds(lance_hip_ctx *ctx, int dtype, const void *x, uint64_t count, double *bounds_host) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && bounds_host && (count == 0 || x), "sq_bounds: NULL argument");
  LH_REQUIRE(dtype == LANCE_HIP_F32 || dtype == LANCE_HIP_F16, "sq_bounds: SQ builder: unsupported data type: element type %d (f32 = 0 and f16 = 1 are supported)",
             dtype);
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  if (count == 0) return LANCE_HIP_OK;
  const unsigned grid = sq_grid(count);
  double *partials = ctx->scratch_t<double>("sq.bounds", (size_t)grid * 2);
  if (!partials) return LANCE_HIP_ENOMEM;
  if (dtype == LANCE_HIP_F16)
    hipLaunchKernelGGL(sq_bounds_kernel<__half>, dim3(grid), dim3(256), 64, ctx->stream, static_cast<const __half *>(x), (int64_t)count, partials);
  else
    hipLaunchKernelGGL(sq_bounds_kernel<float>, dim3(grid), dim3(256), 64, ctx->stream, static_cast<const float *>(x), (int64_t)count, partials);
  LH_CHECK_HIP(hipGetLastError());
  std::vector<double> h((size_t)grid * 2);
  LH_CHECK_HIP(hipMemcpyAsync(h.data(), partials, h.size() * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  double lo = bounds_host[0], hi = bounds_host[1];
  for (unsigned b = 0; b < grid; ++b) {      // f64::min / f64::max: a NaN operand is skipped (the partials never are NaN)
    if (!(lo == lo) || h[2 * b] < lo) lo = h[2 * b];
    if (!(hi == hi) || h[2 * b + 1] > hi) hi = h[2 * b + 1];
  }
  bounds_host[0] = lo; bounds_host[1] = hi;
  return LANCE_HIP_OK;
}

extern "C" int lance_hip_sq_encode(lance_hip_ctx *ctx, int dtype, const void *x, uint64_t n, uint32_t d, const double *bounds_host, uint8_t *codes) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && bounds_host && (n == 0 || (x && codes)), "sq_encode: NULL argument");
  LH_TRY(sq_check_column(dtype, d, "sq_encode"));
  LH_REQUIRE(!(bounds_host[0] != bounds_host[0]) && !(bounds_host[1] != bounds_host[1]), "sq_encode: NaN bounds");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  LH_TRY(sq_encode_launch(ctx, dtype, x, n, d, bounds_host[0], bounds_host[1], (int64_t)d, codes));
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return LANCE_HIP_OK;
}

// encoded, zero-padded queries [nq][ld] and (optionally) their sums of squares, in the scratch arena
static int sq_encode_queries(lance_hip_ctx *ctx, int dtype, const void *q, uint32_t nq, uint32_t d, double lo, double hi, uint32_t ld,
                             uint8_t **qcodes_out, uint32_t **qq_out) {
  uint8_t *qc = ctx->scratch_t<uint8_t>("sq.qcodes", (size_t)nq * ld);
  uint32_t *qq = ctx->scratch_t<uint32_t>("sq.qq", (size_t)nq);
  if (!qc || !qq) return LANCE_HIP_ENOMEM;
  LH_CHECK_HIP(lh::memset_async(qc, 0, (size_t)nq * ld, ctx->stream));
  LH_TRY(sq_encode_launch(ctx, dtype, q, nq, d, lo, hi, (int64_t)ld, qc));
  hipLaunchKernelGGL(sq_norms_kernel, dim3((unsigned)cdiv(nq, 256)), dim3(256), 0, ctx->stream, qc, (int64_t)nq, (int)ld, qq);
  LH_CHECK_HIP(hipGetLastError());
  *qcodes_out = qc; *qq_out = qq;
  return LANCE_HIP_OK;
}

extern "C" int lance_hip_sq_distance(lance_hip_ctx *ctx, int dtype, int metric, const uint8_t *codes, uint64_t n, uint32_t d, const void *q,
                                     uint32_t nq, const double *bounds_host, float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && (n == 0 || codes) && (nq == 0 || q) && (n == 0 || nq == 0 || dists), "sq_distance: NULL argument");
  LH_TRY(sq_check_column(dtype, d, "sq_distance"));
  LH_TRY(sq_check_bounds(bounds_host, "sq_distance"));
  LH_REQUIRE(metric == LANCE_HIP_L2 || metric == LANCE_HIP_DOT || metric == LANCE_HIP_COSINE, "sq_distance: bad metric %d", metric);
  LH_REQUIRE(nq <= 65535, "sq_distance: nq=%u not supported (<= 65535 per call)", nq);
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  if (n == 0 || nq == 0) return LANCE_HIP_OK;
  const uint32_t ld = (d + 15u) & ~15u;
  uint8_t *qc; uint32_t *qq;
  LH_TRY(sq_encode_queries(ctx, dtype, q, nq, d, bounds_host[0], bounds_host[1], ld, &qc, &qq));
  const int dot = metric == LANCE_HIP_DOT;     // L2 and Cosine share l2_distance_uint_scalar (sq/storage.rs:436-442)
  const float r2 = sq_r2(bounds_host[0], bounds_host[1]);
  const dim3 grid((unsigned)cdiv(n, 256), nq);
  const bool wide = d % 16 == 0 && (reinterpret_cast<uintptr_t>(codes) & 15) == 0;
  {
    ScopedTimer t(ctx, "sq_distance");
    if (wide) hipLaunchKernelGGL(sq_distance_kernel<true>, grid, dim3(256), ld, ctx->stream, codes, (int64_t)n, (int)d, qc, (int)ld, dot, r2, dists);
    else hipLaunchKernelGGL(sq_distance_kernel<false>, grid, dim3(256), ld, ctx->stream, codes, (int64_t)n, (int)d, qc, (int)ld, dot, r2, dists);
  }
  LH_CHECK_HIP(hipGetLastError());
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return LANCE_HIP_OK;
}

namespace lh {
int sq_row_sums(lance_hip_ctx *ctx, const uint8_t *codes, uint64_t n, uint32_t ld, uint32_t *out) {
  if (n == 0) return LANCE_HIP_OK;
  hipLaunchKernelGGL(sq_norms_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, ctx->stream, codes, (int64_t)n, (int)ld, out);
  LH_CHECK_HIP(hipGetLastError());
  return LANCE_HIP_OK;
}
}  // namespace lh

extern "C" int lance_hip_ivfsq_create(lance_hip_ctx *ctx, int dtype, int metric, uint32_t d, const void *centroids, uint32_t nlist,
                                      const uint8_t *codes, const uint32_t *part_ids, const uint64_t *row_ids, uint64_t n,
                                      const double *bounds_host, lance_hip_index **out) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && centroids && out && (n == 0 || (codes && part_ids)), "ivfsq_create: NULL argument");
  LH_TRY(sq_check_column(dtype, d, "ivfsq_create"));
  LH_TRY(sq_check_bounds(bounds_host, "ivfsq_create"));
  LH_REQUIRE(metric == LANCE_HIP_L2 || metric == LANCE_HIP_DOT || metric == LANCE_HIP_COSINE, "ivfsq_create: bad metric %d", metric);
  LH_REQUIRE(nlist > 0 && nlist <= 65536, "ivfsq_create: nlist=%u not supported", nlist);
  LH_REQUIRE(n < (1ull << 32), "ivfsq_create: n too large for this version");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  auto *ix = new lance_hip_index();
  ix->device = ctx->device; ix->metric = metric; ix->dtype = dtype; ix->d = d; ix->m = 0;
  ix->nlist = 0;      // see index.h: the IVF_PQ / IVF_FLAT entry points refuse the handle by this
  ix->sq = true; ix->sq_nlist = nlist; ix->sq_lo = bounds_host[0]; ix->sq_hi = bounds_host[1];
  const uint32_t ld = (d + 15u) & ~15u;
  ix->sq_ld = ld;
  auto fail = [&](int r) { delete ix; return r; };
  if (hipMalloc(reinterpret_cast<void **>(&ix->centroids), (size_t)nlist * d * 4) != hipSuccess) return fail(LANCE_HIP_ENOMEM);
  if (hipMalloc(reinterpret_cast<void **>(&ix->part_offsets), (size_t)(nlist + 1) * 4) != hipSuccess) return fail(LANCE_HIP_ENOMEM);
  int r = widen_into(ctx, dtype, centroids, (size_t)nlist * d, ix->centroids);
  if (r != LANCE_HIP_OK) return fail(r);
  uint32_t *perm = ctx->scratch_t<uint32_t>("index.perm", (size_t)(n ? n : 1));
  if (!perm) return fail(LANCE_HIP_ENOMEM);
  r = stable_group(ctx, part_ids, (int64_t)n, (int64_t)n, (int)nlist, 1, ix->part_offsets, perm, (int64_t)n, nullptr);
  if (r != LANCE_HIP_OK) return fail(r);
  ix->part_offsets_h.resize(nlist + 1);
  if (hipMemcpyAsync(ix->part_offsets_h.data(), ix->part_offsets, (size_t)(nlist + 1) * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) { set_error("ivfsq_create: HIP failure"); return fail(LANCE_HIP_ERUNTIME); }
  ix->n = ix->part_offsets_h[nlist];       // rows with part id NONE are dropped
  for (uint32_t p = 0; p < nlist; ++p) ix->max_part = std::max(ix->max_part, ix->part_offsets_h[p + 1] - ix->part_offsets_h[p]);
  const size_t code_bytes = (size_t)ix->n * ld;      // a multiple of 16: the sums that follow stay aligned
  if (hipMalloc(reinterpret_cast<void **>(&ix->codes), std::max<size_t>(code_bytes + (size_t)ix->n * 4, 16)) != hipSuccess) return fail(LANCE_HIP_ENOMEM);
  if (hipMalloc(reinterpret_cast<void **>(&ix->row_ids), std::max<size_t>((size_t)ix->n * 8, 16)) != hipSuccess) return fail(LANCE_HIP_ENOMEM);
  uint32_t *xx = reinterpret_cast<uint32_t *>(ix->codes + code_bytes);
  ix->sq_xx = xx;
  if (ix->n > 0) {
    hipLaunchKernelGGL(sq_gather_kernel, dim3(grid_stride_blocks((uint64_t)ix->n * ld)), dim3(256), 0, ctx->stream, codes, row_ids, perm,
                       (int64_t)ix->n, (int)d, (int)ld, ix->codes, ix->row_ids);
    hipLaunchKernelGGL(sq_norms_kernel, dim3((unsigned)cdiv(ix->n, 256)), dim3(256), 0, ctx->stream, ix->codes, (int64_t)ix->n, (int)ld, xx);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
      set_error("ivfsq_create: gather kernel failed");
      return fail(LANCE_HIP_ERUNTIME);
    }
  }
  *out = ix;
  return LANCE_HIP_OK;
}

static const CandNames SQ_NAMES = {"ivfsq", {"ivfsq_scan", "ivfsq_wide_scan"}, {"ivfsq_merge", "ivfsq_wide_merge"}, {"ivfsq_exact", "ivfsq_wide_exact"}};

// refine_factor == 0: the k best by the SQ distance.  Otherwise (lance_hip_ivfsq_search_refine, which has checked the arguments) the
// keff = k * refine_factor best are candidates [nq][keff] in the scratch arena, re-scored against the raw vectors with the ORIGINAL query
// (cand_search, pair_cand.cuh)
static int ivfsq_search_impl(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k, uint32_t nprobes,
                             const uint32_t *allow, uint64_t *ids, float *dists, uint32_t refine_factor = 0) {
  const bool refine = refine_factor != 0;
  if (!refine) LH_REQUIRE(k > 0 && k <= (uint32_t)SQ_MAX_K, "ivfsq_search: k=%u not supported (1..%d)", k, SQ_MAX_K);
  const uint32_t keff = refine ? k * refine_factor : k;
  if (nq == 0) return LANCE_HIP_OK;
  if (nprobes > idx->sq_nlist) nprobes = idx->sq_nlist;
  LH_REQUIRE(nprobes > 0, "ivfsq_search: nprobes must be > 0");
  const int d = (int)idx->d;
  const uint32_t ld = idx->sq_ld;
  const float *qf;
  LH_TRY(as_f32(ctx, idx->dtype, q, (size_t)nq * d, "f16.q", &qf));
  const float *q_orig = qf;            // what the refine scores with: a cosine index's key is normalised below, the original is not
  uint32_t *probes = ctx->scratch_t<uint32_t>("ivfsq.probes", (size_t)nq * nprobes);
  float *pd = ctx->scratch_t<float>("ivfsq.pdists", (size_t)nq * nprobes);
  if (!probes || !pd) return LANCE_HIP_ENOMEM;
  const bool cosine = idx->metric == LANCE_HIP_COSINE;
  if (cosine) {
    // knn.rs:498 normalises the key of a cosine query; the coarse quantiser of a cosine index works in L2 on normalised vectors
    // (ivf/v2.rs:455-465) and the SQ storage scores L2 between the codes of the normalised key and rows (sq/storage.rs:436-442)
    float *qn = ctx->scratch_t<float>("ivfsq.qn", (size_t)nq * d);
    if (!qn) return LANCE_HIP_ENOMEM;
    LH_TRY(launch_normalize(ctx, qf, (int64_t)nq, d, qn, idx->dtype == LANCE_HIP_F16));   // an f16 key is normalised in f16 arithmetic
    qf = qn;
  }
  LH_TRY(find_partitions_f32(ctx, cosine ? LANCE_HIP_L2 : idx->metric, qf, nq, idx->d, idx->centroids, idx->sq_nlist, nprobes, probes, pd,
                             idx->dtype == LANCE_HIP_F16 && idx->metric == LANCE_HIP_DOT && d > 16));
  uint8_t *qc; uint32_t *qq;
  {
    ScopedTimer t(ctx, "ivfsq_encode_q");      // the key holds f32 values by now (f16 widened exactly, or the normalised key)
    LH_TRY(sq_encode_queries(ctx, LANCE_HIP_F32, qf, nq, idx->d, idx->sq_lo, idx->sq_hi, ld, &qc, &qq));
  }
  SqArgs a = {};
  a.codes = idx->codes; a.xx = idx->sq_xx; a.ld = (int)ld; a.dot = idx->metric == LANCE_HIP_DOT; a.r2 = sq_r2(idx->sq_lo, idx->sq_hi);
  a.w.row_ids = idx->row_ids; a.w.part_offsets = idx->part_offsets; a.w.allow = allow; a.w.nprobes = (int)nprobes; a.w.k = (int)keff;
  a.w.cap = sq_scan_cap(ld, (int)keff);
  auto chunk = [&](const CandLists &w, uint32_t q0) { a.w = w; a.qcodes = qc + (size_t)q0 * ld; a.qq = qq + q0; };
  return cand_search(
      ctx, idx, SQ_NAMES, a.w, probes, nq, k, refine, q_orig, ids, dists,
      [&](const CandLists &w, uint32_t q0, uint32_t nqc) {
        chunk(w, q0);
        hipLaunchKernelGGL(sq_scan_kernel, dim3(nqc * nprobes), dim3(256), sq_scan_lds(ld, w.cap), ctx->stream, a);
      },
      [&](const CandLists &w, uint32_t q0, uint32_t nqc, uint64_t *oid, float *od) {
        chunk(w, q0);
        hipLaunchKernelGGL(sq_exact_kernel, dim3(nqc), dim3(64), sq_replay_lds(ld, w.k), ctx->stream, a, oid, od);
      });
}

static int ivfsq_check(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, const uint64_t *ids, const float *dists) {
  LH_REQUIRE(ctx && idx && (nq == 0 || (q && ids && dists)), "ivfsq_search: NULL argument");
  LH_REQUIRE(idx->sq && idx->codes, "ivfsq_search: not an IVF_SQ index");
  LH_REQUIRE(ctx->device == idx->device, "ivfsq_search: context and index live on different devices");
  return LANCE_HIP_OK;
}

extern "C" int lance_hip_ivfsq_search(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                                      uint32_t nprobes, uint64_t *ids, float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  LH_TRY(ivfsq_check(ctx, idx, q, nq, ids, dists));
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  return ivfsq_search_impl(ctx, idx, q, nq, k, nprobes, nullptr, ids, dists);
}

extern "C" int lance_hip_ivfsq_search_filtered(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                                               uint32_t nprobes, const uint8_t *allow_by_rowid, uint64_t n_allow, uint64_t *ids,
                                               float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  LH_TRY(ivfsq_check(ctx, idx, q, nq, ids, dists));
  LH_REQUIRE(allow_by_rowid || n_allow == 0, "ivfsq_search_filtered: NULL filter");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  const uint32_t *bits = nullptr;
  LH_TRY(build_allow_bits(ctx, idx->row_ids, idx->n, allow_by_rowid, n_allow, &bits));
  return ivfsq_search_impl(ctx, idx, q, nq, k, nprobes, bits, ids, dists);
}

// keff = k * refine_factor candidates by the SQ distance, re-scored against the raw vectors (lance_hip_index_set_raw) with the original query
extern "C" int lance_hip_ivfsq_search_refine(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, uint32_t k,
                                             uint32_t nprobes, uint32_t refine_factor, const uint8_t *allow_by_rowid, uint64_t n_allow,
                                             uint64_t *ids, float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  LH_TRY(ivfsq_check(ctx, idx, q, nq, ids, dists));
  LH_REQUIRE(refine_factor >= 1, "ivfsq_search_refine: refine_factor can not be zero");
  LH_REQUIRE(k >= 1 && (uint64_t)k * refine_factor <= (uint64_t)LANCE_HIP_SQRQ_MAX_CANDIDATES,
             "ivfsq_search_refine: k * refine_factor = %llu not supported (1..%d, LANCE_HIP_SQRQ_MAX_CANDIDATES)",
             (unsigned long long)k * refine_factor, LANCE_HIP_SQRQ_MAX_CANDIDATES);
  LH_REQUIRE(idx->raw != nullptr, "ivfsq_search_refine: refine_factor needs raw vectors (lance_hip_index_set_raw)");
  LH_REQUIRE(allow_by_rowid || n_allow == 0, "ivfsq_search_refine: NULL filter");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  const uint32_t *bits = nullptr;
  if (allow_by_rowid) LH_TRY(build_allow_bits(ctx, idx->row_ids, idx->n, allow_by_rowid, n_allow, &bits));
  return ivfsq_search_impl(ctx, idx, q, nq, k, nprobes, bits, ids, dists, refine_factor);
}
