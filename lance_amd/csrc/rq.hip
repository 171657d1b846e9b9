// rq.hip -- 1-bit RaBitQ (RQ) and the IVF_RQ index: encode, query preparation, distances, search.
//
//   RabitQuantizer::quantize / codes_res_dot_dists                       lance-index/src/vector/bq/builder.rs
//   RQTransformer::transform (add / scale factors)                       bq/transform.rs:95-208
//   rotate_query_vector, quantize_dist_table, compute_rq_distance_flat   bq/storage.rs:130-156, 249-294
//   RabitDistCalculator::distance / distance_all, dist_calculator        bq/storage.rs:296-369, 409-445
//   IvfTransformer::with_rq, preprocess_query                            ivf.rs:281-326, lance/src/index/vector/ivf/v2.rs:316-332
//   FlatIndex::search (the sub-index of IVF_RQ)                          flat/index.rs:82-177
//
// Every floating-point operation below is one f32 rounding in the reference's order (the file is compiled without contraction).
// The build side's rotation is summed in the order of lance_linalg::distance::dot, this project's definition (the reference runs
// a BLAS GEMM there, whose order is not a specification -- DESIGN.md); everything on the query side is the reference's arithmetic.
//
// A row's distance takes one of three branches (bq/storage.rs:296-369):
//   packed     rows [0, n - n % 32) of a partition, no prefilter: u8 table entries summed in integers, saturating at 65535
//   remainder  rows [n - n % 32, n), no prefilter: f32 table entries added in byte order from 0.0
//   filtered   every selected row under a prefilter: the same f32 terms folded by f32::sum (from -0.0)
//
// Search: one workgroup per (query, probed partition) prepares that pair's tables in LDS (residual, rotation, the 16-entry table of
// every 4 dimensions and its u8 quantisation), scans the partition's rows once and keeps the pair's k best (key, storage position);
// the per-pair lists are merged per query by (dist, rowid) with the replay decision, and flagged queries are replayed through std
// BinaryHeap's push / pop in storage order.  Selection, merge and replay are pair_cand.cuh's, shared with IVF_SQ; this file supplies
// the preparation and the row distance.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "exact.cuh"
#include "index.h"
#include "kernels.h"
#include "search_common.cuh"
#include "pair_cand.cuh"

#pragma clang fp contract(off)

namespace lh {

constexpr uint32_t RQ_MAX_DIM = LANCE_HIP_RQ_MAX_DIM;
constexpr int RQ_MAX_K = 128;
constexpr int RQ_BATCH = 32;         // BATCH_SIZE of sum_4bit_dist_table: rows past the last full batch take the f32 branch
enum { RQ_PACKED = 0, RQ_REMAINDER = 1, RQ_FILTERED = 2 };

// dot(P[j], v) in the order of lance_linalg::distance::dot (dot.rs:30-58; dist_exact_rt<METRIC_DOT> restates it): 16 lane
// accumulators over the full chunks, summed in lane order, plus the sequentially summed tail.  pt is P transposed ([i][j], row
// stride D), so the lanes j of a wave read consecutive words.
__device__ __forceinline__ float rq_rot_dot(const float *__restrict__ pt, int D, int j, const float *v, int d) {
  const int full = d / 16 * 16;
  float s = 0.0f;
  if (full != d) {
    float acc = 0.0f;
    for (int i = full; i < d; ++i) acc = acc + pt[(int64_t)i * D + j] * v[i];
    s = acc;
  }
  float sums[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) sums[i] = 0.0f;
  for (int c = 0; c < full; c += 16) {
#pragma unroll
    for (int i = 0; i < 16; ++i) sums[i] = sums[i] + pt[(int64_t)(c + i) * D + j] * v[c + i];
  }
  float tot = 0.0f;
#pragma unroll
  for (int i = 0; i < 16; ++i) tot = tot + sums[i];
  return s + tot;
}

// out[i][j] = in[j][i]
__global__ __launch_bounds__(256) void rq_transpose_kernel(const float *__restrict__ in, int d, float *__restrict__ out) {
  const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (g >= (int64_t)d * d) return;
  const int i = (int)(g / d), j = (int)(g - (int64_t)i * d);
  out[g] = in[(int64_t)j * d + i];
}

// ---- encode (bq/builder.rs quantize + codes_res_dot_dists, bq/transform.rs:95-208) -------------------------------------------
struct RqEncArgs {
  const float *x;            // [n][d]
  int64_t n;
  int d, nlist, dot;
  const uint32_t *part;      // [n] partition of every row (LANCE_HIP_NONE, or anything >= nlist: no partition -- zeros out)
  const float *dvc;          // [n] the distance the partition assignment reported
  const float *cent;         // [nlist][d]
  const float *pt;           // [d][d] rotation, transposed
  float sqrt_d;
  uint8_t *codes;            // [n][d / 8]
  float *add, *scale;        // [n]
};

// rows-per-iteration max(1, 256 / d) rows are staged as residuals in LDS; thread (row, j) rotates, thread (row, byte) packs the sign
// bits, one thread per row folds the sequential sums.  Dynamic LDS: 2 * max(d, 256) floats.
__global__ __launch_bounds__(256) void rq_encode_kernel(RqEncArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int d = a.d, cb = d / 8;
  const int rpi = d >= 256 ? 1 : 256 / d;
  float *res = reinterpret_cast<float *>(smem);        // [rpi][d]
  float *rot = res + (d >= 256 ? d : 256);             // [rpi][d]
  const int t = threadIdx.x;
  for (int64_t base = (int64_t)blockIdx.x * rpi; base < a.n; base += (int64_t)gridDim.x * rpi) {
    for (int idx = t; idx < rpi * d; idx += 256) {
      const int lr = idx / d, i = idx - lr * d;
      const int64_t row = base + lr;
      float v = 0.0f;
      if (row < a.n) {
        const uint32_t p = a.part[row];
        if (p < (uint32_t)a.nlist) v = a.x[row * d + i] - a.cent[(int64_t)p * d + i];
      }
      res[idx] = v;
    }
    __syncthreads();
    for (int idx = t; idx < rpi * d; idx += 256) {
      const int lr = idx / d, j = idx - lr * d;
      rot[idx] = base + lr < a.n ? rq_rot_dot(a.pt, d, j, res + lr * d, d) : 0.0f;
    }
    __syncthreads();
    for (int idx = t; idx < rpi * cb; idx += 256) {
      const int lr = idx / cb, b = idx - lr * cb;
      const int64_t row = base + lr;
      if (row < a.n) {
        uint32_t byte = 0;
        if (a.part[row] < (uint32_t)a.nlist) {
#pragma unroll
          for (int u = 0; u < 8; ++u) byte |= ((__float_as_uint(rot[lr * d + 8 * b + u]) >> 31) ^ 1u) << u;     // is_sign_positive
        }
        a.codes[row * cb + b] = (uint8_t)byte;
      }
    }
    if (t < rpi && base + t < a.n) {
      const int64_t row = base + t;
      const uint32_t p = a.part[row];
      float add = 0.0f, scale = 0.0f;
      if (p < (uint32_t)a.nlist) {
        float sabs = 0.0f;
        for (int j = 0; j < d; ++j) sabs = sabs + fabsf(rot[t * d + j]);
        const float ip = __fdiv_rn(sabs, a.sqrt_d);
        const float dvc = a.dvc[row];
        if (a.dot) {
          float res2 = 0.0f, c2 = 0.0f;      // norm_squared_fsl: v.iter().map(|v| v * v).sum()
          for (int i = 0; i < d; ++i) { const float r = res[t * d + i]; res2 = res2 + r * r; }
          for (int i = 0; i < d; ++i) { const float c = a.cent[(int64_t)p * d + i]; c2 = c2 + c * c; }
          add = dvc + c2;
          scale = ip == 0.0f ? -0.0f : -__fdiv_rn(res2, ip);           // -(res2.div_checked(ip).unwrap_or_default())
        } else {
          add = dvc;
          scale = ip == 0.0f ? 0.0f : __fdiv_rn(-2.0f * dvc, ip);      // (-2.0 * res2).div_checked(ip).unwrap_or_default()
        }
      }
      a.add[row] = add; a.scale[row] = scale;
    }
    __syncthreads();
  }
}

// ---- query preparation (dist_calculator, bq/storage.rs:409-445; build_dist_table_direct; quantize_dist_table) ----------------
struct RqQuery { float sum_q, q_factor, range, sum_min; uint32_t kmin, kmax; };

// LDS of one prepared (query, partition): table f32 [d / 4][16] | etab u8 [d / 4][16] | then the caller's own area.
// During the preparation the residual query lives in etab's bytes (d floats = 4 d bytes, exactly its size) and the rotated query
// in `rqv` (d floats of the caller's area, free again when this returns).  c == NULL: q already is the residual.
template <int BS>
__device__ __forceinline__ void rq_prepare(const float *__restrict__ q, const float *__restrict__ c, const float *__restrict__ pt, int d,
                                           float dist_q_c, int dot, bool quantise, float *table, uint8_t *etab, float *rqv, RqQuery *h) {
  float *qr = reinterpret_cast<float *>(etab);
  const int t = threadIdx.x;
  for (int i = t; i < d; i += BS) qr[i] = c ? q[i] - c[i] : q[i];
  if (t == 0) { h->kmin = 0xFFFFFFFFu; h->kmax = 0u; }
  __syncthreads();
  for (int j = t; j < d; j += BS) rqv[j] = rq_rot_dot(pt, d, j, qr, d);
  __syncthreads();
  uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
  for (int s = t; s < d / 4; s += BS) {
    float tt[16];
    tt[0] = 0.0f;
#pragma unroll
    for (int j = 1; j < 16; ++j) tt[j] = tt[j - (j & -j)] + rqv[4 * s + __builtin_ctz(j)];
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      table[s * 16 + j] = tt[j];
      const uint32_t key = order_key(tt[j]);        // minmax_by(total_cmp)
      kmin = key < kmin ? key : kmin; kmax = key > kmax ? key : kmax;
    }
  }
  if (kmin <= kmax) { atomicMin(&h->kmin, kmin); atomicMax(&h->kmax, kmax); }
  if (t == 0) {
    float sum = -0.0f;                              // f32::sum
    for (int j = 0; j < d; ++j) sum = sum + rqv[j];
    h->sum_q = sum;
    h->q_factor = dot ? dist_q_c - 1.0f : dist_q_c;
  }
  __syncthreads();
  if (quantise) {
    const float qmin = key_to_float(h->kmin), qmax = key_to_float(h->kmax);
    if (qmin == qmax) {                             // "this happens if the query is all zeros"
      for (int i = t; i < 4 * d; i += BS) etab[i] = 0;
    } else {
      const float factor = __fdiv_rn(255.0f, qmax - qmin);
      for (int i = t; i < 4 * d; i += BS) {
        const float r = roundf((table[i] - qmin) * factor);      // f32::round: half away from zero
        etab[i] = !(r > 0.0f) ? (uint8_t)0 : (r >= 255.0f ? (uint8_t)255 : (uint8_t)(int)r);      // `as u8`: saturating, NaN -> 0
      }
    }
    if (t == 0) {
      h->range = __fdiv_rn(qmax - qmin, 255.0f);
      h->sum_min = (float)(d / 4) * qmin;
    }
  }
  __syncthreads();
}

// one row's distance; `row` points at its d / 8 code bytes (16-byte aligned when cb % 16 == 0)
__device__ __forceinline__ float rq_row_distance(const uint8_t *__restrict__ row, int cb, int mode, const float *table, const uint8_t *etab,
                                                 const RqQuery *h, float sqrt_d, float add, float scale) {
  float dist;
  if (mode == RQ_PACKED) {
    uint32_t s = 0;
    if ((cb & 15) == 0) {
      for (int w = 0; w < cb / 16; ++w) {
        const uint4 v = reinterpret_cast<const uint4 *>(row)[w];
        const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const uint32_t code = (ws[u >> 2] >> (8 * (u & 3))) & 255u;
          const int b = 16 * w + u;
          s += (uint32_t)etab[(2 * b) * 16 + (code & 15u)] + (uint32_t)etab[(2 * b + 1) * 16 + (code >> 4)];
        }
      }
    } else {
      for (int b = 0; b < cb; ++b) {
        const uint32_t code = row[b];
        s += (uint32_t)etab[(2 * b) * 16 + (code & 15u)] + (uint32_t)etab[(2 * b + 1) * 16 + (code >> 4)];
      }
    }
    s = s < 65535u ? s : 65535u;                    // u16 saturating adds of non-negative terms
    dist = (float)s * h->range + h->sum_min;
  } else {
    dist = mode == RQ_FILTERED ? -0.0f : 0.0f;      // f32::sum / `dists = vec![0.0; n]`
    if ((cb & 15) == 0) {
      for (int w = 0; w < cb / 16; ++w) {
        const uint4 v = reinterpret_cast<const uint4 *>(row)[w];
        const uint32_t ws[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          const uint32_t code = (ws[u >> 2] >> (8 * (u & 3))) & 255u;
          const int b = 16 * w + u;
          dist = dist + (table[(2 * b) * 16 + (code & 15u)] + table[(2 * b + 1) * 16 + (code >> 4)]);
        }
      }
    } else {
      for (int b = 0; b < cb; ++b) {
        const uint32_t code = row[b];
        dist = dist + (table[(2 * b) * 16 + (code & 15u)] + table[(2 * b + 1) * 16 + (code >> 4)]);
      }
    }
  }
  const float x = __fdiv_rn(2.0f * dist - h->sum_q, sqrt_d);
  return x * scale + add + h->q_factor;
}

// distance_all (quantised != 0) or distance of every row (quantised == 0) of ONE partition's storage [n][cb] against residual queries
// qr [nq][d]: the testable middle.  grid (row blocks, nq); dynamic LDS 24 d + sizeof(RqQuery) bytes.
__global__ __launch_bounds__(256) void rq_distance_kernel(const uint8_t *__restrict__ codes, const float *__restrict__ add, const float *__restrict__ scale,
                                                          int64_t n, int d, const float *__restrict__ qr, const float *__restrict__ dqc,
                                                          const float *__restrict__ pt, int dot, int quantised, float sqrt_d, float *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float *table = reinterpret_cast<float *>(smem);
  uint8_t *etab = reinterpret_cast<uint8_t *>(smem + 16 * (size_t)d);
  float *rqv = reinterpret_cast<float *>(smem + 20 * (size_t)d);
  RqQuery *h = reinterpret_cast<RqQuery *>(smem + 24 * (size_t)d);
  const int q = blockIdx.y, cb = d / 8;
  rq_prepare<256>(qr + (int64_t)q * d, nullptr, pt, d, dqc[q], dot, quantised != 0, table, etab, rqv, h);
  const int64_t np = n - n % RQ_BATCH;
  for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < n; row += (int64_t)gridDim.x * 256) {
    const int mode = quantised ? (row < np ? RQ_PACKED : RQ_REMAINDER) : RQ_FILTERED;
    out[(int64_t)q * n + row] = rq_row_distance(codes + row * cb, cb, mode, table, etab, h, sqrt_d, add[row], scale[row]);
  }
}

// codes [n][cb] and factors -> partition order; one thread per output byte
__global__ __launch_bounds__(256) void rq_gather_kernel(const uint8_t *__restrict__ codes, const float *__restrict__ add, const float *__restrict__ scale,
                                                        const uint64_t *__restrict__ row_ids, const uint32_t *__restrict__ perm, int64_t n_out, int cb,
                                                        uint8_t *__restrict__ out, float *__restrict__ add_out, float *__restrict__ scale_out,
                                                        uint64_t *__restrict__ rid_out) {
  for (int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x; g < n_out * cb; g += (int64_t)gridDim.x * 256) {      // (grid.h)
    const int64_t s = g / cb;
    const int c = (int)(g - s * cb);
    const uint32_t r = perm[s];
    out[g] = codes[(int64_t)r * cb + c];
    if (c == 0) { add_out[s] = add[r]; scale_out[s] = scale[r]; rid_out[s] = row_ids ? row_ids[r] : (uint64_t)r; }
  }
}

// ---- IVF_RQ search (pair_cand.cuh with the RQ preparation and row distance) -------------------------------------------------------
struct RqArgs {
  const uint8_t *codes;          // [n][cb] partition-ordered
  const float *add, *scale;      // [n]
  const float *pdists;           // [nq][nprobes] dist_q_c of every pair
  const float *q;                // [nq][d]
  const float *cent;             // [nlist][d]
  const float *pt;               // [d][d] rotation, transposed
  int d, dot;
  float sqrt_d;
  CandLists w;
};

// dynamic LDS (rq_scan_lds): table 16 d | etab 4 d | u64 entries [w.cap] | RqQuery | CandCtl.  During the preparation the first 4 d bytes of
// the entries hold the rotated query (4 d <= 8 w.cap: rq_scan_cap).
__global__ __launch_bounds__(256) void rq_scan_kernel(RqArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int d = a.d, cb = d / 8;
  float *table = reinterpret_cast<float *>(smem);
  uint8_t *etab = reinterpret_cast<uint8_t *>(smem + 16 * (size_t)d);
  uint64_t *e = reinterpret_cast<uint64_t *>(smem + 20 * (size_t)d);
  RqQuery *h = reinterpret_cast<RqQuery *>(e + a.w.cap);
  CandCtl *ctl = reinterpret_cast<CandCtl *>(h + 1);
  const int pair = blockIdx.x;
  const int qi = pair / a.w.nprobes;
  const uint32_t part = a.w.probes[pair];
  const uint32_t r0 = a.w.part_offsets[part], r1 = a.w.part_offsets[part + 1];
  if (threadIdx.x == 0) { ctl->cnt = 0; ctl->thr = 0xFFFFFFFFu; ctl->amb_key = 0; ctl->amb = 0; }
  if (r1 > r0) {     // (uniform) an empty partition needs no tables
    rq_prepare<256>(a.q + (int64_t)qi * d, a.cent + (int64_t)part * d, a.pt, d, a.pdists[pair], a.dot, a.w.allow == nullptr, table, etab,
                    reinterpret_cast<float *>(e), h);
  } else {
    __syncthreads();
  }
  const uint32_t np = r0 + ((r1 - r0) - (r1 - r0) % RQ_BATCH);      // first row of the f32 remainder
  cand_scan_pair(a.w, pair, r0, r1, e, ctl, [&](uint32_t row) {
    const int mode = a.w.allow ? RQ_FILTERED : (row < np ? RQ_PACKED : RQ_REMAINDER);
    return order_key(rq_row_distance(a.codes + (int64_t)row * cb, cb, mode, table, etab, h, a.sqrt_d, a.add[row], a.scale[row]));
  });
}

struct RqDist {
  const RqArgs &a;
  int qi;
  float *table;
  uint8_t *etab;
  float *rqv;
  RqQuery *h;
  __device__ __forceinline__ void partition(int pi, uint32_t part) {
    rq_prepare<64>(a.q + (int64_t)qi * a.d, a.cent + (int64_t)part * a.d, a.pt, a.d, a.pdists[(int64_t)qi * a.w.nprobes + pi], a.dot,
                   a.w.allow == nullptr, table, etab, rqv, h);
  }
  __device__ __forceinline__ uint32_t key(uint32_t off, int row, int np) const {
    const int cb = a.d / 8;
    const int mode = a.w.allow ? RQ_FILTERED : (row < np - np % RQ_BATCH ? RQ_PACKED : RQ_REMAINDER);
    const int64_t r = (int64_t)off + row;
    return order_key(rq_row_distance(a.codes + r * cb, cb, mode, table, etab, h, a.sqrt_d, a.add[r], a.scale[r]));
  }
};

// the heap replay of a flagged query.  Dynamic LDS (rq_replay_lds): table 16 d | etab 4 d | rotated query 4 d | RqQuery (24 bytes) |
// replay area: at d = 2048 and k = 768 that is 49152 + 24 + 15664 = 64840 of the 65536 bytes.  (Six waves per SIMD: 80 VGPRs.  Left alone
// the allocator takes 81 -- one occupancy step for one register --; held to 80 it needs 77 and spills nothing.)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6))) void rq_exact_kernel(RqArgs a, uint64_t *__restrict__ out_ids, float *__restrict__ out_dists) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int qi = blockIdx.x;
  if (!a.w.flags[qi]) return;
  const size_t d = (size_t)a.d;
  RqDist dist = {a, qi, reinterpret_cast<float *>(smem), reinterpret_cast<uint8_t *>(smem + 16 * d), reinterpret_cast<float *>(smem + 20 * d),
                 reinterpret_cast<RqQuery *>(smem + 24 * d)};
  cand_replay_query(a.w, qi, smem + 24 * d + sizeof(RqQuery), dist, out_ids, out_dists);
}
static_assert(sizeof(RqQuery) % 8 == 0, "the replay area that follows RqQuery holds 64-bit row ids");

// launch sizes.  Up to CAND_NARROW_K the buffer has 512 entries (20 d + 4096 + 40 bytes of LDS) while the rotated query fits into it, i.e. up
// to d = 1024, and 1024 beyond (49,192 bytes at d = 2048); above, the largest that fits.
static inline int rq_scan_cap(uint32_t d, int k) { return cand_scan_cap(k, (size_t)20 * d + sizeof(RqQuery) + sizeof(CandCtl), (size_t)4 * d); }
static inline size_t rq_scan_lds(uint32_t d, int cap) { return (size_t)20 * d + (size_t)cap * 8 + sizeof(RqQuery) + sizeof(CandCtl); }
static inline size_t rq_replay_lds(uint32_t d, int k) { return (size_t)24 * d + sizeof(RqQuery) + cand_replay_bytes(k); }

// ---- host side ---------------------------------------------------------------------------------------------------------------
static int rq_check_shape(int metric, uint32_t d, const char *what) {
  LH_REQUIRE(metric != LANCE_HIP_COSINE,
             "%s: the cosine metric is not supported for IVF_RQ (which distance type the reference's loaded storage carries into q_factor is not established); use l2 or dot",
             what);
  LH_REQUIRE(metric == LANCE_HIP_L2 || metric == LANCE_HIP_DOT, "%s: bad metric %d", what, metric);
  LH_REQUIRE(d >= 8 && d % 8 == 0 && d <= RQ_MAX_DIM, "%s: d=%u not supported (a multiple of 8, 8..%u: one bit per dimension packed into bytes)", what, d,
             RQ_MAX_DIM);
  return LANCE_HIP_OK;
}

// the rotation transposed, in the scratch arena
static int rq_transposed(lance_hip_ctx *ctx, const float *rotation, uint32_t d, const float **out) {
  float *pt = ctx->scratch_t<float>("rq.rot_t", (size_t)d * d);
  if (!pt) return LANCE_HIP_ENOMEM;
  hipLaunchKernelGGL(rq_transpose_kernel, dim3((unsigned)cdiv((uint64_t)d * d, 256)), dim3(256), 0, ctx->stream, rotation, (int)d, pt);
  LH_CHECK_HIP(hipGetLastError());
  *out = pt;
  return LANCE_HIP_OK;
}

static_assert(CAND_MAX_K == LANCE_HIP_SQRQ_MAX_CANDIDATES, "the candidate path's capacity is the public limit");

}  // namespace lh

using namespace lh;

extern "C" int lance_hip_rq_encode(lance_hip_ctx *ctx, int metric, const float *x, uint64_t n, uint32_t d, const uint32_t *part_ids,
                                   const float *dist_v_c, const float *centroids, uint32_t nlist, const float *rotation, uint8_t *codes,
                                   float *add, float *scale) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && centroids && rotation && (n == 0 || (x && part_ids && dist_v_c && codes && add && scale)), "rq_encode: NULL argument");
  LH_TRY(rq_check_shape(metric, d, "rq_encode"));
  LH_REQUIRE(nlist > 0 && nlist <= 65536, "rq_encode: nlist=%u not supported", nlist);
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  if (n == 0) return LANCE_HIP_OK;
  RqEncArgs a;
  LH_TRY(rq_transposed(ctx, rotation, d, &a.pt));
  a.x = x; a.n = (int64_t)n; a.d = (int)d; a.nlist = (int)nlist; a.dot = metric == LANCE_HIP_DOT; a.part = part_ids; a.dvc = dist_v_c;
  a.cent = centroids; a.sqrt_d = std::sqrt((float)d); a.codes = codes; a.add = add; a.scale = scale;
  const uint32_t rpi = d >= 256 ? 1 : 256 / d;
  const unsigned grid = (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(cdiv(n, rpi), 8192));
  {
    ScopedTimer t(ctx, "rq_encode");
    hipLaunchKernelGGL(rq_encode_kernel, dim3(grid), dim3(256), (size_t)8 * std::max<uint32_t>(d, 256), ctx->stream, a);
  }
  LH_CHECK_HIP(hipGetLastError());
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return LANCE_HIP_OK;
}

extern "C" int lance_hip_rq_distance(lance_hip_ctx *ctx, int metric, const uint8_t *codes, const float *add, const float *scale, uint64_t n,
                                     uint32_t d, const float *qr, const float *dist_q_c, uint32_t nq, const float *rotation, int quantised,
                                     float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && rotation && (n == 0 || (codes && add && scale)) && (nq == 0 || (qr && dist_q_c)) && (n == 0 || nq == 0 || dists),
             "rq_distance: NULL argument");
  LH_TRY(rq_check_shape(metric, d, "rq_distance"));
  LH_REQUIRE(nq <= 65535, "rq_distance: nq=%u not supported (<= 65535 per call)", nq);
  LH_REQUIRE(d % 128 != 0 || (reinterpret_cast<uintptr_t>(codes) & 15) == 0, "rq_distance: codes of 16-byte rows must be 16-byte aligned");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  if (n == 0 || nq == 0) return LANCE_HIP_OK;
  const float *pt;
  LH_TRY(rq_transposed(ctx, rotation, d, &pt));
  const dim3 grid((unsigned)std::min<uint64_t>(cdiv(n, 256), 64), nq);
  {
    ScopedTimer t(ctx, "rq_distance");
    hipLaunchKernelGGL(rq_distance_kernel, grid, dim3(256), (size_t)24 * d + sizeof(RqQuery), ctx->stream, codes, add, scale, (int64_t)n, (int)d, qr,
                       dist_q_c, pt, (int)(metric == LANCE_HIP_DOT), quantised, std::sqrt((float)d), dists);
  }
  LH_CHECK_HIP(hipGetLastError());
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return LANCE_HIP_OK;
}

extern "C" int lance_hip_ivfrq_create(lance_hip_ctx *ctx, int metric, uint32_t d, const float *centroids, uint32_t nlist, const float *rotation,
                                      const uint8_t *codes, const float *add, const float *scale, const uint32_t *part_ids,
                                      const uint64_t *row_ids, uint64_t n, lance_hip_index **out) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && centroids && rotation && out && (n == 0 || (codes && add && scale && part_ids)), "ivfrq_create: NULL argument");
  LH_TRY(rq_check_shape(metric, d, "ivfrq_create"));
  LH_REQUIRE(nlist > 0 && nlist <= 65536, "ivfrq_create: nlist=%u not supported", nlist);
  LH_REQUIRE(n < (1ull << 32), "ivfrq_create: n too large for this version");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  auto *ix = new lance_hip_index();
  ix->device = ctx->device; ix->metric = metric; ix->dtype = LANCE_HIP_F32; ix->d = d; ix->m = 0;
  ix->nlist = 0;      // see index.h: the IVF_PQ / IVF_FLAT entry points refuse the handle by this
  ix->rq = true; ix->rq_nlist = nlist;
  const uint32_t cb = d / 8;
  ix->rq_cb = cb;
  auto fail = [&](int r) { delete ix; return r; };
  if (hipMalloc(reinterpret_cast<void **>(&ix->centroids), (size_t)nlist * d * 4) != hipSuccess) return fail(LANCE_HIP_ENOMEM);
  if (hipMalloc(reinterpret_cast<void **>(&ix->rq_rot_t), (size_t)d * d * 4) != hipSuccess) return fail(LANCE_HIP_ENOMEM);
  if (hipMalloc(reinterpret_cast<void **>(&ix->part_offsets), (size_t)(nlist + 1) * 4) != hipSuccess) return fail(LANCE_HIP_ENOMEM);
  if (hipMemcpyAsync(ix->centroids, centroids, (size_t)nlist * d * 4, hipMemcpyDeviceToDevice, ctx->stream) != hipSuccess) {
    set_error("ivfrq_create: HIP failure");
    return fail(LANCE_HIP_ERUNTIME);
  }
  hipLaunchKernelGGL(rq_transpose_kernel, dim3((unsigned)cdiv((uint64_t)d * d, 256)), dim3(256), 0, ctx->stream, rotation, (int)d, ix->rq_rot_t);
  uint32_t *perm = ctx->scratch_t<uint32_t>("index.perm", (size_t)(n ? n : 1));
  if (!perm) return fail(LANCE_HIP_ENOMEM);
  int r = stable_group(ctx, part_ids, (int64_t)n, (int64_t)n, (int)nlist, 1, ix->part_offsets, perm, (int64_t)n, nullptr);
  if (r != LANCE_HIP_OK) return fail(r);
  ix->part_offsets_h.resize(nlist + 1);
  if (hipMemcpyAsync(ix->part_offsets_h.data(), ix->part_offsets, (size_t)(nlist + 1) * 4, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess) { set_error("ivfrq_create: HIP failure"); return fail(LANCE_HIP_ERUNTIME); }
  ix->n = ix->part_offsets_h[nlist];       // rows with part id NONE are dropped
  for (uint32_t p = 0; p < nlist; ++p) ix->max_part = std::max(ix->max_part, ix->part_offsets_h[p + 1] - ix->part_offsets_h[p]);
  const size_t code_bytes = ((size_t)ix->n * cb + 15) & ~(size_t)15;      // the factors that follow stay aligned
  if (hipMalloc(reinterpret_cast<void **>(&ix->codes), std::max<size_t>(code_bytes + (size_t)ix->n * 8, 16)) != hipSuccess) return fail(LANCE_HIP_ENOMEM);
  if (hipMalloc(reinterpret_cast<void **>(&ix->row_ids), std::max<size_t>((size_t)ix->n * 8, 16)) != hipSuccess) return fail(LANCE_HIP_ENOMEM);
  float *add_out = reinterpret_cast<float *>(ix->codes + code_bytes);
  float *scale_out = add_out + ix->n;
  ix->rq_add = add_out; ix->rq_scale = scale_out;
  if (ix->n > 0) {
    hipLaunchKernelGGL(rq_gather_kernel, dim3(grid_stride_blocks((uint64_t)ix->n * cb)), dim3(256), 0, ctx->stream, codes, add, scale, row_ids, perm,
                       (int64_t)ix->n, (int)cb, ix->codes, add_out, scale_out, ix->row_ids);
  }
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
    set_error("ivfrq_create: gather kernel failed");
    return fail(LANCE_HIP_ERUNTIME);
  }
  *out = ix;
  return LANCE_HIP_OK;
}

static const CandNames RQ_NAMES = {"ivfrq", {"ivfrq_scan", "ivfrq_wide_scan"}, {"ivfrq_merge", "ivfrq_wide_merge"}, {"ivfrq_exact", "ivfrq_wide_exact"}};

// refine_factor == 0: the k best by the RQ estimate.  Otherwise (lance_hip_ivfrq_search_refine, which has checked the arguments) the
// keff = k * refine_factor best are candidates [nq][keff] in the scratch arena, re-scored against the raw vectors (cand_search, pair_cand.cuh)
static int ivfrq_search_impl(lance_hip_ctx *ctx, const lance_hip_index *idx, const float *q, uint32_t nq, uint32_t k, uint32_t nprobes,
                             const uint32_t *allow, uint64_t *ids, float *dists, uint32_t refine_factor = 0) {
  const bool refine = refine_factor != 0;
  if (!refine) LH_REQUIRE(k > 0 && k <= (uint32_t)RQ_MAX_K, "ivfrq_search: k=%u not supported (1..%d)", k, RQ_MAX_K);
  const uint32_t keff = refine ? k * refine_factor : k;
  if (nq == 0) return LANCE_HIP_OK;
  if (nprobes > idx->rq_nlist) nprobes = idx->rq_nlist;
  LH_REQUIRE(nprobes > 0, "ivfrq_search: nprobes must be > 0");
  const uint32_t d = idx->d;
  uint32_t *probes = ctx->scratch_t<uint32_t>("ivfrq.probes", (size_t)nq * nprobes);
  float *pd = ctx->scratch_t<float>("ivfrq.pdists", (size_t)nq * nprobes);
  if (!probes || !pd) return LANCE_HIP_ENOMEM;
  LH_TRY(find_partitions_f32(ctx, idx->metric, q, nq, d, idx->centroids, idx->rq_nlist, nprobes, probes, pd, false));
  RqArgs a = {};
  a.codes = idx->codes; a.add = idx->rq_add; a.scale = idx->rq_scale; a.cent = idx->centroids; a.pt = idx->rq_rot_t;
  a.d = (int)d; a.dot = idx->metric == LANCE_HIP_DOT; a.sqrt_d = std::sqrt((float)d);
  a.w.row_ids = idx->row_ids; a.w.part_offsets = idx->part_offsets; a.w.allow = allow; a.w.nprobes = (int)nprobes; a.w.k = (int)keff;
  a.w.cap = rq_scan_cap(d, (int)keff);
  LH_REQUIRE((size_t)4 * d <= (size_t)8 * a.w.cap, "ivfrq_search: the rotated query of d=%u does not fit the %d-entry candidate buffer it borrows", d, a.w.cap);
  auto chunk = [&](const CandLists &w, uint32_t q0) { a.w = w; a.pdists = pd + (size_t)q0 * nprobes; a.q = q + (size_t)q0 * d; };
  return cand_search(
      ctx, idx, RQ_NAMES, a.w, probes, nq, k, refine, q, ids, dists,
      [&](const CandLists &w, uint32_t q0, uint32_t nqc) {
        chunk(w, q0);
        hipLaunchKernelGGL(rq_scan_kernel, dim3(nqc * nprobes), dim3(256), rq_scan_lds(d, w.cap), ctx->stream, a);
      },
      [&](const CandLists &w, uint32_t q0, uint32_t nqc, uint64_t *oid, float *od) {
        chunk(w, q0);
        hipLaunchKernelGGL(rq_exact_kernel, dim3(nqc), dim3(64), rq_replay_lds(d, w.k), ctx->stream, a, oid, od);
      });
}

static int ivfrq_check(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, uint32_t nq, const uint64_t *ids, const float *dists) {
  LH_REQUIRE(ctx && idx && (nq == 0 || (q && ids && dists)), "ivfrq_search: NULL argument");
  LH_REQUIRE(idx->rq && idx->codes && idx->rq_rot_t, "ivfrq_search: not an IVF_RQ index");
  LH_REQUIRE(ctx->device == idx->device, "ivfrq_search: context and index live on different devices");
  return LANCE_HIP_OK;
}

extern "C" int lance_hip_ivfrq_search(lance_hip_ctx *ctx, const lance_hip_index *idx, const float *q, uint32_t nq, uint32_t k,
                                      uint32_t nprobes, uint64_t *ids, float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  LH_TRY(ivfrq_check(ctx, idx, q, nq, ids, dists));
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  return ivfrq_search_impl(ctx, idx, q, nq, k, nprobes, nullptr, ids, dists);
}

extern "C" int lance_hip_ivfrq_search_filtered(lance_hip_ctx *ctx, const lance_hip_index *idx, const float *q, uint32_t nq, uint32_t k,
                                               uint32_t nprobes, const uint8_t *allow_by_rowid, uint64_t n_allow, uint64_t *ids,
                                               float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  LH_TRY(ivfrq_check(ctx, idx, q, nq, ids, dists));
  LH_REQUIRE(allow_by_rowid || n_allow == 0, "ivfrq_search_filtered: NULL filter");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  const uint32_t *bits = nullptr;
  LH_TRY(build_allow_bits(ctx, idx->row_ids, idx->n, allow_by_rowid, n_allow, &bits));
  return ivfrq_search_impl(ctx, idx, q, nq, k, nprobes, bits, ids, dists);
}

// keff = k * refine_factor candidates by the RQ estimate, re-scored against the raw vectors (lance_hip_index_set_raw)
extern "C" int lance_hip_ivfrq_search_refine(lance_hip_ctx *ctx, const lance_hip_index *idx, const float *q, uint32_t nq, uint32_t k,
                                             uint32_t nprobes, uint32_t refine_factor, const uint8_t *allow_by_rowid, uint64_t n_allow,
                                             uint64_t *ids, float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  LH_TRY(ivfrq_check(ctx, idx, q, nq, ids, dists));
  LH_REQUIRE(refine_factor >= 1, "ivfrq_search_refine: refine_factor can not be zero");
  LH_REQUIRE(k >= 1 && (uint64_t)k * refine_factor <= (uint64_t)LANCE_HIP_SQRQ_MAX_CANDIDATES,
             "ivfrq_search_refine: k * refine_factor = %llu not supported (1..%d, LANCE_HIP_SQRQ_MAX_CANDIDATES)",
             (unsigned long long)k * refine_factor, LANCE_HIP_SQRQ_MAX_CANDIDATES);
  LH_REQUIRE(idx->raw != nullptr, "ivfrq_search_refine: refine_factor needs raw vectors (lance_hip_index_set_raw)");
  LH_REQUIRE(allow_by_rowid || n_allow == 0, "ivfrq_search_refine: NULL filter");
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  const uint32_t *bits = nullptr;
  if (allow_by_rowid) LH_TRY(build_allow_bits(ctx, idx->row_ids, idx->n, allow_by_rowid, n_allow, &bits));
  return ivfrq_search_impl(ctx, idx, q, nq, k, nprobes, bits, ids, dists, refine_factor);
}
