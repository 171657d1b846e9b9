// flat_ivf_mc.hip -- IVF_FLAT batched search, partition-major main pass on the bf16 matrix cores for ANY dimension (d % 4 == 0, d <= 4096)
// and for cosine indices: the shapes ivfflat_pm_kernel (flat.hip: f32, L2 / dot, d in 8 .. 128) does not instantiate and that took the
// query-major ivfflat_kernel<0, ..>, which reads a partition's rows once per (query, probe) pair.
//
//   FlatIndex::search / FlatDistanceCal::distance_all    flat/index.rs:82-177, flat/storage.rs:345-402   (the exact arithmetic kept)
//   pool, select, boundary-tie check, exact replay         flat.hip (ivfflat_select_kernel, ivfflat_exact_kernel): unchanged
//
// ivfflat_mc_filter_kernel.  A work item is HALF of one of the index's flat_items: 128 consecutive rows of one partition (the table is
// the index's own, two workgroups per entry).  The workgroup (four waves, 2 x 2) walks the partition's query tiles -- 128 of the
// (query, probe) pairs that stable_group put under this partition -- and for each tile walks d in stages of 64 elements, the loop of
// flat_mfma_wide.hip:
//   global -> registers   the NEXT stage's 32 f32 of a row and 32 bf16 of a query per thread, issued before this stage's matrix work;
//   registers -> LDS      the row values are rounded to bf16 (nearest even) HERE, and their squares are summed from the same registers:
//                         the index keeps no bf16 copy and no norm array; rows of 64 + 8 elements (144 bytes: conflict-free ds_read_b128);
//   LDS -> v_mfma_f32_32x32x16_bf16   queries down the accumulator registers, rows across the lanes, 64 accumulators per lane.
// Tails never touch memory: elements past d, rows past the partition's end and query slots past the tile's last pair are zeros written
// to LDS (the query plane this file prepares is itself padded with zeros to a multiple of the stage, so a query's stage is whole).
// The epilogue is the flat filters' fast reject: one fused multiply-add per pair against the lane's row constant and the query's
// threshold term, folded into a running minimum; only a lane whose minimum passes looks for its pairs and appends the ROW NUMBER to
// those queries' queues (FLAT_MC_QUEUE_CAP entries each).
//
// ivfflat_mc_eval_kernel.  One workgroup per query, one lane per queued row: ivfflat_dist_rt<METRIC> against the row -- what the
// query-major kernel computes --, the same test `key <= tkey[q]` (ties with the bound are kept), the same pool entry (key, row id,
// partition).  A query's pool holds the set today's route leaves there, so selection, the boundary-tie check and the replay counter see
// what they saw.  A queue that overflowed loses rows: the query is flagged (IvfFlatMcArgs::qflag, OR-ed into the replay flags after the
// select kernel) and the heap-emulating exact kernel answers it.
//
// ivfflat_mc_bound_kernel / ivfflat_mc_bound_eval_kernel.  The bound pass of such a batch: a query's bound only has to be at or above the
// exact key of its true k-th neighbour, so the largest EXACT key of any k distinct allowed rows of its nearest partition is one.  The
// tile machinery above (the queries grouped by their FIRST probe) only chooses the rows: per query 256 class minima of (surrogate order
// key, row in partition), class = row in partition % 256; the eval kernel scores the k lowest with ivfflat_dist_rt and writes the largest
// key to tkey.  A bad surrogate loosens the bound and cannot make it wrong: no margin, no guard, no permissive branch on this path.
//
// Margin (the main pass's filter): ONE bf16 product, fixed at compile time (flat_mfma.hip's two-term split was the alternative; the queues are short: DESIGN.md 4f.1).
// flat_mfma_wide.hip derives |x~.q~ - x.q| <= (2^-7 + 2^-16 + d 2^-23) |x| |q| <= 0.00832 |x| |q| for d <= 4096.  Two things differ here: |x|^2
// is summed by two threads in stage order, not in the reference's order, and |q| under cosine is this file's own sqrt of such a sum -- each
// within (d / 2 + 2) 2^-24 <= 1.3e-4 relative of the real value -- so the margins are restated with that room: EW = 0.0088 (L2, dot) and
// EWC = 0.0092 (cosine, where both norms multiply the margined term).  The tests are the wide filter's:
//   L2      |x|^2 (1 - EW) + |q|^2 (1 - EW) - 2 x~.q~ <= T
//   dot     1 - x~.q~ - EW (|x|^2 + |q|^2) - 2^-22 <= T
//   cosine  (1 - EWC - T) |q| |x| - x~.q~ <= 0
// and so are the guards: a pair whose 2^-12 (|x|^2 + |q|^2) is not above 2^-100, a row or query whose squared norm is not below 2^126 (a NaN
// included), and under cosine a norm not above 2^-50, is not filtered -- the exact evaluation decides it.
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "common.h"
#include "exact.cuh"
#include "kernels.h"
#include "search_common.cuh"

#pragma clang fp contract(off)

namespace lh {

typedef short im_bf16x8 __attribute__((ext_vector_type(8)));
typedef float im_f32x16 __attribute__((ext_vector_type(16)));

constexpr int IM_KT = 64, IM_LS = IM_KT + 8;      // elements of d per stage; LDS row stride in bf16 elements
constexpr int IM_TM = 128, IM_TN = 128;           // rows and query slots per tile
constexpr int IM_CAP = FLAT_MC_QUEUE_CAP;
constexpr int IM_CLASSES = 256;                   // bound pass: entries per query, a row's class is its number in the partition % 256
constexpr float IM_EW = 0.0088f;
constexpr float IM_EWC = 0.0092f;
constexpr float IM_E_TINY = 7.888609052210118e-31f;      // 2^-100
constexpr float IM_NORM_HUGE = 8.507059173023462e37f;    // 2^126
constexpr float IM_COS_TINY = 8.881784197001252e-16f;    // 2^-50

__device__ __forceinline__ uint32_t im_bf16_rne(float x) {
  const uint32_t u = __float_as_uint(x);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (u >> 16) | 0x40u;
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}
__device__ __forceinline__ uint32_t im_pack(float lo, float hi) { return im_bf16_rne(lo) | (im_bf16_rne(hi) << 16); }

// a chunk's queries as a bf16 plane [nq][dp] (dp = d rounded up to the stage, zero padded) and |q|^2 (cosine: |q|) beside it
__global__ __launch_bounds__(64) void ivfflat_mc_query_prep_kernel(const float *__restrict__ q, int d, int dp, int cosine, uint16_t *__restrict__ qb,
                                                                   float *__restrict__ qn) {
  const int i = blockIdx.x;
  float s = 0.0f;
  for (int e = threadIdx.x; e < dp; e += 64) {
    const float v = e < d ? q[(int64_t)i * d + e] : 0.0f;
    qb[(int64_t)i * dp + e] = (uint16_t)im_bf16_rne(v);
    s += v * v;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  if (threadIdx.x == 0) qn[i] = cosine ? sqrtf(s) : s;
}

// is this query's norm term usable by the filter?  (the permissive side of every test)
template <int METRIC>
__device__ __forceinline__ bool im_query_odd(float qn) {
  if constexpr (METRIC == METRIC_COSINE) return !(qn > IM_COS_TINY && qn < INFINITY);
  else return !(qn < IM_NORM_HUGE);
}

template <int METRIC>
__device__ __forceinline__ float im_side(float dot, float xk, float t) {
  if constexpr (METRIC == METRIC_COSINE) return __builtin_fmaf(t, xk, -dot);
  else if constexpr (METRIC == METRIC_DOT) return (xk - t) - dot;
  else return __builtin_fmaf(-2.0f, dot, xk - t);
}

// the tile walk of both passes.  BOUND = false: the main pass's filter (a.pair_* = the (query, probe) pairs by partition).  BOUND = true:
// the bound pass (a.pair_* = the queries grouped by their NEAREST partition, one pair per query); staging and products are the same
// instructions, the epilogue publishes instead of testing.
template <int METRIC, bool BOUND>
__device__ __forceinline__ void im_scan_tiles(const IvfFlatMcArgs &a) {
  constexpr int HK = IM_KT / 2;      // a staging thread moves half a stage of one row and of one query
  __shared__ __attribute__((aligned(16))) uint16_t Xs[IM_TM * IM_LS];
  __shared__ __attribute__((aligned(16))) uint16_t Qs[IM_TN * IM_LS];
  __shared__ __attribute__((aligned(16))) float tqs[IM_TN];
  __shared__ float xn2s[IM_TM];
  __shared__ int tqi[IM_TN];      // query of every slot, -1 = padding
  const int d = a.d;
  const int part = a.items[2 * (blockIdx.x >> 1)];
  const uint32_t row0 = (uint32_t)a.items[2 * (blockIdx.x >> 1) + 1] + (uint32_t)IM_TM * (blockIdx.x & 1u);
  const uint32_t r1 = a.part_offsets[part + 1];
  const uint32_t qs = a.pair_starts[part], qe = a.pair_starts[part + 1];
  if (row0 >= r1 || qs == qe) return;      // (uniform: an item's second half past the partition's end, or a partition nobody probes)
  const uint32_t pdiv = BOUND ? 1u : (uint32_t)a.nprobes;      // entries of pair_idx are query * pdiv + probe
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j = lane & 31, g = lane >> 5;
  const int wr = wave >> 1, wq = wave & 1;

  const int sr = threadIdx.x >> 1, sh = threadIdx.x & 1;
  const bool xrow_ok = row0 + (uint32_t)sr < r1;
  const float *xsrc = a.vec + (int64_t)(row0 + (uint32_t)sr) * d + sh * HK;
  const uint16_t *qsrc = nullptr;      // this thread's query of the current tile (NULL: a padding slot)
  f4 px[HK / 4];
  uint4 pq[HK / 8];
  float n2acc = 0.0f;
  bool first = true;      // |x|^2 is summed while the first tile is staged; the later tiles re-read the same rows
  auto fetch = [&](int k0) {
#pragma unroll
    for (int u = 0; u < HK / 4; ++u) {
      const bool in = k0 + sh * HK + u * 4 < d;      // d % 4 == 0: a 16-byte piece is inside or outside
      px[u] = (xrow_ok && in) ? *reinterpret_cast<const f4 *>(xsrc + k0 + u * 4) : f4{0.0f, 0.0f, 0.0f, 0.0f};
    }
#pragma unroll
    for (int u = 0; u < HK / 8; ++u) pq[u] = qsrc ? *reinterpret_cast<const uint4 *>(qsrc + k0 + u * 8) : make_uint4(0, 0, 0, 0);
  };
  auto store = [&]() {
#pragma unroll
    for (int u = 0; u < HK / 8; ++u) {
      const f4 lo = px[2 * u], hi = px[2 * u + 1];
      if (first) {
        n2acc += lo.x * lo.x; n2acc += lo.y * lo.y; n2acc += lo.z * lo.z; n2acc += lo.w * lo.w;
        n2acc += hi.x * hi.x; n2acc += hi.y * hi.y; n2acc += hi.z * hi.z; n2acc += hi.w * hi.w;
      }
      *reinterpret_cast<uint4 *>(&Xs[sr * IM_LS + sh * HK + u * 8]) =
          make_uint4(im_pack(lo.x, lo.y), im_pack(lo.z, lo.w), im_pack(hi.x, hi.y), im_pack(hi.z, hi.w));
      *reinterpret_cast<uint4 *>(&Qs[sr * IM_LS + sh * HK + u * 8]) = pq[u];
    }
  };

  for (uint32_t j0 = qs; j0 < qe; j0 += IM_TN) {
    __syncthreads();      // the previous tile's epilogue has read tqs / tqi
    // per-slot threshold term
    int q_odd = 0;      // this slot's query passes every row
    if (threadIdx.x < IM_TN) {
      float t = METRIC == METRIC_COSINE ? INFINITY : -INFINITY;      // padding slot: nothing passes
      int qi = -1;
      if (j0 + threadIdx.x < qe) qi = (int)(a.pair_idx[j0 + threadIdx.x] / pdiv);
      if (!BOUND && qi >= 0) {      // (the bound pass has no thresholds yet and reads no tqs)
        const uint32_t tk = a.pool.tkey[qi];
        const float T = tk >= 0xFF800000u ? INFINITY : key_to_float(tk);      // no bound (fewer than k rows in the nearest partition) / NaN bound: every row is a candidate
        const float qn = a.qn[qi];
        q_odd = im_query_odd<METRIC>(qn);
        if constexpr (METRIC == METRIC_COSINE) t = q_odd ? -INFINITY : (1.0f - IM_EWC - T) * qn;
        else if constexpr (METRIC == METRIC_DOT) t = T + IM_EW * qn + 4.7683716e-7f;      // (+ 2^-22: products closer than an ulp of 1 tie in the reference's 1 - x.q)
        else t = T - (qn - IM_EW * qn);
      }
      tqs[threadIdx.x] = t;
      tqi[threadIdx.x] = qi;
    }
    qsrc = j0 + (uint32_t)sr < qe ? a.qb + (int64_t)(a.pair_idx[j0 + sr] / pdiv) * a.dp + sh * HK : nullptr;

    im_f32x16 acc[2][2];
#pragma unroll
    for (int bi = 0; bi < 2; ++bi)
#pragma unroll
      for (int bj = 0; bj < 2; ++bj)
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[bi][bj][v] = 0.0f;

    fetch(0);
    store();
    const bool tile_qodd = __syncthreads_or(q_odd) != 0;
    for (int k0 = 0; k0 < d; k0 += IM_KT) {
      const bool more = k0 + IM_KT < d;
      if (more) fetch(k0 + IM_KT);
#pragma unroll
      for (int s = 0; s < IM_KT / 16; ++s) {
        im_bf16x8 aq[2], bx[2];
#pragma unroll
        for (int b = 0; b < 2; ++b) aq[b] = *reinterpret_cast<const im_bf16x8 *>(&Qs[(wq * 64 + b * 32 + j) * IM_LS + s * 16 + g * 8]);
#pragma unroll
        for (int b = 0; b < 2; ++b) bx[b] = *reinterpret_cast<const im_bf16x8 *>(&Xs[(wr * 64 + b * 32 + j) * IM_LS + s * 16 + g * 8]);
#pragma unroll
        for (int bi = 0; bi < 2; ++bi)
#pragma unroll
          for (int bj = 0; bj < 2; ++bj) acc[bi][bj] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(aq[bj], bx[bi], acc[bi][bj], 0, 0, 0);
      }
      __syncthreads();      // every wave has read this stage
      if (more) store();
      __syncthreads();
    }
    if (first) {      // the two halves of a row sit in neighbouring lanes
      const float s = n2acc + __shfl_xor(n2acc, 1, 64);
      if (sh == 0) xn2s[sr] = s;
      first = false;
      __syncthreads();
    }

    // epilogue: lane (j, g) of block (bi, bj) holds row j of the row block against the slots (v & 3) + 8 (v >> 2) + 4 g of the query block
#pragma unroll
    for (int bi = 0; bi < 2; ++bi) {
      const int tr = wr * 64 + bi * 32 + j;
      const uint32_t row = row0 + (uint32_t)tr;
      const bool rvalid = row < r1 && row_allowed(a.allow, row);
      const float n2 = xn2s[tr];
      if constexpr (BOUND) {
        // the accumulator only ORDERS the rows of a query (its own constant dropped): L2 |x|^2 - 2 x~.q~, dot -x~.q~, cosine -x~.q~ / |x|.
        // Every allowed row offers (order key of that value, row in partition) to class `row in partition % 256` of its query; a class
        // keeps its minimum, different classes are different rows.  A NaN value offers nothing.  No margin: the eval kernel scores the rows.
        if (rvalid) {
          const uint32_t rp = row - a.part_offsets[part];
          const float xs = METRIC == METRIC_COSINE ? sqrtf(n2) : n2;
#pragma unroll
          for (int bj = 0; bj < 2; ++bj) {
#pragma unroll
            for (int v = 0; v < 16; ++v) {
              const int qi = tqi[wq * 64 + bj * 32 + 8 * (v >> 2) + 4 * g + (v & 3)];
              if (qi < 0) continue;
              const float dot = acc[bi][bj][v];
              const float val = METRIC == METRIC_COSINE ? -dot / xs : METRIC == METRIC_DOT ? -dot : __builtin_fmaf(-2.0f, dot, xs);
              // (no load ahead of the atomic: a class sees partition size / 256 offers, most pass; with one the pass took 3 to 10 % longer)
              if (val == val) atomicMin(&a.bcls[(int64_t)qi * IM_CLASSES + (rp % IM_CLASSES)], ((unsigned long long)order_key(val) << 32) | rp);
            }
          }
        }
        continue;
      }
      float xk;
      bool odd, tiny = false;      // odd: every query takes the row; tiny: the queries that are tiny too take it
      if constexpr (METRIC == METRIC_COSINE) {
        xk = sqrtf(n2);
        odd = !(xk > IM_COS_TINY && xk < INFINITY);
      } else {
        xk = METRIC == METRIC_DOT ? 1.0f - IM_EW * n2 : n2 - IM_EW * n2;
        odd = !(n2 < IM_NORM_HUGE);
        tiny = !(0.000244140625f * n2 > IM_E_TINY);
      }
      float mn = INFINITY;
#pragma unroll
      for (int bj = 0; bj < 2; ++bj) {
        const float *tqb = tqs + wq * 64 + bj * 32 + 4 * g;
#pragma unroll
        for (int vq = 0; vq < 4; ++vq) {
          const f4 t4 = *reinterpret_cast<const f4 *>(tqb + 8 * vq);
#pragma unroll
          for (int e = 0; e < 4; ++e) mn = __builtin_fminf(mn, im_side<METRIC>(acc[bi][bj][4 * vq + e], xk, t4[e]));      // (a NaN is ignored by the minimum and fails `<=` alike)
        }
      }
      if ((mn <= 0.0f || odd || tiny || tile_qodd) && rvalid) {      // rare per lane: find the pairs, queue the row for each of their queries
#pragma unroll
        for (int bj = 0; bj < 2; ++bj) {
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const int slot = wq * 64 + bj * 32 + 8 * (v >> 2) + 4 * g + (v & 3);
            const int qi = tqi[slot];
            if (qi < 0) continue;
            bool pass = odd || im_side<METRIC>(acc[bi][bj][v], xk, tqs[slot]) <= 0.0f;
            if (!pass && (tile_qodd || tiny)) {
              const float qn = a.qn[qi];
              pass = im_query_odd<METRIC>(qn) || (METRIC != METRIC_COSINE && tiny && !(0.000244140625f * qn > IM_E_TINY));
            }
            if (pass) {
              const uint32_t pos = atomicAdd(&a.scnt[qi], 1u);
              if (pos < (uint32_t)IM_CAP) a.squeue[(int64_t)qi * IM_CAP + pos] = row;
            }
          }
        }
      }
    }
  }
}

template <int METRIC>
__global__ __launch_bounds__(256, 2) void ivfflat_mc_filter_kernel(IvfFlatMcArgs a) { im_scan_tiles<METRIC, false>(a); }

template <int METRIC>
__global__ __launch_bounds__(256, 2) void ivfflat_mc_bound_kernel(IvfFlatMcArgs a) { im_scan_tiles<METRIC, true>(a); }

// the bound of one query from its classes: one workgroup per query, one thread per class.  The k entries of lowest surrogate value are k
// DISTINCT allowed rows of the query's nearest partition; the largest of their EXACT keys (ivfflat_dist_rt, the reference's arithmetic)
// is at or above the exact key of the query's true k-th neighbour, whichever k rows the surrogate chose.  Fewer than k classes filled
// (fewer than k allowed rows, or rows that met in one class): no bound, 0xFFFFFFFF, which the main pass reads as "every row".
template <int METRIC>
__global__ __launch_bounds__(256) void ivfflat_mc_bound_eval_kernel(IvfFlatMcArgs a) {
  extern __shared__ __attribute__((aligned(16))) float qt[];   // [d]
  __shared__ unsigned long long ent[IM_CLASSES];
  __shared__ uint32_t kmax;
  static_assert(IM_CLASSES == 256, "one thread per class");
  const FlatPool &p = a.pool;
  const int qi = blockIdx.x, d = a.d;
  const unsigned long long e = a.bcls[(int64_t)qi * IM_CLASSES + threadIdx.x];
  const bool valid = e != ~0ull;
  ent[threadIdx.x] = e;
  if (threadIdx.x == 0) kmax = 0u;
  for (int i = threadIdx.x; i < d; i += 256) qt[i] = a.q[(int64_t)qi * d + i];
  const int nvalid = __syncthreads_count(valid);
  if (nvalid < p.k) {      // (uniform)
    if (threadIdx.x == 0) { p.tkey[qi] = 0xFFFFFFFFu; p.trid[qi] = ~0ull; }
    return;
  }
  float qnorm = 0.0f;
  if constexpr (METRIC == METRIC_COSINE) qnorm = norm_l2_rt(qt, d);
  int rank = 0;      // entries are distinct (their low words are different rows); an empty class is above every entry
  for (int c = 0; c < IM_CLASSES; ++c) rank += ent[c] < e ? 1 : 0;
  if (valid && rank < p.k) {
    const uint32_t row = a.part_offsets[a.probes[(int64_t)qi * a.nprobes]] + (uint32_t)e;
    atomicMax(&kmax, order_key(ivfflat_dist_rt<METRIC, false>(qt, qnorm, a.vec + (int64_t)row * d, d)));
  }
  __syncthreads();
  if (threadIdx.x == 0) { p.tkey[qi] = kmax; p.trid[qi] = ~0ull; }
}

// exact evaluation of the queued rows: one workgroup per query, one lane per queued row; the query sits in LDS as in ivfflat_kernel<0, ..>
template <int METRIC>
__global__ __launch_bounds__(256) void ivfflat_mc_eval_kernel(IvfFlatMcArgs a) {
  extern __shared__ __attribute__((aligned(16))) float qt[];   // [d]
  const FlatPool &p = a.pool;
  const int qi = blockIdx.x, d = a.d;
  const uint32_t raw = a.scnt[qi];
  if (threadIdx.x == 0) a.qflag[qi] = raw > (uint32_t)IM_CAP ? 1u : 0u;      // rows were lost: the exact kernel answers this query
  if (raw == 0 || raw > (uint32_t)IM_CAP) return;
  for (int i = threadIdx.x; i < d; i += 256) qt[i] = a.q[(int64_t)qi * d + i];
  __syncthreads();
  float qnorm = 0.0f;
  if constexpr (METRIC == METRIC_COSINE) qnorm = norm_l2_rt(qt, d);
  const uint32_t tk = p.tkey[qi];
  for (uint32_t i = threadIdx.x; i < raw; i += 256) {
    const uint32_t row = a.squeue[(int64_t)qi * IM_CAP + i];
    const uint32_t key = order_key(ivfflat_dist_rt<METRIC, false>(qt, qnorm, a.vec + (int64_t)row * d, d));
    if (key <= tk) {       // ties with the bound are kept (the boundary-tie check needs them)
      const uint32_t pos = atomicAdd(&p.cnt[qi], 1u);
      if (pos < (uint32_t)p.cap) {
        p.pkeys[(int64_t)qi * p.cap + pos] = key;
        p.prids[(int64_t)qi * p.cap + pos] = a.row_ids[row];
        a.ppart[(int64_t)qi * p.cap + pos] = find_partition_dev(a.part_offsets, a.nlist, row);
      }
    }
  }
}

__global__ __launch_bounds__(256) void ivfflat_mc_flags_kernel(const uint32_t *__restrict__ qflag, int nq, uint32_t *__restrict__ flags) {
  const int q = blockIdx.x * 256 + threadIdx.x;
  if (q < nq && qflag[q]) flags[q] = 1u;
}

int ivfflat_mc_scratch(lance_hip_ctx *ctx, int qch, int d, IvfFlatMcArgs *a) {
  a->dp = (int)cdiv((uint64_t)d, IM_KT) * IM_KT;
  a->qb = ctx->scratch_t<uint16_t>("ivfflat.mc.qb", (size_t)qch * a->dp);
  a->qn = ctx->scratch_t<float>("ivfflat.mc.qn", (size_t)qch);
  a->scnt = ctx->scratch_t<uint32_t>("ivfflat.mc.scnt", (size_t)qch);
  a->qflag = ctx->scratch_t<uint32_t>("ivfflat.mc.qflag", (size_t)qch);
  a->squeue = ctx->scratch_t<uint32_t>("ivfflat.mc.squeue", (size_t)qch * IM_CAP);
  a->bcls = ctx->scratch_t<unsigned long long>("ivfflat.mc.bcls", (size_t)qch * IM_CLASSES);
  return a->qb && a->qn && a->scnt && a->qflag && a->squeue && a->bcls ? LANCE_HIP_OK : LANCE_HIP_ENOMEM;
}

// once per query chunk: the bf16 plane and the norms of a.q's nqc queries
void ivfflat_mc_prepare_queries(lance_hip_ctx *ctx, const IvfFlatMcArgs &a, int nqc, bool cosine) {
  hipLaunchKernelGGL(ivfflat_mc_query_prep_kernel, dim3(nqc), dim3(64), 0, ctx->stream, a.q, a.d, a.dp, cosine ? 1 : 0, a.qb, a.qn);
}

// the bound pass of one chunk.  a.pair_starts / a.pair_idx: the chunk's queries grouped by their nearest partition; a.probes, a.q, a.qb set.
int launch_ivfflat_mc_bound(lance_hip_ctx *ctx, const IvfFlatMcArgs &a, int metric, unsigned n_items, int nqc) {
  ScopedTimer t(ctx, "ivfflat_mc_bound");
  LH_CHECK_HIP(lh::memset_async(a.bcls, 0xFF, (size_t)nqc * IM_CLASSES * 8, ctx->stream));
  const dim3 grid(2 * n_items);
  const size_t lds = (size_t)((a.d + 3) & ~3) * 4;
  if (metric == LANCE_HIP_COSINE) {
    hipLaunchKernelGGL(ivfflat_mc_bound_kernel<METRIC_COSINE>, grid, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(ivfflat_mc_bound_eval_kernel<METRIC_COSINE>, dim3(nqc), dim3(256), lds, ctx->stream, a);
  } else if (metric == LANCE_HIP_DOT) {
    hipLaunchKernelGGL(ivfflat_mc_bound_kernel<METRIC_DOT>, grid, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(ivfflat_mc_bound_eval_kernel<METRIC_DOT>, dim3(nqc), dim3(256), lds, ctx->stream, a);
  } else {
    hipLaunchKernelGGL(ivfflat_mc_bound_kernel<METRIC_L2>, grid, dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(ivfflat_mc_bound_eval_kernel<METRIC_L2>, dim3(nqc), dim3(256), lds, ctx->stream, a);
  }
  LH_CHECK_HIP(hipGetLastError());
  return LANCE_HIP_OK;
}

// the main pass of one chunk: filter, then evaluate the queues into the pools.  Every threshold (a.pool.tkey) is set, the pairs are grouped.
int launch_ivfflat_mc(lance_hip_ctx *ctx, const IvfFlatMcArgs &a, int metric, unsigned n_items, int nqc) {
  LH_CHECK_HIP(lh::memset_async(a.scnt, 0, (size_t)nqc * 4, ctx->stream));
  const dim3 grid(2 * n_items);
  {
    ScopedTimer t(ctx, "ivfflat_mc");
    if (metric == LANCE_HIP_COSINE) hipLaunchKernelGGL(ivfflat_mc_filter_kernel<METRIC_COSINE>, grid, dim3(256), 0, ctx->stream, a);
    else if (metric == LANCE_HIP_DOT) hipLaunchKernelGGL(ivfflat_mc_filter_kernel<METRIC_DOT>, grid, dim3(256), 0, ctx->stream, a);
    else hipLaunchKernelGGL(ivfflat_mc_filter_kernel<METRIC_L2>, grid, dim3(256), 0, ctx->stream, a);
  }
  {
    ScopedTimer t(ctx, "ivfflat_mc_eval");
    const size_t lds = (size_t)((a.d + 3) & ~3) * 4;
    if (metric == LANCE_HIP_COSINE) hipLaunchKernelGGL(ivfflat_mc_eval_kernel<METRIC_COSINE>, dim3(nqc), dim3(256), lds, ctx->stream, a);
    else if (metric == LANCE_HIP_DOT) hipLaunchKernelGGL(ivfflat_mc_eval_kernel<METRIC_DOT>, dim3(nqc), dim3(256), lds, ctx->stream, a);
    else hipLaunchKernelGGL(ivfflat_mc_eval_kernel<METRIC_L2>, dim3(nqc), dim3(256), lds, ctx->stream, a);
  }
  LH_CHECK_HIP(hipGetLastError());
  if (ctx->timing && !ctx->capturing) {      // measurement runs: rows queued by this pass, read back through "count:ivfflat_mc_queued"
    std::vector<uint32_t> h((size_t)nqc);
    LH_CHECK_HIP(hipMemcpyAsync(h.data(), a.scnt, (size_t)nqc * 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    uint64_t sum = 0;
    for (uint32_t v : h) sum += v;
    ctx->stage_counts["ivfflat_mc_queued"] += sum;
  }
  return LANCE_HIP_OK;
}

// after the select kernel rewrote the replay flags: the queries whose queue overflowed join them
void launch_ivfflat_mc_flags(lance_hip_ctx *ctx, const IvfFlatMcArgs &a, int nqc, uint32_t *flags) {
  hipLaunchKernelGGL(ivfflat_mc_flags_kernel, dim3((unsigned)cdiv((uint64_t)nqc, 256)), dim3(256), 0, ctx->stream, a.qflag, nqc, flags);
}

}  // namespace lh
