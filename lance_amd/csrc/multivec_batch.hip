// multivec_batch.hip -- a BATCH of multivector queries against a multivector column (lance_hip_flat_multivec_topk_batch): for cosine a
// MaxSim surrogate on the matrix cores filters the rows, the few that can reach a query's top k go through multivec.hip's exact
// arithmetic (mv_pair_rt, the key max, mv_finish), and the answers are bit for bit those of lance_hip_flat_multivec_topk per query.
// Everything else (L2, dot, a distance range, d > MVB_MAX_D, a degenerate query, a query whose survivor list overflows) is answered
// by mv_topk_impl, query by query, inside the call.
//
// Layout.
//   * Planes, ONCE PER CALL (mvb_prep_kernel, a wave per row): every vector x of the column is normalised in f32, x^ = x / sqrt(sum x^2),
//     and split into two bf16 planes hi = rne(x^), lo = rne(x^ - hi), rows of K = the power of two >= max(d, 16) elements, zero-padded:
//     4 K bytes per vector of the column (as much as an f32 column of that K), plus one byte per row for `degenerate`.  A vector whose
//     elements are not all finite, whose norm is not above 2^-50 or whose squared norm is not below 2^126 (FW_COS_TINY / FW_NORM_HUGE,
//     flat_mfma_wide.hip) is stored as zeros and makes its ROW degenerate.  The same kernel builds the query planes of a chunk
//     ([columns][K], a column per query vector, the queries packed one after the other) and the per-QUERY degenerate byte.
//   * Surrogate (mvb_filter_kernel).  The rows are cut by VECTOR COUNT into units of whole rows (a binary search in `offsets` per
//     wave); a wave owns a unit and walks it in tiles of 32 vectors.  The tile is the A operand of v_mfma_f32_32x32x16_bf16, held in
//     registers (hi and lo, K / 16 steps); a block of 32 query columns is the B operand, read from LDS, where the workgroup staged the
//     column blocks of its group once.  Three products per step (hi hi, hi lo, lo hi) leave in lane (column j, half g), register v the
//     surrogate similarity of tile vector (v & 3) + 8 (v >> 2) + 4 g and column j.  The rows that touch the tile are walked in order
//     (wave-uniform): a lane takes the maximum over the registers whose vector lies in the row, the two halves are folded with one
//     shuffle; a row that goes on into the next tile leaves its running maxima in a wave-private LDS line (one open row at a time), a
//     row that ends gives its 32 column maxima to LDS, and one lane per PIECE -- the part of one query's columns inside this column
//     block -- adds them in column order and writes P[piece][row].  A padding vector (past the unit, past the column) belongs to no
//     row and a padding column to no piece, so neither enters a maximum or a sum.  Nothing of size [vectors][columns] exists.
//   * D~(query, row) = 1 - ((0 + P[first piece]) + ...) in piece order (mvb_dtilde).
//   * Threshold (mvb_kth_kernel, a batched keys-only form of mv_select_kernel's rounds): t = the k-th smallest D~ over the
//     non-degenerate rows, +inf when there are fewer.  Survivors (mvb_survivor_kernel): D~ <= t + 2 E or a degenerate row, appended with a
//     device atomic to the query's list of MV_SEL entries; the final sort makes their order irrelevant.
//   * Exact (mvb_eval_kernel): a wave per surviving (query, row) pair in the lane layout of mv_scan_generic_kernel<.., false>;
//     mvb_final_kernel, a block per query, sorts (key, row id) and writes the answer.
// The queries are taken in chunks of at most MVB_CHUNK_Q queries and MVB_CHUNK_COLS columns, so a chunk has at most
// MVB_MAX_PIECES = MVB_CHUNK_Q + MVB_CHUNK_COLS / 32 pieces and the scratch besides the planes is bounded whatever B is:
// P 4 MVB_MAX_PIECES n_rows = 512 n_rows bytes, the threshold rounds <= 3 MVB_CHUNK_Q k (n_rows / MV_SEL + 1) * 4 <= 384 n_rows + 1 MiB,
// the lists and exact distances MVB_CHUNK_Q MV_SEL 8 = 1 MiB, the query planes 4 K MVB_CHUNK_COLS <= 2 MiB.
//
// Margin.  E(nqv, K) with |D~ - D| <= E, D the f32 value the exact kernels compute, for a non-degenerate row and query.  u = 2^-24.
//   (a) normalisation.  s = fl(sum x^2) in any order is |x|^2 (1 + th), |th| <= d u (1 + 2^-10); the square root halves that and adds u,
//       the division adds u: x^_f = (x / |x|)(1 + e), |e| <= (d / 2 + 3) u.  On both sides: |x^_f . q^_f - c| <= (d + 7) u, c the cosine
//       in real numbers, and |x^_f|, |q^_f| <= 1 + 2^-15.
//   (b) operands.  bf16 keeps 8 significant bits: |x^_f - hi| <= 2^-8 |x^_f|, |x^_f - hi - lo| <= 2^-16 |x^_f| per element (hi, lo and
//       the difference are exact f32 values; an f16 element, were it not normalised, would split exactly).  The product keeps
//       hi hi + hi lo + lo hi and drops lo lo (<= 2^-16) and the two residuals (<= 2^-16 (1 + 2^-8) each): by Cauchy-Schwarz
//       <= 3.001 * 2^-16 |x^_f| |q^_f| <= 3.002 * 2^-16 per pair -- under the 2^-14 of flat_mfma.hip's bf16x3.
//   (c) accumulation.  The 3 K products (each exact in f32; the padding adds zeros) are summed by the matrix pipe, whatever it rounds
//       inside: <= 2 * 3 K u * (sum of |terms| <= 1.02) <= 6.2 K u  (twice the textbook bound, as in flat_mfma_wide.hip).
//   (d) the exact side.  The dot product in f32, any order, fused or not: <= d u (1 + 2^-10) |x| |q|; x_norm and sqrt(y_norm) (both
//       arms: cosine_exact_rt, whose y_norm squares a square root again, and cosine_scalar32_rt) (d / 2 + 4) u each; two divisions, or
//       a product and a division: 2 u; 1 - quot <= 2 u, one_minus u: |sim_exact - c| <= (2 d + 13) u.
//   (e) underflow.  The norms are above 2^-50, so squares and products that fall into the denormal range change s and the dot product
//       by less than d 2^-149 / 2^-100 relative; a normalised element under 2^-126 is flushed: together far below 2^-30.
//   EP(K) = 3.002 * 2^-16 + (9.2 K + 20) u + 2^-30   >= (a) + (b) + (c) + (d) + (e) since d <= K   (K = 128: 1.17e-4 < 2^-13)
//   A maximum moves by no more than its terms do: |max~_i - max_i| <= EP.  The maxima are below 1.001 in magnitude on both sides; a
//   sequential f32 sum of nqv of them errs by <= u sum_k k 1.001, the last 1 - s by <= u (nqv + 1) 1.001: per side <= nqv (nqv + 3) u
//   (the surrogate's sum is taken piece by piece, which is no worse).  The test D~ <= fl(t + fl(2 E)) rounds by <= (nqv + 3) 2^-23.
//   E(nqv, K) = nqv EP(K) + (nqv + 1)(nqv + 3) 2^-23
// Threshold.  If a non-degenerate row has D~ > t + 2 E, k non-degenerate rows have D~ <= t, so D <= t + E < D~ - E <= D of the row: k
// rows beat it strictly and it is in no top k.  A degenerate row takes no part in t and survives unconditionally; a degenerate query
// has no margin and goes to the loop.  tests/multivec_batch_spec.py restates E and the surrogate, tests/test_multivec_batch_spec.py
// holds both to the bound (an adversarial fixture included) and catches the mutants of each term.
#include <algorithm>
#include <cmath>
#include <vector>

#include "common.h"
#include "exact.cuh"
#include "kernels.h"
#include "multivec.cuh"

#pragma clang fp contract(off)

namespace lh {

typedef short mvb_bf16x8 __attribute__((ext_vector_type(8)));
typedef float mvb_f32x16 __attribute__((ext_vector_type(16)));

constexpr int MVB_MAX_D = 256;                  // the largest d the margin is derived (and the A operand's registers are sized) for
constexpr int MVB_CHUNK_Q = 64;                 // queries per chunk
constexpr int MVB_CHUNK_COLS = 2048;            // query vectors (columns) per chunk
constexpr int MVB_MAX_PIECES = MVB_CHUNK_Q + MVB_CHUNK_COLS / 32;
constexpr int MVB_WAVES = 4;                    // units in flight per workgroup
constexpr int MVB_MAX_GROUP = 4;                // column blocks a workgroup stages at most
static_assert(MVB_MAX_D == 256, "mvb_prep_kernel holds a vector as 2 x 2 elements per lane");
constexpr float MVB_TINY = 8.881784197001252e-16f;      // 2^-50   (FW_COS_TINY)
constexpr float MVB_HUGE = 8.507059173023462e37f;       // 2^126   (FW_NORM_HUGE)

__device__ __forceinline__ uint32_t mvb_bf16_rne(float x) {      // x finite
  const uint32_t u = __float_as_uint(x);
  return (u + 0x7FFFu + ((u >> 16) & 1u)) >> 16;
}

// Vectors -> normalised bf16 hi / lo planes, a wave per bag (a row of the column, or a query of the chunk).  offsets are absolute
// vector positions into vals; plane row = position - o_first.  A bag with o1 <= o0, or one that leaves [o_first, o_last] (which the
// offsets can only do by decreasing somewhere), raises the flag word of multivec.hip's scans and is not read.
template <typename TV>
__global__ __launch_bounds__(256) void mvb_prep_kernel(const TV *__restrict__ vals, const uint64_t *__restrict__ offsets, uint64_t n_bags,
                                                       uint64_t o_first, uint64_t o_last, int d, int kpad, uint16_t *__restrict__ hi,
                                                       uint16_t *__restrict__ lo, uint8_t *__restrict__ degen, uint32_t *flag) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (uint64_t r = (uint64_t)blockIdx.x * 4 + wave; r < n_bags; r += (uint64_t)gridDim.x * 4) {
    const uint64_t o0 = offsets[r], o1 = offsets[r + 1];
    if (o1 <= o0 || o0 < o_first || o1 > o_last) {
      if (lane == 0) { atomicOr(flag, (o1 <= o0 && o1 == o0) ? 1u : 2u); degen[r] = 1; }
      continue;
    }
    bool bad = false;
    for (uint64_t v = o0; v < o1; ++v) {
      // kpad <= MVB_MAX_D = 256: lane l holds the elements 128 i + 2 l, + 1 (i = 0, 1) -- one read of the vector, one 4-byte store per plane
      const TV *src = vals + v * (uint64_t)d;
      float x[2][2];
      float s = 0.0f;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const int e = 128 * i + 2 * lane + h;
          x[i][h] = e < d ? ld_elem(src, e) : 0.0f;
          s += x[i][h] * x[i][h];
        }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      const float n = sqrtf(s);
      const bool ok = n > MVB_TINY && s < MVB_HUGE;      // a NaN or an inf element fails one of the two
      bad = bad || !ok;
      uint32_t *hrow = reinterpret_cast<uint32_t *>(hi + (v - o_first) * (uint64_t)kpad);
      uint32_t *lrow = reinterpret_cast<uint32_t *>(lo + (v - o_first) * (uint64_t)kpad);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int e2 = 64 * i + lane;
        if (e2 < kpad / 2) {
          uint32_t hw = 0, lw = 0;
          if (ok) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
              const float xn = x[i][h] / n;      // (an element past d is 0)
              const uint32_t hb = mvb_bf16_rne(xn);
              const uint32_t lb = mvb_bf16_rne(xn - __uint_as_float(hb << 16));
              hw |= hb << (16 * h); lw |= lb << (16 * h);
            }
          }
          hrow[e2] = hw; lrow[e2] = lw;
        }
      }
    }
    if (lane == 0) degen[r] = bad ? 1 : 0;
  }
}

// multivec.hip's mv_qnorm_kernel over all the query vectors of the batch: the x_norm the exact arithmetic divides by
template <bool H32>
__global__ __launch_bounds__(64) void mvb_qnorm_kernel(const float *__restrict__ q, int n, int d, float *__restrict__ out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < n) out[i] = H32 ? norm_l2_rt<float, 32>(q + (int64_t)i * d, d) : norm_l2_rt<float>(q + (int64_t)i * d, d);
}

struct MvbArgs {
  const uint16_t *xhi, *xlo;     // [nvec][kpad]
  const uint64_t *offsets;       // [n_rows + 1], checked by mvb_prep_kernel: strictly increasing
  uint64_t n_rows, o_first, nvec;
  const uint16_t *qhi, *qlo;     // [32 ncb][kpad], the chunk's columns, zero rows behind the last
  int kpad;
  int ncb;                       // column blocks of the chunk
  int cbg;                       // column blocks per workgroup (gridDim.y groups)
  const uint32_t *pb;            // [ncb + 1]: the pieces of column block c are pb[c] .. pb[c + 1] - 1 (at most 32)
  const uint32_t *pinfo;         // [pieces]: first column inside the block | columns << 8
  float *P;                      // [pieces][n_rows]
  uint32_t units;                // waves' units of rows
  uint64_t vpu;                  // vectors per unit (a multiple of 32)
};

// first row whose offset is >= target (offsets increase strictly); n_rows when there is none
__device__ __forceinline__ uint64_t mvb_lower_row(const uint64_t *__restrict__ offsets, uint64_t n_rows, uint64_t target) {
  uint64_t lo = 0, hi = n_rows;
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (offsets[mid] < target) lo = mid + 1; else hi = mid;
  }
  return lo;
}

template <int KS>      // kpad = 16 KS
__global__ __launch_bounds__(64 * MVB_WAVES) void mvb_filter_kernel(MvbArgs a) {
  extern __shared__ __attribute__((aligned(16))) char mvb_smem[];
  constexpr int KP = 16 * KS, LS = KP + 8;      // LDS row stride in bf16 elements: 16 bytes of padding, conflict-free ds_read_b128
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, j = lane & 31, g = lane >> 5;
  const int cb0 = blockIdx.y * a.cbg, ncbl = min(a.cbg, a.ncb - cb0);
  uint16_t *Qh = reinterpret_cast<uint16_t *>(mvb_smem);                       // [cbg * 32][LS]
  uint16_t *Ql = Qh + (size_t)a.cbg * 32 * LS;
  float *carry = reinterpret_cast<float *>(Ql + (size_t)a.cbg * 32 * LS) + wave * (MVB_MAX_GROUP * 32);      // the open row's maxima, per column
  float *cm = reinterpret_cast<float *>(Ql + (size_t)a.cbg * 32 * LS) + MVB_WAVES * MVB_MAX_GROUP * 32 + wave * 32;
  uint32_t *pbs = reinterpret_cast<uint32_t *>(reinterpret_cast<float *>(Ql + (size_t)a.cbg * 32 * LS) + MVB_WAVES * (MVB_MAX_GROUP + 1) * 32);      // [MVB_MAX_GROUP + 1]
  uint32_t *pis = pbs + 8;                                                                                                                      // [MVB_MAX_GROUP * 32]
  // stage the group's query columns (16-byte pieces) and its pieces
  for (int i = threadIdx.x; i < ncbl * 32 * (KP / 8); i += 64 * MVB_WAVES) {
    const int c = i / (KP / 8), u = i - c * (KP / 8);
    const size_t src = ((size_t)cb0 * 32 + c) * KP + u * 8;
    *reinterpret_cast<uint4 *>(&Qh[c * LS + u * 8]) = *reinterpret_cast<const uint4 *>(a.qhi + src);
    *reinterpret_cast<uint4 *>(&Ql[c * LS + u * 8]) = *reinterpret_cast<const uint4 *>(a.qlo + src);
  }
  if (threadIdx.x <= (unsigned)ncbl) pbs[threadIdx.x] = a.pb[cb0 + threadIdx.x];
  __syncthreads();
  for (int c = 0; c < ncbl; ++c) {
    const uint32_t p0 = pbs[c], np = pbs[c + 1] - p0;
    if (threadIdx.x < np && threadIdx.x < 32) pis[c * 32 + threadIdx.x] = a.pinfo[p0 + threadIdx.x];
  }
  __syncthreads();

  const uint64_t o_end = a.o_first + a.nvec;
  for (uint32_t unit = blockIdx.x * MVB_WAVES + wave; unit < a.units; unit += gridDim.x * MVB_WAVES) {
    const uint64_t t_lo = a.o_first + (uint64_t)unit * a.vpu, t_hi = t_lo + a.vpu;
    const uint64_t ra = unit == 0 ? 0 : mvb_lower_row(a.offsets, a.n_rows, t_lo);
    const uint64_t rb = (unit + 1 == a.units || t_hi >= o_end) ? a.n_rows : mvb_lower_row(a.offsets, a.n_rows, t_hi);
    if (ra >= rb) continue;
    const uint64_t vs = a.offsets[ra], ve = a.offsets[rb];
    uint64_t r = ra;                                         // the first row that touches the current tile
    for (uint64_t t0 = vs; t0 < ve; t0 += 32) {
      // the tile's operand: lane (j, g) holds elements 16 s + 8 g .. + 7 of vector t0 + j
      mvb_bf16x8 ah[KS], al[KS];
      {
        const uint64_t v = t0 + j - a.o_first;
        const bool in = t0 + j < o_end;
        const uint16_t *ph = a.xhi + v * (uint64_t)KP + g * 8, *pl = a.xlo + v * (uint64_t)KP + g * 8;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          uint4 h4 = make_uint4(0, 0, 0, 0), l4 = make_uint4(0, 0, 0, 0);
          if (in) { h4 = *reinterpret_cast<const uint4 *>(ph + s * 16); l4 = *reinterpret_cast<const uint4 *>(pl + s * 16); }
          ah[s] = *reinterpret_cast<mvb_bf16x8 *>(&h4); al[s] = *reinterpret_cast<mvb_bf16x8 *>(&l4);
        }
      }
      uint64_t rr = r;
      for (int c = 0; c < ncbl; ++c) {
        mvb_f32x16 acc;
#pragma unroll
        for (int v = 0; v < 16; ++v) acc[v] = 0.0f;
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const mvb_bf16x8 bh = *reinterpret_cast<const mvb_bf16x8 *>(&Qh[(c * 32 + j) * LS + s * 16 + g * 8]);
          const mvb_bf16x8 bl = *reinterpret_cast<const mvb_bf16x8 *>(&Ql[(c * 32 + j) * LS + s * 16 + g * 8]);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[s], bh, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s], bl, acc, 0, 0, 0);
          acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[s], bh, acc, 0, 0, 0);
        }
        const uint32_t p0 = pbs[c], np = pbs[c + 1] - p0;
        rr = r;
        while (rr < rb) {
          const uint64_t o0 = a.offsets[rr];
          if (o0 >= t0 + 32) break;
          const uint64_t o1 = a.offsets[rr + 1];
          const int la = o0 > t0 ? (int)(o0 - t0) : 0, lb = o1 < t0 + 32 ? (int)(o1 - t0) : 32;
          float m = -INFINITY;
#pragma unroll
          for (int v = 0; v < 16; ++v) {
            const int idx = (v & 3) + 8 * (v >> 2) + 4 * g;
            m = (idx >= la && idx < lb) ? fmaxf(m, acc[v]) : m;
          }
          m = fmaxf(m, __shfl_xor(m, 32, 64));
          if (o0 < t0) m = fmaxf(m, carry[c * 32 + j]);
          if (o1 > t0 + 32) {                                // the row goes on: it is the tile's last
            if (g == 0) carry[c * 32 + j] = m;
            break;
          }
          if (g == 0) cm[j] = m;
          wave_sync();
          if ((uint32_t)lane < np) {
            const uint32_t info = pis[c * 32 + lane];
            const int f = (int)(info & 255u), cnt = (int)(info >> 8);
            float s = 0.0f;
            for (int i = 0; i < cnt; ++i) s = s + cm[f + i];
            a.P[(uint64_t)(p0 + lane) * a.n_rows + rr] = s;
          }
          wave_sync();
          ++rr;
        }
      }
      r = rr;
      wave_sync();      // the carry lines written for this tile are read by the next
    }
  }
}

// the surrogate distance of (query, row): the pieces of the query in order
__device__ __forceinline__ float mvb_dtilde(const float *__restrict__ P, uint64_t n_rows, uint32_t p0, uint32_t p1, uint64_t r) {
  float s = 0.0f;
  for (uint32_t p = p0; p < p1; ++p) s = s + P[(uint64_t)p * n_rows + r];
  return 1.0f - s;
}

template <typename F>
__device__ __forceinline__ void mvb_bitonic(int n, F swap_if) {      // n a power of two; swap_if(ix, px, up) under __syncthreads
  for (int k2 = 2; k2 <= n; k2 <<= 1) {
    for (int jj = k2 >> 1; jj > 0; jj >>= 1) {
      for (int i = threadIdx.x; i < n / 2; i += 256) {
        const int ix = 2 * jj * (i / jj) + (i % jj);
        swap_if(ix, ix + jj, (ix & k2) == 0);
      }
      __syncthreads();
    }
  }
}

// One block sorts MV_SEL surrogate keys of one query (blockIdx.y) and keeps the k smallest; rounds as in mv_topk_impl.  First round
// (in_keys NULL): the keys are the rows' D~, a degenerate row loads as the empty sentinel.  Last round (tkey set): the k-th smallest.
__global__ __launch_bounds__(256) void mvb_kth_kernel(const float *__restrict__ P, const uint32_t *__restrict__ pq, const uint8_t *__restrict__ degen,
                                                      uint64_t n_rows, const uint32_t *__restrict__ in_keys, uint64_t n_in, uint64_t in_stride, int k,
                                                      uint32_t *__restrict__ out_keys, uint64_t out_stride, uint32_t *__restrict__ tkey) {
  __shared__ uint32_t key[MV_SEL];
  const uint32_t b = blockIdx.y;
  const uint64_t base = (uint64_t)blockIdx.x * MV_SEL;
  for (int i = threadIdx.x; i < MV_SEL; i += 256) {
    const uint64_t gi = base + i;
    uint32_t kk = 0xFFFFFFFFu;
    if (gi < n_in) {
      if (in_keys) kk = in_keys[(uint64_t)b * in_stride + gi];
      else if (!degen[gi]) kk = order_key(mvb_dtilde(P, n_rows, pq[b], pq[b + 1], gi));
    }
    key[i] = kk;
  }
  __syncthreads();
  mvb_bitonic(MV_SEL, [&](int ix, int px, bool up) {
    const uint32_t kx = key[ix], ky = key[px];
    if ((kx > ky) == up) { key[ix] = ky; key[px] = kx; }
  });
  if (tkey) { if (threadIdx.x == 0) tkey[b] = key[k - 1]; }
  else for (int i = threadIdx.x; i < k; i += 256) out_keys[(uint64_t)b * out_stride + (uint64_t)blockIdx.x * k + i] = key[i];
}

// rows with D~ <= t + 2 E, and the degenerate rows, go to the query's list
__global__ __launch_bounds__(256) void mvb_survivor_kernel(const float *__restrict__ P, const uint32_t *__restrict__ pq, const uint8_t *__restrict__ degen,
                                                           uint64_t n_rows, const uint32_t *__restrict__ tkey, const float *__restrict__ e2,
                                                           uint32_t *__restrict__ cnt, uint32_t *__restrict__ list) {
  const uint32_t b = blockIdx.y;
  const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  bool pass = degen[r] != 0;
  if (!pass) {
    const uint32_t tk = tkey[b];
    const float thr = tk == 0xFFFFFFFFu ? INFINITY : key_to_float(tk) + e2[b];
    pass = !(mvb_dtilde(P, n_rows, pq[b], pq[b + 1], r) > thr);
  }
  if (pass) {
    const uint32_t pos = atomicAdd(&cnt[b], 1u);
    if (pos < (uint32_t)MV_SEL) list[(uint64_t)b * MV_SEL + pos] = (uint32_t)r;
  }
}

// The exact distance of every listed (query, row) pair: a wave per pair, mv_scan_generic_kernel<V, TV, false>'s lanes -- lane (sub, qi)
// owns query vector qi and the row's vectors sub, sub + 64 / QP, ..; the maximum is order-free, the sum is mv_finish's.
template <int V, typename TV>
__global__ __launch_bounds__(64 * MV_WAVES) void mvb_eval_kernel(const TV *__restrict__ vals, const uint64_t *__restrict__ offsets, int d,
                                                                 const float *__restrict__ qf, const float *__restrict__ qnorm,
                                                                 const uint64_t *__restrict__ qo, const uint32_t *__restrict__ cnt,
                                                                 const uint32_t *__restrict__ list, float *__restrict__ ed) {
  __shared__ uint32_t best_all[MV_WAVES * MV_MAX_NQV];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint32_t *best = best_all + wave * MV_MAX_NQV;
  const uint32_t b = blockIdx.y, n = cnt[b];
  if (n > (uint32_t)MV_SEL) return;                       // the list overflowed: the loop answers this query
  const int nqv = (int)(qo[b + 1] - qo[b]);
  const float *q = qf + qo[b] * (uint64_t)d, *qn = qnorm + qo[b];
  int qp_log2 = 0;
  while ((1 << qp_log2) < min(nqv, 64)) ++qp_log2;
  const int qp = 1 << qp_log2, qi = lane & (qp - 1), sub = lane >> qp_log2, nsub = 64 >> qp_log2;
  for (uint32_t sidx = blockIdx.x * MV_WAVES + wave; sidx < n; sidx += gridDim.x * MV_WAVES) {
    const uint32_t r = list[(uint64_t)b * MV_SEL + sidx];
    const uint64_t o0 = offsets[r], len = offsets[r + 1] - o0;
    const TV *src = vals + o0 * (uint64_t)d;
    uint32_t bk[MV_PASSES];
#pragma unroll
    for (int ps = 0; ps < MV_PASSES; ++ps) bk[ps] = 0u;
#pragma unroll
    for (int ps = 0; ps < MV_PASSES; ++ps) {
      const int qq = ps * 64 + qi;
      if (ps * 64 < nqv && qq < nqv) {
        const float *qv = q + (int64_t)qq * d;
        const float qnv = qn[qq];
        for (uint64_t jv = sub; jv < len; jv += nsub) bk[ps] = max(bk[ps], order_key(one_minus(mv_pair_rt<V, TV>(qv, qnv, src + jv * (uint64_t)d, d))));
      }
    }
#pragma unroll
    for (int ps = 0; ps < MV_PASSES; ++ps) {
      uint32_t bb = bk[ps];
      for (int off = qp; off < 64; off <<= 1) bb = max(bb, (uint32_t)__shfl_xor((int)bb, off));
      const int qq = ps * 64 + qi;
      if (sub == 0 && qq < nqv) best[qq] = bb;
    }
    wave_sync();
    if (lane == 0) ed[(uint64_t)b * MV_SEL + sidx] = mv_finish(best, nqv);
    wave_sync();
  }
}

// a block per query: the listed rows by (key, row id), the first k written (mv_select_kernel's last round)
__global__ __launch_bounds__(256) void mvb_final_kernel(const float *__restrict__ ed, const uint32_t *__restrict__ list, const uint32_t *__restrict__ cnt,
                                                        const uint64_t *__restrict__ row_ids, int k, uint64_t *__restrict__ ids, float *__restrict__ dists) {
  __shared__ uint64_t rid[MV_SEL];
  __shared__ uint32_t key[MV_SEL];
  const uint32_t b = blockIdx.x, n = cnt[b];
  if (n > (uint32_t)MV_SEL) return;
  for (int i = threadIdx.x; i < MV_SEL; i += 256) {
    uint32_t kk = 0xFFFFFFFFu;
    uint64_t rr = ~0ull;
    if ((uint32_t)i < n) {
      const uint32_t r = list[(uint64_t)b * MV_SEL + i];
      kk = order_key(ed[(uint64_t)b * MV_SEL + i]); rr = row_ids ? row_ids[r] : r;
    }
    key[i] = kk; rid[i] = rr;
  }
  __syncthreads();
  mvb_bitonic(MV_SEL, [&](int ix, int px, bool up) {
    const uint32_t kx = key[ix], ky = key[px];
    const uint64_t rx = rid[ix], ry = rid[px];
    const bool gt = kx > ky || (kx == ky && rx > ry);
    if (gt == up) { key[ix] = ky; key[px] = kx; rid[ix] = ry; rid[px] = rx; }
  });
  for (int i = threadIdx.x; i < k; i += 256) {
    ids[(uint64_t)b * k + i] = rid[i];
    dists[(uint64_t)b * k + i] = rid[i] != ~0ull ? key_to_float(key[i]) : INFINITY;
  }
}

static int mvb_kpad(uint32_t d) {
  int k = 16;
  while ((uint32_t)k < d) k <<= 1;
  return k;
}

// E(nqv, K) of the header, rounded up to f32
static float mvb_margin(uint32_t nqv, int kpad) {
  const double u = std::ldexp(1.0, -24);
  const double ep = 3.002 * std::ldexp(1.0, -16) + (9.2 * kpad + 20.0) * u + std::ldexp(1.0, -30);
  const double e = nqv * ep + (nqv + 1.0) * (nqv + 3.0) * std::ldexp(1.0, -23);
  return std::nextafterf((float)e, INFINITY);
}

static size_t mvb_filter_lds(int kpad, int cbg) {
  return (size_t)cbg * 32 * (kpad + 8) * 2 * 2 + (size_t)MVB_WAVES * (MVB_MAX_GROUP + 1) * 32 * 4 + (8 + MVB_MAX_GROUP * 32) * 4;
}

template <typename TV>
static void mvb_launch_prep(lance_hip_ctx *ctx, const void *vals, const uint64_t *offsets, uint64_t n_bags, uint64_t o_first, uint64_t o_last,
                            int d, int kpad, uint16_t *hi, uint16_t *lo, uint8_t *degen, uint32_t *flag) {
  const unsigned grid = (unsigned)std::min<uint64_t>(cdiv(n_bags, 4), (uint64_t)ctx->num_cus * 8);
  hipLaunchKernelGGL(mvb_prep_kernel<TV>, dim3(grid), dim3(256), 0, ctx->stream, static_cast<const TV *>(vals), offsets, n_bags, o_first, o_last, d,
                     kpad, hi, lo, degen, flag);
}

static void mvb_launch_filter(lance_hip_ctx *ctx, const MvbArgs &a, unsigned gx, unsigned gy, size_t lds) {
  const dim3 g(gx, gy), b(64 * MVB_WAVES);
  switch (a.kpad) {
    case 16: hipLaunchKernelGGL(mvb_filter_kernel<1>, g, b, lds, ctx->stream, a); break;
    case 32: hipLaunchKernelGGL(mvb_filter_kernel<2>, g, b, lds, ctx->stream, a); break;
    case 64: hipLaunchKernelGGL(mvb_filter_kernel<4>, g, b, lds, ctx->stream, a); break;
    case 128: hipLaunchKernelGGL(mvb_filter_kernel<8>, g, b, lds, ctx->stream, a); break;
    default: hipLaunchKernelGGL(mvb_filter_kernel<16>, g, b, lds, ctx->stream, a);
  }
}

// The filter route for the whole batch.  need_loop[b] = 1: query b is left to the loop (degenerate, or its list overflowed).
// LH_NOT_TAKEN: the route does not serve the call (the planes do not fit the device, a column that is refused anyway): the loop answers.
static int mvb_filter_route(lance_hip_ctx *ctx, int dtype, const void *values, const uint64_t *offsets, const uint64_t *row_ids, uint64_t n_rows,
                            uint32_t d, const void *q, const uint64_t *qoff, uint32_t B, uint32_t k, uint64_t *ids, float *dists,
                            uint32_t *survivors, std::vector<uint8_t> &need_loop) {
  const bool f16 = dtype == LANCE_HIP_F16;
  const int kpad = mvb_kpad(d);
  const size_t esz = f16 ? 2 : 4;
  uint64_t ends[2] = {0, 0};
  LH_CHECK_HIP(hipMemcpyAsync(&ends[0], offsets, 8, hipMemcpyDeviceToHost, ctx->stream));
  LH_CHECK_HIP(hipMemcpyAsync(&ends[1], offsets + n_rows, 8, hipMemcpyDeviceToHost, ctx->stream));
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  if (ends[1] <= ends[0] || ends[1] - ends[0] < n_rows) return LH_NOT_TAKEN;      // a zero-length row or a decrease somewhere: the loop refuses it
  const uint64_t nvec = ends[1] - ends[0];
  if (nvec >= (1ull << 40)) return LH_NOT_TAKEN;
  uint16_t *xhi = static_cast<uint16_t *>(ctx->scratch_exact("mvb.xhi", nvec * kpad * 2));
  uint16_t *xlo = xhi ? static_cast<uint16_t *>(ctx->scratch_exact("mvb.xlo", nvec * kpad * 2)) : nullptr;
  float *P = xlo ? static_cast<float *>(ctx->scratch_exact("mvb.P", (size_t)MVB_MAX_PIECES * n_rows * 4)) : nullptr;
  if (!P) return LH_NOT_TAKEN;
  uint8_t *degen = ctx->scratch_t<uint8_t>("mvb.degen", n_rows);
  uint32_t *flag = ctx->scratch_t<uint32_t>("mvb.flag", 2);
  const uint64_t qtot = qoff[B];
  const float *qf = nullptr;
  LH_TRY(as_f32(ctx, dtype, q, (size_t)qtot * d, "mvb.q", &qf));
  float *qnorm = ctx->scratch_t<float>("mvb.qnorm", qtot);
  uint64_t *qo_dev = ctx->scratch_t<uint64_t>("mvb.qo", (size_t)B + 1);
  uint16_t *qhi = ctx->scratch_t<uint16_t>("mvb.qhi", (size_t)MVB_CHUNK_COLS * kpad);
  uint16_t *qlo = ctx->scratch_t<uint16_t>("mvb.qlo", (size_t)MVB_CHUNK_COLS * kpad);
  uint8_t *qdegen = ctx->scratch_t<uint8_t>("mvb.qdegen", MVB_CHUNK_Q);
  // per chunk, one block of tables: pb [65] | pq [65] | pinfo [128] | e2 [64] | chunk-relative query offsets u64 [65]
  constexpr size_t TAB_PB = 0, TAB_PQ = 80, TAB_PI = 160, TAB_E2 = 160 + MVB_MAX_PIECES, TAB_QO = TAB_E2 + MVB_CHUNK_Q, TAB_WORDS = TAB_QO + 2 * (MVB_CHUNK_Q + 2);
  uint32_t *tab = ctx->scratch_t<uint32_t>("mvb.tab", TAB_WORDS);
  uint32_t *tkey = ctx->scratch_t<uint32_t>("mvb.tkey", MVB_CHUNK_Q);
  uint32_t *cnt = ctx->scratch_t<uint32_t>("mvb.cnt", MVB_CHUNK_Q);
  uint32_t *list = ctx->scratch_t<uint32_t>("mvb.list", (size_t)MVB_CHUNK_Q * MV_SEL);
  float *ed = ctx->scratch_t<float>("mvb.ed", (size_t)MVB_CHUNK_Q * MV_SEL);
  const uint64_t nb0 = cdiv(n_rows, MV_SEL);
  const uint64_t st0 = nb0 * k, st1 = cdiv(st0, MV_SEL) * k;
  uint32_t *sk0 = nullptr, *sk1 = nullptr;
  if (nb0 > 1) {
    sk0 = ctx->scratch_t<uint32_t>("mvb.selk0", (size_t)MVB_CHUNK_Q * st0);
    sk1 = ctx->scratch_t<uint32_t>("mvb.selk1", (size_t)MVB_CHUNK_Q * st1);
    if (!sk0 || !sk1) return LANCE_HIP_ENOMEM;
  }
  uint32_t *htab = static_cast<uint32_t *>(ctx->host_staging((TAB_WORDS + 2 * (size_t)(B + 1) + 4 * MVB_CHUNK_Q) * 4));
  if (!degen || !flag || !qnorm || !qo_dev || !qhi || !qlo || !qdegen || !tab || !tkey || !cnt || !list || !ed || !htab) return LANCE_HIP_ENOMEM;
  uint64_t *h_qo = reinterpret_cast<uint64_t *>(htab + TAB_WORDS);
  uint32_t *h_cnt = htab + TAB_WORDS + 2 * (size_t)(B + 1);
  uint8_t *h_qdegen = reinterpret_cast<uint8_t *>(h_cnt + MVB_CHUNK_Q);
  uint32_t *h_flag = h_cnt + 2 * MVB_CHUNK_Q;

  // the row planes, and the column's check
  LH_CHECK_HIP(lh::memset_async(flag, 0, 8, ctx->stream));
  {
    ScopedTimer t(ctx, "multivec_mc_planes");
    if (f16) mvb_launch_prep<__half>(ctx, values, offsets, n_rows, ends[0], ends[1], (int)d, kpad, xhi, xlo, degen, flag);
    else mvb_launch_prep<float>(ctx, values, offsets, n_rows, ends[0], ends[1], (int)d, kpad, xhi, xlo, degen, flag);
  }
  LH_CHECK_HIP(hipGetLastError());
  LH_CHECK_HIP(hipMemcpyAsync(h_flag, flag, 4, hipMemcpyDeviceToHost, ctx->stream));
  for (uint32_t b = 0; b <= B; ++b) h_qo[b] = qoff[b];
  LH_CHECK_HIP(hipMemcpyAsync(qo_dev, h_qo, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
  if (f16) hipLaunchKernelGGL(mvb_qnorm_kernel<true>, dim3((unsigned)cdiv(qtot, 64)), dim3(64), 0, ctx->stream, qf, (int)qtot, (int)d, qnorm);
  else hipLaunchKernelGGL(mvb_qnorm_kernel<false>, dim3((unsigned)cdiv(qtot, 64)), dim3(64), 0, ctx->stream, qf, (int)qtot, (int)d, qnorm);
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  LH_REQUIRE((*h_flag & 2u) == 0, "flat_multivec_topk_batch: offsets decrease");
  LH_REQUIRE((*h_flag & 1u) == 0, "flat_multivec_topk_batch: a row holds no vector (zero-length rows are refused: the reference unwraps a None there)");

  MvbArgs a;
  a.xhi = xhi; a.xlo = xlo; a.offsets = offsets; a.n_rows = n_rows; a.o_first = ends[0]; a.nvec = nvec; a.qhi = qhi; a.qlo = qlo; a.kpad = kpad;
  a.P = P;
  a.cbg = kpad <= 128 ? MVB_MAX_GROUP : 2;
  const size_t lds = mvb_filter_lds(kpad, a.cbg);
  LH_REQUIRE(lds <= MV_LDS_LIMIT, "flat_multivec_topk_batch: %zu bytes of LDS", lds);
  const uint64_t want_units = std::min<uint64_t>(cdiv(nvec, 32), (uint64_t)ctx->num_cus * MVB_WAVES * 8);
  a.vpu = cdiv(cdiv(nvec, want_units), 32) * 32;
  a.units = (uint32_t)cdiv(nvec, a.vpu);

  for (uint32_t b0 = 0; b0 < B;) {
    uint32_t b1 = b0;
    while (b1 < B && b1 - b0 < (uint32_t)MVB_CHUNK_Q && qoff[b1 + 1] - qoff[b0] <= (uint64_t)MVB_CHUNK_COLS) ++b1;      // (a query holds <= 256 vectors: b1 > b0)
    const uint32_t bc = b1 - b0;
    const uint32_t cols = (uint32_t)(qoff[b1] - qoff[b0]);
    const int ncb = (int)cdiv(cols, 32);
    // the pieces: query b's columns [c0, c1) cut at the column blocks
    uint32_t np = 0;
    for (int c = 0; c <= ncb; ++c) htab[TAB_PB + c] = 0;
    for (uint32_t b = 0; b < bc; ++b) {
      htab[TAB_PQ + b] = np;
      uint32_t c0 = (uint32_t)(qoff[b0 + b] - qoff[b0]);
      const uint32_t c1 = (uint32_t)(qoff[b0 + b + 1] - qoff[b0]);
      while (c0 < c1) {
        const uint32_t cb = c0 / 32, e = std::min(c1, (cb + 1) * 32);
        htab[TAB_PI + np] = (c0 - cb * 32) | ((e - c0) << 8);
        ++htab[TAB_PB + cb + 1];
        ++np; c0 = e;
      }
      const float e2 = 2.0f * mvb_margin(c1 - (uint32_t)(qoff[b0 + b] - qoff[b0]), kpad);
      memcpy(&htab[TAB_E2 + b], &e2, 4);
      reinterpret_cast<uint64_t *>(htab + TAB_QO)[b] = qoff[b0 + b] - qoff[b0];
    }
    htab[TAB_PQ + bc] = np;
    reinterpret_cast<uint64_t *>(htab + TAB_QO)[bc] = cols;
    for (int c = 0; c < ncb; ++c) htab[TAB_PB + c + 1] += htab[TAB_PB + c];
    LH_CHECK_HIP(hipMemcpyAsync(tab, htab, TAB_WORDS * 4, hipMemcpyHostToDevice, ctx->stream));
    a.ncb = ncb; a.pb = tab + TAB_PB; a.pinfo = tab + TAB_PI;
    const uint32_t *pq = tab + TAB_PQ;
    const float *e2 = reinterpret_cast<const float *>(tab + TAB_E2);
    const uint64_t *cqo = reinterpret_cast<const uint64_t *>(tab + TAB_QO);
    {
      ScopedTimer t(ctx, "multivec_mc_filter");
      LH_CHECK_HIP(lh::memset_multi(ctx->stream, {{qhi, 0, (size_t)MVB_CHUNK_COLS * kpad * 2}, {qlo, 0, (size_t)MVB_CHUNK_COLS * kpad * 2},
                                                  {cnt, 0, (size_t)MVB_CHUNK_Q * 4}, {flag + 1, 0, 4}}));
      const void *qc = static_cast<const char *>(q) + (size_t)qoff[b0] * d * esz;
      if (f16) mvb_launch_prep<__half>(ctx, qc, cqo, bc, 0, cols, (int)d, kpad, qhi, qlo, qdegen, flag + 1);
      else mvb_launch_prep<float>(ctx, qc, cqo, bc, 0, cols, (int)d, kpad, qhi, qlo, qdegen, flag + 1);
      const unsigned gy = (unsigned)cdiv(ncb, a.cbg);
      const unsigned gx = (unsigned)std::min<uint64_t>(cdiv(a.units, MVB_WAVES), std::max<uint64_t>(1, (uint64_t)ctx->num_cus * 4 / gy));
      mvb_launch_filter(ctx, a, gx, gy, lds);
      // the k-th smallest surrogate per query
      uint64_t n_in = n_rows, in_stride = 0;
      const uint32_t *in = nullptr;
      int cur = -1;
      for (;;) {
        const uint64_t nb = std::max<uint64_t>(1, cdiv(n_in, MV_SEL));
        const bool last = nb == 1;
        const int nxt = cur == 0 ? 1 : 0;
        uint32_t *out = last ? nullptr : (nxt == 0 ? sk0 : sk1);
        const uint64_t out_stride = nxt == 0 ? st0 : st1;
        hipLaunchKernelGGL(mvb_kth_kernel, dim3((unsigned)nb, bc), dim3(256), 0, ctx->stream, P, pq, degen, n_rows, in, n_in, in_stride, (int)k, out,
                           out_stride, last ? tkey : nullptr);
        if (last) break;
        n_in = nb * k; in = out; in_stride = out_stride; cur = nxt;
      }
      hipLaunchKernelGGL(mvb_survivor_kernel, dim3((unsigned)cdiv(n_rows, 256), bc), dim3(256), 0, ctx->stream, P, pq, degen, n_rows, tkey, e2, cnt, list);
    }
    {
      ScopedTimer t(ctx, "multivec_mc_eval");
      const dim3 g(MV_SEL / MV_WAVES / 4, bc), blk(64 * MV_WAVES);
      const uint64_t *qo_b = qo_dev + b0;
      if (f16) hipLaunchKernelGGL((mvb_eval_kernel<MV_COS_H, __half>), g, blk, 0, ctx->stream, static_cast<const __half *>(values), offsets, (int)d, qf, qnorm, qo_b, cnt, list, ed);
      else hipLaunchKernelGGL((mvb_eval_kernel<MV_COS, float>), g, blk, 0, ctx->stream, static_cast<const float *>(values), offsets, (int)d, qf, qnorm, qo_b, cnt, list, ed);
    }
    {
      ScopedTimer t(ctx, "multivec_mc_select");
      hipLaunchKernelGGL(mvb_final_kernel, dim3(bc), dim3(256), 0, ctx->stream, ed, list, cnt, row_ids, (int)k, ids + (uint64_t)b0 * k, dists + (uint64_t)b0 * k);
    }
    LH_CHECK_HIP(hipGetLastError());
    LH_CHECK_HIP(hipMemcpyAsync(h_cnt, cnt, (size_t)bc * 4, hipMemcpyDeviceToHost, ctx->stream));
    LH_CHECK_HIP(hipMemcpyAsync(h_qdegen, qdegen, bc, hipMemcpyDeviceToHost, ctx->stream));
    LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));      // (the tables in the staging block are free again)
    for (uint32_t b = 0; b < bc; ++b) {
      if (h_cnt[b] > (uint32_t)MV_SEL) { ctx->count_stage("multivec_batch_overflow"); need_loop[b0 + b] = 1; }
      else if (h_qdegen[b]) need_loop[b0 + b] = 1;
      else if (survivors) survivors[b0 + b] = h_cnt[b];
    }
    b0 = b1;
  }
  return LANCE_HIP_OK;
}

}  // namespace lh

using namespace lh;

extern "C" int lance_hip_flat_multivec_topk_batch(lance_hip_ctx *ctx, int dtype, int metric, const void *values, const uint64_t *offsets,
                                                  const uint64_t *row_ids, uint64_t n_rows, uint32_t d, const void *q, const uint64_t *q_offsets,
                                                  uint32_t n_queries, uint32_t k, int has_lower, float lower, int has_upper, float upper,
                                                  uint64_t *ids, float *dists, uint32_t *survivors) {
  const char *what = "flat_multivec_topk_batch";
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && q_offsets, "%s: NULL argument", what);
  LH_REQUIRE(n_queries >= 1 && n_queries <= 65535u, "%s: %u queries: a batch holds 1..65535", what, n_queries);
  for (uint32_t b = 0; b < n_queries; ++b) {
    LH_REQUIRE(q_offsets[b + 1] >= q_offsets[b], "%s: q_offsets decrease at query %u", what, b);
    const uint64_t nqv = q_offsets[b + 1] - q_offsets[b];
    LH_REQUIRE(nqv >= 1 && nqv <= (uint64_t)MV_MAX_NQV, "%s: query %u holds %llu vectors: a multivector query holds 1..%d vectors", what, b,
               (unsigned long long)nqv, MV_MAX_NQV);
  }
  LH_TRY(mv_check_args(what, ctx, dtype, metric, values, offsets, n_rows, d, q, (uint32_t)(q_offsets[1] - q_offsets[0])));
  LH_REQUIRE(ids && dists, "%s: NULL argument", what);
  LH_REQUIRE(k > 0 && k <= (uint32_t)MV_SEL / 2, "%s: k=%u not supported (1..%d)", what, k, MV_SEL / 2);
  const FlatRange rg = flat_range(has_lower, lower, has_upper, upper);
  LH_REQUIRE(!(rg.has_lower && rg.has_upper) || rg.lo_key <= rg.hi_key, "%s: lower bound %g is above the upper bound %g", what, (double)lower, (double)upper);
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  std::vector<uint8_t> need_loop(n_queries, 0);
  bool filtered = false;
  if (metric == LANCE_HIP_COSINE && !rg.any() && d <= (uint32_t)MVB_MAX_D && n_rows >= 1 && n_rows < (1ull << 31)) {
    const int r = mvb_filter_route(ctx, dtype, values, offsets, row_ids, n_rows, d, q, q_offsets, n_queries, k, ids, dists, survivors, need_loop);
    if (r != LH_NOT_TAKEN) {
      LH_TRY(r);
      filtered = true;
    }
  }
  const size_t esz = dtype == LANCE_HIP_F16 ? 2 : 4;
  for (uint32_t b = 0; b < n_queries; ++b) {
    if (filtered && !need_loop[b]) continue;
    ctx->count_stage("multivec_batch_loop");
    const void *qb = static_cast<const char *>(q) + (size_t)q_offsets[b] * d * esz;
    LH_TRY(mv_topk_impl(what, ctx, dtype, metric, values, offsets, row_ids, n_rows, d, qb, (uint32_t)(q_offsets[b + 1] - q_offsets[b]), k, rg,
                        ids + (uint64_t)b * k, dists + (uint64_t)b * k));
    if (survivors) survivors[b] = (uint32_t)std::min<uint64_t>(n_rows, 0xFFFFFFFFull);
  }
  return LANCE_HIP_OK;
}
