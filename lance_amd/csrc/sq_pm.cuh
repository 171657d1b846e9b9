// sq_pm.cuh -- IVF_SQ batched search, partition major: the scan stage of large batches on the int8 matrix cores.  Included by sq.hip alone
// (it scores with sq.hip's sq_sum / sq_finish and fills pair_cand.cuh's CandLists; merge, replay decision, replay and refine are untouched).
//
// sq_scan_kernel runs one workgroup per (query, probed partition) pair, so every pair reads its partition's codes again.  Here the pairs
// are grouped by partition (group.hip) and cut into blocks of SQPM_QB = 32 queries; a work item is (partition, query block) and reads the
// partition ONCE for its 32 queries.  The distances of a block against a row tile are one exact integer GEMM:
//
//   v_mfma_i32_32x32x32_i8   A = 32 code rows, B = 32 encoded queries, 16 bytes of K per lane, i32 accumulators.
//
// The operands are signed and the codes are u8, so bit 7 of both sides is flipped as they are staged (x ^ 0x80 == x - 128 as i8) and
//   sum((x - 128)(q - 128)) = xq - 128 sum(x) - 128 sum(q) + 16384 ld          over the ld staged bytes of a row, zero padding included
// gives xq back exactly (bytes staged beyond ld are 0 AFTER the flip and add nothing).  Every term stays inside i32 up to ld = 16384:
// |S| <= ld 128^2 = 2^28, 128 sum(x) and 128 sum(q) <= 128 * 255 * 16384 < 2^29.1, 16384 ld = 2^28, and any partial sum of the four is
// below 2^28 + 2 * 2^29.1 < 2^31; xq itself is at most 16384 * 255^2 < 2^30.  So the i32 accumulator holds the integer v_dot4_u32_u8 gives
// sq_scan_kernel, and key = order_key(sq_finish(sq_sum(..))) is the same word: no surrogate, no margin, no re-check.
//
// Work split (256 threads, 4 waves): a row tile is SQPM_TILE = 128 rows, wave w multiplies rows 32 w .. 32 w + 31 with all 32 queries; lane
// (j = lane & 31, g = lane >> 5) ends with 16 rows of query j.  K is walked in SQPM_KT = 64-byte steps (two MFMAs per wave) so that rows of
// any ld <= 16384 are served.  The row slab of a K step goes through LDS (coalesced 16-byte loads, fetched into registers one step ahead
// so that they fly while the matrix cores and the selection work); a lane's query operand does not: up to ld = 128 it is 16 registers
// loaded once per item, longer queries are fetched step by step beside the rows.  sum(x) of a row is one v_dot4 against 0x01010101 per 4
// codes while the row is staged, shared by the 32 queries; sum(q) is computed once per query and item.
//
// Selection is cand_scan_pair's, per pair: a row whose key is <= the pair's falling threshold goes into that pair's buffer of SQPM_CAP = 256
// entries; a buffer that holds more than SQPM_CAP - SQPM_TILE entries after a tile is sorted and cut to keff by the wave that owns the pair
// (8 pairs per wave, no workgroup barrier inside the sort) and a cut tie is recorded as cand_sort_truncate records it.  pair_cand.cuh's
// contract does not depend on the capacity, so the lists are bit for bit sq_scan_kernel's.  All 32 buffers live in LDS at once, which is
// why the route serves keff <= CAND_NARROW_K only.
//
// LDS per workgroup (sqpm_lds_bytes): 32 x 256 x 8 = 65,536 candidate entries | 128 x 80 row slab | 128 row sums | 128 row norms |
// 7 x 32 control words = 77,696 bytes: two workgroups fit a CU's 160 KiB.  The 16 bytes of padding per staged row keep ds_read_b128 of 16
// consecutive rows on 16 different bank groups.
#pragma once

namespace lh {

constexpr int SQPM_QB = 32;        // queries per work item: N of the MFMA tile
constexpr int SQPM_TILE = 128;     // rows per tile: 32 per wave
constexpr int SQPM_CAP = 256;      // entries of a pair's buffer
constexpr int SQPM_KT = 64;        // bytes of a row staged per K step
constexpr int SQPM_QK = 128;       // bytes of a query a lane keeps in registers for the whole item
constexpr int SQPM_RS = SQPM_KT + 16;                             // LDS stride of a staged row
static_assert(CAND_NARROW_K + SQPM_TILE <= SQPM_CAP, "the kept entries and one row tile fit a pair's buffer");
static_assert(SQPM_QB == CAND_BLOCK_PAIRS && SQPM_CAP == CAND_BLOCK_CAP, "the block selection of pair_cand.cuh");
static_assert(SQPM_TILE * (SQPM_KT / 16) == 512 && SQPM_QK == 2 * SQPM_KT, "staging: two row chunks per thread; resident queries span two K steps");

// ---- the plan: which scan serves an IVF_SQ batch.  Decided once per call, before anything is enqueued. ---------------------------------------
// Grouped when the lists fit the narrow capacity and the pairs per partition reach SQPM_MIN_PAIRS_PER_LIST on average.  Measured on 1M x 128
// rows, IVF256, nprobes 10 (profiles/sq_grouped_probe.json): a work item walks its whole partition whether its block holds 3 queries or 32,
// so small batches are faster on the pair-major scan's nq * nprobes workgroups; the routes cross between 32 and 64 pairs per partition.
constexpr uint32_t SQPM_MIN_PAIRS_PER_LIST = 64;
static inline bool plan_ivfsq_grouped(uint32_t nq, uint32_t nprobes, uint32_t nlist, uint32_t keff, bool switched_off,
                                      uint32_t min_pairs_per_list = SQPM_MIN_PAIRS_PER_LIST) {
  if (switched_off || keff > (uint32_t)CAND_NARROW_K) return false;
  return (uint64_t)nq * nprobes >= (uint64_t)min_pairs_per_list * nlist;
}

static inline size_t sqpm_lds_bytes() {
  return (size_t)SQPM_QB * SQPM_CAP * 8 + (size_t)SQPM_TILE * SQPM_RS + (size_t)SQPM_TILE * 8 + (size_t)7 * SQPM_QB * 4;
}

typedef int sqpm_i32x4 __attribute__((ext_vector_type(4)));
typedef int sqpm_i32x16 __attribute__((ext_vector_type(16)));

__device__ __forceinline__ uint32_t sqpm_sum16(uint4 v, uint32_t acc) {
  acc = sq_udot4(v.x, 0x01010101u, acc); acc = sq_udot4(v.y, 0x01010101u, acc);
  acc = sq_udot4(v.z, 0x01010101u, acc); return sq_udot4(v.w, 0x01010101u, acc);
}
__device__ __forceinline__ sqpm_i32x4 sqpm_vec(uint4 v) { return sqpm_i32x4{(int)v.x, (int)v.y, (int)v.z, (int)v.w}; }
__device__ __forceinline__ uint4 sqpm_flip(uint4 v) { return make_uint4(v.x ^ 0x80808080u, v.y ^ 0x80808080u, v.z ^ 0x80808080u, v.w ^ 0x80808080u); }

struct SqPmCtl : CandBlockCtl {    // pair_cand.cuh's selection words, and per pair of the block:
  uint32_t qq[SQPM_QB], qsum[SQPM_QB];
};

// grid: one workgroup per work item; desc[item] = {partition, first grouped pair, pairs (1..32), 0}, partition -1 = no item.
// Dynamic LDS: sqpm_lds_bytes().
__global__ __launch_bounds__(256) void ivfsq_pm_scan_kernel(SqArgs a, const uint32_t *__restrict__ pair_idx, const int4 *__restrict__ desc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int4 item = desc[blockIdx.x];
  if (item.x < 0) return;
  uint64_t *ebuf = reinterpret_cast<uint64_t *>(smem);                               // [32][SQPM_CAP]
  char *rows = smem + (size_t)SQPM_QB * SQPM_CAP * 8;                                // [128][SQPM_RS]
  uint32_t *xs = reinterpret_cast<uint32_t *>(rows + SQPM_TILE * SQPM_RS);           // [128] sum(x) | allowed << 31
  uint32_t *xxs = xs + SQPM_TILE;                                                    // [128] sum(x^2) (0 under dot)
  SqPmCtl *ctl = reinterpret_cast<SqPmCtl *>(xxs + SQPM_TILE);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, g = lane >> 5;
  const int ld = a.ld, k = a.w.k, nprobes = a.w.nprobes, np = item.z;
  const uint32_t r0 = a.w.part_offsets[item.x], r1 = a.w.part_offsets[item.x + 1];
  if (tid < SQPM_QB) {
    const int pair = tid < np ? (int)pair_idx[(uint32_t)item.y + tid] : -1;
    ctl->pair[tid] = pair; ctl->cnt[tid] = 0; ctl->thr[tid] = 0xFFFFFFFFu; ctl->amb[tid] = 0; ctl->amb_key[tid] = 0;
    ctl->qq[tid] = pair >= 0 ? a.qq[pair / nprobes] : 0u;
  }
  __syncthreads();
  // sum(q), once per query: wave w sums the queries of pairs 8 w .. 8 w + 7
  for (int u = 0; u < SQPM_QB / 4; ++u) {
    const int p = wave * (SQPM_QB / 4) + u, pair = ctl->pair[p];
    uint32_t s = 0;
    if (pair >= 0) {
      const uint4 *qp = reinterpret_cast<const uint4 *>(a.qcodes + (int64_t)(pair / nprobes) * ld);
      for (int c = lane; c < ld / 16; c += 64) s = sqpm_sum16(qp[c], s);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) ctl->qsum[p] = s;
  }
  __syncthreads();
  const int my_pair = ctl->pair[j];
  const int qterm = 128 * (int)ctl->qsum[j] - 16384 * ld;
  const uint32_t my_qq = ctl->qq[j];
  uint64_t *my_e = ebuf + j * SQPM_CAP;
  const int nkt = (ld + SQPM_KT - 1) / SQPM_KT;
  // B operands: lane (j, g) holds bytes 16 g .. 16 g + 15 of every 32-byte K step of query j, bit 7 flipped, 0 beyond ld.  Up to
  // ld = SQPM_QK they stay in 16 registers for the whole item; longer queries are fetched step by step, one step ahead like the rows.
  const bool q_resident = ld <= SQPM_QK;
  const uint8_t *my_q = a.qcodes + (int64_t)(my_pair >= 0 ? my_pair / nprobes : 0) * ld + g * 16;
  auto q_operand = [&](int kk) {
    uint4 v = make_uint4(0, 0, 0, 0);
    if (my_pair >= 0 && kk + g * 16 < ld) v = sqpm_flip(*reinterpret_cast<const uint4 *>(my_q + kk));
    return v;
  };
  uint4 qres[SQPM_QK / 32], nq[2] = {make_uint4(0, 0, 0, 0), make_uint4(0, 0, 0, 0)};
#pragma unroll
  for (int s = 0; s < SQPM_QK / 32; ++s) qres[s] = q_resident ? q_operand(32 * s) : make_uint4(0, 0, 0, 0);
  // what a thread stages per K step: two 16-byte chunks of the 128 x 64-byte slab, and with a row's first chunk its sum of squares and
  // its prefilter bit.  Fetched into registers one step ahead: the loads fly while the matrix cores and the selection work.
  uint4 nx[2];
  uint32_t nxx[2] = {0u, 0u};
  bool nok[2] = {false, false};
  auto fetch = [&](uint32_t base, int kt) {
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      const int i = tid + 256 * u, rl = i >> 2, c = i & 3, kk = kt * SQPM_KT + c * 16;
      const uint32_t row = base + (uint32_t)rl;
      nx[u] = make_uint4(0, 0, 0, 0);
      if (row < r1 && kk < ld) nx[u] = *reinterpret_cast<const uint4 *>(a.codes + (int64_t)row * ld + kk);
      if (c == 0 && kt == 0) {
        nxx[u] = (!a.dot && row < r1) ? a.xx[row] : 0u;
        nok[u] = row < r1 && row_allowed(a.w.allow, row);
      }
    }
    if (!q_resident) { nq[0] = q_operand(kt * SQPM_KT); nq[1] = q_operand(kt * SQPM_KT + 32); }
  };
  if (r0 < r1) fetch(r0, 0);

  for (uint32_t base = r0; base < r1; base += SQPM_TILE) {
    sqpm_i32x16 acc;
#pragma unroll
    for (int v = 0; v < 16; ++v) acc[v] = 0;
    for (int kt = 0; kt < nkt; ++kt) {
#pragma unroll
      for (int u = 0; u < 2; ++u) {                              // 128 rows x 4 chunks of 16 bytes
        const int i = tid + 256 * u, rl = i >> 2, c = i & 3, kk = kt * SQPM_KT + c * 16;
        const bool in = base + (uint32_t)rl < r1 && kk < ld;
        uint32_t s = sqpm_sum16(nx[u], 0u);                      // (a chunk that was not read is 0)
        *reinterpret_cast<uint4 *>(rows + rl * SQPM_RS + c * 16) = in ? sqpm_flip(nx[u]) : make_uint4(0, 0, 0, 0);
        s += __shfl_xor(s, 1, 64);
        s += __shfl_xor(s, 2, 64);
        if (c == 0) {                                            // the one thread that ever writes xs[rl] and xxs[rl]
          if (kt == 0) { xs[rl] = s | (nok[u] ? 0x80000000u : 0u); xxs[rl] = nxx[u]; }
          else xs[rl] += s;
        }
      }
      const uint4 b0 = q_resident ? (kt ? qres[2] : qres[0]) : nq[0], b1 = q_resident ? (kt ? qres[3] : qres[1]) : nq[1];
      __syncthreads();
      if (kt + 1 < nkt) fetch(base, kt + 1);
      else if (base + SQPM_TILE < r1) fetch(base + SQPM_TILE, 0);
      const char *my_row = rows + (wave * 32 + j) * SQPM_RS + g * 16;
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*reinterpret_cast<const sqpm_i32x4 *>(my_row), sqpm_vec(b0), acc, 0, 0, 0);
      acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(*reinterpret_cast<const sqpm_i32x4 *>(my_row + 32), sqpm_vec(b1), acc, 0, 0, 0);
      __syncthreads();      // the slab is read before the next step overwrites it; after the last step xs is complete
    }
    if (my_pair >= 0) {
      const uint32_t thr = ctl->thr[j];
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int rl = wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * g;      // the accumulator's row of the 32 x 32 tile
        const uint32_t sx = xs[rl];
        if (sx >> 31) {
          const uint32_t row = base + (uint32_t)rl;
          const uint32_t xq = (uint32_t)(acc[v] + 128 * (int)(sx & 0x7FFFFFFFu) + qterm);
          const uint32_t key = order_key(sq_finish(a.dot, sq_sum(a.dot, xq, xxs[rl], my_qq), a.r2));
          if (key <= thr) {      // rows tied with the k-th key come in too: the sort decides by position and records the cut tie
            const int slot = atomicAdd(&ctl->cnt[j], 1);
            my_e[slot] = ((uint64_t)key << 32) | row;
          }
        }
      }
    }
    __syncthreads();
    // before a tile at most SQPM_CAP - SQPM_TILE entries are held (k <= 128 after a cut), so its 128 rows always fit
    for (int u = 0; u < SQPM_QB / 4; ++u) {
      const int p = wave * (SQPM_QB / 4) + u;
      if (ctl->cnt[p] > SQPM_CAP - SQPM_TILE) cand_block_sort_truncate(ebuf + p * SQPM_CAP, ctl, p, k, lane);
    }
    __syncthreads();
  }
  cand_block_write(a.w, ebuf, ctl, k, wave, lane);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
struct SqPmScratch {
  uint32_t *pair_starts = nullptr, *pair_idx = nullptr, *item_start = nullptr;
  int4 *desc = nullptr;
  uint32_t max_items = 0;
};

// LANCE_HIP_NO_SQ_GROUPED, read once per process: every batch takes the pair-major scan (A/B runs)
static bool sqpm_switched_off() {
  static const bool off = getenv("LANCE_HIP_NO_SQ_GROUPED") != nullptr;
  return off;
}

// LANCE_HIP_SQ_GROUPED_G=<g>, read once per process: grouped from g pairs per partition on (the sweep that chose the default)
static int sqpm_forced_g() {
  static const int g = getenv("LANCE_HIP_SQ_GROUPED_G") ? std::max(0, atoi(getenv("LANCE_HIP_SQ_GROUPED_G"))) : -1;
  return g;
}

// the grouping's slots for chunks of at most `pairs` pairs: every partition's last block may be ragged, so pairs / 32 + nlist items bound the table
static int sqpm_scratch(lance_hip_ctx *ctx, size_t pairs, uint32_t nlist, SqPmScratch *s) {
  s->max_items = (uint32_t)(pairs / SQPM_QB + nlist + 1);
  s->pair_starts = ctx->scratch_t<uint32_t>("ivfsq.pm.pair_starts", (size_t)nlist + 1);
  s->pair_idx = ctx->scratch_t<uint32_t>("ivfsq.pm.pair_idx", pairs);
  s->item_start = ctx->scratch_t<uint32_t>("ivfsq.pm.item_start", (size_t)nlist + 1);
  s->desc = ctx->scratch_t<int4>("ivfsq.pm.desc", s->max_items);
  return s->pair_starts && s->pair_idx && s->item_start && s->desc ? LANCE_HIP_OK : LANCE_HIP_ENOMEM;
}

// the scan stage of one chunk of nqc queries: group the pairs (a.w.probes) by partition, cut them into blocks, scan.  Every pair's list is
// written at its own index, so the merge does not notice the reordering.
static int sqpm_scan(lance_hip_ctx *ctx, const SqArgs &a, uint32_t nqc, uint32_t nlist, const SqPmScratch &s) {
  const int64_t pairs = (int64_t)nqc * a.w.nprobes;
  {
    ScopedTimer t(ctx, "ivfsq_pm_group");
    LH_TRY(stable_group(ctx, a.w.probes, pairs, pairs, (int)nlist, 1, s.pair_starts, s.pair_idx, pairs, nullptr));
    LH_TRY(qscan_items(ctx, s.pair_starts, (int)nlist, SQPM_QB, s.item_start, s.desc, s.max_items));
  }
  {
    ScopedTimer t(ctx, "ivfsq_pm_scan");
    hipLaunchKernelGGL(ivfsq_pm_scan_kernel, dim3(s.max_items), dim3(256), sqpm_lds_bytes(), ctx->stream, a, s.pair_idx, s.desc);
  }
  LH_CHECK_HIP(hipGetLastError());
  return LANCE_HIP_OK;
}

}  // namespace lh
