// rq_pm.cuh -- IVF_RQ batched search, partition major: the scan stage of large batches on the int8 matrix cores.  Included by rq.hip alone,
// behind its device code (it prepares with rq_rot_dot, scores with rq_packed_tail / rq_row_distance and fills pair_cand.cuh's CandLists; merge,
// replay decision, replay and refine are untouched).
//
// rq_scan_kernel runs one workgroup per (query, probed partition) pair: every pair reads its partition's codes again and looks every code
// nibble up in its u8 table, 32 LDS lookups per (row, pair) at d = 128.  Here the pairs are grouped by partition (group.hip) and cut into
// blocks of RQPM_QB = 32; a work item is (partition, block) and reads the partition ONCE for its 32 pairs.  The lookups become a product:
//
//   sum_b etab[2b][code_b & 15] + etab[2b+1][code_b >> 4]  =  onehot(row) . etab          K = 4 d: 16 one-hot int8 per 4-bit segment
//   v_mfma_i32_32x32x32_i8   A = 32 rows x (two segments = one code byte), B = 32 pairs' table bytes of those segments, i32 accumulators.
//
// The operands are signed and the table is u8, so the table is stored with bit 7 flipped (e ^ 0x80 == e - 128 as i8).  A row has exactly
// one 1 per segment, so the product is sum(e - 128) over d / 4 segments = s - 32 d: s = acc + 32 d, |acc| <= 128 d / 4, exact in i32.  The
// integer is rq_row_distance's, the tail that follows it is the same text (rq_packed_tail): no surrogate, no margin, no re-check.
//
// Phase 1 -- the block's pairs are prepared side by side by the whole workgroup, rq_prepare's arithmetic operation for operation, split
// thread per (pair, component): residual q - c, rq_rot_dot, the lowbit table, total_cmp min / max through order_key, f32::sum from -0.0,
// q_factor, the u8 table with roundf and the saturating cast, qmin == qmax.  The f32 tables (16 d bytes per pair) live only here, in the
// candidate buffers' 64 KiB: 32 pairs at d = 128, sub-blocks of 65536 / (16 d) pairs beyond.  While a pair's f32 table is live the
// partition's last n % 32 rows (RQ_REMAINDER: f32 terms in byte order, never the u8 table) are scored for it into a side array and pushed
// into its buffer before the tiles start.  What stays per pair: its flipped u8 table (4 d bytes + 16 of padding: ds_read_b128 of 16
// consecutive pairs falls on 16 bank groups) and its RqQuery.
//
// Phase 2 -- tiles of RQPM_TILE = 128 rows over the packed rows; wave w multiplies rows 32 w .. 32 w + 31 with the 32 pairs.  Lane
// (i = lane & 31, g = lane >> 5) loads row i's code words straight from HBM into registers (16 bytes at a time and one chunk ahead where
// d / 8 is a multiple of 16, byte by byte otherwise, as rq_row_distance does) and builds its A operand of a step -- code byte t, segment
// 2 t + g -- as a single 0x01 at byte (code_t >> 4 g) & 15; its B operand is bytes 32 t + 16 g .. of pair (lane & 31)'s table, read from
// LDS.  No row goes through LDS and there is no workgroup barrier in the K loop.  Lane (j, g) ends with 16 rows of pair j, finishes them
// with the tile's staged add / scale factors and pushes rows at or under pair j's falling threshold.  Selection is the block selection
// of pair_cand.cuh, shared with sq_pm.cuh.
//
// LDS per workgroup (rqpm_lds_bytes): 32 x 256 x 8 = 65,536 candidate entries | 32 x (4 d + 16) tables | min(32, 4096 / d) x 4 d rotated
// queries | 32 x 31 remainder keys | 2 x 128 tile factors | 12 x 32 control words: 105,344 bytes at d = 128, 121,728 at d = 256 -- one
// workgroup per CU either way (the buffers alone leave no room for two beside the tables); d = 584 is the last that fits 160 KiB.
#pragma once

namespace lh {

constexpr int RQPM_QB = 32;        // pairs per work item: N of the MFMA tile
constexpr int RQPM_TILE = 128;     // rows per tile: 32 per wave
constexpr int RQPM_CAP = 256;      // entries of a pair's buffer
constexpr int RQPM_REM = RQ_BATCH - 1;                            // remainder rows of a partition, at most
constexpr size_t RQPM_LDS_LIMIT = (size_t)160 * 1024;             // one workgroup's LDS
static_assert(CAND_NARROW_K + RQPM_TILE <= RQPM_CAP && RQPM_REM <= RQPM_CAP - RQPM_TILE, "the kept entries (or the remainder) and one row tile fit a pair's buffer");
static_assert(RQPM_QB == CAND_BLOCK_PAIRS && RQPM_CAP == CAND_BLOCK_CAP && RQPM_TILE % RQ_BATCH == 0, "the block selection of pair_cand.cuh; waves are whole batches");

// pairs prepared at a time: as many as have their f32 tables (16 d bytes) in the candidate buffers
__host__ __device__ static inline int rqpm_sub_block(int d) { const int fit = (RQPM_QB * RQPM_CAP * 8) / (16 * d); return fit < RQPM_QB ? fit : RQPM_QB; }
__host__ __device__ static inline int rqpm_table_stride(int d) { return 4 * d + 16; }
__host__ __device__ static inline int rqpm_rot_bytes(int d) { return d < 128 ? RQPM_QB * 4 * d : RQPM_QB * RQPM_CAP * 8 / 4; }      // >= rqpm_sub_block(d) * 4 d

struct RqPmCtl : CandBlockCtl {    // pair_cand.cuh's selection words, and per pair of the block:
  RqQuery h[RQPM_QB];
  float factor[RQPM_QB];           // 255 / (qmax - qmin)
};

static inline size_t rqpm_lds_bytes(uint32_t d) {
  return (size_t)RQPM_QB * RQPM_CAP * 8 + (size_t)RQPM_QB * rqpm_table_stride((int)d) + (size_t)rqpm_rot_bytes((int)d) + (size_t)RQPM_QB * RQPM_REM * 4 +
         (size_t)RQPM_TILE * 8 + sizeof(RqPmCtl);
}

// ---- the plan: which scan serves an IVF_RQ batch.  Decided once per call, before anything is enqueued. ---------------------------------------
// Grouped when there is an integer sum to multiply (no prefilter: under one every row takes the f32 fold), the lists fit the narrow capacity,
// a block of d-dimensional tables fits one workgroup's LDS and the pairs per partition reach RQPM_MIN_PAIRS_PER_LIST on average.
// Measured on 1M x 128 rows, IVF256, nprobes 10 (profiles/rq_grouped_probe.json): the route did NOT win at any of
// 4 .. 128 pairs per partition (3.47 .. 3.52 ms against 1.07 .. 1.11 ms at 128; 8.9 .. 9.1 against 3.05 .. 3.21 on the whole batch), so by
// the rule the sweep was run under the gate is the largest point swept.
constexpr uint32_t RQPM_MIN_PAIRS_PER_LIST = 128;
static inline bool plan_ivfrq_grouped(uint32_t nq, uint32_t nprobes, uint32_t nlist, uint32_t keff, uint32_t d, bool filtered, bool switched_off,
                                      uint32_t min_pairs_per_list = RQPM_MIN_PAIRS_PER_LIST) {
  if (switched_off || filtered || keff > (uint32_t)CAND_NARROW_K) return false;
  if (d < 8 || d % 8 != 0 || d > RQ_MAX_DIM || rqpm_lds_bytes(d) > RQPM_LDS_LIMIT) return false;
  return (uint64_t)nq * nprobes >= (uint64_t)min_pairs_per_list * nlist;
}

typedef int rqpm_i32x4 __attribute__((ext_vector_type(4)));
typedef int rqpm_i32x16 __attribute__((ext_vector_type(16)));

// the A operand of one K step: a segment's nibble as 16 one-hot int8, 0x01 at byte n
__device__ __forceinline__ rqpm_i32x4 rqpm_onehot(uint32_t n) {
  const int one = 1 << (8 * (n & 3u));
  const uint32_t w = n >> 2;
  return rqpm_i32x4{w == 0u ? one : 0, w == 1u ? one : 0, w == 2u ? one : 0, w == 3u ? one : 0};
}

// grid: one workgroup per work item; desc[item] = {partition, first grouped pair, pairs (1..32), 0}, partition -1 = no item.
// Dynamic LDS: rqpm_lds_bytes(d).  a.w.allow == NULL (plan_ivfrq_grouped).
__global__ __launch_bounds__(256) void ivfrq_pm_scan_kernel(RqArgs a, const uint32_t *__restrict__ pair_idx, const int4 *__restrict__ desc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int4 item = desc[blockIdx.x];
  if (item.x < 0) return;
  const int d = a.d, cb = d / 8, ts = rqpm_table_stride(d), nseg = d / 4, sub = rqpm_sub_block(d);
  uint64_t *ebuf = reinterpret_cast<uint64_t *>(smem);                               // [32][RQPM_CAP]; phase 1: f32 tables [sub][4 d]
  uint8_t *etabs = reinterpret_cast<uint8_t *>(smem + (size_t)RQPM_QB * RQPM_CAP * 8);      // [32][ts] u8 tables, bit 7 flipped; first the residuals
  float *rqv = reinterpret_cast<float *>(etabs + RQPM_QB * ts);                      // [sub][d] rotated queries
  uint32_t *remk = reinterpret_cast<uint32_t *>(reinterpret_cast<char *>(rqv) + rqpm_rot_bytes(d));      // [32][RQPM_REM] keys of the remainder rows
  float *fadd = reinterpret_cast<float *>(remk + RQPM_QB * RQPM_REM);                // [128] the tile's factors
  float *fscale = fadd + RQPM_TILE;
  RqPmCtl *ctl = reinterpret_cast<RqPmCtl *>(fscale + RQPM_TILE);
  float *tables = reinterpret_cast<float *>(smem);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, j = lane & 31, g = lane >> 5;
  const int k = a.w.k, nprobes = a.w.nprobes, npairs = item.z;
  const uint32_t r0 = a.w.part_offsets[item.x], r1 = a.w.part_offsets[item.x + 1];
  const int nrem = (int)((r1 - r0) % RQ_BATCH);
  const uint32_t np = r1 - (uint32_t)nrem;                                           // first row of the f32 remainder
  if (tid < RQPM_QB) {
    ctl->pair[tid] = tid < npairs ? (int)pair_idx[(uint32_t)item.y + tid] : -1;
    ctl->cnt[tid] = 0; ctl->thr[tid] = 0xFFFFFFFFu; ctl->amb[tid] = 0; ctl->amb_key[tid] = 0;
    ctl->h[tid].kmin = 0xFFFFFFFFu; ctl->h[tid].kmax = 0u;
  }
  __syncthreads();
  if (r0 < r1) {      // (uniform) an empty partition needs no tables
    // ---- phase 1: rq_prepare for the block's pairs, a sub-block at a time ----
    const float *cent = a.cent + (int64_t)item.x * d;
    for (int p0 = 0; p0 < npairs; p0 += sub) {
      const int nsb = min(sub, npairs - p0);
      for (int idx = tid; idx < nsb * d; idx += 256) {
        const int pl = idx / d, i = idx - pl * d;
        reinterpret_cast<float *>(etabs + (p0 + pl) * ts)[i] = a.q[(int64_t)(ctl->pair[p0 + pl] / nprobes) * d + i] - cent[i];
      }
      __syncthreads();
      for (int idx = tid; idx < nsb * d; idx += 256) {
        const int pl = idx / d, c = idx - pl * d;
        rqv[idx] = rq_rot_dot(a.pt, d, c, reinterpret_cast<const float *>(etabs + (p0 + pl) * ts), d);
      }
      __syncthreads();
      for (int it = tid; it < nsb * nseg; it += 256) {
        const int pl = it / nseg, s = it - pl * nseg;
        const float *rv = rqv + pl * d + 4 * s;
        float *tb = tables + pl * 4 * d + s * 16;
        float tt[16];
        tt[0] = 0.0f;
#pragma unroll
        for (int u = 1; u < 16; ++u) tt[u] = tt[u - (u & -u)] + rv[__builtin_ctz(u)];
        uint32_t kmin = 0xFFFFFFFFu, kmax = 0u;
#pragma unroll
        for (int u = 0; u < 16; ++u) {
          tb[u] = tt[u];
          const uint32_t key = order_key(tt[u]);        // minmax_by(total_cmp)
          kmin = key < kmin ? key : kmin; kmax = key > kmax ? key : kmax;
        }
        atomicMin(&ctl->h[p0 + pl].kmin, kmin); atomicMax(&ctl->h[p0 + pl].kmax, kmax);
      }
      if (tid < nsb) {
        RqQuery *h = &ctl->h[p0 + tid];
        float sum = -0.0f;                              // f32::sum
        for (int c = 0; c < d; ++c) sum = sum + rqv[tid * d + c];
        const float dqc = a.pdists[ctl->pair[p0 + tid]];
        h->sum_q = sum;
        h->q_factor = a.dot ? dqc - 1.0f : dqc;
      }
      __syncthreads();
      if (tid < nsb) {
        RqQuery *h = &ctl->h[p0 + tid];
        const float qmin = key_to_float(h->kmin), qmax = key_to_float(h->kmax);
        ctl->factor[p0 + tid] = __fdiv_rn(255.0f, qmax - qmin);
        h->range = __fdiv_rn(qmax - qmin, 255.0f);
        h->sum_min = (float)nseg * qmin;
      }
      // the remainder rows while the f32 table is live: terms in byte order from +0.0
      for (int it = tid; it < nsb * nrem; it += 256) {
        const int pl = it / nrem, rr = it - pl * nrem;
        const uint32_t row = np + (uint32_t)rr;
        remk[(p0 + pl) * RQPM_REM + rr] = order_key(rq_row_distance(a.codes + (int64_t)row * cb, cb, RQ_REMAINDER, tables + pl * 4 * d, nullptr,
                                                                    &ctl->h[p0 + pl], a.sqrt_d, a.add[row], a.scale[row]));
      }
      __syncthreads();
      for (int idx = tid; idx < nsb * 4 * d; idx += 256) {
        const int pl = idx / (4 * d), i = idx - pl * 4 * d;
        const RqQuery *h = &ctl->h[p0 + pl];
        const float qmin = key_to_float(h->kmin), qmax = key_to_float(h->kmax);
        uint8_t e = 0;                                  // qmin == qmax: "this happens if the query is all zeros"
        if (!(qmin == qmax)) {
          const float r = roundf((tables[idx] - qmin) * ctl->factor[p0 + pl]);      // f32::round: half away from zero
          e = !(r > 0.0f) ? (uint8_t)0 : (r >= 255.0f ? (uint8_t)255 : (uint8_t)(int)r);      // `as u8`: saturating, NaN -> 0
        }
        etabs[(p0 + pl) * ts + i] = e ^ (uint8_t)0x80;  // over the residual, which the rotation has consumed
      }
      __syncthreads();      // the f32 tables are read before the next sub-block, or the candidates, overwrite them
    }
    for (int it = tid; it < npairs * nrem; it += 256) {
      const int p = it / nrem, rr = it - p * nrem;
      ebuf[p * RQPM_CAP + rr] = ((uint64_t)remk[p * RQPM_REM + rr] << 32) | (np + (uint32_t)rr);
    }
    if (tid < npairs) ctl->cnt[tid] = nrem;
    __syncthreads();

    // ---- phase 2: the packed rows [r0, np), a tile of 128 at a time ----
    const int my_pair = ctl->pair[j];
    const RqQuery hq = ctl->h[j];
    const uint8_t *my_b = etabs + j * ts + 16 * g;
    uint64_t *my_e = ebuf + j * RQPM_CAP;
    const int bias = 32 * d;
    const bool wide = (cb & 15) == 0;
    const int cw = cb / 16;
    auto load16 = [&](uint32_t tile, int w) {
      const uint32_t row = tile + (uint32_t)(32 * wave + j);
      return row < np ? reinterpret_cast<const uint4 *>(a.codes + (int64_t)row * cb)[w] : make_uint4(0, 0, 0, 0);
    };
    uint4 nxt = wide && r0 < np ? load16(r0, 0) : make_uint4(0, 0, 0, 0);
    for (uint32_t base = r0; base < np; base += RQPM_TILE) {
      if (tid < RQPM_TILE) fadd[tid] = base + (uint32_t)tid < np ? a.add[base + (uint32_t)tid] : 0.0f;
      else fscale[tid - RQPM_TILE] = base + (uint32_t)(tid - RQPM_TILE) < np ? a.scale[base + (uint32_t)(tid - RQPM_TILE)] : 0.0f;
      const bool live = base + (uint32_t)(32 * wave) < np;      // (wave-uniform: np - r0 is a multiple of 32)
      rqpm_i32x16 acc;
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[v] = 0;
      if (live && wide) {
        for (int w = 0; w < cw; ++w) {
          const uint4 cur = nxt;
          if (w + 1 < cw) nxt = load16(base, w + 1);
          else if (base + RQPM_TILE < np) nxt = load16(base + RQPM_TILE, 0);
          const uint32_t ws[4] = {cur.x, cur.y, cur.z, cur.w};
          const uint8_t *bp = my_b + 512 * w;
#pragma unroll
          for (int u = 0; u < 16; ++u) {
            const uint32_t nib = (ws[u >> 2] >> (8 * (u & 3) + 4 * g)) & 15u;
            acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(rqpm_onehot(nib), *reinterpret_cast<const rqpm_i32x4 *>(bp + 32 * u), acc, 0, 0, 0);
          }
        }
      } else if (live) {
        const uint8_t *rp = a.codes + (int64_t)(base + (uint32_t)(32 * wave + j)) * cb;
        for (int b = 0; b < cb; ++b) {
          const uint32_t nib = ((uint32_t)rp[b] >> (4 * g)) & 15u;
          acc = __builtin_amdgcn_mfma_i32_32x32x32_i8(rqpm_onehot(nib), *reinterpret_cast<const rqpm_i32x4 *>(my_b + 32 * b), acc, 0, 0, 0);
        }
      }
      __syncthreads();      // the tile's factors are staged
      if (live && my_pair >= 0) {
        const uint32_t thr = ctl->thr[j];
#pragma unroll
        for (int v = 0; v < 16; ++v) {
          const int rl = wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * g;      // the accumulator's row of the 32 x 32 tile
          const uint32_t key = order_key(rq_packed_tail((uint32_t)(acc[v] + bias), &hq, a.sqrt_d, fadd[rl], fscale[rl]));
          if (key <= thr) {      // rows tied with the k-th key come in too: the sort decides by position and records the cut tie
            const int slot = atomicAdd(&ctl->cnt[j], 1);
            my_e[slot] = ((uint64_t)key << 32) | (base + (uint32_t)rl);
          }
        }
      }
      __syncthreads();
      // before a tile at most RQPM_CAP - RQPM_TILE entries are held (k <= 128 after a cut, 31 before the first), so its 128 rows always fit
      for (int u = 0; u < RQPM_QB / 4; ++u) {
        const int p = wave * (RQPM_QB / 4) + u;
        if (ctl->cnt[p] > RQPM_CAP - RQPM_TILE) cand_block_sort_truncate(ebuf + p * RQPM_CAP, ctl, p, k, lane);
      }
      __syncthreads();
    }
  }
  cand_block_write(a.w, ebuf, ctl, k, wave, lane);
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------------
struct RqPmScratch {
  uint32_t *pair_starts = nullptr, *pair_idx = nullptr, *item_start = nullptr;
  int4 *desc = nullptr;
  uint32_t max_items = 0;
};

// LANCE_HIP_NO_RQ_GROUPED, read once per process: every batch takes the pair-major scan (A/B runs)
static bool rqpm_switched_off() {
  static const bool off = getenv("LANCE_HIP_NO_RQ_GROUPED") != nullptr;
  return off;
}

// LANCE_HIP_RQ_GROUPED_G=<g>, read once per process: grouped from g pairs per partition on (the sweep that chose the default)
static int rqpm_forced_g() {
  static const int g = getenv("LANCE_HIP_RQ_GROUPED_G") ? std::max(0, atoi(getenv("LANCE_HIP_RQ_GROUPED_G"))) : -1;
  return g;
}

// the grouping's slots for chunks of at most `pairs` pairs: every partition's last block may be ragged, so pairs / 32 + nlist items bound the table
static int rqpm_scratch(lance_hip_ctx *ctx, size_t pairs, uint32_t nlist, RqPmScratch *s) {
  s->max_items = (uint32_t)(pairs / RQPM_QB + nlist + 1);
  s->pair_starts = ctx->scratch_t<uint32_t>("ivfrq.pm.pair_starts", (size_t)nlist + 1);
  s->pair_idx = ctx->scratch_t<uint32_t>("ivfrq.pm.pair_idx", pairs);
  s->item_start = ctx->scratch_t<uint32_t>("ivfrq.pm.item_start", (size_t)nlist + 1);
  s->desc = ctx->scratch_t<int4>("ivfrq.pm.desc", s->max_items);
  return s->pair_starts && s->pair_idx && s->item_start && s->desc ? LANCE_HIP_OK : LANCE_HIP_ENOMEM;
}

// the scan stage of one chunk of nqc queries: group the pairs (a.w.probes) by partition, cut them into blocks, scan.  Every pair's list is
// written at its own index, so the merge does not notice the reordering.
static int rqpm_scan(lance_hip_ctx *ctx, const RqArgs &a, uint32_t nqc, uint32_t nlist, const RqPmScratch &s) {
  const int64_t pairs = (int64_t)nqc * a.w.nprobes;
  {
    ScopedTimer t(ctx, "ivfrq_pm_group");
    LH_TRY(stable_group(ctx, a.w.probes, pairs, pairs, (int)nlist, 1, s.pair_starts, s.pair_idx, pairs, nullptr));
    LH_TRY(qscan_items(ctx, s.pair_starts, (int)nlist, RQPM_QB, s.item_start, s.desc, s.max_items));
  }
  {
    ScopedTimer t(ctx, "ivfrq_pm_scan");
    hipLaunchKernelGGL(ivfrq_pm_scan_kernel, dim3(s.max_items), dim3(256), rqpm_lds_bytes((uint32_t)a.d), ctx->stream, a, s.pair_idx, s.desc);
  }
  LH_CHECK_HIP(hipGetLastError());
  return LANCE_HIP_OK;
}

}  // namespace lh
