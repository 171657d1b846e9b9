// pair_cand.cuh -- the candidate path of IVF_SQ / IVF_RQ searches: the FlatIndex sub-index of a probed partition keeps its keff best rows
// (keff = k, or k * refine_factor under a refine_factor: knn.rs:642, scanner.rs:2884-2904), up to CAND_MAX_K.  Written once, run at two
// capacities: keff <= CAND_NARROW_K in small buffers (a plain search, and most refined ones), larger keff in the largest that fit.
//   scan    one workgroup per (query, probed partition): the keff best (key, storage position) of the pair and the cut-tie flag.  The
//           candidate buffer's capacity `cap` is a launch parameter (a power of two, >= keff + 256; cand_scan_cap); it is sorted and cut to
//           keff once more than cap - 256 entries are held, i.e. when the next 256-row chunk might not fit.
//   merge   per query SortExec(dist, rowid).fetch(keff) over its pairs' lists (scanner.rs:3440-3468) and the replay decision: a pair is
//           ambiguous when a row tied with its keff-th key had to be left out, a query is flagged when an ambiguous pair's keff-th key is
//           not above the keff-th key of the merged candidates.  Two instances, by the buffer the keff kept entries and a round of new ones
//           need: <CAND_MERGE_NARROW, CAND_NARROW_K> and <CAND_MERGE_WIDE, CAND_MAX_K>.
//   replay  flagged queries through std BinaryHeap's push / pop in storage order, a heap of keff per partition
// The row distance is the caller's (sq.hip: sq_row_xq / sq_sum / sq_finish; rq.hip: rq_prepare / rq_row_distance), handed in as a callable.
//
// A capacity cannot change a result: the threshold only falls, so every row whose key equals the pair's final keff-th key is admitted; such
// a row is cut only at a truncation whose keff-th key is that same key, and that truncation records it.  Hence the cut-tie flag is set
// exactly when more than keff allowed rows have a key <= the final keff-th key, and the kept list is the keff smallest by (key, position),
// whenever the buffer happened to be sorted.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>

#include "common.h"
#include "exact.cuh"
#include "index.h"
#include "kernels.h"
#include "search_common.cuh"

namespace lh {

// ---- pair candidates: device code ----------------------------------------------------------------------------------------------
constexpr int CAND_MAX_K = 768;          // LANCE_HIP_SQRQ_MAX_CANDIDATES: 768 kept + one 256-row chunk = 1024, the smallest wide buffer
constexpr int CAND_NARROW_K = 128;       // the largest keff of the narrow capacity: 128 kept + one 256-row chunk, padded to 512
constexpr int CAND_CHUNK = 256;          // rows per step of the scan = threads of its workgroup

struct CandLists {
  const uint64_t *row_ids;       // [n] by storage position
  const uint32_t *part_offsets;  // [nlist+1]
  const uint32_t *probes;        // [nq][nprobes]
  const uint32_t *allow;         // prefilter: one bit per storage position, NULL = none
  int nprobes, k, cap;           // k = keff; cap = entries of the scan's candidate buffer
  uint32_t *pkey, *ppos;         // [nq * nprobes][k] the k best of every pair, sorted by (key, position)
  uint32_t *pcnt;                // [nq * nprobes] entries of the pair
  uint32_t *pamb;                // [nq * nprobes] 1 = a row tied with the pair's k-th key was left out
  uint32_t *flags;               // [nq] 1 = replay
  uint32_t *n_replay;            // [1] number of replayed queries of the call
};

struct CandCtl { int cnt; uint32_t thr; uint32_t amb_key; int amb; };

// ascending bitonic sort of P (a power of two) packed (key << 32 | position) entries in LDS, 256 threads
__device__ __forceinline__ void cand_sort_u64(uint64_t *e, int P) {
  for (int k2 = 2; k2 <= P; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = threadIdx.x; i < P / 2; i += 256) {
        const int ix = 2 * j * (i / j) + (i % j);
        const int px = ix + j;
        const bool up = (ix & k2) == 0;
        const uint64_t a = e[ix], b = e[px];
        if ((a > b) == up) { e[ix] = b; e[px] = a; }
      }
      __syncthreads();
    }
  }
}

// sort the buffer, keep the k best; a tie cut at the k-th key is remembered (thresholds only fall, so only the last one can matter)
__device__ __forceinline__ void cand_sort_truncate(uint64_t *e, CandCtl *ctl, int k) {
  const int cnt = ctl->cnt;
  int P = 2;
  while (P < cnt) P <<= 1;
  for (int i = cnt + threadIdx.x; i < P; i += 256) e[i] = ~0ull;
  __syncthreads();
  cand_sort_u64(e, P);
  if (threadIdx.x == 0 && cnt > k) {
    const uint32_t kth = (uint32_t)(e[k - 1] >> 32);
    if ((uint32_t)(e[k] >> 32) == kth) { ctl->amb = 1; ctl->amb_key = kth; }
    ctl->thr = kth;
    ctl->cnt = k;
  }
  __syncthreads();
}

// rows [r0, r1) of one pair through the buffer e [w.cap] (256 threads; *ctl initialised and a barrier passed); row_key(row) -> order key.
// Before a chunk at most cap - 256 entries are held (k <= cap - 256 after a cut), so its 256 rows always fit.
template <class RowKey>
__device__ __forceinline__ void cand_scan_pair(const CandLists &w, int pair, uint32_t r0, uint32_t r1, uint64_t *e, CandCtl *ctl, RowKey row_key) {
  const int k = w.k, room = w.cap - CAND_CHUNK;
  for (uint32_t base = r0; base < r1; base += CAND_CHUNK) {
    const uint32_t row = base + threadIdx.x;
    if (row < r1 && row_allowed(w.allow, row)) {
      const uint32_t key = row_key(row);
      if (key <= ctl->thr) {        // rows tied with the k-th key come in too: the sort decides by position and records the cut tie
        const int slot = atomicAdd(&ctl->cnt, 1);
        e[slot] = ((uint64_t)key << 32) | row;
      }
    }
    __syncthreads();
    const int filled = ctl->cnt;
    __syncthreads();               // every wave has read the same count before the next chunk adds to it
    if (filled > room) cand_sort_truncate(e, ctl, k);
  }
  if (ctl->cnt > 0) cand_sort_truncate(e, ctl, k);
  const int got = min(ctl->cnt, k);
  for (int i = threadIdx.x; i < got; i += 256) {
    w.pkey[(int64_t)pair * k + i] = (uint32_t)(e[i] >> 32);
    w.ppos[(int64_t)pair * k + i] = (uint32_t)e[i];
  }
  if (threadIdx.x == 0) {
    w.pcnt[pair] = (uint32_t)got;
    w.pamb[pair] = (got == k && ctl->amb && ctl->amb_key == (uint32_t)(e[k - 1] >> 32)) ? 1u : 0u;
  }
}

// per query: SortExec(dist, rowid).fetch(k) over the candidates of its pairs, then the replay decision.  MBUF entries hold the k <= KMAX
// kept ones and a round of MBUF - KMAX new ones.  Dynamic LDS: cand_merge_bytes(MBUF).
template <int MBUF, int KMAX>
__global__ __launch_bounds__(256) void cand_merge_kernel(CandLists w, uint64_t *__restrict__ out_ids, float *__restrict__ out_dists) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint64_t *rid = reinterpret_cast<uint64_t *>(smem);          // [MBUF]
  uint32_t *key = reinterpret_cast<uint32_t *>(rid + MBUF);    // [MBUF]
  uint32_t *pos = key + MBUF;                                  // [MBUF]
  int *ctl = reinterpret_cast<int *>(pos + MBUF);              // [0] entries kept, [1] real entries of this round, [2] replay
  const int q = blockIdx.x, k = w.k;
  const int total = w.nprobes * k;
  constexpr int ROUND = MBUF - KMAX;
  if (threadIdx.x == 0) { ctl[0] = 0; ctl[1] = 0; ctl[2] = 0; }
  __syncthreads();
  for (int c0 = 0; c0 < total; c0 += ROUND) {
    const int kept = ctl[0];
    const int span = min(ROUND, total - c0);
    int P = 2;
    while (P < kept + span) P <<= 1;
    __syncthreads();
    for (int j = threadIdx.x; j < P - kept; j += 256) {
      const int c = c0 + j;
      uint32_t kk = 0xFFFFFFFFu, pp = 0xFFFFFFFFu;
      uint64_t rr = ~0ull;
      if (j < span) {
        const int pair = q * w.nprobes + c / k, i = c % k;
        if ((uint32_t)i < w.pcnt[pair]) {
          kk = w.pkey[(int64_t)pair * k + i]; pp = w.ppos[(int64_t)pair * k + i]; rr = w.row_ids[pp];
          atomicAdd(&ctl[1], 1);
        }
      }
      key[kept + j] = kk; pos[kept + j] = pp; rid[kept + j] = rr;
    }
    __syncthreads();
    bitonic_sort_kr<256>(key, rid, pos, P);
    if (threadIdx.x == 0) { ctl[0] = min(kept + ctl[1], k); ctl[1] = 0; }
    __syncthreads();
  }
  const int got = ctl[0];
  // an ambiguous pair matters when rows at its k-th key may be part of the answer: k-th key not above the merged k-th key
  if (got == k) {
    const uint32_t mk = key[k - 1];
    for (int p = threadIdx.x; p < w.nprobes; p += 256) {
      const int pair = q * w.nprobes + p;
      if (w.pamb[pair] && w.pkey[(int64_t)pair * k + k - 1] <= mk) ctl[2] = 1;
    }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    w.flags[q] = (uint32_t)ctl[2];
    if (ctl[2]) atomicAdd(w.n_replay, 1u);
  }
  for (int i = threadIdx.x; i < k; i += 256) {
    out_ids[(int64_t)q * k + i] = i < got ? rid[i] : ~0ull;
    out_dists[(int64_t)q * k + i] = i < got ? key_to_float(key[i]) : INFINITY;
  }
}

// Exact replay of one flagged query by ONE wave: every probed partition through a max-heap of k with std BinaryHeap semantics (push while
// len < k, else replace the root only if root.dist > dist), rows in storage order; distances by all 64 lanes, a ballot drops rows that
// cannot enter, lane 0 replays the rest; partition heaps are merged by (dist, rowid).  `area`: 8-byte aligned LDS of
// cand_replay_bytes(k) bytes: trid u64 [k] | tkey [k] | hk [k + 4] | hp [k + 4] | skey [64] | 4 ints.
// dist.partition(pi, part) prepares a partition (every lane calls it; it may use barriers), dist.key(off, row, np) is the order key of
// row `row` of the np rows stored from position `off`.
template <class Dist>
__device__ __forceinline__ void cand_replay_query(const CandLists &w, int qi, char *area, Dist &dist, uint64_t *__restrict__ out_ids,
                                                  float *__restrict__ out_dists) {
  const int lane = threadIdx.x, k = w.k;
  uint64_t *trid = reinterpret_cast<uint64_t *>(area);            // [k]
  uint32_t *tkey = reinterpret_cast<uint32_t *>(trid + k);        // [k]
  uint32_t *hk = tkey + k;                                        // [k + 4]
  uint32_t *hp = hk + k + 4;                                      // [k + 4]
  uint32_t *skey = hp + k + 4;                                    // [64]
  int *ctl = reinterpret_cast<int *>(skey + 64);                  // [0] heap length, [1] merged entries
  if (lane == 0) { ctl[0] = 0; ctl[1] = 0; }
  __syncthreads();
  for (int pi = 0; pi < w.nprobes; ++pi) {
    const uint32_t part = w.probes[(int64_t)qi * w.nprobes + pi];
    const uint32_t off = w.part_offsets[part];
    const int np = (int)(w.part_offsets[part + 1] - off);
    if (np == 0) continue;
    dist.partition(pi, part);
    if (lane == 0) ctl[0] = 0;
    __syncthreads();
    for (int base = 0; base < np; base += 64) {
      const int row = base + lane;
      uint32_t key = 0xFFFFFFFFu;
      bool cand = false;
      if (row < np && row_allowed(w.allow, off + (uint32_t)row)) {
        key = dist.key(off, row, np);
        cand = ctl[0] < k || key < hk[0];
      }
      const uint64_t mask = __ballot(cand);
      skey[lane] = key;
      __syncthreads();
      if (lane == 0 && mask) {
        int hl = ctl[0];
        uint64_t mm = mask;
        while (mm) {
          const int b = __ffsll((long long)mm) - 1;
          mm &= mm - 1;
          const uint32_t kk = skey[b];
          if (hl < k) {
            heap_push(hk, hp, hl, kk, off + (uint32_t)(base + b));
          } else if (hk[0] > kk) {
            heap_pop(hk, hp, hl);
            heap_push(hk, hp, hl, kk, off + (uint32_t)(base + b));
          }
        }
        ctl[0] = hl;
      }
      __syncthreads();
    }
    if (lane == 0) {
      int tc = ctl[1];
      for (int i = 0; i < ctl[0]; ++i) {
        const uint32_t kk = hk[i];
        const uint64_t rr = w.row_ids[hp[i]];
        if (tc == k) {
          const uint32_t wk = tkey[tc - 1];
          const uint64_t wr = trid[tc - 1];
          if (!(kk < wk || (kk == wk && rr < wr))) continue;
        }
        int pos = tc < k ? tc : k - 1;
        while (pos > 0) {
          const uint32_t pk = tkey[pos - 1];
          const uint64_t pr = trid[pos - 1];
          if (pk < kk || (pk == kk && pr < rr)) break;
          tkey[pos] = pk; trid[pos] = pr;
          --pos;
        }
        tkey[pos] = kk; trid[pos] = rr;
        if (tc < k) ++tc;
      }
      ctl[1] = tc;
    }
    __syncthreads();
  }
  const int got = ctl[1];
  for (int i = lane; i < k; i += 64) {
    out_ids[(int64_t)qi * k + i] = i < got ? trid[i] : ~0ull;
    out_dists[(int64_t)qi * k + i] = i < got ? key_to_float(tkey[i]) : INFINITY;
  }
}

// ---- pair candidates: launch sizes (plain host functions: the library and the CPU emulator programs size their launches by them) -----
constexpr int CAND_MERGE_NARROW = 512;   // merge buffer up to CAND_NARROW_K: a round of 384 new entries
constexpr int CAND_MERGE_WIDE = 2048;    // ... up to CAND_MAX_K: a round of 1280
static_assert(CAND_NARROW_K + CAND_CHUNK <= 512 && CAND_MAX_K + CAND_CHUNK <= 1024, "kept entries and one chunk fit the smallest buffers");

static inline size_t cand_merge_bytes(int mbuf) { return (size_t)mbuf * 16 + 16; }
// cand_replay_query's `area`
static inline size_t cand_replay_bytes(int k) { return (size_t)k * 12 + (size_t)(k + 4) * 8 + 64 * 4 + 16; }
// Entries of the scan's buffer.  k <= CAND_NARROW_K: 512, doubled until the `borrow` bytes a kernel parks in the buffer before the scan fit
// (IVF_RQ's rotated query, 4 d bytes: 1024 entries past d = 1024); the footprint stays small, many workgroups share a CU.  Above: the
// largest power of two whose 8-byte entries fit beside `fixed` bytes in 64 KiB of dynamic LDS -- the fewer sorts, the better.
static inline int cand_scan_cap(int k, size_t fixed, size_t borrow = 0) {
  int cap = k <= CAND_NARROW_K ? 512 : 1024;
  while (k <= CAND_NARROW_K ? (size_t)cap * 8 < borrow : fixed + (size_t)cap * 16 <= 65536) cap <<= 1;
  return cap;
}
// ---- pair candidates: end of the code the emulator programs compile -----------------------------------------------------------------

// ---- host side: one search, around the scan and the replay launch of the index type ---------------------------------------------------
// timers [0]: keff <= CAND_NARROW_K, [1]: above -- the name says which capacity class ran.  String literals: a captured call keeps the pointers.
struct CandNames {
  const char *slots;             // prefix of the scratch slots ("ivfsq")
  const char *scan[2], *merge[2], *exact[2];
};

// sq.hip: the merge launch (one instantiation of each merge instance in the library), picked by w.k
int cand_merge_lists(lance_hip_ctx *ctx, const CandLists &w, uint32_t nq, uint64_t *ids, float *dists, const char *timer);

// w: the index's lists, the prefilter, nprobes, k = keff and cap; probes [nq][nprobes].  scan(w, q0, nqc) and replay(w, q0, nqc, ids, dists)
// enqueue the index type's kernels for queries [q0, q0 + nqc): w.probes / w.flags start at q0, the outputs are that chunk's.
// refine: the keff best are candidates in the scratch arena, re-scored against the raw vectors with q_orig (launch_refine: flat_knn's
// arithmetic) into ids / dists [nq][kout]; otherwise they are the answer.
template <class Scan, class Replay>
static int cand_search(lance_hip_ctx *ctx, const lance_hip_index *idx, const CandNames &nm, CandLists w, const uint32_t *probes, uint32_t nq,
                       uint32_t kout, bool refine, const float *q_orig, uint64_t *ids, float *dists, Scan scan, Replay replay) {
  const uint32_t k = (uint32_t)w.k, nprobes = (uint32_t)w.nprobes;
  const int wide = k > (uint32_t)CAND_NARROW_K;
  auto slot = [&](const char *what) { return std::string(nm.slots) + what; };
  // queries per launch: the per-pair candidate lists stay within 2^24 entries
  const uint32_t qch = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(nq, (1ull << 24) / ((uint64_t)nprobes * k)));
  const size_t pairs = (size_t)qch * nprobes;
  w.pkey = ctx->scratch_t<uint32_t>(slot(".pkey").c_str(), pairs * k);
  w.ppos = ctx->scratch_t<uint32_t>(slot(".ppos").c_str(), pairs * k);
  w.pcnt = ctx->scratch_t<uint32_t>(slot(".pcnt").c_str(), pairs);
  w.pamb = ctx->scratch_t<uint32_t>(slot(".pamb").c_str(), pairs);
  uint32_t *flags = ctx->scratch_t<uint32_t>(slot(".flags").c_str(), (size_t)nq + 1);
  if (!w.pkey || !w.ppos || !w.pcnt || !w.pamb || !flags) return LANCE_HIP_ENOMEM;
  uint64_t *cand = nullptr;
  float *cand_d = nullptr;
  uint32_t *cand_cnt = nullptr, *rflags = nullptr;
  if (refine) {
    cand = ctx->scratch_t<uint64_t>(slot(".cand").c_str(), (size_t)nq * k);
    cand_d = ctx->scratch_t<float>(slot(".cand_d").c_str(), (size_t)nq * k);
    cand_cnt = ctx->scratch_t<uint32_t>(slot(".cand_cnt").c_str(), (size_t)nq);
    rflags = ctx->scratch_t<uint32_t>(slot(".rflags").c_str(), (size_t)nq);
    if (!cand || !cand_d || !cand_cnt || !rflags) return LANCE_HIP_ENOMEM;
    LH_CHECK_HIP(lh::memset_async(rflags, 0, (size_t)nq * 4, ctx->stream));
  }
  LH_CHECK_HIP(lh::memset_async(flags, 0, ((size_t)nq + 1) * 4, ctx->stream));
  w.n_replay = flags + nq;
  ctx->last_replay_counter = w.n_replay;
  for (uint32_t q0 = 0; q0 < nq; q0 += qch) {
    const uint32_t nqc = std::min(qch, nq - q0);
    w.probes = probes + (size_t)q0 * nprobes; w.flags = flags + q0;
    uint64_t *oid = (refine ? cand : ids) + (size_t)q0 * k;
    float *od = (refine ? cand_d : dists) + (size_t)q0 * k;
    {
      ScopedTimer t(ctx, nm.scan[wide]);
      scan(w, q0, nqc);
    }
    LH_TRY(cand_merge_lists(ctx, w, nqc, oid, od, nm.merge[wide]));
    {
      ScopedTimer t(ctx, nm.exact[wide]);
      replay(w, q0, nqc, oid, od);
    }
  }
  LH_CHECK_HIP(hipGetLastError());
  if (refine) {
    LH_TRY(launch_cand_count(ctx, cand, nq, k, cand_cnt));
    LH_TRY(launch_refine(ctx, idx, q_orig, nq, (int)idx->d, cand, cand_cnt, k, kout, ids, dists, rflags, nullptr));
    return check_flags(ctx, rflags, nq);      // synchronises; a stored row id beyond the raw vectors is an error, not a rank
  }
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return LANCE_HIP_OK;
}

}  // namespace lh
