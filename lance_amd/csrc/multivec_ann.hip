// multivec_ann.hip -- ANN search of a MULTIVECTOR column: the per-query-vector candidate lists of an index over the flattened
// vectors, joined by row id and scored with XTR-style imputation.
//
//   Scanner::multivec_ann        lance/src/dataset/scanner.rs:3471-3552   one ANN search per query vector, k = k * overfetch
//   MultivectorScoringExec       lance/src/io/exec/knn.rs:1132-1329       per list: min_sim, first occurrence per row id; the join
//
// The contract (include/lance_hip.h, tests/multivec_ann_spec.py).  For a query of nqv vectors, list j = the candidates of query
// vector j in (dist, rowid) order, every operation one f32 rounding, lists taken in order j = 0 .. nqv - 1:
//   min_sim_j = 1 - (dist of the last entry), 0 for an empty list          sim_j(r) = 1 - dist of r's FIRST entry in list j
//   missed_j  = ((0 + min_sim_0) + min_sim_1) + ... + min_sim_{j-1}
//   s(r)      = sim_{j0}(r) + missed_{j0} (j0 = r's first list), then s += (r in list j ? sim_j(r) : min_sim_j) for j = j0 + 1 ..
//   distance  = (float)nqv - s
//
// Three kernels, no atomics but an LDS counter and one output cursor per query:
//   mva_sort_kernel    one workgroup per list: a copy of the list sorted by (row id, position) in LDS (12 bytes per entry, 48 KiB at
//                      keff = 4096), written out as (row id, sim); the FIRST entry of a run of equal ids is the row's first occurrence
//                      in list order, and a lower-bound search lands on it.  Also the list's length and min_sim.
//   mva_score_kernel   one workgroup per list j0: a lane per first occurrence (j0, r).  r found in a list < j0: that list owns the row,
//                      drop.  Otherwise the sequential loop over j0 + 1 .. nqv - 1, one binary search per list, and (key, row id) is
//                      appended at the query's cursor.  Every row is emitted once; their order in memory is arbitrary, the selection's
//                      (key, row id) order is total.
//   mva_select_kernel  multivec.hip's selection with a batch dimension: blocks of 2048 candidates are sorted in LDS and keep their
//                      k_out best, repeated until one block is left.
#include <algorithm>
#include <vector>

#include "common.h"
#include "exact.cuh"
#include "index.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace lh {

// ---- multivector ANN: device code
constexpr int MVA_THREADS = 256;
constexpr int MVA_MAX_NQV = 256;          // LANCE_HIP_MULTIVEC_MAX_QUERY_VECTORS
constexpr int MVA_MAX_KEFF = 4096;        // LANCE_HIP_MULTIVEC_ANN_MAX_KEFF
constexpr int MVA_SEL = 2048;             // candidates one selection block sorts; k_out <= MVA_SEL / 2
constexpr uint64_t MVA_NONE = ~0ull;

extern __shared__ __attribute__((aligned(16))) char smem[];

struct MvaArgs {
  const uint64_t *cand_ids;      // [lists][keff] valid entries first, then MVA_NONE
  const float *cand_dists;       // [lists][keff]
  int keff;
  int P;                         // the power of two >= keff
  uint64_t *srid;                // [lists][keff] the list's row ids sorted by (row id, position); MVA_NONE behind the valid ones
  float *ssim;                   // [lists][keff] 1 - dist, aligned with srid
  uint32_t *ln;                  // [lists] valid entries
  float *lmin;                   // [lists] min_sim
  const uint32_t *list_query;    // [lists] the multivector query a list belongs to
  const uint32_t *q_first;       // [B + 1] first list of every query
  uint32_t *cursor;              // [B] rows emitted (zeroed)
  uint32_t *out_key;             // [lists * keff] query b's rows start at q_first[b] * keff
  uint64_t *out_rid;
};

// index of the first entry of rid[0 .. n) equal to r, or -1
__device__ __forceinline__ int mva_find(const uint64_t *__restrict__ rid, uint32_t n, uint64_t r) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (rid[mid] < r) lo = mid + 1;
    else hi = mid;
  }
  return lo < n && rid[lo] == r ? (int)lo : -1;
}

// dynamic LDS: P * 12 + 16 bytes
__global__ __launch_bounds__(MVA_THREADS) void mva_sort_kernel(MvaArgs a) {
  uint64_t *rid = reinterpret_cast<uint64_t *>(smem);                            // [P]
  uint32_t *pos = reinterpret_cast<uint32_t *>(smem + (size_t)a.P * 8);          // [P]
  uint32_t *cnt = pos + a.P;                                                     // [1]
  const int t = threadIdx.x;
  const size_t base = (size_t)blockIdx.x * a.keff;
  const uint64_t *ids = a.cand_ids + base;
  const float *ds = a.cand_dists + base;
  if (t == 0) *cnt = 0u;
  __syncthreads();
  uint32_t mine = 0;
  for (int i = t; i < a.P; i += MVA_THREADS) {
    const uint64_t r = i < a.keff ? ids[i] : MVA_NONE;
    rid[i] = r; pos[i] = (uint32_t)i;
    mine += r != MVA_NONE ? 1u : 0u;
  }
  if (mine) atomicAdd(cnt, mine);
  __syncthreads();
  for (int k2 = 2; k2 <= a.P; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = t; i < a.P / 2; i += MVA_THREADS) {
        const int ix = 2 * j * (i / j) + (i % j);
        const int px = ix + j;
        const bool up = (ix & k2) == 0;
        const uint64_t rx = rid[ix], ry = rid[px];
        const uint32_t ox = pos[ix], oy = pos[px];
        const bool gt = rx > ry || (rx == ry && ox > oy);
        if (gt == up) { rid[ix] = ry; rid[px] = rx; pos[ix] = oy; pos[px] = ox; }
      }
      __syncthreads();
    }
  }
  const uint32_t n = *cnt;
  for (int i = t; i < a.keff; i += MVA_THREADS) {
    const uint64_t r = rid[i];
    a.srid[base + i] = r;
    a.ssim[base + i] = r != MVA_NONE ? 1.0f - ds[pos[i]] : 0.0f;
  }
  if (t == 0) {
    a.ln[blockIdx.x] = n;
    a.lmin[blockIdx.x] = n ? 1.0f - ds[n - 1] : 0.0f;
  }
}

// dynamic LDS: MVA_MAX_NQV * 8 + 16 bytes
__global__ __launch_bounds__(MVA_THREADS) void mva_score_kernel(MvaArgs a) {
  float *msim = reinterpret_cast<float *>(smem);                                 // [MVA_MAX_NQV] min_sim of the query's lists
  uint32_t *cn = reinterpret_cast<uint32_t *>(smem + (size_t)MVA_MAX_NQV * 4);   // [MVA_MAX_NQV] their lengths
  float *missed = reinterpret_cast<float *>(smem + (size_t)MVA_MAX_NQV * 8);     // [1]
  const int t = threadIdx.x;
  const uint32_t l = blockIdx.x;
  const uint32_t b = a.list_query[l];
  const uint32_t l0 = a.q_first[b], nqv = a.q_first[b + 1] - l0, j0 = l - l0;
  for (uint32_t j = t; j < nqv; j += MVA_THREADS) { msim[j] = a.lmin[l0 + j]; cn[j] = a.ln[l0 + j]; }
  __syncthreads();
  if (t == 0) {
    float m = 0.0f;
    for (uint32_t j = 0; j < j0; ++j) m = m + msim[j];
    *missed = m;
  }
  __syncthreads();
  const float ms = *missed;
  const uint32_t n = cn[j0];
  const size_t keff = (size_t)a.keff;
  const uint64_t *mr = a.srid + (size_t)l * keff;
  const float *msi = a.ssim + (size_t)l * keff;
  const size_t obase = (size_t)l0 * keff, ocap = (size_t)nqv * keff;
  for (uint32_t i = t; i < n; i += MVA_THREADS) {
    const uint64_t r = mr[i];
    if (i > 0 && mr[i - 1] == r) continue;                     // not the row's first entry in this list
    bool owned = false;
    for (uint32_t j = 0; j < j0 && !owned; ++j) owned = mva_find(a.srid + (size_t)(l0 + j) * keff, cn[j], r) >= 0;
    if (owned) continue;                                       // an earlier list emits the row
    float s = msi[i] + ms;
    for (uint32_t j = j0 + 1; j < nqv; ++j) {
      const int f = mva_find(a.srid + (size_t)(l0 + j) * keff, cn[j], r);
      s = s + (f >= 0 ? a.ssim[(size_t)(l0 + j) * keff + f] : msim[j]);
    }
    const float dist = (float)nqv - s;
    const uint32_t at = atomicAdd(a.cursor + b, 1u);
    if (at < ocap) { a.out_key[obase + at] = order_key(dist); a.out_rid[obase + at] = r; }
  }
}

struct MvaSel {
  const uint32_t *in_key;
  const uint64_t *in_rid;
  const uint32_t *q_first;       // first round: query b's candidates start at q_first[b] * keff and cnt[b] of them are valid
  const uint32_t *cnt;
  int keff;
  uint64_t in_stride, n_in;      // later rounds: query b's candidates are in_key[b * in_stride .. + n_in)
  int k;
  uint32_t *out_key;             // [B][gridDim.x * k], or NULL in the last round
  uint64_t *out_rid;
  uint64_t *ids;                 // [B][k] the last round's output
  float *dists;
};

// One block sorts MVA_SEL candidates of query blockIdx.y by (key, row id) and keeps the k best.  dynamic LDS: MVA_SEL * 12 bytes
__global__ __launch_bounds__(MVA_THREADS) void mva_select_kernel(MvaSel p) {
  uint64_t *rid = reinterpret_cast<uint64_t *>(smem);                            // [MVA_SEL]
  uint32_t *key = reinterpret_cast<uint32_t *>(smem + (size_t)MVA_SEL * 8);      // [MVA_SEL]
  const int t = threadIdx.x;
  const uint32_t b = blockIdx.y;
  const uint64_t src = p.q_first ? (uint64_t)p.q_first[b] * (uint64_t)p.keff : (uint64_t)b * p.in_stride;
  uint64_t n = p.n_in;
  if (p.q_first) {
    const uint64_t cap = (uint64_t)(p.q_first[b + 1] - p.q_first[b]) * (uint64_t)p.keff;
    n = p.cnt[b] < cap ? p.cnt[b] : cap;
  }
  const uint64_t first = (uint64_t)blockIdx.x * MVA_SEL;
  for (int i = t; i < MVA_SEL; i += MVA_THREADS) {
    const uint64_t g = first + i;
    uint32_t kk = 0xFFFFFFFFu;
    uint64_t rr = MVA_NONE;
    if (g < n) { kk = p.in_key[src + g]; rr = p.in_rid[src + g]; }
    key[i] = kk; rid[i] = rr;
  }
  __syncthreads();
  for (int k2 = 2; k2 <= MVA_SEL; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = t; i < MVA_SEL / 2; i += MVA_THREADS) {
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
  for (int i = t; i < p.k; i += MVA_THREADS) {
    if (p.ids) {
      p.ids[(uint64_t)b * p.k + i] = rid[i];
      p.dists[(uint64_t)b * p.k + i] = rid[i] != MVA_NONE ? key_to_float(key[i]) : __uint_as_float(0x7F800000u);
    } else {
      const uint64_t o = ((uint64_t)b * gridDim.x + blockIdx.x) * p.k + i;
      p.out_key[o] = key[i];
      p.out_rid[o] = rid[i];
    }
  }
}
// ---- multivector ANN: host side

static_assert(MVA_MAX_NQV == LANCE_HIP_MULTIVEC_MAX_QUERY_VECTORS && MVA_MAX_KEFF == LANCE_HIP_MULTIVEC_ANN_MAX_KEFF &&
              MVA_SEL / 2 == LANCE_HIP_MULTIVEC_ANN_MAX_K_OUT, "the kernels' constants are the header's limits");

// the queries of a batch: q_offsets [B + 1] (host) -> the number of lists; every limit on nqv is checked here
static int mva_check_queries(const char *what, const uint64_t *q_offsets, uint32_t B, uint64_t *lists_out) {
  LH_REQUIRE(q_offsets[0] == 0, "%s: q_offsets must start at 0, got %llu", what, (unsigned long long)q_offsets[0]);
  for (uint32_t b = 0; b < B; ++b) {
    LH_REQUIRE(q_offsets[b + 1] >= q_offsets[b], "%s: q_offsets decrease at query %u", what, b);
    const uint64_t nqv = q_offsets[b + 1] - q_offsets[b];
    LH_REQUIRE(nqv >= 1 && nqv <= (uint64_t)MVA_MAX_NQV, "%s: query %u holds %llu vectors: a multivector query holds 1..%d vectors", what, b,
               (unsigned long long)nqv, MVA_MAX_NQV);
  }
  *lists_out = q_offsets[B];
  return LANCE_HIP_OK;
}

static int mva_check_sizes(const char *what, uint32_t keff, uint32_t k_out) {
  LH_REQUIRE(keff >= 1 && keff <= (uint32_t)MVA_MAX_KEFF, "%s: keff = k * overfetch = %u candidates per query vector not supported (1..%d)", what, keff,
             MVA_MAX_KEFF);
  LH_REQUIRE(k_out >= 1 && k_out <= (uint32_t)MVA_SEL / 2, "%s: k_out = k * refine_factor = %u not supported (1..%d)", what, k_out, MVA_SEL / 2);
  return LANCE_HIP_OK;
}

// enqueues sort, score and select on the context's stream (arguments checked by the callers)
static int mva_score_enqueue(lance_hip_ctx *ctx, const uint64_t *cand_ids, const float *cand_dists, const uint64_t *q_offsets, uint32_t B,
                             uint64_t lists, uint32_t keff, uint32_t k_out, uint64_t *ids, float *dists) {
  const size_t entries = (size_t)lists * keff;
  MvaArgs a;
  a.cand_ids = cand_ids; a.cand_dists = cand_dists; a.keff = (int)keff;
  a.P = 1;
  while ((uint32_t)a.P < keff) a.P <<= 1;
  a.srid = ctx->scratch_t<uint64_t>("mva.srid", entries);
  a.ssim = ctx->scratch_t<float>("mva.ssim", entries);
  a.ln = ctx->scratch_t<uint32_t>("mva.ln", lists);
  a.lmin = ctx->scratch_t<float>("mva.lmin", lists);
  uint32_t *lq = ctx->scratch_t<uint32_t>("mva.list_query", lists);
  uint32_t *qf = ctx->scratch_t<uint32_t>("mva.q_first", (size_t)B + 1);
  a.cursor = ctx->scratch_t<uint32_t>("mva.cursor", B);
  a.out_key = ctx->scratch_t<uint32_t>("mva.out_key", entries);
  a.out_rid = ctx->scratch_t<uint64_t>("mva.out_rid", entries);
  if (!a.srid || !a.ssim || !a.ln || !a.lmin || !lq || !qf || !a.cursor || !a.out_key || !a.out_rid) return LANCE_HIP_ENOMEM;
  a.list_query = lq; a.q_first = qf;
  std::vector<uint32_t> h(lists + B + 1);
  uint64_t max_nqv = 0;
  for (uint32_t b = 0; b < B; ++b) {
    for (uint64_t l = q_offsets[b]; l < q_offsets[b + 1]; ++l) h[l] = b;
    h[lists + b] = (uint32_t)q_offsets[b];
    max_nqv = std::max(max_nqv, q_offsets[b + 1] - q_offsets[b]);
  }
  h[lists + B] = (uint32_t)lists;
  // pageable source: the copies have left the vector when the calls return
  LH_CHECK_HIP(hipMemcpyAsync(lq, h.data(), (size_t)lists * 4, hipMemcpyHostToDevice, ctx->stream));
  LH_CHECK_HIP(hipMemcpyAsync(qf, h.data() + lists, ((size_t)B + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  LH_CHECK_HIP(lh::memset_async(a.cursor, 0, (size_t)B * 4, ctx->stream));
  {
    ScopedTimer t(ctx, "multivec_ann_sort");
    hipLaunchKernelGGL(mva_sort_kernel, dim3((unsigned)lists), dim3(MVA_THREADS), (size_t)a.P * 12 + 16, ctx->stream, a);
  }
  {
    ScopedTimer t(ctx, "multivec_ann_score");
    hipLaunchKernelGGL(mva_score_kernel, dim3((unsigned)lists), dim3(MVA_THREADS), (size_t)MVA_MAX_NQV * 8 + 16, ctx->stream, a);
  }
  LH_CHECK_HIP(hipGetLastError());
  // selection: every query is given the blocks of the longest one (blocks past a query's rows sort padding)
  uint64_t nb = std::max<uint64_t>(1, cdiv(max_nqv * keff, MVA_SEL));
  uint32_t *sk[2] = {nullptr, nullptr};
  uint64_t *sr[2] = {nullptr, nullptr};
  if (nb > 1) {
    const uint64_t nb1 = cdiv(nb * k_out, MVA_SEL);
    sk[0] = ctx->scratch_t<uint32_t>("mva.selk0", (size_t)B * nb * k_out);
    sr[0] = ctx->scratch_t<uint64_t>("mva.selr0", (size_t)B * nb * k_out);
    sk[1] = ctx->scratch_t<uint32_t>("mva.selk1", (size_t)B * nb1 * k_out);
    sr[1] = ctx->scratch_t<uint64_t>("mva.selr1", (size_t)B * nb1 * k_out);
    if (!sk[0] || !sr[0] || !sk[1] || !sr[1]) return LANCE_HIP_ENOMEM;
  }
  {
    ScopedTimer t(ctx, "multivec_ann_select");
    MvaSel s;
    s.in_key = a.out_key; s.in_rid = a.out_rid; s.q_first = qf; s.cnt = a.cursor; s.keff = (int)keff; s.in_stride = 0; s.n_in = 0; s.k = (int)k_out;
    int cur = -1;
    for (;;) {
      const bool last = nb == 1;
      const int nxt = cur == 0 ? 1 : 0;
      s.out_key = last ? nullptr : sk[nxt]; s.out_rid = last ? nullptr : sr[nxt];
      s.ids = last ? ids : nullptr; s.dists = last ? dists : nullptr;
      hipLaunchKernelGGL(mva_select_kernel, dim3((unsigned)nb, B), dim3(MVA_THREADS), (size_t)MVA_SEL * 12, ctx->stream, s);
      if (last) break;
      s.in_key = sk[nxt]; s.in_rid = sr[nxt]; s.q_first = nullptr; s.cnt = nullptr;
      s.in_stride = s.n_in = nb * k_out;
      nb = cdiv(nb * k_out, MVA_SEL);
      cur = nxt;
    }
  }
  LH_CHECK_HIP(hipGetLastError());
  return LANCE_HIP_OK;
}

}  // namespace lh

using namespace lh;

extern "C" int lance_hip_multivec_xtr_score(lance_hip_ctx *ctx, const uint64_t *cand_ids, const float *cand_dists, const uint64_t *q_offsets,
                                            uint32_t B, uint32_t keff, uint32_t k_out, uint64_t *ids, float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && q_offsets && (B == 0 || (cand_ids && cand_dists && ids && dists)), "multivec_xtr_score: NULL argument");
  LH_TRY(mva_check_sizes("multivec_xtr_score", keff, k_out));
  LH_REQUIRE(B <= 65535, "multivec_xtr_score: %u queries in one batch not supported (at most 65535)", B);
  uint64_t lists = 0;
  LH_TRY(mva_check_queries("multivec_xtr_score", q_offsets, B, &lists));
  if (B == 0) return LANCE_HIP_OK;
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  LH_TRY(mva_score_enqueue(ctx, cand_ids, cand_dists, q_offsets, B, lists, keff, k_out, ids, dists));
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return LANCE_HIP_OK;
}

extern "C" int lance_hip_ivfpq_multivec_search(lance_hip_ctx *ctx, const lance_hip_index *idx, const void *q, const uint64_t *q_offsets, uint32_t B,
                                               uint32_t k, uint32_t nprobes, uint32_t overfetch, uint32_t k_out, const uint8_t *allow_by_rowid,
                                               uint64_t n_allow, uint64_t *ids, float *dists) {
  lh::CtxLock _ctx_lock(ctx);
  LH_REQUIRE(ctx && idx && q_offsets && (B == 0 || (q && ids && dists)), "ivfpq_multivec_search: NULL argument");
  LH_REQUIRE(ctx->device == idx->device, "ivfpq_multivec_search: context and index live on different devices");
  LH_REQUIRE(idx->m != 0, "ivfpq_multivec_search: not an IVF_PQ index");
  LH_REQUIRE(idx->metric == LANCE_HIP_COSINE, "ivfpq_multivec_search: multivector type supports only cosine distance");
  LH_REQUIRE(k >= 1 && overfetch >= 1, "ivfpq_multivec_search: k=%u, overfetch=%u: both must be at least 1", k, overfetch);
  const uint64_t keff64 = (uint64_t)k * overfetch;
  LH_TRY(mva_check_sizes("ivfpq_multivec_search", (uint32_t)std::min<uint64_t>(keff64, 0xFFFFFFFFu), k_out));
  LH_REQUIRE(B <= 65535, "ivfpq_multivec_search: %u queries in one batch not supported (at most 65535)", B);
  LH_REQUIRE(allow_by_rowid || n_allow == 0, "ivfpq_multivec_search: NULL filter");
  uint64_t lists = 0;
  LH_TRY(mva_check_queries("ivfpq_multivec_search", q_offsets, B, &lists));
  if (B == 0) return LANCE_HIP_OK;
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  const uint32_t keff = (uint32_t)keff64;
  uint64_t *cid = ctx->scratch_t<uint64_t>("mva.cand_ids", (size_t)lists * keff);
  float *cds = ctx->scratch_t<float>("mva.cand_dists", (size_t)lists * keff);
  if (!cid || !cds) return LANCE_HIP_ENOMEM;
  // the existing search, unchanged: k = keff, no refine; slices keep its (query, probe) pairs within the batched kernels' scratch
  const size_t esz = idx->dtype == LANCE_HIP_F16 ? 2 : idx->dtype == LANCE_HIP_I8 ? 1 : 4;
  const uint64_t step = std::max<uint64_t>(1, 1500000 / std::max<uint32_t>(1, nprobes));
  {
    ScopedTimer search_timer(ctx, "multivec_ann_search");
    for (uint64_t l = 0; l < lists; l += step) {
      const uint32_t nq = (uint32_t)std::min<uint64_t>(step, lists - l);
      const void *qs = static_cast<const char *>(q) + (size_t)l * idx->d * esz;
      if (allow_by_rowid)
        LH_TRY(lance_hip_ivfpq_search_filtered(ctx, idx, qs, nq, keff, nprobes, 0, allow_by_rowid, n_allow, cid + (size_t)l * keff, cds + (size_t)l * keff));
      else
        LH_TRY(lance_hip_ivfpq_search(ctx, idx, qs, nq, keff, nprobes, 0, cid + (size_t)l * keff, cds + (size_t)l * keff));
    }
  }
  LH_TRY(mva_score_enqueue(ctx, cid, cds, q_offsets, B, lists, keff, k_out, ids, dists));
  LH_CHECK_HIP(hipStreamSynchronize(ctx->stream));
  return LANCE_HIP_OK;
}
