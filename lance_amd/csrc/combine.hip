// combine.hip -- the stage that joins an ANN list with a flat scan of the rows no index covers yet: `take` + `flat_knn` over candidate lists.
//
//   Scanner::nearest / vector_search      rust/lance/src/dataset/scanner.rs:2847-3030  (ANN over the deltas, refine, knn_combined)
//   Scanner::flat_knn / knn_combined      scanner.rs:3336-3468  (UnionExec of the ANN list and the flat KNN of the unindexed fragments -- no
//                                         de-duplication --, then KNNVectorDistanceExec over the union: EVERY distance is recomputed from the
//                                         column, LanceFilterExec(_distance >= lower AND _distance < upper), SortExec(_distance, _rowid).fetch(k))
//   refine                                scanner.rs:2884-2904  (take the k * refine_factor rows, flat_knn over them)
//
// One workgroup of 256 threads per query.  The candidates of the two lists are gathered into (key, row id) entries in LDS; the four
// waves then stage the candidate rows into their LDS slices with coalesced loads of whole rows (16 bytes per lane when the column is on
// the 16-byte grid and a row is a whole number of 16-byte words, element by element otherwise), and one lane per staged row walks it with
// the exact.cuh function the flat scan and the refine kernels use for that element type and metric -- so a distance here is the bits
// lance_hip_flat_topk returns for that (row, query).  Rows longer than a wave's slice are read in place, one lane per row.  The bounds
// are tested on the order keys, the entries sorted by (key, row id) (bitonic_sort_kr) and the first k written.  No atomics on global
// memory: the bad-row flag of a query is gathered in LDS and written once.
#include <algorithm>
#include <cstdio>

#include "common.h"
#include "exact.cuh"
#include "kernels.h"
#include "search_common.cuh"

#pragma clang fp contract(off)

namespace lh {

// ---- take_flat_knn: device code and the launch-size functions behind it (cut out by tests/test_knn_combined_kernel_cpu.py) ----
constexpr int TFK_MAX_CAND = 4096;        // ca + cb: 4096 entries of 16 bytes are 64 KiB of LDS
constexpr int TFK_WAVES = 4;
constexpr int TFK_STAGE_BYTES = 8192;     // a wave's slice of staged rows

struct TakeArgs {
  const float *q;            // [nq][d], widened to f32
  int d;
  uint64_t n_rows;
  const uint64_t *ids_a;     // [nq][ca]
  const uint64_t *ids_b;     // [nq][cb] (NULL: cb = 0)
  const float *dists_b;      // [nq][cb] or NULL: list B is scored like list A
  int ca, cb;
  int has_lower, has_upper;
  uint32_t lo_key, hi_key;
  int k, P;                  // P: entries sorted, a power of two >= max(ca + cb, 64)
  int rows_per_step;         // rows a wave stages at a time; 0: a row does not fit a slice, rows are read in place
  int row_stride;            // bytes between staged rows: an ODD number of dwords, so lanes walking different rows hit different banks
  uint64_t *out_ids;         // [nq][k]
  float *out_dists;
  uint32_t *flags;           // [nq]: FLAG_BADROW when a candidate id is >= n_rows (written for every query, no need to zero)
};

static inline int tfk_entries(int cand) {
  int p = 64;
  while (p < cand) p <<= 1;
  return p;
}
static inline int64_t tfk_row_stride(int64_t d, int esz) { return (((d * esz + 3) / 4) | 1) * 4; }
static inline int tfk_rows_per_step(int64_t d, int esz) { return (int)std::min<int64_t>(64, TFK_STAGE_BYTES / tfk_row_stride(d, esz)); }
// dynamic LDS of a launch: the entries, 16 bytes of per-query words (query norm, bad-row flag), the four slices
static inline size_t take_flat_knn_bytes(int cand, int64_t d, int esz) {
  return (size_t)tfk_entries(cand) * 16 + 16 + (tfk_rows_per_step(d, esz) > 0 ? (size_t)TFK_WAVES * TFK_STAGE_BYTES : 0);
}

// the distance lance_hip_flat_topk and launch_refine compute for this element type and metric (flat_scan_generic_kernel, refine_kernel)
template <int METRIC, typename TR, bool H32>
__device__ __forceinline__ float tfk_distance(const float *qv, float qnorm, const TR *row, int d) {
  if constexpr (METRIC == METRIC_COSINE) {
    return H32 ? cosine_scalar32_rt<TR>(qv, qnorm, row, d) : cosine_exact_rt<TR>(qv, qnorm, row, d);
  } else {
    return finish_metric<METRIC>(dist_exact_rt<METRIC, TR, (H32 && METRIC == METRIC_DOT) ? 32 : 16, METRIC == METRIC_L2>(qv, row, d));      // (L2: row - q, exact.cuh SWAP)
  }
}

template <int METRIC, typename TR, bool H32>
__global__ __launch_bounds__(256) void take_flat_knn_kernel(TakeArgs a, const TR *__restrict__ x) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int P = a.P, d = a.d;
  uint64_t *rid = reinterpret_cast<uint64_t *>(smem);
  uint32_t *key = reinterpret_cast<uint32_t *>(rid + P);
  uint32_t *pos = key + P;                                   // 1: the row is still to be scored; the sort's payload afterwards
  float *s_qnorm = reinterpret_cast<float *>(pos + P);
  uint32_t *s_bad = reinterpret_cast<uint32_t *>(s_qnorm + 1);
  char *stage = reinterpret_cast<char *>(pos + P) + 16;
  const int qi = blockIdx.x, tid = threadIdx.x;
  const float *qv = a.q + (int64_t)qi * d;
  const int cand = a.ca + a.cb;
  if (tid == 0) {
    *s_bad = 0u;
    float qn = 0.0f;
    if constexpr (METRIC == METRIC_COSINE) qn = H32 ? norm_l2_rt<float, 32>(qv, d) : norm_l2_rt(qv, d);      // cosine_batch: x_norm = norm_l2(x)
    *s_qnorm = qn;
  }
  __syncthreads();
  // the two lists -> entries.  ~0 is an empty slot; an id >= n_rows is flagged and never read; no de-duplication (UnionExec does none)
  for (int i = tid; i < P; i += 256) {
    uint64_t r = ~0ull;
    uint32_t kk = 0xFFFFFFFFu, todo = 0u;
    if (i < cand) {
      const bool from_b = i >= a.ca;
      r = from_b ? a.ids_b[(int64_t)qi * a.cb + (i - a.ca)] : a.ids_a[(int64_t)qi * a.ca + i];
      if (r != ~0ull) {
        if (r >= a.n_rows) { *s_bad = 1u; r = ~0ull; }
        else if (from_b && a.dists_b) kk = order_key(a.dists_b[(int64_t)qi * a.cb + (i - a.ca)]);      // the flat scan's own bits
        else todo = 1u;
      }
    }
    rid[i] = r; key[i] = kk; pos[i] = todo;
  }
  __syncthreads();
  const float qnorm = *s_qnorm;
  if (a.rows_per_step == 0) {
    // a row longer than a wave's slice: one lane per row, read in place (the scalar walk of refine_kernel)
    for (int i = tid; i < cand; i += 256)
      if (pos[i]) key[i] = order_key(tfk_distance<METRIC, TR, H32>(qv, qnorm, x + rid[i] * (uint64_t)d, d));
  } else {
    const int wave = tid >> 6, lane = tid & 63, R = a.rows_per_step;
    char *mine = stage + (size_t)wave * TFK_STAGE_BYTES;
    const bool vec = (reinterpret_cast<uintptr_t>(x) & 15) == 0 && ((size_t)d * sizeof(TR)) % 16 == 0;
    const int nvec = (int)((size_t)d * sizeof(TR) / 16);
    for (int step0 = 0; step0 < cand; step0 += TFK_WAVES * R) {      // uniform over the workgroup: both barriers are met by every wave
      const int base = step0 + wave * R;
      const int nr = max(0, min(R, cand - base));
      if (vec) {
        for (int it = lane; it < nr * nvec; it += 64) {
          const int row = it / nvec, v = it - row * nvec;
          if (!pos[base + row]) continue;
          const uint4 u = reinterpret_cast<const uint4 *>(x + rid[base + row] * (uint64_t)d)[v];
          uint32_t *o = reinterpret_cast<uint32_t *>(mine + (size_t)row * a.row_stride) + 4 * v;
          o[0] = u.x; o[1] = u.y; o[2] = u.z; o[3] = u.w;
        }
      } else {
        for (int64_t it = lane; it < (int64_t)nr * d; it += 64) {
          const int row = (int)(it / d), e = (int)(it - (int64_t)row * d);
          if (!pos[base + row]) continue;
          reinterpret_cast<TR *>(mine + (size_t)row * a.row_stride)[e] = x[rid[base + row] * (uint64_t)d + e];
        }
      }
      __syncthreads();
      if (lane < nr && pos[base + lane])
        key[base + lane] = order_key(tfk_distance<METRIC, TR, H32>(qv, qnorm, reinterpret_cast<const TR *>(mine + (size_t)lane * a.row_stride), d));
      __syncthreads();
    }
  }
  __syncthreads();
  // lower <= d < upper in the total order on f32, on the exact distances; an absent bound is not tested
  for (int i = tid; i < P; i += 256) {
    if (rid[i] != ~0ull) {
      const uint32_t kk = key[i];
      if ((a.has_lower && kk < a.lo_key) || (a.has_upper && kk >= a.hi_key)) { rid[i] = ~0ull; key[i] = 0xFFFFFFFFu; }
    }
    pos[i] = (uint32_t)i;
  }
  __syncthreads();
  bitonic_sort_kr<256>(key, rid, pos, P);
  for (int i = tid; i < a.k; i += 256) {
    const bool have = i < P && rid[i] != ~0ull;
    a.out_ids[(int64_t)qi * a.k + i] = have ? rid[i] : ~0ull;
    a.out_dists[(int64_t)qi * a.k + i] = have ? key_to_float(key[i]) : INFINITY;
  }
  if (tid == 0) a.flags[qi] = *s_bad ? FLAG_BADROW : 0u;
}
// ---- take_flat_knn: end of the code the emulator program compiles ----

template <int METRIC, typename TR, bool H32>
static void launch_take(lance_hip_ctx *ctx, const TakeArgs &a, const void *x, uint32_t nq, size_t lds) {
  hipLaunchKernelGGL((take_flat_knn_kernel<METRIC, TR, H32>), dim3(nq), dim3(256), lds, ctx->stream, a, static_cast<const TR *>(x));
}

template <typename TR, bool F16>
static void launch_take_metric(lance_hip_ctx *ctx, int metric, const TakeArgs &a, const void *x, uint32_t nq, size_t lds) {
  // f16 columns under dot / cosine: half::f16's own 32-lane orders (flat.hip h32, refine_kernel H32); f16 L2 widens per element
  if (metric == LANCE_HIP_COSINE) launch_take<METRIC_COSINE, TR, F16>(ctx, a, x, nq, lds);
  else if (metric == LANCE_HIP_DOT) launch_take<METRIC_DOT, TR, F16>(ctx, a, x, nq, lds);
  else launch_take<METRIC_L2, TR, false>(ctx, a, x, nq, lds);
}

}  // namespace lh

using namespace lh;

extern "C" int lance_hip_take_flat_knn(lance_hip_ctx *ctx, int dtype, int metric, const void *x, uint64_t n_rows, uint32_t d, const void *q,
                                       uint32_t nq, const uint64_t *ids_a, uint32_t ca, const uint64_t *ids_b, const float *dists_b,
                                       uint32_t cb, int has_lower, float lower, int has_upper, float upper, uint32_t k, uint64_t *out_ids,
                                       float *out_dists) {
  lh::CtxLock _ctx_lock(ctx);
  const char *what = "take_flat_knn";
  LH_REQUIRE(ctx && (n_rows == 0 || x) && (nq == 0 || (q && out_ids && out_dists)), "%s: NULL argument", what);
  LH_REQUIRE((ca == 0 || nq == 0 || ids_a) && (cb == 0 || nq == 0 || ids_b), "%s: a candidate list of %u / %u slots was given as NULL", what, ca, cb);
  LH_TRY(check_dtype(dtype, what));
  LH_REQUIRE(metric == LANCE_HIP_L2 || metric == LANCE_HIP_DOT || metric == LANCE_HIP_COSINE, "%s: bad metric %d", what, metric);
  LH_REQUIRE(!(dtype == LANCE_HIP_I8 && metric == LANCE_HIP_COSINE), "%s: int8 cosine is not supported (no normalised int8 rows)", what);
  LH_REQUIRE(d > 0, "%s: d must be > 0", what);
  LH_REQUIRE(k > 0 && k <= 1024, "%s: k=%u not supported (1..1024)", what, k);
  LH_REQUIRE((uint64_t)ca + cb >= 1 && (uint64_t)ca + cb <= (uint64_t)TFK_MAX_CAND, "%s: %llu candidates per query not supported (1..%d)", what,
             (unsigned long long)((uint64_t)ca + cb), TFK_MAX_CAND);
  const FlatRange rg = flat_range(has_lower, lower, has_upper, upper);
  LH_REQUIRE(!(rg.has_lower && rg.has_upper) || rg.lo_key <= rg.hi_key, "%s: lower bound %g is above the upper bound %g", what, (double)lower,
             (double)upper);
  LH_CHECK_HIP(hipSetDevice(ctx->device));
  if (nq == 0) return LANCE_HIP_OK;
  const float *qf;
  LH_TRY(as_f32(ctx, dtype, q, (size_t)nq * d, "take.q", &qf));
  uint32_t *flags = ctx->scratch_t<uint32_t>("take.flags", nq);
  if (!flags) return LANCE_HIP_ENOMEM;
  const int esz = dtype == LANCE_HIP_F32 ? 4 : dtype == LANCE_HIP_F16 ? 2 : 1;
  TakeArgs a;
  a.q = qf; a.d = (int)d; a.n_rows = n_rows;
  a.ids_a = ids_a; a.ids_b = cb ? ids_b : nullptr; a.dists_b = cb ? dists_b : nullptr; a.ca = (int)ca; a.cb = (int)cb;
  a.has_lower = rg.has_lower; a.has_upper = rg.has_upper; a.lo_key = rg.lo_key; a.hi_key = rg.hi_key;
  a.k = (int)k; a.P = tfk_entries((int)(ca + cb));
  a.rows_per_step = tfk_rows_per_step(d, esz);
  a.row_stride = a.rows_per_step > 0 ? (int)tfk_row_stride(d, esz) : 0;
  a.out_ids = out_ids; a.out_dists = out_dists; a.flags = flags;
  const size_t lds = take_flat_knn_bytes((int)(ca + cb), d, esz);
  {
    ScopedTimer t(ctx, "take_flat_knn");
    if (dtype == LANCE_HIP_I8) launch_take_metric<int8_t, false>(ctx, metric, a, x, nq, lds);
    else if (dtype == LANCE_HIP_F16) launch_take_metric<__half, true>(ctx, metric, a, x, nq, lds);
    else launch_take_metric<float, false>(ctx, metric, a, x, nq, lds);
  }
  LH_CHECK_HIP(hipGetLastError());
  // a candidate id >= n_rows was never read: reported after the stream is drained (launch_refine / check_flags do the same)
  char msg[192];
  snprintf(msg, sizeof msg, "%s: a candidate row id is >= n_rows = %llu (the column must be indexed by the row ids of the lists)", what,
           (unsigned long long)n_rows);
  return check_flags(ctx, flags, nq, msg);
}
