// search_plan.h -- which kernels serve an IVF-PQ search batch: decided ONCE per uncaptured call, on the host, by the pure function below.
// Plain C++17 (no HIP, no environment, no locks, no device pointers): tests/c/search_plan_main.cpp compiles it alone.  The executors
// (search.hip, search_pm.hip, search_q.hip, search_qt.hip, search_ms.hip) follow the plan and LH_REQUIRE what it guarantees; DESIGN.md has
// the same rules as a table.
//
// Lazy constants: a plan whose passes run on the matrix cores needs lance_hip_index::ms.  plan_ivfpq_search() treats MS_NOT_BUILT as usable
// and sets wants_ms_constants; the caller then builds them (mscan_prepare), fills ms_state again and plans a SECOND time -- that plan is
// final.  Only a key's first, uncaptured call can see MS_NOT_BUILT, so planning never synchronises or allocates during a graph capture.
#pragma once
#include <algorithm>
#include <cstdint>
#include "../../include/lance_hip.h"

namespace lh {

// mirrors of kernel constants (static_asserts in search_pm.hip and search_q.hip keep them equal)
constexpr uint32_t PLAN_MAX_KEFF = 128;   // SCAN_MAX_KEFF: the scan kernels' per-query heap; larger k * refine goes to the exact kernel alone
constexpr uint64_t PLAN_SEG_CAP = 256;    // Q_CAP: survivors kept per (query, probe)
constexpr uint64_t PLAN_Q_G = 4;          // Q_G: queries per work item of the integer scan
constexpr uint64_t PLAN_SCRATCH_MAX = 2ull << 30;   // one scratch slot: at most 2 GiB

// Every A/B switch that takes part in the route (LANCE_HIP_<name>), read once per process by plan_switches_from_env() (search.hip).
struct PlanSwitches {
  bool no_pm = false, no_qscan = false, no_mscan = false, no_msbound = false, no_dot_flow = false, exact_bound = false, pm_nobound = false;
  int qpt = 2;                    // QPT: 0 off, 1 per-query tables after the bound pass, 2 before it and shared by both passes (r04g: C3 716 k -> 788 k q/s at nprobes 10, 348 k -> 508 k at 50)
  uint32_t mscan_minq = 96;       // MSCAN_MINQ: (query, probe) pairs per list from which the matrix-core scan is taken
  uint32_t bound_lists = 1;       // BOUND_LISTS: lists per query in the L2 / cosine matrix-core bound pass
  uint32_t dot_bound_lists = 3;   // DOT_BOUND_LISTS: the same for dot
  double dot_flow_skew = 1e18;    // DOT_FLOW_SKEW: largest list / mean list up to which dot takes the quantised flow (default: no limit)
};

enum PlanMsState { MS_NOT_BUILT, MS_USABLE, MS_UNUSABLE };   // lance_hip_index::ms (MS_UNUSABLE: an all-zero codebook, nothing to scale by)
struct PlanIndex {
  int metric = LANCE_HIP_L2, dtype = LANCE_HIP_F32;
  uint32_t d = 0, m = 0, nbits = 8, nlist = 0, max_part = 0;
  uint64_t n = 0;
  bool model_finite = true, has_cb_mean = false;
  bool codes_aligned16 = true, codebook_aligned16 = true, centroids_aligned8 = true, query_aligned8 = true;
  PlanMsState ms_state = MS_NOT_BUILT;
};
struct PlanBatch { uint32_t nq = 0, nprobes = 0, keff = 0; bool has_range = false; };

enum PlanRoute { ROUTE_QM8, ROUTE_QM4, ROUTE_EXACT_ONLY, ROUTE_PAIR_SCAN, ROUTE_QUANTISED };
enum PlanBound { BOUND_EXACT_PAIR, BOUND_PT, BOUND_MATRIX, BOUND_INTEGER };
enum PlanMain { MAIN_MATRIX, MAIN_INTEGER, MAIN_TILED, MAIN_PT };
enum PlanClassB { CLASSB_PAIR, CLASSB_RESCAN };
struct IvfpqPlan {
  PlanRoute route = ROUTE_QM8;
  // ROUTE_QUANTISED only: bound pass -> main (filter) pass -> class B (queries the bound pass gave no bound) -> merge
  PlanBound bound = BOUND_INTEGER;
  uint32_t bound_lists = 1;       // lists per query the bound pass scans (1..4)
  PlanMain main = MAIN_INTEGER;
  PlanClassB class_b = CLASSB_PAIR;
  int pool_cap = 0;               // ROUTE_QUANTISED and ROUTE_PAIR_SCAN: entries of a query's candidate pool
  bool pair_bound_pass = true;    // ROUTE_PAIR_SCAN: false (PM_NOBOUND) = the two-class flow without a bound pass
  bool wants_ms_constants = false;
  const char *why = "";           // why the batch did not get the next faster route (LANCE_HIP_Q_STATS prints it)
};

// M = 48 / 64 / 96: the table is tiled over the sub-quantisers (search_qt.hip); no exact pair kernel exists at these sizes
inline bool qscan_tiled_shape(int m, int sd) { return (m == 48 || m == 64 || m == 96) && (sd == 4 || sd == 8 || sd == 16); }
// the matrix-core passes (search_ms.hip): d = 128 with M = 16 / 32, d = 64 with M = 16
inline bool ms_shape(uint32_t d, uint32_t m) { return (d == 128 && (m == 16 || m == 32)) || (d == 64 && m == 16); }

// The index-only part of "the matrix-core passes may serve this index" (lance_hip_index_prewarm builds the constants on it): nullptr = yes.
inline const char *plan_index_ms_refusal(const PlanIndex &ix, const PlanSwitches &sw) {
  if (sw.no_mscan) return "LANCE_HIP_NO_MSCAN";
  if (ix.nbits != 8 || !ms_shape(ix.d, ix.m)) return "not a matrix-core shape (d 128 with M 16 / 32, d 64 with M 16; 8-bit)";
  if (!ix.model_finite) return "NaN / infinite centroids or codewords";
  if (ix.ms_state == MS_UNUSABLE) return "all-zero codebook";
  if (ix.metric != LANCE_HIP_DOT) return nullptr;
  // dot: the quantised flow is the matrix-core bound pass + scan or nothing (the integer tables need entries >= 0)
  if (sw.no_msbound || sw.no_dot_flow) return "dot: LANCE_HIP_NO_MSBOUND / LANCE_HIP_NO_DOT_FLOW";
  if (!ix.has_cb_mean) return "dot: no codebook means";
  // Lists as uneven as the rows' norms (dot over unnormalised rows with components of one sign: at the C2 shape the largest of 256 lists held 82,424
  // of the 10^6 rows and was every query's nearest): with the bound of the NEAREST list alone a fifth of the segments overflowed into exact rescans of
  // whole lists and the flow measured slower than the exact pair scan (3.94 against 3.46 ms per 10,000-query batch, r06zu); with the bound pass
  // over three lists it is 1.88 (r06zzg).  DOT_FLOW_SKEW keeps a guard for A/B runs.
  if ((double)ix.max_part * (double)ix.nlist > sw.dot_flow_skew * (double)ix.n) return "dot: list sizes more uneven than LANCE_HIP_DOT_FLOW_SKEW";
  return nullptr;
}

inline IvfpqPlan plan_ivfpq_search(const PlanIndex &ix, const PlanBatch &b, const PlanSwitches &sw) {
  IvfpqPlan p;
  const uint64_t pairs = (uint64_t)b.nq * b.nprobes;
  const int m = (int)ix.m, sd = (m > 0 && ix.d % ix.m == 0) ? (int)(ix.d / ix.m) : 0;
  const bool tiled = qscan_tiled_shape(m, sd), dot = ix.metric == LANCE_HIP_DOT;
  auto leave = [&](PlanRoute r, const char *why) { p.route = r; p.why = why; return p; };
  if (b.keff > PLAN_MAX_KEFF) return leave(ROUTE_EXACT_ONLY, "k * refine above the scan kernels' heap");
  // ---- partition major (queries of a list share its rows and LDS gathers) or query major ----
  const PlanRoute qm = ix.nbits == 4 ? ROUTE_QM4 : ROUTE_QM8;
  if (sw.no_pm) return leave(qm, "LANCE_HIP_NO_PM");
  if (ix.nbits != 8 || b.has_range) return leave(qm, "4-bit codes or a distance range: query major only");
  if (!(sd == 4 || sd == 8 || sd == 16) || !(tiled || m == 16 || m == 32)) return leave(qm, "no partition-major kernel for this M / sub-dimension");
  if (!ix.codes_aligned16 || !ix.codebook_aligned16) return leave(qm, "codes / codebook not 16-byte aligned");
  // large enough to pair queries (tiled shapes: a work item's table build is as long as a query-major workgroup's, so sharing it pays earlier)
  if (pairs < (tiled ? 2048u : 4096u)) return leave(qm, "fewer (query, probe) pairs than the partition-major scan needs");
  // a (query, list) publishes at most ~keff (+ ties) rows, usually far fewer once the bound is tight
  auto pool = [&](uint64_t cap) { return (int)((std::min<uint64_t>(cap, std::max<uint64_t>(512, (uint64_t)b.nprobes * (b.keff + 28))) + 255) & ~255ull); };
  p.pool_cap = pool(8192);
  p.pair_bound_pass = !sw.pm_nobound;
  // ---- quantised flow or exact pair scan ----
  const char *ms_no = plan_index_ms_refusal(ix, sw);
  // The matrix-core scan pays once a partition sees a few tiles' worth of queries: a wave's 32-row chunk costs a gather (codes -> 8 codewords ->
  // |c^|^2) worth ~4 tiles before its first MFMA.  Measured (r04v): 390 pairs per partition (C2) 0.188 + 0.047 ms against 0.354 + 0.021 for the integer
  // scan; 24 pairs per partition (C4 shape, nlist 4096, 10k x 10) 0.463 + 0.110 against 0.324 + 0.023 -- slower.  Per (row, query) cell the model
  // (G + t C) / (1024 t) crosses the integer scan's cost near t = 3 tiles.
  if (!ms_no && pairs < (uint64_t)sw.mscan_minq * ix.nlist) ms_no = "fewer than LANCE_HIP_MSCAN_MINQ (96) pairs per list";
  // per-query tables (tiled shapes; an f16 column rounds the residual to f16, so r is not q - centroid any more)
  const bool pt = sw.qpt != 0 && tiled && ix.dtype != LANCE_HIP_F16 && !dot;
  p.main = !ms_no ? MAIN_MATRIX : pt ? MAIN_PT : tiled ? MAIN_TILED : MAIN_INTEGER;
  const char *q_no = nullptr;
  if (sw.pm_nobound) q_no = "LANCE_HIP_PM_NOBOUND";
  else if (sw.no_qscan) q_no = "LANCE_HIP_NO_QSCAN";
  else if (!ix.model_finite) q_no = "NaN / infinite centroids or codewords: the exact kernels decide";
  else if (ix.metric != LANCE_HIP_L2 && ix.metric != LANCE_HIP_COSINE && !dot) q_no = "metric without a quantised flow";
  else if (dot && p.main != MAIN_MATRIX) q_no = ms_no;
  else if (pairs * PLAN_SEG_CAP * 4 > PLAN_SCRATCH_MAX) q_no = "survivor segments above 2 GiB of scratch";
  // item residuals likewise -- where the main pass reads them: neither the per-query-table filter nor the matrix-core scan does.  (The check used to
  // apply to both: a 10,000-query batch at nprobes = 50 on the C3 shape fell back to the query-major kernel, 62 ms instead of ~6: r04v.)
  else if ((p.main == MAIN_INTEGER || p.main == MAIN_TILED) && (pairs / PLAN_Q_G + ix.nlist + 1) * ix.d * 16 > PLAN_SCRATCH_MAX)
    q_no = "item residuals above 2 GiB of scratch";
  if (!q_no) {
    if (sw.exact_bound && !tiled && !dot) p.bound = BOUND_EXACT_PAIR;   // A/B: the exact pair kernel has no M > 32 instantiation
    else if (p.main == MAIN_PT && sw.qpt == 2) p.bound = BOUND_PT;
    // u16 bins: a bin never holds more rows than the list has (L2: larger lists keep the integer pass; dot: the kernel counts the first 65,535 rows)
    else if (p.main == MAIN_MATRIX && !sw.no_msbound && ix.has_cb_mean && (dot || ix.max_part < 65536u) && ix.query_aligned8 && ix.centroids_aligned8)
      p.bound = BOUND_MATRIX;
    else if (dot) q_no = "dot: the matrix-core bound pass cannot take the batch (unaligned queries / centroids)";
    else p.bound = BOUND_INTEGER;
  }
  if (q_no) return leave(tiled ? qm : ROUTE_PAIR_SCAN, q_no);   // tiled shapes: only the quantised flow exists (the exact pair table would not fit in LDS)
  p.route = ROUTE_QUANTISED;
  p.why = p.main == MAIN_MATRIX ? (p.bound == BOUND_MATRIX ? "" : "bound pass off the matrix cores (switch, list >= 65536 rows, alignment or no codebook means)") : ms_no;
  p.wants_ms_constants = p.main == MAIN_MATRIX && ix.ms_state == MS_NOT_BUILT;
  // dot: the bound pass runs over each query's THREE nearest lists and keeps the smallest bound -- without residuals the list a query's best rows sit in
  // is often not the one with the largest centroid score, and the nearest list's k*refine-th distance then lets hundreds of that list's rows through.
  // C2 shape, ms per 10,000-query batch with 1 / 2 / 3 / 4 lists (r06zzf, r06zzg): unit-normalised rows 0.951 / 0.854 / 0.860 / 0.867 (overflowed
  // segments 5,311 -> 2,852 with two), centred rows 1.150 / 0.911 / 0.900 / 0.910, SIFT-like rows as they are (largest list 82,424 of 10^6 rows) 3.94 / 2.29 /
  // 1.88 against 3.46 on the exact pair scan.  L2 / cosine: one list; BOUND_LISTS = 2 .. 4 is an A/B switch of the matrix-core bound pass.
  p.bound_lists = std::min(std::min(dot ? sw.dot_bound_lists : (p.bound == BOUND_MATRIX ? sw.bound_lists : 1u), 4u), b.nprobes);
  p.class_b = tiled ? CLASSB_RESCAN : CLASSB_PAIR;
  // tiled shapes have no exact pair kernel: EVERY segment of a query without a bound goes through the rescan kernel and publishes ~keff rows to the
  // pool, so the pool follows nprobes there (nprobes = 100 with refine 10 overflowed the 8192-entry pool of every such query and sent it
  // to the query-major replay), within 1 GiB of scratch
  uint64_t pool_max = tiled ? 65536 : 8192;
  while (pool_max > 8192 && (uint64_t)b.nq * pool_max * 8 > (1ull << 30)) pool_max /= 2;
  p.pool_cap = pool(pool_max);
  return p;
}

}  // namespace lh
