// Stand-alone driver of lance_amd/csrc/search_plan.h (plain C++: no HIP, no GPU) for tests/test_search_plan_cpu.py.
// stdin: one case per line, `name=value` tokens (anything not named keeps the struct's default); stdout: one line per case.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

#include "search_plan.h"

using namespace lh;

int main() {
  static const char *routes[] = {"qm8", "qm4", "exact_only", "pair_scan", "quantised"};
  static const char *bounds[] = {"exact_pair", "pt", "matrix", "integer"};
  static const char *mains[] = {"matrix", "integer", "tiled", "pt"};
  std::string line;
  while (std::getline(std::cin, line)) {
    PlanIndex ix;
    PlanBatch b;
    PlanSwitches sw;
    std::istringstream in(line);
    std::string tok;
    while (in >> tok) {
      const size_t eq = tok.find('=');
      if (eq == std::string::npos) { fprintf(stderr, "bad token %s\n", tok.c_str()); return 2; }
      const std::string k = tok.substr(0, eq);
      const double v = atof(tok.c_str() + eq + 1);
      if (k == "metric") ix.metric = (int)v; else if (k == "dtype") ix.dtype = (int)v; else if (k == "d") ix.d = (uint32_t)v;
      else if (k == "m") ix.m = (uint32_t)v; else if (k == "nbits") ix.nbits = (uint32_t)v; else if (k == "nlist") ix.nlist = (uint32_t)v;
      else if (k == "n") ix.n = (uint64_t)v; else if (k == "max_part") ix.max_part = (uint32_t)v; else if (k == "finite") ix.model_finite = v != 0;
      else if (k == "cb_mean") ix.has_cb_mean = v != 0; else if (k == "a_codes") ix.codes_aligned16 = v != 0;
      else if (k == "a_codebook") ix.codebook_aligned16 = v != 0; else if (k == "a_centroids") ix.centroids_aligned8 = v != 0;
      else if (k == "a_query") ix.query_aligned8 = v != 0; else if (k == "ms") ix.ms_state = (PlanMsState)(int)v;
      else if (k == "nq") b.nq = (uint32_t)v; else if (k == "nprobes") b.nprobes = (uint32_t)v; else if (k == "keff") b.keff = (uint32_t)v;
      else if (k == "range") b.has_range = v != 0;
      else if (k == "no_pm") sw.no_pm = v != 0; else if (k == "no_qscan") sw.no_qscan = v != 0; else if (k == "no_mscan") sw.no_mscan = v != 0;
      else if (k == "no_msbound") sw.no_msbound = v != 0; else if (k == "no_dot_flow") sw.no_dot_flow = v != 0;
      else if (k == "exact_bound") sw.exact_bound = v != 0; else if (k == "pm_nobound") sw.pm_nobound = v != 0; else if (k == "qpt") sw.qpt = (int)v;
      else if (k == "mscan_minq") sw.mscan_minq = (uint32_t)v; else if (k == "bound_lists") sw.bound_lists = (uint32_t)v;
      else if (k == "dot_bound_lists") sw.dot_bound_lists = (uint32_t)v; else if (k == "dot_flow_skew") sw.dot_flow_skew = v;
      else { fprintf(stderr, "unknown field %s\n", k.c_str()); return 2; }
    }
    const IvfpqPlan p = plan_ivfpq_search(ix, b, sw);
    const bool q = p.route == ROUTE_QUANTISED;
    printf("route=%s bound=%s lists=%u main=%s class_b=%s pool=%d pair_bound=%d wants_ms=%d prewarm_ms=%d why=%s\n", routes[p.route],
           q ? bounds[p.bound] : "-", q ? p.bound_lists : 0u, q ? mains[p.main] : "-", q ? (p.class_b == CLASSB_RESCAN ? "rescan" : "pair") : "-",
           p.pool_cap, p.pair_bound_pass ? 1 : 0, p.wants_ms_constants ? 1 : 0, plan_index_ms_refusal(ix, sw) ? 0 : 1, p.why ? p.why : "(null)");
  }
  return 0;
}
