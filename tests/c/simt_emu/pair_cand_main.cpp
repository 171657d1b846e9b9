// Runs the candidate kernels (lance_amd/csrc/pair_cand.cuh and their IVF_SQ / IVF_RQ instances in sq.hip / rq.hip) on the CPU (simt_emu.h)
// under AddressSanitizer + UBSan at a capacity the caller names: every global buffer has exactly the size the library gives it, and the
// dynamic LDS of every launch is what the library's own sizing functions say (simt_launch_lds: within 64 KiB, the bytes behind it untouched).
// pair_device_code.inc is cut out of the sources by tests/test_wide_cand_kernels_cpu.py, which also builds the index storage with
// tests/sq_spec.py / tests/rq_spec.py, writes the problem file and compares the outputs with the specification.
#include "simt_emu.h"

// what rq.hip uses beyond the IVF_SQ kernels' needs
static inline uint32_t atomicMin(uint32_t *p, uint32_t v) {
  uint32_t old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (v < old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  return old;
}
static inline uint32_t atomicMax(uint32_t *p, uint32_t v) {
  uint32_t old = __atomic_load_n(p, __ATOMIC_SEQ_CST);
  while (v > old && !__atomic_compare_exchange_n(p, &old, v, false, __ATOMIC_SEQ_CST, __ATOMIC_SEQ_CST)) {}
  return old;
}

namespace lh {
#include "pair_device_code.inc"
}
using namespace lh;

template <typename T>
static std::vector<T> rd(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { puts("short read"); exit(2); }
  return v;
}
template <typename T>
static void wr(FILE *f, const T *p, size_t n) { if (n && fwrite(p, sizeof(T), n, f) != n) { puts("short write"); exit(2); } }
static uint8_t *aligned_copy(const std::vector<uint8_t> &src) {      // 16-byte aligned, NOT padded beyond a multiple of 16
  const size_t bytes = std::max<size_t>(16, (src.size() + 15) & ~(size_t)15);
  uint8_t *p = static_cast<uint8_t *>(aligned_alloc(16, bytes));
  memset(p, 0, bytes);
  if (!src.empty()) memcpy(p, src.data(), src.size());
  return p;
}

// in: u32 kind (0 = IVF_SQ, 1 = IVF_RQ), n_kept, d, nlist, nq, nprobes, keff, cap (0 = the library's), dot, has_allow | u32 offs[nlist + 1] |
// u64 rid[n_kept] (stored order) | u32 probes[nq][nprobes] | u32 allow_bits[n_kept / 32 + 4] (if has_allow) | then
//   IVF_SQ: f32 r2 | u8 codes[n_kept][ld] | u32 xx[n_kept] | u8 qcodes[nq][ld] | u32 qq[nq]
//   IVF_RQ: u8 codes[n_kept][d / 8] | f32 add[n_kept], scale[n_kept] | f32 pdists[nq][nprobes] | f32 q[nq][d] | f32 cent[nlist][d] | f32 pt[d][d]
// out: u32 pkey, ppos [pairs][keff] | u32 pcnt, pamb [pairs] | u64 fast ids, f32 fast dists [nq][keff] | u32 flags [nq + 1] |
//      u64 ids, f32 dists [nq][keff]
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  const auto h = rd<uint32_t>(f, 10);
  const uint32_t kind = h[0], n = h[1], d = h[2], nlist = h[3], nq = h[4], nprobes = h[5], keff = h[6], dot = h[8], has_allow = h[9];
  // cap = 0: the capacity the library picks for this search (printed: the caller knows which it expects)
  const uint32_t cap = h[7] ? h[7] : (uint32_t)(kind == 0 ? sq_scan_cap((d + 15u) & ~15u, (int)keff) : rq_scan_cap(d, (int)keff));
  printf("cap %u\n", cap);
  const auto offs = rd<uint32_t>(f, nlist + 1);
  const auto rid = rd<uint64_t>(f, n);
  const auto probes = rd<uint32_t>(f, (size_t)nq * nprobes);
  const auto allow = rd<uint32_t>(f, has_allow ? n / 32 + 4 : 0);
  const size_t pairs = (size_t)nq * nprobes;
  std::vector<uint32_t> pkey(pairs * keff, 0xDEADBEEFu), ppos(pairs * keff, 0xDEADBEEFu), pcnt(pairs), pamb(pairs), flags(nq + 1, 0);
  std::vector<uint64_t> ids((size_t)nq * keff);
  std::vector<float> dists((size_t)nq * keff);
  CandLists w;
  w.row_ids = rid.data(); w.part_offsets = offs.data(); w.probes = probes.data(); w.allow = has_allow ? allow.data() : nullptr;
  w.nprobes = (int)nprobes; w.k = (int)keff; w.cap = (int)cap;
  w.pkey = pkey.data(); w.ppos = ppos.data(); w.pcnt = pcnt.data(); w.pamb = pamb.data(); w.flags = flags.data(); w.n_replay = flags.data() + nq;
  std::vector<uint64_t> fast_ids;
  std::vector<float> fast_dists;
  auto merge = [&] {
    if (keff <= (uint32_t)CAND_NARROW_K)      // cand_merge_lists (sq.hip)
      simt_launch_lds(cand_merge_bytes(CAND_MERGE_NARROW), nq, 256, [&] { cand_merge_kernel<CAND_MERGE_NARROW, CAND_NARROW_K>(w, ids.data(), dists.data()); });
    else
      simt_launch_lds(cand_merge_bytes(CAND_MERGE_WIDE), nq, 256, [&] { cand_merge_kernel<CAND_MERGE_WIDE, CAND_MAX_K>(w, ids.data(), dists.data()); });
    fast_ids = ids; fast_dists = dists;
  };
  if (kind == 0) {
    const uint32_t ld = (d + 15u) & ~15u;
    const float r2 = rd<float>(f, 1)[0];
    uint8_t *codes = aligned_copy(rd<uint8_t>(f, (size_t)n * ld));
    const auto xx = rd<uint32_t>(f, n);
    uint8_t *qc = aligned_copy(rd<uint8_t>(f, (size_t)nq * ld));
    const auto qq = rd<uint32_t>(f, nq);
    SqArgs a;
    a.codes = codes; a.xx = xx.data(); a.qcodes = qc; a.qq = qq.data(); a.ld = (int)ld; a.dot = (int)dot; a.r2 = r2; a.w = w;
    simt_launch_lds(sq_scan_lds(ld, (int)cap), nq * nprobes, 256, [&] { sq_scan_kernel(a); });
    merge();
    simt_launch_lds(sq_replay_lds(ld, (int)keff), nq, 64, [&] { sq_exact_kernel(a, ids.data(), dists.data()); });
    free(codes); free(qc);
  } else {
    const uint32_t cb = d / 8;
    uint8_t *codes = aligned_copy(rd<uint8_t>(f, (size_t)n * cb));
    const auto add = rd<float>(f, n), scale = rd<float>(f, n);
    const auto pdists = rd<float>(f, (size_t)nq * nprobes);
    const auto q = rd<float>(f, (size_t)nq * d), cent = rd<float>(f, (size_t)nlist * d), pt = rd<float>(f, (size_t)d * d);
    RqArgs a;
    a.codes = codes; a.add = add.data(); a.scale = scale.data(); a.pdists = pdists.data(); a.q = q.data(); a.cent = cent.data(); a.pt = pt.data();
    a.d = (int)d; a.dot = (int)dot; a.sqrt_d = std::sqrt((float)d); a.w = w;
    if ((size_t)4 * d > (size_t)8 * cap) { printf("the rotated query of d = %u does not fit %u entries\n", d, cap); return 3; }
    simt_launch_lds(rq_scan_lds(d, (int)cap), nq * nprobes, 256, [&] { rq_scan_kernel(a); });
    merge();
    simt_launch_lds(rq_replay_lds(d, (int)keff), nq, 64, [&] { rq_exact_kernel(a, ids.data(), dists.data()); });
    free(codes);
  }
  fclose(f);
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  wr(o, pkey.data(), pkey.size()); wr(o, ppos.data(), ppos.size()); wr(o, pcnt.data(), pcnt.size()); wr(o, pamb.data(), pamb.size());
  wr(o, fast_ids.data(), fast_ids.size()); wr(o, fast_dists.data(), fast_dists.size()); wr(o, flags.data(), flags.size());
  wr(o, ids.data(), ids.size()); wr(o, dists.data(), dists.size());
  fclose(o);
  puts("ok");
  return 0;
}
