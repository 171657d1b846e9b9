// Runs the device code of lance_amd/csrc/sq.hip (and of pair_cand.cuh, which its search instantiates) on the CPU (simt_emu.h) under
// AddressSanitizer + UBSan: every buffer has exactly the size the library gives it, so a read past a row or a write past a list is an
// error here, and the search's launches get the dynamic LDS the library's sizing functions give them (simt_launch_lds).  sq_device_code.inc is
// cut out of the sources by tests/test_sq_kernels_cpu.py, which also writes the problem file and compares the outputs with tests/sq_spec.py.
#include "simt_emu.h"

namespace lh {
#include "sq_device_code.inc"
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
static uint8_t *aligned_copy(const uint8_t *src, size_t bytes) {      // 16-byte aligned, NOT padded beyond a multiple of 16
  uint8_t *p = static_cast<uint8_t *>(aligned_alloc(16, std::max<size_t>(16, (bytes + 15) & ~(size_t)15)));
  if (src) memcpy(p, src, bytes); else memset(p, 0, bytes);
  return p;
}

// exactly `bytes` bytes that start `shift` bytes past a 16-byte boundary and end the heap block: the base is off the grid, and a read past
// the last element is an error
struct Shifted {
  void *base = nullptr;
  uint8_t *p;
  Shifted(const void *src, size_t bytes, size_t shift) {
    if (posix_memalign(&base, 16, bytes + shift + (bytes + shift == 0))) exit(2);
    p = static_cast<uint8_t *>(base) + shift;
    if (bytes) memcpy(p, src, bytes);
  }
  Shifted(const Shifted &) = delete;
  ~Shifted() { free(base); }
};

// argv[3] (optional): bytes every caller-owned base is moved off the 16-byte grid -- the codes handed to sq_distance always, the rows
// and keys (f32) when it is a multiple of 4.  The host's gate (lance_hip_sq_distance: `wide`) is applied as the library applies it.
// in: u32 n, d, nlist, nq, nprobes, k, dot, has_allow | f64 lo, hi | f32 x[n][d] | f32 q[nq][d] (the rows / keys AS STORED: normalised
// for cosine) | u32 part[n] (the stable grouping is the caller's: perm follows) | u32 n_kept, perm[n_kept], offs[nlist + 1] |
// u64 row_ids[n] | u32 probes[nq][nprobes] | u32 allow_bits[n_kept / 32 + 4] (if has_allow)
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const size_t shift = argc > 3 ? (size_t)atoi(argv[3]) : 0;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  const auto h = rd<uint32_t>(f, 8);
  const uint32_t n = h[0], d = h[1], nlist = h[2], nq = h[3], nprobes = h[4], k = h[5], dot = h[6], has_allow = h[7];
  const auto b = rd<double>(f, 2);
  const auto x_in = rd<float>(f, (size_t)n * d);
  const auto q_in = rd<float>(f, (size_t)nq * d);
  const size_t fshift = shift % 4 == 0 ? shift : 0;
  const Shifted xs(x_in.data(), x_in.size() * 4, fshift), qs_(q_in.data(), q_in.size() * 4, fshift);
  struct FView { const float *p; const float *data() const { return p; } } x{reinterpret_cast<const float *>(xs.p)}, q{reinterpret_cast<const float *>(qs_.p)};
  if (reinterpret_cast<uintptr_t>(x.p) % 16 != fshift % 16 || reinterpret_cast<uintptr_t>(q.p) % 16 != fshift % 16) return 4;
  const auto nk = rd<uint32_t>(f, 1);
  const uint32_t n_kept = nk[0];
  const auto perm = rd<uint32_t>(f, n_kept);
  const auto offs = rd<uint32_t>(f, nlist + 1);
  const auto row_ids = rd<uint64_t>(f, n);
  const auto probes = rd<uint32_t>(f, (size_t)nq * nprobes);
  const auto allow = rd<uint32_t>(f, has_allow ? n_kept / 32 + 4 : 0);
  fclose(f);
  const double lo = b[0], hi = b[1];
  const uint32_t ld = (d + 15u) & ~15u;
  const float r = (float)(hi - lo), r2 = r * r;

  // bounds of the column, folded on the host as lance_hip_sq_bounds does
  std::vector<double> partials(2 * 3);
  simt_launch(3, 1, 256, [&] { sq_bounds_kernel<float>(x.data(), (int64_t)n * d, partials.data()); });
  double fold[2] = {1.7976931348623157e308, -1.7976931348623157e308};
  for (int i = 0; i < 3; ++i) { fold[0] = std::min(fold[0], partials[2 * i]); fold[1] = std::max(fold[1], partials[2 * i + 1]); }
  // encode rows (tight) and keys (padded)
  std::vector<uint8_t> codes((size_t)n * d, 77);
  simt_launch(3, 1, 256, [&] { sq_encode_kernel<float>(x.data(), (int64_t)n * d, (int)d, (int64_t)d, lo, hi - lo, lo == hi, codes.data()); });
  uint8_t *qc = aligned_copy(nullptr, (size_t)nq * ld);
  simt_launch(2, 1, 256, [&] { sq_encode_kernel<float>(q.data(), (int64_t)nq * d, (int)d, (int64_t)ld, lo, hi - lo, lo == hi, qc); });
  std::vector<uint32_t> qq(nq);
  simt_launch((nq + 255) / 256, 1, 256, [&] { sq_norms_kernel(qc, (int64_t)nq, (int)ld, qq.data()); });
  // distance_all, both row readers
  std::vector<float> dist_words((size_t)nq * n), dist_wide((size_t)nq * n, -1.0f);
  const Shifted cs(codes.data(), codes.size(), shift);
  if (reinterpret_cast<uintptr_t>(cs.p) % 16 != shift % 16) return 4;
  simt_launch((n + 255) / 256, nq, 256, [&] { sq_distance_kernel<false>(cs.p, (int64_t)n, (int)d, qc, (int)ld, (int)dot, r2, dist_words.data()); });
  uint8_t *codes_al = aligned_copy(codes.data(), codes.size());
  if (d % 16 == 0) {      // the second reader as lance_hip_sq_distance picks it for this base
    const uint8_t *cp = shift ? cs.p : codes_al;
    const bool wide = d % 16 == 0 && (reinterpret_cast<uintptr_t>(cp) & 15) == 0;
    printf("sq_distance wide %d\n", (int)wide);
    if (wide) simt_launch((n + 255) / 256, nq, 256, [&] { sq_distance_kernel<true>(cp, (int64_t)n, (int)d, qc, (int)ld, (int)dot, r2, dist_wide.data()); });
    else simt_launch((n + 255) / 256, nq, 256, [&] { sq_distance_kernel<false>(cp, (int64_t)n, (int)d, qc, (int)ld, (int)dot, r2, dist_wide.data()); });
  }
  // the index: gather + norms
  uint8_t *stored = aligned_copy(nullptr, (size_t)n_kept * ld);
  std::vector<uint64_t> rid(n_kept);
  std::vector<uint32_t> xx(n_kept);
  if (n_kept) {
    // (the kernel walks its bytes with a grid-stride loop; 48 workgroups here, a thread each per lane, take the later ones in further turns)
    simt_launch(std::min<size_t>(((size_t)n_kept * ld + 255) / 256, 48), 1, 256, [&] { sq_gather_kernel(codes.data(), row_ids.data(), perm.data(), (int64_t)n_kept, (int)d, (int)ld, stored, rid.data()); });
    simt_launch((n_kept + 255) / 256, 1, 256, [&] { sq_norms_kernel(stored, (int64_t)n_kept, (int)ld, xx.data()); });
  }
  // search: scan, merge, replay
  const size_t pairs = (size_t)nq * nprobes;
  std::vector<uint32_t> pkey(pairs * k), ppos(pairs * k), pcnt(pairs), pamb(pairs), flags(nq + 1, 0);
  std::vector<uint64_t> ids((size_t)nq * k);
  std::vector<float> dists((size_t)nq * k);
  SqArgs a;
  a.codes = stored; a.xx = xx.data(); a.qcodes = qc; a.qq = qq.data(); a.ld = (int)ld; a.dot = (int)dot; a.r2 = r2;
  a.w.row_ids = rid.data(); a.w.part_offsets = offs.data(); a.w.probes = probes.data(); a.w.allow = has_allow ? allow.data() : nullptr;
  a.w.nprobes = (int)nprobes; a.w.k = (int)k; a.w.cap = sq_scan_cap(ld, (int)k);
  a.w.pkey = pkey.data(); a.w.ppos = ppos.data(); a.w.pcnt = pcnt.data(); a.w.pamb = pamb.data(); a.w.flags = flags.data(); a.w.n_replay = flags.data() + nq;
  if (k > (uint32_t)CAND_MAX_K) return 5;
  printf("scan capacity %d\n", a.w.cap);
  simt_launch_lds(sq_scan_lds(ld, a.w.cap), nq * nprobes, 256, [&] { sq_scan_kernel(a); });
  if (k <= (uint32_t)CAND_NARROW_K)      // the merge instance cand_merge_lists picks
    simt_launch_lds(cand_merge_bytes(CAND_MERGE_NARROW), nq, 256, [&] { cand_merge_kernel<CAND_MERGE_NARROW, CAND_NARROW_K>(a.w, ids.data(), dists.data()); });
  else
    simt_launch_lds(cand_merge_bytes(CAND_MERGE_WIDE), nq, 256, [&] { cand_merge_kernel<CAND_MERGE_WIDE, CAND_MAX_K>(a.w, ids.data(), dists.data()); });
  const std::vector<uint64_t> fast_ids = ids;
  simt_launch_lds(sq_replay_lds(ld, (int)k), nq, 64, [&] { sq_exact_kernel(a, ids.data(), dists.data()); });

  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  wr(o, fold, 2); wr(o, codes.data(), codes.size()); wr(o, dist_words.data(), dist_words.size()); wr(o, dist_wide.data(), dist_wide.size());
  wr(o, ids.data(), ids.size()); wr(o, dists.data(), dists.size()); wr(o, flags.data(), flags.size()); wr(o, fast_ids.data(), fast_ids.size());
  fclose(o);
  free(qc); free(codes_al); free(stored);
  puts("ok");
  return 0;
}
