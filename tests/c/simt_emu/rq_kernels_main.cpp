// Runs the device code of lance_amd/csrc/rq.hip (and of pair_cand.cuh, which its search instantiates) on the CPU (simt_emu.h) under
// AddressSanitizer + UBSan: every buffer has exactly the size the library gives it, so a read past a row or a write past a list is an
// error here, and the search's launches get the dynamic LDS the library's sizing functions give them (simt_launch_lds).  rq_device_code.inc is
// cut out of the sources by tests/test_rq_kernels_cpu.py, which also writes the problem file and compares the outputs with tests/rq_spec.py.
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
#include "rq_device_code.inc"
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
static uint8_t *aligned_bytes(size_t bytes) {      // 16-byte aligned, NOT padded beyond a multiple of 16
  uint8_t *p = static_cast<uint8_t *>(aligned_alloc(16, std::max<size_t>(16, (bytes + 15) & ~(size_t)15)));
  memset(p, 0, std::max<size_t>(16, (bytes + 15) & ~(size_t)15));
  return p;
}

// exactly `bytes` bytes that start `shift` bytes past a 16-byte boundary and end the heap block
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

// argv[3] (optional): bytes a caller-owned base is moved off the 16-byte grid -- the partition's codes handed to rq_distance always (rows
// of whole 16-byte words are refused there, as lance_hip_rq_distance refuses them: counted, and run aligned), the f32 rows given to
// rq_encode when it is a multiple of 4.
// in: u32 n, d, nlist, nq, nprobes, k, dot, has_allow | f32 x[n][d] | f32 q[nq][d] | f32 cent[nlist][d] | f32 P[d][d] | u32 part[n] |
// f32 dist_v_c[n] | u32 n_kept, perm[n_kept], offs[nlist + 1] | u64 row_ids[n] | u32 probes[nq][nprobes] | f32 pdists[nq][nprobes] |
// f32 dist_q_c[nq][nlist] (every pair, for the per-partition distance kernel) | u32 allow_bits[n_kept / 32 + 4] (if has_allow)
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  const size_t shift = argc > 3 ? (size_t)atoi(argv[3]) : 0;
  unsigned refused = 0;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  const auto h = rd<uint32_t>(f, 8);
  const uint32_t n = h[0], d = h[1], nlist = h[2], nq = h[3], nprobes = h[4], k = h[5], dot = h[6], has_allow = h[7];
  const auto x_in = rd<float>(f, (size_t)n * d);
  const Shifted xs(x_in.data(), x_in.size() * 4, shift % 4 == 0 ? shift : 0);
  struct FView { const float *p; const float *data() const { return p; } } x{reinterpret_cast<const float *>(xs.p)};
  const auto q = rd<float>(f, (size_t)nq * d);
  const auto cent = rd<float>(f, (size_t)nlist * d);
  const auto P = rd<float>(f, (size_t)d * d);
  const auto part = rd<uint32_t>(f, n);
  const auto dvc = rd<float>(f, n);
  const uint32_t n_kept = rd<uint32_t>(f, 1)[0];
  const auto perm = rd<uint32_t>(f, n_kept);
  const auto offs = rd<uint32_t>(f, nlist + 1);
  const auto row_ids = rd<uint64_t>(f, n);
  const auto probes = rd<uint32_t>(f, (size_t)nq * nprobes);
  const auto pdists = rd<float>(f, (size_t)nq * nprobes);
  const auto dqc_all = rd<float>(f, (size_t)nq * nlist);
  const auto allow = rd<uint32_t>(f, has_allow ? n_kept / 32 + 4 : 0);
  fclose(f);
  const uint32_t cb = d / 8;
  const float sqrt_d = std::sqrt((float)d);

  std::vector<float> pt((size_t)d * d);
  simt_launch((d * d + 255) / 256, 1, 256, [&] { rq_transpose_kernel(P.data(), (int)d, pt.data()); });

  // encode: three blocks over all rows
  std::vector<uint8_t> codes((size_t)n * cb, 77);
  std::vector<float> add(n, -1.0f), scale(n, -1.0f);
  RqEncArgs ea;
  ea.x = x.data(); ea.n = n; ea.d = (int)d; ea.nlist = (int)nlist; ea.dot = (int)dot; ea.part = part.data(); ea.dvc = dvc.data(); ea.cent = cent.data();
  ea.pt = pt.data(); ea.sqrt_d = sqrt_d; ea.codes = codes.data(); ea.add = add.data(); ea.scale = scale.data();
  simt_launch(3, 1, 256, [&] { rq_encode_kernel(ea); });

  // the index: gather into partition order
  uint8_t *stored = aligned_bytes((size_t)n_kept * cb);
  std::vector<float> sadd(n_kept), sscale(n_kept);
  std::vector<uint64_t> rid(n_kept);
  if (n_kept)
    simt_launch(((size_t)n_kept * cb + 255) / 256, 1, 256, [&] {
      rq_gather_kernel(codes.data(), add.data(), scale.data(), row_ids.data(), perm.data(), (int64_t)n_kept, (int)cb, stored, sadd.data(), sscale.data(), rid.data());
    });

  // distance_all and distance of every partition's storage against every query's residual
  std::vector<float> dist_out;
  for (uint32_t p = 0; p < nlist; ++p) {
    const uint32_t np = offs[p + 1] - offs[p];
    if (np == 0) continue;
    std::vector<float> qr((size_t)nq * d), dqc(nq);
    for (uint32_t i = 0; i < nq; ++i) {
      dqc[i] = dqc_all[(size_t)i * nlist + p];
      for (uint32_t j = 0; j < d; ++j) qr[(size_t)i * d + j] = q[(size_t)i * d + j] - cent[(size_t)p * d + j];
    }
    // the partition alone: reads past its last row are errors.  lance_hip_rq_distance: "codes of 16-byte rows must be 16-byte aligned"
    const bool refuse = d % 128 == 0 && shift % 16 != 0;
    refused += refuse;
    const Shifted pcs(stored + (size_t)offs[p] * cb, (size_t)np * cb, refuse ? 0 : shift);
    const uint8_t *pc = pcs.p;
    if (reinterpret_cast<uintptr_t>(pc) % 16 != (refuse ? 0 : shift % 16)) return 4;
    for (int quantised = 1; quantised >= 0; --quantised) {
      std::vector<float> out((size_t)nq * np, -7.0f);
      simt_launch(std::min<uint32_t>((np + 255) / 256, 64), nq, 256, [&] {
        rq_distance_kernel(pc, sadd.data() + offs[p], sscale.data() + offs[p], (int64_t)np, (int)d, qr.data(), dqc.data(), pt.data(), (int)dot, quantised,
                           sqrt_d, out.data());
      });
      dist_out.insert(dist_out.end(), out.begin(), out.end());
    }
  }

  // search: scan, merge, replay
  const size_t pairs = (size_t)nq * nprobes;
  std::vector<uint32_t> pkey(pairs * k), ppos(pairs * k), pcnt(pairs), pamb(pairs), flags(nq + 1, 0);
  std::vector<uint64_t> ids((size_t)nq * k);
  std::vector<float> dists((size_t)nq * k);
  RqArgs a;
  a.codes = stored; a.add = sadd.data(); a.scale = sscale.data(); a.pdists = pdists.data(); a.q = q.data(); a.cent = cent.data(); a.pt = pt.data();
  a.d = (int)d; a.dot = (int)dot; a.sqrt_d = sqrt_d;
  a.w.row_ids = rid.data(); a.w.part_offsets = offs.data(); a.w.probes = probes.data(); a.w.allow = has_allow ? allow.data() : nullptr;
  a.w.nprobes = (int)nprobes; a.w.k = (int)k; a.w.cap = rq_scan_cap(d, (int)k);
  a.w.pkey = pkey.data(); a.w.ppos = ppos.data(); a.w.pcnt = pcnt.data(); a.w.pamb = pamb.data(); a.w.flags = flags.data(); a.w.n_replay = flags.data() + nq;
  if (k > (uint32_t)CAND_NARROW_K || (size_t)4 * d > (size_t)8 * a.w.cap) return 5;      // (narrow cases; the host's check of the borrowed buffer)
  simt_launch_lds(rq_scan_lds(d, a.w.cap), nq * nprobes, 256, [&] { rq_scan_kernel(a); });
  simt_launch_lds(cand_merge_bytes(CAND_MERGE_NARROW), nq, 256, [&] { cand_merge_kernel<CAND_MERGE_NARROW, CAND_NARROW_K>(a.w, ids.data(), dists.data()); });
  const std::vector<uint64_t> fast_ids = ids;
  simt_launch_lds(rq_replay_lds(d, (int)k), nq, 64, [&] { rq_exact_kernel(a, ids.data(), dists.data()); });

  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  wr(o, codes.data(), codes.size()); wr(o, add.data(), add.size()); wr(o, scale.data(), scale.size());
  wr(o, dist_out.data(), dist_out.size());
  wr(o, ids.data(), ids.size()); wr(o, dists.data(), dists.size()); wr(o, flags.data(), flags.size()); wr(o, fast_ids.data(), fast_ids.size());
  fclose(o);
  free(stored);
  printf("refused %u\n", refused);
  puts("ok");
  return 0;
}
