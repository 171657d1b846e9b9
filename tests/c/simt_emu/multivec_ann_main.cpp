// multivec_ann_main.cpp -- the device code of lance_amd/csrc/multivec_ann.hip (sort, score, select) on the CPU, a thread per lane
// (simt_emu.h), built with AddressSanitizer + UBSan by tests/test_multivec_ann_kernels_cpu.py, which cuts the kernels' text out of the
// source into multivec_ann_device_code.inc.  Every global buffer is a heap block of exactly the elements the library asks its scratch
// arena for, so an index that strays by one element is reported; every launch states its dynamic LDS, which must stay within 64 KiB,
// and the bytes behind it are guarded.  The launch sequence is mva_score_enqueue's.
//
//   in : u32 B, keff, k_out, lists;  u64 q_offsets[B + 1];  u64 cand_ids[lists * keff];  f32 cand_dists[lists * keff]
//   out: u64 ids[B * k_out];  f32 dists[B * k_out];  u32 cursor[B]
#include "simt_emu.h"

#include "multivec_ann_device_code.inc"

template <typename T>
struct Block {      // exactly n elements, in a malloc block of their own
  T *p;
  size_t n;
  explicit Block(size_t n_) : p(static_cast<T *>(malloc(n_ * sizeof(T) + (n_ == 0)))), n(n_) {}
  Block(const Block &) = delete;
  ~Block() { free(p); }
};

static FILE *fin, *fout;
static void rd(void *p, size_t bytes) { if (bytes && fread(p, 1, bytes, fin) != bytes) { fprintf(stderr, "short input\n"); exit(2); } }
static void wr(const void *p, size_t bytes) { if (bytes && fwrite(p, 1, bytes, fout) != bytes) { fprintf(stderr, "short output\n"); exit(2); } }
static uint32_t rd32() { uint32_t v; rd(&v, 4); return v; }
static uint64_t cdiv(uint64_t a, uint64_t b) { return (a + b - 1) / b; }

// a launch with `lds` bytes of dynamic LDS: within 64 KiB, and nothing behind them is written
constexpr size_t GUARD = 4096;
static size_t max_lds = 0;
static void launch_lds(size_t lds, unsigned gx, unsigned gy, const std::function<void()> &kernel) {
  if (lds > 65536) { printf("dynamic LDS of %zu bytes\n", lds); exit(3); }
  max_lds = std::max(max_lds, lds);
  memset(smem, 0x5A, lds);            // a kernel must not count on zeroed LDS
  memset(smem + lds, 0xA5, GUARD);
  simt_launch(gx, gy, MVA_THREADS, kernel);
  for (size_t i = 0; i < GUARD; ++i)
    if ((unsigned char)smem[lds + i] != 0xA5) { printf("LDS byte %zu behind the %zu of the launch was written\n", i, lds); exit(3); }
}

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  fin = fopen(argv[1], "rb"); fout = fopen(argv[2], "wb");
  if (!fin || !fout) return 2;
  const uint32_t B = rd32(), keff = rd32(), k_out = rd32(), lists = rd32();
  if (keff < 1 || keff > (uint32_t)MVA_MAX_KEFF || k_out < 1 || k_out > (uint32_t)MVA_SEL / 2) { fprintf(stderr, "limits\n"); return 2; }
  std::vector<uint64_t> q_offsets(B + 1);
  rd(q_offsets.data(), (B + 1) * 8);
  if (q_offsets[0] != 0 || q_offsets[B] != lists) { fprintf(stderr, "offsets\n"); return 2; }
  const size_t entries = (size_t)lists * keff;
  Block<uint64_t> cand_ids(entries), srid(entries), out_rid(entries), ids((size_t)B * k_out);
  Block<float> cand_dists(entries), ssim(entries), lmin(lists), dists((size_t)B * k_out);
  Block<uint32_t> ln(lists), lq(lists), qf(B + 1), cursor(B), out_key(entries);
  rd(cand_ids.p, entries * 8); rd(cand_dists.p, entries * 4);
  uint64_t max_nqv = 0;
  for (uint32_t b = 0; b < B; ++b) {
    const uint64_t nqv = q_offsets[b + 1] - q_offsets[b];
    if (nqv < 1 || nqv > (uint64_t)MVA_MAX_NQV) { fprintf(stderr, "nqv\n"); return 2; }
    for (uint64_t l = q_offsets[b]; l < q_offsets[b + 1]; ++l) lq.p[l] = b;
    qf.p[b] = (uint32_t)q_offsets[b];
    max_nqv = std::max(max_nqv, nqv);
  }
  qf.p[B] = lists;
  memset(cursor.p, 0, (size_t)B * 4);
  MvaArgs a;
  a.cand_ids = cand_ids.p; a.cand_dists = cand_dists.p; a.keff = (int)keff;
  a.P = 1;
  while ((uint32_t)a.P < keff) a.P <<= 1;
  a.srid = srid.p; a.ssim = ssim.p; a.ln = ln.p; a.lmin = lmin.p; a.list_query = lq.p; a.q_first = qf.p; a.cursor = cursor.p;
  a.out_key = out_key.p; a.out_rid = out_rid.p;
  launch_lds((size_t)a.P * 12 + 16, lists, 1, [&] { mva_sort_kernel(a); });
  launch_lds((size_t)MVA_MAX_NQV * 8 + 16, lists, 1, [&] { mva_score_kernel(a); });
  uint64_t nb = std::max<uint64_t>(1, cdiv(max_nqv * keff, MVA_SEL));
  const uint64_t nb1 = cdiv(nb * k_out, MVA_SEL);
  Block<uint32_t> sk0(nb > 1 ? (size_t)B * nb * k_out : 0), sk1(nb > 1 ? (size_t)B * nb1 * k_out : 0);
  Block<uint64_t> sr0(nb > 1 ? (size_t)B * nb * k_out : 0), sr1(nb > 1 ? (size_t)B * nb1 * k_out : 0);
  uint32_t *sk[2] = {sk0.p, sk1.p};
  uint64_t *sr[2] = {sr0.p, sr1.p};
  MvaSel s;
  s.in_key = a.out_key; s.in_rid = a.out_rid; s.q_first = qf.p; s.cnt = a.cursor; s.keff = (int)keff; s.in_stride = 0; s.n_in = 0; s.k = (int)k_out;
  int cur = -1, rounds = 0;
  for (;;) {
    const bool last = nb == 1;
    const int nxt = cur == 0 ? 1 : 0;
    s.out_key = last ? nullptr : sk[nxt]; s.out_rid = last ? nullptr : sr[nxt];
    s.ids = last ? ids.p : nullptr; s.dists = last ? dists.p : nullptr;
    launch_lds((size_t)MVA_SEL * 12, (unsigned)nb, B, [&] { mva_select_kernel(s); });
    ++rounds;
    if (last) break;
    s.in_key = sk[nxt]; s.in_rid = sr[nxt]; s.q_first = nullptr; s.cnt = nullptr;
    s.in_stride = s.n_in = nb * k_out;
    nb = cdiv(nb * k_out, MVA_SEL);
    cur = nxt;
  }
  printf("largest dynamic LDS %zu bytes, %d selection rounds\n", max_lds, rounds);
  wr(ids.p, (size_t)B * k_out * 8); wr(dists.p, (size_t)B * k_out * 4); wr(cursor.p, (size_t)B * 4);
  fclose(fout);
  puts("ok");
  return 0;
}
