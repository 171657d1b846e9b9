// rebalance_main.cpp -- the device code of lance_amd/csrc/rebalance.hip on the CPU, a thread per lane (simt_emu.h), built with
// AddressSanitizer + UBSan by tests/test_rebalance_kernels_cpu.py, which cuts the kernel's text, the exact.cuh functions it calls and the
// host's choice of the route (rb_lds_bytes) out of the sources into rebalance_device_code.inc.  Every global buffer is a heap block of
// exactly the bytes the library's contract gives it, and the workgroup's LDS block is poisoned beyond the bytes the launch asks for, so
// an index that strays by one element is reported.  Two workgroups, so the tile loop runs with a stride.
//
//   argv[3] (optional): bytes the raw vectors' base is moved off the 16-byte grid (a multiple of 4: f32 elements)
//   in : u32 metric, mode, d, n_raw, n, n_cand, part1, part2;  f32 raw[n_raw * d], u64 ids[n], u32 seg_offs[n_cand + 2],
//        f32 seg_cent[(n_cand + 1) * d], u32 cand_ids[n_cand], f32 c12[2 * d] (split only)
//   out: u32 flag, staged (1: table and rows in LDS), dest[n]
#include "simt_emu.h"

#include <sanitizer/asan_interface.h>

#define __host__
static inline float __fmaf_rn(float a, float b, float c) { return std::fmaf(a, b, c); }

#include "rebalance_device_code.inc"

struct Block {      // exactly `bytes` usable bytes, starting `shift` bytes past a 16-byte boundary
  void *base = nullptr;
  uint8_t *p = nullptr;
  size_t bytes = 0;
  explicit Block(size_t n, size_t shift = 0) : bytes(n) {
    if (posix_memalign(&base, 16, n + shift + (n + shift == 0))) exit(2);
    p = static_cast<uint8_t *>(base) + shift;
  }
  Block(const Block &) = delete;
  ~Block() { free(base); }
  template <typename T> T *as() { return reinterpret_cast<T *>(p); }
};

static FILE *fin, *fout;
static void rd(Block &b) { if (b.bytes && fread(b.p, 1, b.bytes, fin) != b.bytes) { fprintf(stderr, "short input\n"); exit(2); } }
static uint32_t rd32() { uint32_t v; if (fread(&v, 4, 1, fin) != 1) { fprintf(stderr, "short input\n"); exit(2); } return v; }

int main(int argc, char **argv) {
  if (argc != 3 && argc != 4) return 2;
  const size_t shift = argc == 4 ? (size_t)atoi(argv[3]) : 0;
  if (shift % 4) return 2;
  fin = fopen(argv[1], "rb"); fout = fopen(argv[2], "wb");
  if (!fin || !fout) return 2;
  const uint32_t metric = rd32(), mode = rd32(), d = rd32(), n_raw = rd32(), n = rd32(), C = rd32(), part1 = rd32(), part2 = rd32();
  if (C > (uint32_t)RB_MAX_CAND || (mode == 1 && C == 0)) return 2;
  Block raw((size_t)n_raw * d * 4, shift), ids((size_t)n * 8), seg((size_t)(C + 2) * 4), cent((size_t)(C + 1) * d * 4), cand((size_t)C * 4);
  Block c12(mode == 0 ? (size_t)2 * d * 4 : 0), dest((size_t)n * 4), flag(4);
  if (reinterpret_cast<uintptr_t>(raw.p) % 16 != shift % 16) return 4;
  rd(raw); rd(ids); rd(seg); rd(cent); rd(cand); rd(c12);
  memset(flag.p, 0, 4);
  memset(dest.p, 0xEE, dest.bytes);
  RbArgs a;
  a.raw = raw.as<float>(); a.n_raw = n_raw; a.ids = ids.as<uint64_t>(); a.n = (int64_t)n; a.seg_offs = seg.as<uint32_t>();
  a.seg_cent = cent.as<float>(); a.cand_ids = cand.as<uint32_t>(); a.c12 = mode == 0 ? c12.as<float>() : nullptr;
  a.dest = dest.as<uint32_t>(); a.flag = flag.as<uint32_t>(); a.d = (int)d; a.n_cand = (int)C; a.join = (int)mode;
  a.part1 = part1; a.part2 = part2;
  const int64_t staged = rb_lds_bytes((int)d, (int)C, a.join);
  a.lds = staged <= 65536 ? 1 : 0;
  const size_t lds = a.lds ? (size_t)staged : (size_t)RB_W_HEAD * 4;
  if (lds > 65536) { fprintf(stderr, "%zu bytes of LDS\n", lds); return 3; }
  ASAN_POISON_MEMORY_REGION(smem + lds, sizeof(smem) - lds);
  if (n > 0) {
    // the library's dispatch: the staged route is an instantiation of its own
    if (metric == 0) simt_launch(2, 1, 256, [&] { a.lds ? rb_reassign_kernel<METRIC_L2, true>(a) : rb_reassign_kernel<METRIC_L2, false>(a); });
    else if (metric == 1) simt_launch(2, 1, 256, [&] { a.lds ? rb_reassign_kernel<METRIC_COSINE, true>(a) : rb_reassign_kernel<METRIC_COSINE, false>(a); });
    else simt_launch(2, 1, 256, [&] { a.lds ? rb_reassign_kernel<METRIC_DOT, true>(a) : rb_reassign_kernel<METRIC_DOT, false>(a); });
  }
  ASAN_UNPOISON_MEMORY_REGION(smem + lds, sizeof(smem) - lds);
  const uint32_t staged_u = (uint32_t)a.lds;
  fwrite(flag.p, 4, 1, fout); fwrite(&staged_u, 4, 1, fout);
  if (dest.bytes) fwrite(dest.p, 1, dest.bytes, fout);
  fclose(fout);
  puts("ok");
  return 0;
}
