// Runs take_flat_knn_kernel (lance_amd/csrc/combine.hip) on the CPU (simt_emu.h) under AddressSanitizer + UBSan: every global buffer has
// exactly the size the caller of lance_hip_take_flat_knn gives it, the launch geometry and the dynamic LDS are what the library's own
// functions say (tfk_entries, tfk_rows_per_step, tfk_row_stride, take_flat_knn_bytes), and the bytes behind the LDS of the launch must
// stay untouched.  take_device_code.inc is cut out of the sources by tests/test_knn_combined_kernel_cpu.py, which writes the problem
// file and compares the outputs with tests/knn_combined_spec.py.
#include "simt_emu.h"

static inline float __fmaf_rn(float a, float b, float c) { return std::fmaf(a, b, c); }

namespace lh {
enum { METRIC_L2 = 0, METRIC_COSINE = 1, METRIC_DOT = 2 };
#include "take_device_code.inc"
}
using namespace lh;

template <typename T>
static std::vector<T> rd(FILE *f, size_t n) {
  std::vector<T> v(n);
  if (n && fread(v.data(), sizeof(T), n, f) != n) { puts("short read"); exit(2); }
  return v;
}

// a launch with `lds` bytes of dynamic LDS (up to the 160 KiB of a workgroup, as far as the emulator's array goes): nothing behind them is written
static void launch_guarded(size_t lds, unsigned grid, const std::function<void()> &kernel) {
  if (lds + SIMT_LDS_GUARD > sizeof(smem)) { printf("dynamic LDS of %zu bytes\n", lds); exit(3); }
  memset(smem + lds, 0xA5, SIMT_LDS_GUARD);
  simt_launch(grid, 1, 256, kernel);
  for (size_t i = 0; i < SIMT_LDS_GUARD; ++i)
    if ((unsigned char)smem[lds + i] != 0xA5) { printf("LDS byte %zu behind the %zu of the launch was written\n", i, lds); exit(3); }
}

template <typename TR>
static void run(int metric, const TakeArgs &a, const void *x, unsigned nq, size_t lds) {
  const TR *xp = static_cast<const TR *>(x);
  constexpr bool F16 = sizeof(TR) == 2;
  if (metric == METRIC_COSINE) launch_guarded(lds, nq, [&] { take_flat_knn_kernel<METRIC_COSINE, TR, F16>(a, xp); });
  else if (metric == METRIC_DOT) launch_guarded(lds, nq, [&] { take_flat_knn_kernel<METRIC_DOT, TR, F16>(a, xp); });
  else launch_guarded(lds, nq, [&] { take_flat_knn_kernel<METRIC_L2, TR, false>(a, xp); });
}

// in: u32 dtype (0 f32, 1 f16, 2 i8), metric (0 l2, 1 cosine, 2 dot), n, d, nq, ca, cb, has_dists_b, has_lower, has_upper, k, shift (bytes the
//     column is moved off the 16-byte grid) | u32 lo_key, hi_key | x [n][d] in its element type | f32 q [nq][d] (widened) | u64 ids_a [nq][ca] |
//     u64 ids_b [nq][cb] | f32 dists_b [nq][cb] (if has_dists_b)
// out: u64 ids [nq][k] | f32 dists [nq][k] | u32 flags [nq]
int main(int argc, char **argv) {
  if (argc < 3) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  const auto h = rd<uint32_t>(f, 12);
  const uint32_t dtype = h[0], metric = h[1], n = h[2], d = h[3], nq = h[4], ca = h[5], cb = h[6], has_db = h[7], k = h[10], shift = h[11];
  const auto keys = rd<uint32_t>(f, 2);
  const int esz = dtype == 0 ? 4 : dtype == 1 ? 2 : 1;
  const auto xbytes = rd<uint8_t>(f, (size_t)n * d * esz);
  const auto q = rd<float>(f, (size_t)nq * d);
  const auto ids_a = rd<uint64_t>(f, (size_t)nq * ca);
  const auto ids_b = rd<uint64_t>(f, (size_t)nq * cb);
  const auto dists_b = rd<float>(f, has_db ? (size_t)nq * cb : 0);
  fclose(f);
  // the column: 16-byte aligned plus `shift`, and not one byte longer than its rows
  const size_t xlen = xbytes.size();
  void *xbase = nullptr;
  if (posix_memalign(&xbase, 16, shift + xlen + (shift + xlen == 0)) != 0) return 2;
  uint8_t *x = static_cast<uint8_t *>(xbase) + shift;
  memcpy(x, xbytes.data(), xlen);
  std::vector<uint64_t> out_ids((size_t)nq * k, 0x1111111111111111ull);
  std::vector<float> out_dists((size_t)nq * k, -1.0f);
  std::vector<uint32_t> flags(nq, 0xDEADBEEFu);
  TakeArgs a;
  a.q = q.data(); a.d = (int)d; a.n_rows = n;
  a.ids_a = ids_a.data(); a.ids_b = cb ? ids_b.data() : nullptr; a.dists_b = has_db ? dists_b.data() : nullptr; a.ca = (int)ca; a.cb = (int)cb;
  a.has_lower = (int)h[8]; a.has_upper = (int)h[9]; a.lo_key = keys[0]; a.hi_key = keys[1];
  a.k = (int)k; a.P = tfk_entries((int)(ca + cb));
  a.rows_per_step = tfk_rows_per_step(d, esz);
  a.row_stride = a.rows_per_step > 0 ? (int)tfk_row_stride(d, esz) : 0;
  a.out_ids = out_ids.data(); a.out_dists = out_dists.data(); a.flags = flags.data();
  const size_t lds = take_flat_knn_bytes((int)(ca + cb), d, esz);
  printf("lds %zu rows_per_step %d vec %d\n", lds, a.rows_per_step, (int)((((uintptr_t)x & 15) == 0) && ((size_t)d * esz) % 16 == 0));
  if (dtype == 0) run<float>((int)metric, a, x, nq, lds);
  else if (dtype == 1) run<__half>((int)metric, a, x, nq, lds);
  else run<int8_t>((int)metric, a, x, nq, lds);
  free(xbase);
  FILE *o = fopen(argv[2], "wb");
  if (!o) return 2;
  fwrite(out_ids.data(), 8, out_ids.size(), o); fwrite(out_dists.data(), 4, out_dists.size(), o); fwrite(flags.data(), 4, flags.size(), o);
  fclose(o);
  puts("ok");
  return 0;
}
