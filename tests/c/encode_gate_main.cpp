// The host's gate of the lane-per-row encoder (lance_amd/csrc/encode_fused.hip: encode_fused_supported) next to the code-row stores of
// its kernel, both cut out of the source by tests/test_encode_gate_cpu.py (encode_gate.inc), built with AddressSanitizer + UBSan: for
// every instantiated shape and every byte offset of the caller's `codes` (and of x / centroids / codebook) the gate is asked, and where
// it answers yes the kernel's own store statements run on a buffer that ends with the last row -- a store wider than the pointer
// allows is a misaligned-store report, one past the rows a heap overflow.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "lance_hip.h"

struct alignas(16) uint4 { uint32_t x, y, z, w; };      // HIP's uint4: 16-byte aligned
static inline uint4 make_uint4(uint32_t x, uint32_t y, uint32_t z, uint32_t w) { return uint4{x, y, z, w}; }

#include "encode_gate.inc"      // bool encode_fused_supported(...); template <int M> void store_row(uint8_t *codes, int64_t row, const uint32_t *packed)

template <int M>
static int shape(int d, int *accepted) {
  const int64_t rows = 5;
  for (int off = 0; off < 32; ++off) {
    void *base = nullptr;
    if (posix_memalign(&base, 64, (size_t)(off + rows * M))) return 2;
    uint8_t *codes = static_cast<uint8_t *>(base) + off;       // [rows][M], the block ends with the last row
    alignas(64) static float model[64];
    for (int dtype = 0; dtype < 3; ++dtype) {
      const size_t es = dtype == LANCE_HIP_F16 ? 2 : (dtype == LANCE_HIP_I8 ? 1 : 4);
      for (int xoff = 0; xoff < 32; xoff += (int)es) {
        const char *x = reinterpret_cast<const char *>(model) + xoff;
        const bool ok = encode_fused_supported(dtype, d, M, 8, x, model, model, codes);
        if (ok && (reinterpret_cast<uintptr_t>(x) % (4 * es)) != 0) { printf("rows accepted at %d bytes off (element %zu)\n", xoff, es); return 1; }
        if (!ok) continue;
        ++*accepted;
        uint32_t packed[(M + 3) / 4];
        for (int i = 0; i < (M + 3) / 4; ++i) packed[i] = 0x03020100u + 0x04040404u * (uint32_t)i;
        for (int64_t row = 0; row < rows; ++row) store_row<M>(codes, row, packed);
        for (int64_t i = 0; i < rows * M; ++i)
          if (codes[i] != (uint8_t)(i % M)) { printf("row bytes differ at offset %d\n", off); return 1; }
        memset(codes, 0xEE, (size_t)(rows * M));
      }
    }
    if (encode_fused_supported(0, d, M, 8, model, model + 1, model, codes) || encode_fused_supported(0, d, M, 8, model, model, model + 2, codes)) {
      puts("model accepted off the 16-byte grid");
      return 1;
    }
    free(base);
  }
  return 0;
}

int main() {
  int accepted = 0;
  int rc = shape<32>(128, &accepted);      // sub-dimension 4
  if (!rc) rc = shape<16>(128, &accepted);
  if (!rc) rc = shape<8>(128, &accepted);
  if (!rc) rc = shape<16>(64, &accepted);
  if (!rc) rc = shape<8>(64, &accepted);
  if (rc) return rc;
  printf("accepted %d\nok\n", accepted);
  return 0;
}
