// Host arithmetic of lance_amd/csrc/grid.h, compiled alone (tests/test_large_column_spec.py): a grid-stride launch never asks for 2^32
// work-items or more, whatever the item count, and still starts a thread for every item of a small array.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "grid.h"

static void require(bool ok, const char *what, unsigned long long v) {
  if (!ok) { fprintf(stderr, "FAILED: %s (%llu)\n", what, v); exit(1); }
}

int main() {
  using namespace lh;
  const uint64_t P = 4099;
  const uint64_t items[] = {0, 1, 255, 256, 257, 1u << 20, (1ull << 25) * 128, ((1ull << 25) + P) * 128,      // the SQ codes of the large-column test
                            ((1ull << 24) + P) * 128, (1ull << 32) - 1, 1ull << 32, (1ull << 32) + 1, ((1ull << 32) - 1) * 4096};
  for (uint64_t n : items) {
    const unsigned b = grid_stride_blocks(n);
    require(b >= 1, "at least one workgroup", n);
    require((uint64_t)b * 256 <= GRID_MAX_WORK_ITEMS, "the grid stays below 2^32 work-items", n);
    require(grid_fits(b, 256), "grid_fits agrees", n);
    require(b <= GRID_STRIDE_MAX_BLOCKS, "capped", n);
    if (n <= (uint64_t)GRID_STRIDE_MAX_BLOCKS * 256) require((uint64_t)b * 256 >= n, "one thread per item below the cap", n);
  }
  // the kernels' loop, `for (g = blockIdx.x * 256 + threadIdx.x; g < n; g += gridDim.x * 256)`, run thread by thread on small arrays under
  // caps of one to three workgroups: every item is visited exactly once, whether the grid covers the array, loops once or many times
  for (unsigned cap = 1; cap <= 3; ++cap) {
    for (uint64_t n : {0ull, 1ull, 255ull, 256ull, 257ull, 511ull, 512ull, 513ull, 767ull, 768ull, 769ull, 5000ull}) {
      const unsigned b = grid_stride_blocks(n, 256, cap);
      require(b >= 1 && b <= cap, "the cap holds", n);
      std::vector<int> seen(n, 0);
      for (unsigned blk = 0; blk < b; ++blk)
        for (unsigned t = 0; t < 256; ++t)
          for (uint64_t g = (uint64_t)blk * 256 + t; g < n; g += (uint64_t)b * 256) ++seen[g];
      for (uint64_t g = 0; g < n; ++g) require(seen[g] == 1, "an item is visited exactly once", g);
    }
  }
  // the launch the large-column test caught: one thread per byte of 2^25 + 4099 rows of 128 code bytes
  const uint64_t blocks = (((1ull << 25) + P) * 128 + 255) / 256;
  require(!grid_fits(blocks, 256), "one thread per code byte does not fit a grid", blocks);
  require((unsigned)(blocks * 256) != blocks * 256, "its work-item count does not fit 32 bits", blocks);
  require(grid_fits(((1ull << 26) - 4 + 3) / 4, 256) && !grid_fits(((1ull << 26) - 3 + 3) / 4, 256), "a wave per row: up to 2^26 - 4 rows", 0);
  printf("ok\n");
  return 0;
}
