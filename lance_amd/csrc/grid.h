// grid.h -- sizes of one-dimensional launches.  Host arithmetic only, no HIP types: tests/c/grid_main.cpp compiles it alone.
#pragma once
#include <algorithm>
#include <cstdint>

namespace lh {

// HIP counts a grid in WORK-ITEMS with 32 bits: blocks x threads per block must stay below 2^32.  One thread per byte of a
// column-sized array crosses that long before the row count does -- 2^25 rows of 128-byte SQ codes are 2^32 threads -- and such a launch
// did not cover its rows (tests/test_zz_gpu_large_columns.py: the last list of an IVF_SQ index was left unwritten).  Kernels whose item
// count is not bounded by their caller walk their items with a grid-stride loop over grid_stride_blocks(items) workgroups.
constexpr uint64_t GRID_MAX_WORK_ITEMS = (1ull << 32) - 1;
constexpr unsigned GRID_STRIDE_MAX_BLOCKS = 1u << 20;      // 2^28 threads of 256: every CU busy many times over, far below the limit

// max_blocks: a smaller cap where a kernel was tuned with one (the SQ element passes: 2048; index maintenance: 65536)
inline unsigned grid_stride_blocks(uint64_t items, unsigned block = 256, unsigned max_blocks = GRID_STRIDE_MAX_BLOCKS) {
  const uint64_t want = (items + block - 1) / block;
  return (unsigned)std::max<uint64_t>(1, std::min<uint64_t>(want, std::min(max_blocks, GRID_STRIDE_MAX_BLOCKS)));
}

// a launch of `blocks` workgroups of `block` threads that does NOT loop: true when the grid can be expressed
inline bool grid_fits(uint64_t blocks, unsigned block) { return blocks < (1ull << 31) && blocks * block <= GRID_MAX_WORK_ITEMS; }

}  // namespace lh
