// simt_emu.h -- a minimal SIMT stand-in for running a HIP kernel's SOURCE on the CPU, lane by lane: one thread per lane of a
// workgroup, a pthread barrier for __syncthreads, wave-wide votes and shuffles through a shared slot array (workgroups of one wave
// only for __ballot).  Workgroups run one after the other.  Enough for kernels built from barriers, LDS and LDS atomics
// (tests/test_sq_kernels_cpu.py); nothing here models timing, and the packed dot product takes its portable definition.
#pragma once
#include <pthread.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <thread>
#include <vector>

#define __global__
#define __device__
#define __forceinline__ inline
#define __restrict__
#define __launch_bounds__(...)
#define __shared__
struct simt_dim3 { unsigned x = 1, y = 1, z = 1; };
static thread_local simt_dim3 threadIdx, blockIdx;
static simt_dim3 gridDim;
struct uint4 { uint32_t x, y, z, w; };
struct __half { uint16_t bits; };
static inline float __half2float(__half h) {      // binary16 -> binary32, exact
  const uint32_t s = (uint32_t)(h.bits >> 15) << 31, e = (h.bits >> 10) & 31u, m = h.bits & 1023u;
  float f;
  if (e == 0) { f = std::ldexp((float)m, -24); uint32_t u; memcpy(&u, &f, 4); u |= s; memcpy(&f, &u, 4); return f; }
  const uint32_t u = s | (e == 31 ? 0x7F800000u : (e + 112u) << 23) | (m << 13);
  memcpy(&f, &u, 4);
  return f;
}
alignas(16) static char smem[1 << 17];             // the workgroup's dynamic LDS
static pthread_barrier_t simt_barrier;
static uint64_t simt_vote[64];
static double simt_slot[1024];
static inline void __syncthreads() { pthread_barrier_wait(&simt_barrier); }
template <typename T> static inline T atomicAdd(T *p, T v) { return __atomic_fetch_add(p, v, __ATOMIC_SEQ_CST); }
static inline uint32_t __float_as_uint(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static inline float __uint_as_float(uint32_t u) { float f; memcpy(&f, &u, 4); return f; }
static inline double __dsub_rn(double a, double b) { return a - b; }
static inline double __dmul_rn(double a, double b) { return a * b; }
static inline double __ddiv_rn(double a, double b) { return a / b; }
static inline float __fsub_rn(float a, float b) { return a - b; }
static inline float __fmul_rn(float a, float b) { return a * b; }
static inline float __fdiv_rn(float a, float b) { return a / b; }
static inline uint64_t __ballot(bool p) {          // workgroups of ONE wave
  simt_vote[threadIdx.x & 63] = p;
  __syncthreads();
  uint64_t m = 0;
  for (int i = 0; i < 64; ++i) m |= (uint64_t)(simt_vote[i] != 0) << i;
  __syncthreads();
  return m;
}
static inline double __shfl_xor(double v, int o, int) {
  simt_slot[threadIdx.x] = v;
  __syncthreads();
  const double r = simt_slot[threadIdx.x ^ (unsigned)o];
  __syncthreads();
  return r;
}
static inline int __ffsll(long long v) { return __builtin_ffsll(v); }
using std::max;
using std::min;

static inline void simt_launch(unsigned grid_x, unsigned grid_y, unsigned block, const std::function<void()> &kernel) {
  gridDim.x = grid_x; gridDim.y = grid_y;
  for (unsigned by = 0; by < grid_y; ++by)
    for (unsigned bx = 0; bx < grid_x; ++bx) {
      pthread_barrier_init(&simt_barrier, nullptr, block);
      std::vector<std::thread> lanes;
      for (unsigned t = 0; t < block; ++t)
        lanes.emplace_back([&kernel, t, bx, by] { threadIdx.x = t; blockIdx.x = bx; blockIdx.y = by; kernel(); });
      for (auto &l : lanes) l.join();
      pthread_barrier_destroy(&simt_barrier);
    }
}

// a launch with `lds` bytes of dynamic LDS, counted as the library counts them: within 64 KiB, and nothing behind them is written
constexpr size_t SIMT_LDS_GUARD = 4096;
static inline void simt_launch_lds(size_t lds, unsigned grid, unsigned block, const std::function<void()> &kernel) {
  if (lds > 65536) { printf("dynamic LDS of %zu bytes\n", lds); exit(3); }
  memset(smem + lds, 0xA5, SIMT_LDS_GUARD);
  simt_launch(grid, 1, block, kernel);
  for (size_t i = 0; i < SIMT_LDS_GUARD; ++i)
    if ((unsigned char)smem[lds + i] != 0xA5) { printf("LDS byte %zu behind the %zu of the launch was written\n", i, lds); exit(3); }
}
