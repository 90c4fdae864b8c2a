// The block-wide inclusive min-scan of the recover's next-anchor scan (telemetry_recover.hip): the
// sibling of block_scan.hpp, whose operator is a 64-bit add. Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bh {

// Inclusive min-scan of one value per thread over the block of BLOCK threads; `total` is the block's
// minimum. wave_mins holds one entry per wave. Every thread of the block must call it.
template <int BLOCK>
__device__ __forceinline__ int32_t block_min_scan(int32_t x, int32_t* wave_mins, int32_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const int32_t y = __shfl_up(x, d);
    if (lane >= d && y < x) x = y;
  }
  __syncthreads();  // the previous call's readers are done with wave_mins
  if (lane == 63) wave_mins[wave] = x;
  __syncthreads();
  int32_t before = INT32_MAX, all = INT32_MAX;
  for (int w = 0; w < BLOCK / 64; ++w) {
    const int32_t t = wave_mins[w];
    if (w < wave && t < before) before = t;
    if (t < all) all = t;
  }
  total = all;
  return before < x ? before : x;
}

}  // namespace bh
