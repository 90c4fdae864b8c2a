// The block-wide inclusive scan shared by the extract's prefix sum (telemetry_select.hip) and the
// shard's totals scan (telemetry_shard.hip). Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bh {

// Inclusive scan of one value per thread over the block of BLOCK threads; `total` is the block's
// sum. wave_sums holds one entry per wave. Every thread of the block must call it.
template <int BLOCK>
__device__ __forceinline__ uint64_t block_scan(uint64_t x, uint64_t* wave_sums, uint64_t& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const uint64_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  __syncthreads();  // the previous call's readers are done with wave_sums
  if (lane == 63) wave_sums[wave] = x;
  __syncthreads();
  uint64_t before = 0, all = 0;
  for (int w = 0; w < BLOCK / 64; ++w) {
    const uint64_t t = wave_sums[w];
    if (w < wave) before += t;
    all += t;
  }
  total = all;
  return x + before;
}

}  // namespace bh
