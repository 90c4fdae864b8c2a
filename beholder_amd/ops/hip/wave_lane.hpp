// A value of one lane of the wave as a scalar: what the emit kernels of the rewriting commands
// (telemetry_normalise.hip, telemetry_anonymise.hip, telemetry_export.hip, telemetry_import.hip) read
// the plan of the frame in hand with. Device code only; the plan headers (telemetry_*.hpp) stay free
// of it, so that a host compiler reads them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace bh {

// x of lane i, i the same in every lane: a scalar.
__device__ __forceinline__ int32_t from_lane(int32_t x, int i) { return __builtin_amdgcn_readlane(x, i); }
__device__ __forceinline__ uint32_t from_lane(uint32_t x, int i) {
  return static_cast<uint32_t>(__builtin_amdgcn_readlane(static_cast<int32_t>(x), i));
}

}  // namespace bh
