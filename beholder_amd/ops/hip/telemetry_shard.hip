// Split a framed telemetry stream by media into N framed streams on the GPU (gfx950): the device
// half of `python -m beholder_amd shard --device gpu` (beholder_amd/shard.py, ops/gpu_shard.py).
//
// Input is what the fold, the extract and the coalesce take (telemetry_fold.hip): the capture as it
// lies in the file and `offs[n + 1]`, the frame starts from the host's one pass over the length
// headers. The kernels here end at the arrays the extract's gather takes (telemetry_select.hip
// gather_search, gather_walk), which is called as it is: the output is one buffer with the shards
// back to back, shard 0 first, every shard in stream order.
//
//  route, shard_route, one lane per frame. Reads the frame by its topic (telemetry_readers.hpp, upb
//    in its STRICT form) and decides it (telemetry_shard.hpp route): shard_of[m] is the shard, or -1
//    for a dropped frame. Frames left to the host go to an overflow list through an atomic cursor
//    with shard_of -1; the host decides them and scatters their shards in before the partition.
//  partition, three launches: a stable counting sort of the frames by shard over (1, frame length),
//    both in one 64-bit add as count << 32 | bytes (the input is below 2^31 bytes).
//      shard_count   per block of 1,024 frames (four tiles of 256, a frame per thread and tile: a
//                    quarter of the totals a block of 256 would give), the per-shard totals, summed
//                    in LDS (integer adds, so the order in which they land does not show) and
//                    written shard-major: totals[s * blocks + b];
//      shard_totals  one block scans all shards * blocks totals in tiles of 2048 (8 per thread) with
//                    a running carry. Shard-major order is output order, so base[s * blocks + b] is
//                    where block b's frames of shard s start, base[s * blocks] where shard s starts
//                    and base[shards * blocks] the grand total;
//      shard_apply   per block, every frame's exclusive (rank, bytes) among the earlier frames of
//                    its shard in the block: within the wave by one of two methods (below), across
//                    the tile's waves by per-wave per-shard sums in LDS, across the block's tiles by
//                    a per-shard running sum in LDS that starts at the block's base. That is
//                    pos[m] (output index << 32 | output byte offset); it also writes keep_len[m]
//                    (the length, 0 for a dropped frame) and the compacted out_offs[k], indices[k].
//    The in-wave methods, both exact and both free of any order of arrival:
//      walk    64 fixed steps: lane j's shard and length are read with v_readlane, and every later
//              lane of the same shard adds them. The cost does not depend on the data.
//      ballot  a wave-uniform loop over the shards present in the wave: __ballot finds the lanes of
//              the first undone lane's shard, their rank is a popcount of the mask below the lane
//              and their byte offset a masked 6-step scan. The cost grows with the shards present.
//    ops/gpu_shard.py picks; scripts/gpu_shard_probe.py times both.
//
// Visibility is the fold's rule: within a launch workgroups meet only in atomics (the overflow
// cursor); every plain load reads what an earlier launch or the host wrote. No kernel waits for
// another workgroup, which is why the partition is three launches.
#include "block_scan.hpp"
#include "telemetry_shard.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;           // threads per block
constexpr int TILES = 4;             // a block takes TILES * BLOCK consecutive frames, BLOCK at a time:
                                     // a quarter of the totals; ops/gpu_shard.py BLOCK_FRAMES
constexpr int TOTALS_PER_THREAD = 8; // consecutive totals a thread of shard_totals sums by itself
constexpr int WAVES = BLOCK / 64;
static_assert(BLOCK >= static_cast<int>(MAX_SHARDS), "one thread per shard zeroes and writes the LDS totals");

constexpr int METHOD_WALK = 0, METHOD_BALLOT = 1;

template <int DIALECT>
__global__ __launch_bounds__(BLOCK) void shard_route(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                     int n, const ShardParams s, int32_t* __restrict__ shard_of,
                                                     uint32_t* __restrict__ cursor, int32_t* __restrict__ overflow) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const int r = route<DIALECT>(buf, offs[m], offs[m + 1], s);
  if (r == ROUTE_HOST) overflow[atomicAdd(cursor, 1u)] = m;  // at most one per frame: stays below n
  shard_of[m] = r >= 0 ? r : -1;
}

__device__ __forceinline__ unsigned long long packed(int32_t len) {
  return (1ull << 32) | static_cast<uint32_t>(len);
}

__global__ __launch_bounds__(BLOCK) void shard_count(const int32_t* __restrict__ shard_of,
                                                     const int32_t* __restrict__ offs, int n, uint32_t shards,
                                                     uint64_t* __restrict__ totals) {
  __shared__ unsigned long long tot[MAX_SHARDS];
  if (threadIdx.x < MAX_SHARDS) tot[threadIdx.x] = 0ull;
  __syncthreads();
  BH_UNROLL
  for (int t = 0; t < TILES; ++t) {
    const long long m = (static_cast<long long>(blockIdx.x) * TILES + t) * BLOCK + threadIdx.x;
    if (m < n) {
      const uint32_t s = static_cast<uint32_t>(shard_of[m]);
      if (s < shards) atomicAdd(&tot[s], packed(offs[m + 1] - offs[m]));  // -1 and anything out of range: dropped
    }
  }
  __syncthreads();
  if (threadIdx.x < shards) totals[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x] = tot[threadIdx.x];
}

// One block. base[i] = totals[0] + ... + totals[i - 1] for i in [0, count]; base[count] is the sum.
__global__ __launch_bounds__(BLOCK) void shard_totals(const uint64_t* __restrict__ totals, long long count,
                                                      uint64_t* __restrict__ base) {
  __shared__ uint64_t wave_sums[WAVES];
  uint64_t carry = 0;
  for (long long tile = 0; tile < count; tile += BLOCK * TOTALS_PER_THREAD) {  // the same trip count for every thread
    const long long first = tile + static_cast<long long>(threadIdx.x) * TOTALS_PER_THREAD;
    uint64_t v[TOTALS_PER_THREAD];
    uint64_t sum = 0;
    BH_UNROLL
    for (int k = 0; k < TOTALS_PER_THREAD; ++k) {
      v[k] = first + k < count ? totals[first + k] : 0ull;
      sum += v[k];
    }
    uint64_t total;
    uint64_t run = carry + block_scan<BLOCK>(sum, wave_sums, total) - sum;
    BH_UNROLL
    for (int k = 0; k < TOTALS_PER_THREAD; ++k) {
      if (first + k < count) base[first + k] = run;
      run += v[k];
    }
    carry += total;
  }
  if (threadIdx.x == 0) base[count] = carry;
}

template <int METHOD>
__global__ __launch_bounds__(BLOCK) void shard_apply(const int32_t* __restrict__ shard_of,
                                                     const int32_t* __restrict__ offs, int n, uint32_t shards,
                                                     const uint64_t* __restrict__ base, uint64_t* __restrict__ pos,
                                                     int32_t* __restrict__ keep_len, int32_t* __restrict__ out_offs,
                                                     int32_t* __restrict__ indices) {
  __shared__ unsigned long long wave_tot[WAVES][MAX_SHARDS];  // this tile's sums per wave and shard
  __shared__ unsigned long long before[MAX_SHARDS];           // where the tile's frames of a shard start
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (threadIdx.x < MAX_SHARDS)
    before[threadIdx.x] =
        threadIdx.x < shards ? base[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x] : 0ull;
  if (blockIdx.x == 0 && threadIdx.x == 0) {  // out_offs[kept] = kept bytes, for gather_search
    const uint64_t all = base[static_cast<size_t>(shards) * gridDim.x];
    out_offs[all >> 32] = static_cast<int32_t>(all & 0xffffffffull);  // kept <= n, and out_offs holds n + 1
  }
  for (int t = 0; t < TILES; ++t) {  // the same trip count for every thread: no lane leaves before the end
    // thread s owns column s of wave_tot and before[s] between the tiles: it alone reads and rewrites them
    if (threadIdx.x < MAX_SHARDS) {
      BH_UNROLL
      for (int w = 0; w < WAVES; ++w) wave_tot[w][threadIdx.x] = 0ull;
    }
    __syncthreads();
    const long long m = (static_cast<long long>(blockIdx.x) * TILES + t) * BLOCK + threadIdx.x;
    int key = -1, len = 0;  // -1: no frame here, or a dropped one
    if (m < n) {
      const uint32_t s = static_cast<uint32_t>(shard_of[m]);
      if (s < shards) {
        key = static_cast<int>(s);
        len = offs[m + 1] - offs[m];
      }
    }
    // rank and bytes of the earlier lanes of this wave with the same key
    uint32_t rank = 0, bytes = 0;
    if (METHOD == METHOD_WALK) {
      BH_UNROLL
      for (int j = 0; j < 63; ++j) {  // lane 63 is earlier than nobody
        const int kj = __builtin_amdgcn_readlane(key, j);
        const int lj = __builtin_amdgcn_readlane(len, j);
        if (j < lane && kj == key) {
          ++rank;
          bytes += static_cast<uint32_t>(lj);
        }
      }
    } else {
      const unsigned long long below = (1ull << lane) - 1ull;
      unsigned long long todo = __ballot(key >= 0);
      while (todo) {  // wave-uniform
        const int leader = __ffsll(todo) - 1;
        const int k0 = __shfl(key, leader);
        const bool mine = key == k0;
        const unsigned long long mask = __ballot(mine);
        todo &= ~mask;
        uint32_t v = mine ? static_cast<uint32_t>(len) : 0u;
        for (int d = 1; d < 64; d <<= 1) {
          const uint32_t y = __shfl_up(v, d);
          if (lane >= d) v += y;
        }
        if (mine) {
          rank = static_cast<uint32_t>(__popcll(mask & below));
          bytes = v - static_cast<uint32_t>(len);
        }
      }
    }
    if (key >= 0) atomicAdd(&wave_tot[wave][key], packed(len));
    __syncthreads();
    if (key >= 0) {
      uint64_t p = before[key] + ((static_cast<uint64_t>(rank) << 32) | bytes);
      for (int w = 0; w < WAVES; ++w)
        if (w < wave) p += wave_tot[w][key];
      pos[m] = p;
      keep_len[m] = len;
      const uint32_t k = static_cast<uint32_t>(p >> 32);  // below the kept count, which is at most n
      out_offs[k] = static_cast<int32_t>(p & 0xffffffffull);
      indices[k] = static_cast<int32_t>(m);
    } else if (m < n) {
      pos[m] = 0ull;
      keep_len[m] = 0;
    }
    __syncthreads();  // every lane has read before[] and wave_tot[][]
    if (threadIdx.x < MAX_SHARDS) {
      unsigned long long sum = 0ull;
      BH_UNROLL
      for (int w = 0; w < WAVES; ++w) sum += wave_tot[w][threadIdx.x];
      before[threadIdx.x] += sum;
    }
  }
}

}  // namespace

// C ABI for ctypes (ops/gpu_shard.py). All pointers but `params` are device pointers from torch
// tensors on the caller's device; `stream` is the torch stream (hipStream_t). Each returns a
// hipError_t and launches nothing for n <= 0.

// route. `params` is a host pointer to a ShardParams, copied into the kernel's arguments.
//   dialect      0 = upb, 1 = protobufjs
//   shard_of     n int32, written for every frame: the shard, or -1
//   cursor       one uint32, zeroed by the caller: the length of `overflow` afterwards
//   overflow     n int32: the frames left to the host, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_shard_route(
    const void* buf, const void* offs, int n, int dialect, const void* params, void* shard_of, void* cursor,
    void* overflow, void* stream) {
  if (n <= 0) return 0;
  if ((dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) || !params || !buf || !offs || !shard_of || !cursor ||
      !overflow)
    return static_cast<int>(hipErrorInvalidValue);
  const ShardParams s = *static_cast<const ShardParams*>(params);
  if (s.shards < 1 || s.shards > MAX_SHARDS) return static_cast<int>(hipErrorInvalidValue);
  const int grid = (n + BLOCK - 1) / BLOCK;
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* so = static_cast<int32_t*>(shard_of);
  auto* cu = static_cast<uint32_t*>(cursor);
  auto* ov = static_cast<int32_t*>(overflow);
  if (dialect == DIALECT_PROTOBUFJS)
    hipLaunchKernelGGL(shard_route<DIALECT_PROTOBUFJS>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, s, so, cu, ov);
  else
    hipLaunchKernelGGL(shard_route<DIALECT_UPB>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, s, so, cu, ov);
  return static_cast<int>(hipGetLastError());
}

// partition. With blocks = ceil(n / 1024):
//   shard_of     n int32: a value outside [0, shards) is a dropped frame
//   totals       `shards * blocks` uint64, scratch
//   base         `shards * blocks + 1` uint64; base[s * blocks] is (frames << 32 | bytes) before shard s,
//                base[shards * blocks] the grand total
//   pos          n uint64: output index << 32 | output byte offset of every routed frame, 0 for the others
//   keep_len     n int32: the frame's length, 0 for a dropped frame
//   out_offs     n + 1 int32: the first kept + 1 are the output's frame starts
//   indices      n int32: the first `kept` are the input indices in output order
//   method       0 = walk, 1 = ballot (above)
//   stages       bit 0 count, bit 1 totals, bit 2 apply; the probe times them apart, everything else
//                passes 7. A later stage reads what the earlier ones of an earlier call wrote.
extern "C" __attribute__((visibility("default"))) int bh_shard_partition(
    const void* shard_of, const void* offs, int n, int shards, void* totals, void* base, void* pos, void* keep_len,
    void* out_offs, void* indices, int method, int stages, void* stream) {
  if (n <= 0) return 0;
  if (shards < 1 || shards > static_cast<int>(MAX_SHARDS) || (method != METHOD_WALK && method != METHOD_BALLOT) ||
      stages < 1 || stages > 7 || !shard_of || !offs || !totals || !base || !pos || !keep_len || !out_offs || !indices)
    return static_cast<int>(hipErrorInvalidValue);
  const int blocks = static_cast<int>((static_cast<long long>(n) + BLOCK * TILES - 1) / (BLOCK * TILES));
  const long long count = static_cast<long long>(shards) * blocks;
  if (count >= (1ll << 31)) return static_cast<int>(hipErrorInvalidValue);
  auto st = static_cast<hipStream_t>(stream);
  const auto* so = static_cast<const int32_t*>(shard_of);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* tt = static_cast<uint64_t*>(totals);
  auto* bs = static_cast<uint64_t*>(base);
  const uint32_t S = static_cast<uint32_t>(shards);
  hipError_t err = hipSuccess;
  if (stages & 1) {
    hipLaunchKernelGGL(shard_count, dim3(blocks), dim3(BLOCK), 0, st, so, o, n, S, tt);
    err = hipGetLastError();
    if (err != hipSuccess) return static_cast<int>(err);
  }
  if (stages & 2) {
    hipLaunchKernelGGL(shard_totals, dim3(1), dim3(BLOCK), 0, st, tt, count, bs);
    err = hipGetLastError();
    if (err != hipSuccess) return static_cast<int>(err);
  }
  if (stages & 4) {
    auto* ps = static_cast<uint64_t*>(pos);
    auto* kl = static_cast<int32_t*>(keep_len);
    auto* oo = static_cast<int32_t*>(out_offs);
    auto* ix = static_cast<int32_t*>(indices);
    if (method == METHOD_WALK)
      hipLaunchKernelGGL(shard_apply<METHOD_WALK>, dim3(blocks), dim3(BLOCK), 0, st, so, o, n, S, bs, ps, kl, oo, ix);
    else
      hipLaunchKernelGGL(shard_apply<METHOD_BALLOT>, dim3(blocks), dim3(BLOCK), 0, st, so, o, n, S, bs, ps, kl, oo, ix);
    err = hipGetLastError();
  }
  return static_cast<int>(err);
}
