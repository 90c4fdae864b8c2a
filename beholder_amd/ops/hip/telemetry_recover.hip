// Salvage the frames of a damaged capture on the GPU (gfx950): the device half of
// `python -m beholder_amd recover --device gpu` (beholder_amd/recover.py, ops/gpu_recover.py).
//
// Input is the capture as it lies in the file, n <= 2^28 bytes, and no frame index: the framing is
// what is broken. Every table is per byte offset. Output is the list of the walk's nodes and, per node,
// where its frame starts; the host cuts the gaps out of its own copy of the bytes.
//
// The stages, each its own launch (or launches) on one stream:
//
//  candidates, rc_candidates, one lane per byte offset. The block's 256 bytes and the 16 behind them
//    are staged in LDS with 16-byte loads, and header and topic byte are put together from there. A lane
//    whose header does not fit leaves at once, which is almost every lane. The others read the body
//    from global memory (candidate_of_header, telemetry_recover.hpp) and store one flag byte and
//    end[p]. An offset whose decode is the host's (RC_ASK_HOST, upb only) goes to the overflow list
//    through an atomic cursor; the host writes its flag back before the next stage.
//  next anchor, three launches in the shape of the extract's scan, over the n + 1 values
//    (anchor(q) ? q : n) with a min, from the back:
//      rc_next_reduce   per block of 256 offsets, the block's minimum;
//      rc_next_totals   one block scans the minima from the last tile to the first with a running
//                       carry: sfx[b] is the minimum of blocks b and later, sfx[blocks] = n;
//      rc_next_apply    per block, thread t takes the block's offset 255 - t, so the forward scan in
//                       LDS is the suffix minimum: next[p] is the first anchor at or behind p, or n.
//                       The successor is fused in: succ[p] from flags, end and next[p + 1], which is the
//                       neighbour thread's value or sfx[b + 1] (successor, telemetry_recover.hpp).
//  reach, rc_reach_init and doubling_rounds(n) launches of rc_reach_round. reach[start] = 1 with
//    start = 0, or next[0] when the part is entered with a gap open. In each round every p with
//    reach[p] stores 1 to reach[jump[p]], and jump'[p] = jump[jump[p]] goes to the other buffer, so a
//    round reads only the previous powers. A node marked early in a round only marks nodes that are
//    reachable anyway, and stores of the same 1 do not race for a value: the final set is exact and
//    the same from run to run. Nothing is read back between rounds.
//  mark, rc_mark: keep_len[p] = 1 for a reached, decided offset, else 0. The extract's scan
//    (bh_select_scan) compacts those into the ascending list of the walk's nodes.
//  resolve, rc_resolve, one lane per node: where the node's frame starts (the node itself where it is
//    well framed, else next[p + 1], n for none) and whether the node is well framed.
//
// Visibility is the fold's rule: within a launch workgroups meet only in atomics (the overflow
// cursor) and in the reach bytes, where every store is the same 1; every other plain load reads what
// an earlier launch or the host wrote. No kernel waits for another workgroup.
#include "block_min_scan.hpp"
#include "launch_grid.hpp"
#include "telemetry_recover.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;     // offsets per block in every kernel here
constexpr int STAGE_WORDS = BLOCK / 16 + 1;  // the block's bytes and a halo of 16, in 16-byte words

template <int DIALECT>
__global__ __launch_bounds__(BLOCK) void rc_candidates(const uint8_t* __restrict__ buf, int n, int decided, int max_frame,
                                                       uint8_t* __restrict__ flags, int32_t* __restrict__ end,
                                                       uint32_t* __restrict__ cursor, int32_t* __restrict__ overflow) {
  __shared__ uint4 stage[STAGE_WORDS];
  const int first = blockIdx.x * BLOCK;
  // buf holds at least ceil(n / 256) * 256 + 16 bytes and is 16-byte aligned (the entry point checks)
  if (threadIdx.x < STAGE_WORDS) stage[threadIdx.x] = reinterpret_cast<const uint4*>(buf + first)[threadIdx.x];
  __syncthreads();
  const int p = first + threadIdx.x;
  if (p >= n) return;
  int e = n, f = 0;
  if (p < decided && p + 4 <= n) {
    const uint8_t* near = reinterpret_cast<const uint8_t*>(stage) + threadIdx.x;  // near[0 .. 4]: inside the halo
    const uint32_t L = static_cast<uint32_t>(near[0]) | static_cast<uint32_t>(near[1]) << 8 |
                       static_cast<uint32_t>(near[2]) << 16 | static_cast<uint32_t>(near[3]) << 24;
    f = candidate_of_header<DIALECT>(buf, n, max_frame, p, L, near[4], e);
    if (f & RC_ASK_HOST) overflow[atomicAdd(cursor, 1u)] = p;  // at most one per offset: stays below n
  }
  flags[p] = static_cast<uint8_t>(f);
  end[p] = e;
}

__device__ __forceinline__ int32_t anchor_or_n(const uint8_t* __restrict__ flags, int n, int p) {
  return p < n && (flags[p] & RC_ANCHOR) ? p : n;
}

__global__ __launch_bounds__(BLOCK) void rc_next_reduce(const uint8_t* __restrict__ flags, int n,
                                                        int32_t* __restrict__ mins) {
  __shared__ int32_t wave_mins[BLOCK / 64];
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  int32_t total;
  block_min_scan<BLOCK>(anchor_or_n(flags, n, p), wave_mins, total);
  if (threadIdx.x == 0) mins[blockIdx.x] = total;
}

// One block. sfx[b] = min(mins[b], ..., mins[blocks - 1]) for b in [0, blocks), sfx[blocks] = n.
__global__ __launch_bounds__(BLOCK) void rc_next_totals(const int32_t* __restrict__ mins, int blocks, int n,
                                                        int32_t* __restrict__ sfx) {
  __shared__ int32_t wave_mins[BLOCK / 64];
  int32_t carry = n;
  if (threadIdx.x == 0) sfx[blocks] = n;
  for (int top = blocks - 1; top >= 0; top -= BLOCK) {  // the trip count is the same for every thread
    const int b = top - static_cast<int>(threadIdx.x);
    int32_t total;
    const int32_t incl = block_min_scan<BLOCK>(b >= 0 ? mins[b] : n, wave_mins, total);
    if (b >= 0) sfx[b] = incl < carry ? incl : carry;
    if (total < carry) carry = total;
  }
}

// Covers the n + 1 offsets 0 .. n: next[n] = succ[n] = n.
__global__ __launch_bounds__(BLOCK) void rc_next_apply(const uint8_t* __restrict__ flags, const int32_t* __restrict__ end,
                                                       int n, int decided, const int32_t* __restrict__ sfx,
                                                       int32_t* __restrict__ next, int32_t* __restrict__ succ) {
  __shared__ int32_t wave_mins[BLOCK / 64];
  __shared__ int32_t behind[BLOCK];  // behind[t]: the first anchor at or behind thread t's offset
  const int t = threadIdx.x;
  const int p = blockIdx.x * BLOCK + (BLOCK - 1 - t);
  const int32_t later = sfx[blockIdx.x + 1];
  int32_t total;
  int32_t mine = block_min_scan<BLOCK>(anchor_or_n(flags, n, p), wave_mins, total);
  if (later < mine) mine = later;
  behind[t] = mine;
  __syncthreads();
  if (p > n) return;
  next[p] = mine;
  succ[p] = p == n ? n : successor(flags, end, n, decided, p, t > 0 ? behind[t - 1] : later);
}

__global__ void rc_reach_init(const int32_t* __restrict__ next, int resync, uint8_t* __restrict__ reach) {
  reach[resync ? next[0] : 0] = 1;  // next[0] <= n, and reach holds n + 1
}

// jump_in, jump_out and reach hold n + 1 entries, and every jump lies in [0, n].
__global__ __launch_bounds__(BLOCK) void rc_reach_round(const int32_t* __restrict__ jump_in,
                                                        int32_t* __restrict__ jump_out, uint8_t* reach, int n) {
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  if (p > n) return;
  const int j = jump_in[p];
  if (reach[p]) reach[j] = 1;
  jump_out[p] = jump_in[j];
}

__global__ __launch_bounds__(BLOCK) void rc_mark(const uint8_t* __restrict__ reach, int n, int decided,
                                                 int32_t* __restrict__ keep_len) {
  const int p = blockIdx.x * BLOCK + threadIdx.x;
  if (p < n) keep_len[p] = p < decided && reach[p] ? 1 : 0;
}

__global__ __launch_bounds__(BLOCK) void rc_resolve(const int32_t* __restrict__ nodes, int count,
                                                    const uint8_t* __restrict__ flags, const int32_t* __restrict__ next,
                                                    int32_t* __restrict__ frame_at, uint8_t* __restrict__ framed) {
  const int k = blockIdx.x * BLOCK + threadIdx.x;
  if (k >= count) return;
  const int p = nodes[k];  // a decided offset: below n
  const bool wf = (flags[p] & RC_WF) != 0;
  frame_at[k] = wf ? p : next[p + 1];
  framed[k] = wf ? 1 : 0;
}

bool sized(int n, int decided) { return n >= 1 && n <= RC_LIMIT && decided >= 0 && decided <= n; }

}  // namespace

// C ABI for ctypes (ops/gpu_recover.py). All pointers are device pointers from torch tensors on the
// caller's device; `stream` is the torch stream (hipStream_t). Each returns a hipError_t, launches
// nothing for n <= 0 and refuses n > 2^28. `decided` is recover.decided_end: n for the last part.

// candidates.
//   buf, padded  the bytes, 16-byte aligned, in a buffer of `padded` >= ceil(n / 256) * 256 + 16 bytes
//   dialect      0 = upb, 1 = protobufjs
//   flags        n + 1 uint8; [0, n) written
//   end          n int32, written for every offset: end(p), or n where p is not well framed
//   cursor       one uint32, zeroed by the caller: the length of `overflow` afterwards
//   overflow     n int32: the offsets left to the host, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_recover_candidates(
    const void* buf, long long padded, int n, int decided, int max_frame, int dialect, void* flags, void* end,
    void* cursor, void* overflow, void* stream) {
  if (n <= 0) return 0;
  if (!sized(n, decided) || (dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) || max_frame < 1 ||
      max_frame > (16 << 20) || !buf || (reinterpret_cast<uintptr_t>(buf) & 15) != 0 ||
      padded < static_cast<long long>(blocks_of(n, BLOCK)) * BLOCK + 16 || !flags || !end || !cursor || !overflow)
    return static_cast<int>(hipErrorInvalidValue);
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  auto* f = static_cast<uint8_t*>(flags);
  auto* e = static_cast<int32_t*>(end);
  auto* c = static_cast<uint32_t*>(cursor);
  auto* o = static_cast<int32_t*>(overflow);
  if (dialect == DIALECT_PROTOBUFJS)
    hipLaunchKernelGGL(rc_candidates<DIALECT_PROTOBUFJS>, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, st, b, n, decided,
                       max_frame, f, e, c, o);
  else
    hipLaunchKernelGGL(rc_candidates<DIALECT_UPB>, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, st, b, n, decided,
                       max_frame, f, e, c, o);
  return static_cast<int>(hipGetLastError());
}

// next anchor and successor. With blocks = ceil((n + 1) / 256):
//   mins         `blocks` int32, scratch
//   sfx          `blocks + 1` int32, scratch
//   next, succ   n + 1 int32 each
extern "C" __attribute__((visibility("default"))) int bh_recover_next(
    const void* flags, const void* end, int n, int decided, void* mins, void* sfx, void* next, void* succ,
    void* stream) {
  if (n <= 0) return 0;
  if (!sized(n, decided) || !flags || !end || !mins || !sfx || !next || !succ)
    return static_cast<int>(hipErrorInvalidValue);
  const int blocks = blocks_of(static_cast<long long>(n) + 1, BLOCK);
  auto st = static_cast<hipStream_t>(stream);
  const auto* f = static_cast<const uint8_t*>(flags);
  auto* mn = static_cast<int32_t*>(mins);
  auto* sx = static_cast<int32_t*>(sfx);
  hipLaunchKernelGGL(rc_next_reduce, dim3(blocks), dim3(BLOCK), 0, st, f, n, mn);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return static_cast<int>(err);
  hipLaunchKernelGGL(rc_next_totals, dim3(1), dim3(BLOCK), 0, st, mn, blocks, n, sx);
  err = hipGetLastError();
  if (err != hipSuccess) return static_cast<int>(err);
  hipLaunchKernelGGL(rc_next_apply, dim3(blocks), dim3(BLOCK), 0, st, f, static_cast<const int32_t*>(end), n, decided,
                     sx, static_cast<int32_t*>(next), static_cast<int32_t*>(succ));
  return static_cast<int>(hipGetLastError());
}

// reach: the init and doubling_rounds(n) rounds.
//   next         bh_recover_next's
//   jump, spare  n + 1 int32 each: `jump` holds succ on entry; both are scratch afterwards
//   reach        n + 1 uint8, zeroed by the caller: 1 at every node of the walk afterwards (and at n)
//   resync       1: the part is entered with a gap open at 0
extern "C" __attribute__((visibility("default"))) int bh_recover_reach(
    const void* next, void* jump, void* spare, void* reach, int n, int resync, void* stream) {
  if (n <= 0) return 0;
  if (n > RC_LIMIT || !next || !jump || !spare || !reach || (resync != 0 && resync != 1))
    return static_cast<int>(hipErrorInvalidValue);
  auto st = static_cast<hipStream_t>(stream);
  auto* r = static_cast<uint8_t*>(reach);
  auto* in = static_cast<int32_t*>(jump);
  auto* out = static_cast<int32_t*>(spare);
  hipLaunchKernelGGL(rc_reach_init, dim3(1), dim3(1), 0, st, static_cast<const int32_t*>(next), resync, r);
  hipError_t err = hipGetLastError();
  const int grid = blocks_of(static_cast<long long>(n) + 1, BLOCK);
  for (int round = doubling_rounds(n); round > 0 && err == hipSuccess; --round) {
    hipLaunchKernelGGL(rc_reach_round, dim3(grid), dim3(BLOCK), 0, st, in, out, r, n);
    err = hipGetLastError();
    auto* swap = in;
    in = out;
    out = swap;
  }
  return static_cast<int>(err);
}

// mark. keep_len: n int32, written for every offset.
extern "C" __attribute__((visibility("default"))) int bh_recover_mark(const void* reach, int n, int decided,
                                                                      void* keep_len, void* stream) {
  if (n <= 0) return 0;
  if (!sized(n, decided) || !reach || !keep_len) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(rc_mark, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(reach), n, decided, static_cast<int32_t*>(keep_len));
  return static_cast<int>(hipGetLastError());
}

// resolve. nodes: the scan's `indices`, of which the first `count` are the walk's nodes, each below n.
//   frame_at     `count` int32;  framed  `count` uint8
extern "C" __attribute__((visibility("default"))) int bh_recover_resolve(
    const void* nodes, int count, const void* flags, const void* next, void* frame_at, void* framed, void* stream) {
  if (count <= 0) return 0;
  if (count > RC_LIMIT || !nodes || !flags || !next || !frame_at || !framed)
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(rc_resolve, dim3(blocks_of(count, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const int32_t*>(nodes), count, static_cast<const uint8_t*>(flags),
                     static_cast<const int32_t*>(next), static_cast<int32_t*>(frame_at), static_cast<uint8_t*>(framed));
  return static_cast<int>(hipGetLastError());
}
