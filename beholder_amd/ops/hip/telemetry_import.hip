// Read NDJSON rows back into a framed capture on the GPU (gfx950): the device half of
// `python -m beholder_amd import --device gpu` (beholder_amd/import_rows.py, ops/gpu_import.py).
//
// Input is text as it lies in the file, with a `\n` after its last line: what `export` writes, or
// what jq, DuckDB or an editor made of it. Nothing frames it, so the first two kernels find the lines;
// after them `starts[n_lines + 1]` plays the part that the host's `offs` play for every other command.
// Output is a framed stream (telemetry_import.hpp): the length headers, the tags and varints, the
// strings unescaped and the base64 decoded, every byte of it computed here.
//
// Four kernels, with the extract's scan (telemetry_select.hip, bh_select_scan) run twice between them:
//
//  count, im_count, a block per tile of 4096 bytes: each of 256 lanes loads 16 bytes wide and counts
//    their `\n` bytes (newline_mask); the block's sum is the tile's count. The scan over the tiles'
//    counts gives every tile the number of newlines before it, and the one word that says how many
//    lines there are.
//  starts, im_starts, the same tiles: a lane's newlines get their rank from the block-wide scan of the
//    lanes' counts plus the tile's base, and newline `rank` at byte p writes starts[rank + 1] = p + 1.
//  classify, im_classify, one lane per line. Reads the row with import_classify and stores its 48-byte
//    plan and keep_len[m], the frame's exact length, 0 for a blank line. A line the device does not
//    write (IM_HOST) goes to the overflow list through an atomic cursor with keep_len 0; the host
//    asks import_rows.frame_of_row and scatters the lengths of its frames into keep_len before the
//    scan. Events, base64 rows and blank lines are counted per block in LDS, then by one atomic each.
//  emit, im_emit, in the shape of the export's ex_emit: a wave takes 64 lines and writes the frames
//    the device plans one after the other at their output offsets pos[m]. Every lane loads its own
//    line's plan once; the plan of the line in hand is read from its lane into scalar registers.
//    Wherever a frame's byte is a function of its position (the header, tags and varints, base64, a
//    string without escapes) lane b produces bytes b, b + 64, ... with frame_byte. A string whose
//    text has escapes is walked in pieces of 64 text bytes: a ballot of the backslashes, with a carry
//    between the pieces, gives the mask of the bytes that begin a unit (Pieces::next), a lane's place
//    is the count of the mask's bits below it, and a beginning lane writes its one byte (unit_byte).
//    Host rows have a span in the output (their scattered length) that this kernel leaves alone.
//
// Visibility is the fold's rule: within a launch workgroups meet only in atomics (the cursor, the
// counts); every plain load reads what an earlier launch or the host wrote. No kernel waits for
// another workgroup. Every lane's loops are bounded by the line's own length.
#include "block_scan.hpp"
#include "launch_grid.hpp"
#include "telemetry_import.hpp"
#include "wave_lane.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;  // threads per block
static_assert(SPLIT_TILE_BYTES == BLOCK * SPLIT_LANE_BYTES, "a block takes one tile");

// counters[]: ops/gpu_import.py reads the same layout
constexpr int C_EVENTS = 0, C_CARRIED = 1, C_BLANK = 2, C_OVERFLOW = 3;

__global__ __launch_bounds__(BLOCK) void im_count(const uint8_t* __restrict__ buf, int64_t size,
                                                  int32_t* __restrict__ tile_counts) {
  __shared__ uint64_t wave_sums[BLOCK / 64];
  const int64_t at = static_cast<int64_t>(blockIdx.x) * SPLIT_TILE_BYTES + threadIdx.x * SPLIT_LANE_BYTES;
  uint64_t total;
  block_scan<BLOCK>(static_cast<uint64_t>(__popc(newline_mask(buf, size, at))), wave_sums, total);
  if (threadIdx.x == 0) tile_counts[blockIdx.x] = static_cast<int32_t>(total);
}

// pos[tile] & 0xffffffff is the number of newlines in the tiles before this one.
__global__ __launch_bounds__(BLOCK) void im_starts(const uint8_t* __restrict__ buf, int64_t size,
                                                   const uint64_t* __restrict__ pos, int n_lines,
                                                   int32_t* __restrict__ starts) {
  __shared__ uint64_t wave_sums[BLOCK / 64];
  const int64_t at = static_cast<int64_t>(blockIdx.x) * SPLIT_TILE_BYTES + threadIdx.x * SPLIT_LANE_BYTES;
  uint32_t mask = newline_mask(buf, size, at);
  const uint64_t mine = static_cast<uint64_t>(__popc(mask));
  uint64_t total;
  const uint64_t incl = block_scan<BLOCK>(mine, wave_sums, total);
  int64_t rank = static_cast<int64_t>(pos[blockIdx.x] & 0xffffffffull) + static_cast<int64_t>(incl - mine);
  if (blockIdx.x == 0 && threadIdx.x == 0) starts[0] = 0;
  while (mask) {  // at most 16 turns
    const int k = __ffs(mask) - 1;
    mask &= mask - 1;
    // rank < n_lines wherever n_lines is the scan's total; the check keeps the store inside starts whatever it is
    if (rank < n_lines) starts[rank + 1] = static_cast<int32_t>(at + k + 1);
    ++rank;
  }
}

__global__ __launch_bounds__(BLOCK) void im_classify(const uint8_t* __restrict__ buf, const int32_t* __restrict__ starts,
                                                     int n, FramePlan* __restrict__ plans,
                                                     int32_t* __restrict__ keep_len, uint32_t* __restrict__ counters,
                                                     int32_t* __restrict__ overflow) {
  __shared__ uint32_t local[3];
  if (threadIdx.x < 3) local[threadIdx.x] = 0;
  __syncthreads();
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n) {
    FramePlan plan;
    const int kind = import_classify(buf, starts[m], starts[m + 1] - 1, plan);  // the line without its newline
    if (kind == IM_HOST) overflow[atomicAdd(&counters[C_OVERFLOW], 1u)] = m;  // at most one per line: stays below n
    else atomicAdd(&local[kind == IM_BLANK ? C_BLANK : kind == IM_B64 ? C_CARRIED : C_EVENTS], 1u);
    plans[m] = plan;
    keep_len[m] = plan.out_len;
  }
  __syncthreads();
  if (threadIdx.x < 3 && local[threadIdx.x]) atomicAdd(&counters[threadIdx.x], local[threadIdx.x]);
}

// Bytes [from, to) of the frame in hand to out + d, lane b taking from + b, from + b + 64, ...
__device__ __forceinline__ void plain_bytes(const uint8_t* __restrict__ buf, const FramePlan& plan,
                                            uint8_t* __restrict__ out, int d, int from, int to, int lane) {
  for (int b = from + lane; b < to; b += 64) out[d + b] = static_cast<uint8_t>(frame_byte(buf, plan, b));
}

// The len bytes that the text buf[off, off + text) decodes to, to out + d: pieces of 64 text bytes,
// one per lane. Every lane of the wave is here, with the same arguments but its own `lane`.
__device__ __forceinline__ void unescaped_bytes(const uint8_t* __restrict__ buf, int off, int text, int len,
                                                uint8_t* __restrict__ out, int d, int lane) {
  Pieces pieces;
  int cursor = 0;  // wave-uniform: the bytes of the pieces before this one
  for (int piece = 0; piece < text; piece += 64) {
    const int k = piece + lane;
    const bool live = k < text;
    const uint32_t c = live ? buf[off + k] : 0u;
    const uint64_t begins = pieces.next(__ballot(c == '\\'), __ballot(c == 'u'), __ballot(live));
    const int place = cursor + __popcll(begins & ((1ull << lane) - 1));
    // place < len for a text that read_string measured; the check keeps the store inside the frame whatever it holds
    if (((begins >> lane) & 1) && place < len) out[d + place] = static_cast<uint8_t>(unit_byte(buf + off, k, text));
    cursor += __popcll(begins);
  }
}

// One wave per 64 lines; pos[m] & 0xffffffff is line m's output byte offset.
__global__ __launch_bounds__(BLOCK) void im_emit(const uint8_t* __restrict__ buf, const FramePlan* __restrict__ plans,
                                                 const uint64_t* __restrict__ pos, int n, uint8_t* __restrict__ out) {
  const int m = blockIdx.x * BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  FramePlan mine{IM_BLANK, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  int my_dst = 0;
  if (m < n) {
    mine = plans[m];
    my_dst = static_cast<int>(pos[m] & 0xffffffffull);
  }
  unsigned long long todo = __ballot(mine.kind == IM_B64 || mine.kind == IM_STATUS || mine.kind == IM_PROGRESS);
  while (todo) {  // wave-uniform
    const int i = __ffsll(todo) - 1;
    todo &= todo - 1;
    // the line in hand is lane i's: its plan goes to scalar registers, one memory round trip for all
    // 64 lines instead of one per line
    const FramePlan plan{from_lane(mine.kind, i),      from_lane(mine.topic, i),     from_lane(mine.id_off, i),
                         from_lane(mine.id_text, i),   from_lane(mine.id_len, i),    from_lane(mine.host_off, i),
                         from_lane(mine.host_text, i), from_lane(mine.host_len, i),  from_lane(mine.status, i),
                         from_lane(mine.progress, i),  from_lane(mine.out_len, i),   0};
    const int d = from_lane(my_dst, i);
    int at = 0;  // what is written of the frame
    if (plan.kind != IM_B64 && (plan.id_text != plan.id_len || plan.host_text != plan.host_len)) {
      int32_t id_start, host_start;
      string_starts(plan, id_start, host_start);
      if (plan.id_text != plan.id_len) {
        plain_bytes(buf, plan, out, d, at, id_start, lane);
        unescaped_bytes(buf, plan.id_off, plan.id_text, plan.id_len, out, d + id_start, lane);
        at = id_start + plan.id_len;
      }
      if (plan.host_text != plan.host_len) {
        plain_bytes(buf, plan, out, d, at, host_start, lane);
        unescaped_bytes(buf, plan.host_off, plan.host_text, plan.host_len, out, d + host_start, lane);
        at = host_start + plan.host_len;
      }
    }
    plain_bytes(buf, plan, out, d, at, plan.out_len, lane);
  }
}

constexpr long long SIZE_LIMIT = 1ll << 31;  // starts are int32

}  // namespace

// C ABI for ctypes (ops/gpu_import.py). All pointers are device pointers from torch tensors on the
// caller's device; `stream` is the torch stream (hipStream_t). Each returns a hipError_t and launches
// nothing where there is nothing to do.

// count.
//   buf          the text, 16-byte aligned
//   size         its length, below 2^31
//   tile_counts  (size + 4095) / 4096 int32, written for every tile: its `\n` bytes
extern "C" __attribute__((visibility("default"))) int bh_import_count(const void* buf, long long size, void* tile_counts,
                                                                      void* stream) {
  if (size <= 0) return 0;
  if (size >= SIZE_LIMIT || !buf || (reinterpret_cast<uintptr_t>(buf) & 15u) || !tile_counts)
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(im_count, dim3(blocks_of(size, SPLIT_TILE_BYTES)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(buf), static_cast<int64_t>(size), static_cast<int32_t*>(tile_counts));
  return static_cast<int>(hipGetLastError());
}

// starts, after the scan over tile_counts.
//   pos          one uint64 per tile, the scan's: the low word is the count of `\n` before the tile
//   n_lines      the scan's total: the `\n` bytes of the text
//   starts       n_lines + 1 int32, all written: starts[0] = 0, starts[k + 1] = one past newline k
extern "C" __attribute__((visibility("default"))) int bh_import_starts(const void* buf, long long size, const void* pos,
                                                                       int n_lines, void* starts, void* stream) {
  if (size <= 0) return 0;
  if (size >= SIZE_LIMIT || n_lines < 0 || n_lines > size || !buf || (reinterpret_cast<uintptr_t>(buf) & 15u) || !pos ||
      !starts)
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(im_starts, dim3(blocks_of(size, SPLIT_TILE_BYTES)), dim3(BLOCK), 0,
                     static_cast<hipStream_t>(stream), static_cast<const uint8_t*>(buf), static_cast<int64_t>(size),
                     static_cast<const uint64_t*>(pos), n_lines, static_cast<int32_t*>(starts));
  return static_cast<int>(hipGetLastError());
}

// classify.
//   starts       n + 1 int32 from bh_import_starts: line m is buf[starts[m], starts[m + 1] - 1)
//   plans        n FramePlan (48 bytes each), written for every line
//   keep_len     n int32, written for every line: the frame's length, 0 for a blank line and for one
//                left to the host
//   counters     4 uint32, zeroed by the caller: frames from json rows, frames from b64 rows, blank
//                lines (the host's lines are in none of the three), and the length of `overflow`
//   overflow     n int32: the lines left to the host, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_import_classify(const void* buf, const void* starts, int n,
                                                                         void* plans, void* keep_len, void* counters,
                                                                         void* overflow, void* stream) {
  if (n <= 0) return 0;
  if (!buf || !starts || !plans || !keep_len || !counters || !overflow) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(im_classify, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(buf), static_cast<const int32_t*>(starts), n,
                     static_cast<FramePlan*>(plans), static_cast<int32_t*>(keep_len), static_cast<uint32_t*>(counters),
                     static_cast<int32_t*>(overflow));
  return static_cast<int>(hipGetLastError());
}

// emit, after the scan over keep_len (with the host's lengths scattered in).
//   plans        classify's
//   pos          n uint64, the scan's: output index << 32 | output byte offset of every line
//   out          the output buffer, exactly the scan's total of bytes: a planned line m is written at
//                [pos[m], pos[m] + plans[m].out_len), which the scan placed inside it
extern "C" __attribute__((visibility("default"))) int bh_import_emit(const void* buf, int n, const void* plans,
                                                                     const void* pos, void* out, void* stream) {
  if (n <= 0) return 0;
  if (!buf || !plans || !pos || !out) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(im_emit, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(buf), static_cast<const FramePlan*>(plans),
                     static_cast<const uint64_t*>(pos), n, static_cast<uint8_t*>(out));
  return static_cast<int>(hipGetLastError());
}
