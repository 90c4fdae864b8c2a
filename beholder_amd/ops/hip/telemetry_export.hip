// Write a capture as NDJSON rows on the GPU (gfx950): the device half of
// `python -m beholder_amd export --device gpu` (beholder_amd/export.py, ops/gpu_export.py).
//
// Input is what the fold takes (telemetry_fold.hip): the capture as it lies in the file and
// `offs[n + 1]`, the frame starts from the host's one pass over the length headers. Output is text:
// one row per frame (telemetry_export.hpp), every byte of it computed here: the key text, the decimal
// digits, the JSON string escapes and the base64.
//
// Two kernels, with the extract's scan (telemetry_select.hip, bh_select_scan) between them:
//
//  classify, ex_classify, one lane per frame. Reads the frame by its topic (export_classify, upb in its
//    STRICT form) and stores its 48-byte plan and keep_len[m], the row's exact length, 0 for a dropped
//    frame. A frame the device does not write (EX_HOST) goes to the overflow list through an atomic
//    cursor with keep_len 0; the host asks export.row_of and scatters the lengths of its rows into
//    keep_len before the scan. Events, decode errors, other topics and rows too long for any output
//    are counted per block in LDS, then by one atomic each.
//  emit, ex_emit, in the shape of the normalise's nm_emit: a wave takes 64 frames and writes the rows
//    the device plans one after the other at their output offsets pos[m]. Every lane loads its own
//    frame's plan once; the plan of the frame in hand is read from its lane into scalar registers.
//    Wherever a row's byte is a constant-time function of its position (key text, digits, the name,
//    base64, a string without escapes) lane b produces bytes b, b + 64, ... with row_byte:
//    consecutive lanes, consecutive bytes. A string with escapes has no such function: it is walked
//    in pieces of 64 input bytes, each lane takes one byte, its width (1, 2 or 6) goes through a
//    wave-wide prefix sum, and the lane writes its bytes at the cursor plus the widths before it.
//    Host frames have a span in the output (their scattered length) that this kernel leaves alone:
//    the host splices their bytes in after readback and never looks at what the device left there.
//
// Visibility is the fold's rule: within a launch workgroups meet only in atomics (the cursor, the
// counts); every plain load reads what an earlier launch or the host wrote. No kernel waits for
// another workgroup. Every lane's loops are bounded by the frame's own length.
#include "launch_grid.hpp"
#include "telemetry_export.hpp"
#include "wave_lane.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;  // threads per block

// counters[]: ops/gpu_export.py reads the same layout
constexpr int C_EVENTS = 0, C_ERRORS = 1, C_OTHER = 2, C_TOO_LONG = 3, C_OVERFLOW = 4;

template <int DIALECT>
__global__ __launch_bounds__(BLOCK) void ex_classify(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                     int n, int drop, uint64_t base, RowPlan* __restrict__ plans,
                                                     int32_t* __restrict__ keep_len, uint32_t* __restrict__ counters,
                                                     int32_t* __restrict__ overflow) {
  __shared__ uint32_t local[4];
  if (threadIdx.x < 4) local[threadIdx.x] = 0;
  __syncthreads();
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n) {
    const int head = offs[m], end = offs[m + 1];
    RowPlan plan;
    const int kind = export_classify<DIALECT>(buf, head, end, drop != 0, base + static_cast<uint64_t>(m), plan);
    if (kind == EX_HOST) overflow[atomicAdd(&counters[C_OVERFLOW], 1u)] = m;  // at most one per frame: stays below n
    else if (kind == EX_STATUS || kind == EX_PROGRESS) atomicAdd(&local[C_EVENTS], 1u);
    else if (kind == EX_TOO_LONG) atomicAdd(&local[C_TOO_LONG], 1u);
    else atomicAdd(&local[plan.topic == 1 || plan.topic == 2 ? C_ERRORS : C_OTHER], 1u);
    plans[m] = plan;
    keep_len[m] = plan.row_len;
  }
  __syncthreads();
  if (threadIdx.x < 4 && local[threadIdx.x]) atomicAdd(&counters[threadIdx.x], local[threadIdx.x]);
}

// Bytes [from, to) of the row in hand to out + d, lane b taking from + b, from + b + 64, ...
__device__ __forceinline__ void plain_bytes(const uint8_t* __restrict__ buf, const RowPlan& plan, uint64_t index,
                                            uint8_t* __restrict__ out, int d, int from, int to, int lane) {
  for (int b = from + lane; b < to; b += 64) out[d + b] = static_cast<uint8_t>(row_byte(buf, plan, index, b));
}

// The JSON text of buf[off, off + len) to out + d: pieces of 64 input bytes, one per lane. Every lane
// of the wave is here, with the same arguments but its own `lane`.
__device__ __forceinline__ void escaped_bytes(const uint8_t* __restrict__ buf, int off, int len,
                                              uint8_t* __restrict__ out, int d, int lane) {
  int cursor = 0;  // wave-uniform: the text bytes of the pieces before this one
  for (int piece = 0; piece < len; piece += 64) {
    const int k = piece + lane;
    const bool live = k < len;
    const uint32_t c = live ? buf[off + k] : 0u;
    const int w = live ? esc_width(c) : 0;
    int before = w;  // an inclusive prefix sum over the wave
    for (int step = 1; step < 64; step <<= 1) {
      const int up = __shfl_up(before, step, 64);
      if (lane >= step) before += up;
    }
    const int total = __shfl(before, 63, 64);
    before -= w;
    for (int j = 0; j < w; ++j) out[d + cursor + before + j] = static_cast<uint8_t>(esc_byte(c, j));
    cursor += total;
  }
}

// One wave per 64 frames; pos[m] & 0xffffffff is frame m's output byte offset.
__global__ __launch_bounds__(BLOCK) void ex_emit(const uint8_t* __restrict__ buf, const RowPlan* __restrict__ plans,
                                                 const uint64_t* __restrict__ pos, int n, uint64_t base,
                                                 uint8_t* __restrict__ out) {
  const int m = blockIdx.x * BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  RowPlan mine{0, 0, 0, 0, 0, 0, 0, 0, EX_DROP, 0, 0, 0};
  int my_dst = 0;
  if (m < n) {
    mine = plans[m];
    my_dst = static_cast<int>(pos[m] & 0xffffffffull);
  }
  unsigned long long todo = __ballot(mine.kind == EX_B64 || mine.kind == EX_STATUS || mine.kind == EX_PROGRESS);
  const uint64_t first = base + static_cast<uint64_t>(m - lane);  // the index of lane 0's frame
  while (todo) {  // wave-uniform
    const int i = __ffsll(todo) - 1;
    todo &= todo - 1;
    // the frame in hand is lane i's: its plan goes to scalar registers, one memory round trip for
    // all 64 frames instead of one per frame
    const RowPlan plan{from_lane(mine.id_off, i),   from_lane(mine.id_len, i),   from_lane(mine.status, i),
                       from_lane(mine.progress, i), from_lane(mine.host_off, i), from_lane(mine.host_len, i),
                       from_lane(mine.id_esc, i),   from_lane(mine.host_esc, i), from_lane(mine.kind, i),
                       from_lane(mine.topic, i),    from_lane(mine.row_len, i),  0};
    const int d = from_lane(my_dst, i);
    const uint64_t index = first + static_cast<uint64_t>(i);
    int at = 0;  // what is written of the row
    if (plan.kind != EX_B64 && (plan.id_esc != plan.id_len || plan.host_esc != plan.host_len)) {
      int32_t id_start, host_start;
      string_starts(plan, index, id_start, host_start);
      if (plan.id_esc != plan.id_len) {
        plain_bytes(buf, plan, index, out, d, at, id_start, lane);
        escaped_bytes(buf, plan.id_off, plan.id_len, out, d + id_start, lane);
        at = id_start + plan.id_esc;
      }
      if (plan.host_esc != plan.host_len) {
        plain_bytes(buf, plan, index, out, d, at, host_start, lane);
        escaped_bytes(buf, plan.host_off, plan.host_len, out, d + host_start, lane);
        at = host_start + plan.host_esc;
      }
    }
    plain_bytes(buf, plan, index, out, d, at, plan.row_len, lane);
  }
}

}  // namespace

// C ABI for ctypes (ops/gpu_export.py). All pointers are device pointers from torch tensors on the
// caller's device; `stream` is the torch stream (hipStream_t). Each returns a hipError_t and launches
// nothing for n <= 0.

// classify.
//   dialect      0 = upb, 1 = protobufjs
//   drop         0: undecoded frames become base64 rows; 1: they are dropped
//   base         the index of frame 0 in the whole input: frame m's row says base + m
//   plans        n RowPlan (48 bytes each), written for every frame
//   keep_len     n int32, written for every frame: the row's length, 0 for a dropped frame, for one
//                left to the host and for one whose row would reach 2^31 bytes
//   counters     5 uint32, zeroed by the caller: decoded events, decode errors, other topics (the
//                host's frames are in none of the three), rows too long, and the length of `overflow`
//   overflow     n int32: the frames left to the host, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_export_classify(
    const void* buf, const void* offs, int n, int dialect, int drop, long long base, void* plans, void* keep_len,
    void* counters, void* overflow, void* stream) {
  if (n <= 0) return 0;
  if ((dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) || (drop != 0 && drop != 1) || base < 0 || !buf ||
      !offs || !plans || !keep_len || !counters || !overflow)
    return static_cast<int>(hipErrorInvalidValue);
  const int grid = blocks_of(n, BLOCK);
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  const auto first = static_cast<uint64_t>(base);
  auto* pl = static_cast<RowPlan*>(plans);
  auto* kl = static_cast<int32_t*>(keep_len);
  auto* c = static_cast<uint32_t*>(counters);
  auto* ov = static_cast<int32_t*>(overflow);
  if (dialect == DIALECT_PROTOBUFJS)
    hipLaunchKernelGGL(ex_classify<DIALECT_PROTOBUFJS>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, drop, first, pl, kl, c,
                       ov);
  else
    hipLaunchKernelGGL(ex_classify<DIALECT_UPB>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, drop, first, pl, kl, c, ov);
  return static_cast<int>(hipGetLastError());
}

// emit, after the scan over keep_len (with the host's lengths scattered in).
//   base         classify's
//   plans        classify's
//   pos          n uint64, the scan's: output index << 32 | output byte offset of every frame
//   out          the output buffer, exactly the scan's total of bytes: a planned frame m is written
//                at [pos[m], pos[m] + plans[m].row_len), which the scan placed inside it
extern "C" __attribute__((visibility("default"))) int bh_export_emit(const void* buf, int n, long long base,
                                                                     const void* plans, const void* pos, void* out,
                                                                     void* stream) {
  if (n <= 0) return 0;
  if (base < 0 || !buf || !plans || !pos || !out) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(ex_emit, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(buf), static_cast<const RowPlan*>(plans),
                     static_cast<const uint64_t*>(pos), n, static_cast<uint64_t>(base), static_cast<uint8_t*>(out));
  return static_cast<int>(hipGetLastError());
}
