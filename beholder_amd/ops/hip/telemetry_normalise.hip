// Rewrite a capture's events in canonical form on the GPU (gfx950): the device half of
// `python -m beholder_amd normalise --device gpu` (beholder_amd/normalise.py, ops/gpu_normalise.py).
//
// Input is what the fold takes (telemetry_fold.hip): the capture as it lies in the file and
// `offs[n + 1]`, the frame starts from the host's one pass over the length headers. Output is a
// framed stream again, but not a cut of the input: every decoded event is written as the service's
// encoder would write it (telemetry_normalise.hpp), so an output frame has a length of its own.
//
// Two kernels, with the extract's scan (telemetry_select.hip, bh_select_scan) between them:
//
//  classify, nm_classify, one lane per frame. Reads the frame by its topic (norm_classify, upb in its
//    STRICT form) and stores its 32-byte plan and keep_len[m], the output frame's length: the
//    canonical length of a decoded event, the input length of a frame that stays as it is, 0 for a
//    dropped one. A frame the device does not write (NM_HOST) goes to the overflow list through an
//    atomic cursor with keep_len 0; the host asks normalise.canon_of and scatters the lengths of its
//    frames into keep_len before the scan. Events, decode errors and other topics are counted per
//    block in LDS, then by one atomic each.
//  emit, nm_emit, in the shape of the extract's gather_walk: a wave takes 64 frames and writes the
//    ones the device plans one after the other, lane b producing bytes b, b + 64, ... of the frame
//    at its output offset pos[m]: consecutive lanes, consecutive bytes. Every lane loads its own
//    frame's plan once; the plan of the frame in hand is read from its lane into scalar registers,
//    so it is wave-uniform and costs no memory round trip per frame; tag and varint bytes come from
//    canon_byte, string bytes from the input span. Where the output length equals the input length
//    each lane compares its bytes with the input's and a ballot decides whether the event was
//    rewritten; an event of another length is rewritten by definition. Host frames have a span in
//    the output (their scattered length) that this kernel leaves alone: the host splices their bytes
//    in after readback and never looks at what the device left there.
//
// Visibility is the fold's rule: within a launch workgroups meet only in atomics (the cursor, the
// counts); every plain load reads what an earlier launch or the host wrote. No kernel waits for
// another workgroup. Every lane's loops are bounded by the frame's own length.
#include "launch_grid.hpp"
#include "telemetry_normalise.hpp"
#include "wave_lane.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;  // threads per block

// counters[]: ops/gpu_normalise.py reads the same layout
constexpr int C_EVENTS = 0, C_ERRORS = 1, C_OTHER = 2, C_OVERFLOW = 3, C_REWRITTEN = 4;

template <int DIALECT>
__global__ __launch_bounds__(BLOCK) void nm_classify(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                     int n, int drop, Plan* __restrict__ plans,
                                                     int32_t* __restrict__ keep_len, uint32_t* __restrict__ counters,
                                                     int32_t* __restrict__ overflow) {
  __shared__ uint32_t local[3];
  if (threadIdx.x < 3) local[threadIdx.x] = 0;
  __syncthreads();
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n) {
    const int head = offs[m], end = offs[m + 1];
    Plan plan;
    const int kind = norm_classify<DIALECT>(buf, head, end, drop != 0, plan);
    if (kind == NM_HOST) overflow[atomicAdd(&counters[C_OVERFLOW], 1u)] = m;  // at most one per frame: stays below n
    else if (kind == NM_STATUS || kind == NM_PROGRESS) atomicAdd(&local[C_EVENTS], 1u);
    else {
      const uint32_t topic = buf[head + 4];
      atomicAdd(&local[topic == 1 || topic == 2 ? C_ERRORS : C_OTHER], 1u);
    }
    plans[m] = plan;
    keep_len[m] = plan.out_len;
  }
  __syncthreads();
  if (threadIdx.x < 3 && local[threadIdx.x]) atomicAdd(&counters[threadIdx.x], local[threadIdx.x]);
}

// One wave per 64 frames; pos[m] & 0xffffffff is frame m's output byte offset.
__global__ __launch_bounds__(BLOCK) void nm_emit(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                 const Plan* __restrict__ plans, const uint64_t* __restrict__ pos, int n,
                                                 uint8_t* __restrict__ out, uint32_t* __restrict__ counters) {
  const int m = blockIdx.x * BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  Plan mine{0, 0, 0, 0, 0, 0, NM_DROP, 0};
  int my_dst = 0, my_head = 0, my_length = 0;
  if (m < n) {
    mine = plans[m];
    my_dst = static_cast<int>(pos[m] & 0xffffffffull);
    my_head = offs[m];
    my_length = offs[m + 1] - my_head;
  }
  unsigned long long todo = __ballot(mine.kind == NM_COPY || mine.kind == NM_STATUS || mine.kind == NM_PROGRESS);
  uint32_t rewritten = 0;  // counted alike in every lane
  while (todo) {  // wave-uniform
    const int i = __ffsll(todo) - 1;
    todo &= todo - 1;
    // the frame in hand is lane i's: its plan goes to scalar registers, one memory round trip for
    // all 64 frames instead of one per frame
    const Plan plan{from_lane(mine.id_off, i),   from_lane(mine.id_len, i),   from_lane(mine.status, i),
                    from_lane(mine.progress, i), from_lane(mine.host_off, i), from_lane(mine.host_len, i),
                    from_lane(mine.kind, i),     from_lane(mine.out_len, i)};
    const int d = from_lane(my_dst, i);
    const int L = plan.out_len;
    if (plan.kind == NM_COPY) {
      const int s = plan.id_off;
      for (int b = lane; b < L; b += 64) out[d + b] = buf[s + b];
      continue;
    }
    const int head = from_lane(my_head, i);
    const bool same_length = from_lane(my_length, i) == L;
    bool differs = false;
    for (int b = lane; b < L; b += 64) {
      const uint32_t byte = canon_byte(buf, plan, b);
      if (same_length) differs |= byte != buf[head + b];
      out[d + b] = static_cast<uint8_t>(byte);
    }
    if (!same_length || __ballot(differs)) ++rewritten;
  }
  if (lane == 0 && rewritten) atomicAdd(&counters[C_REWRITTEN], rewritten);
}

}  // namespace

// C ABI for ctypes (ops/gpu_normalise.py). All pointers are device pointers from torch tensors on the
// caller's device; `stream` is the torch stream (hipStream_t). Each returns a hipError_t and launches
// nothing for n <= 0.

// classify.
//   dialect      0 = upb, 1 = protobufjs
//   drop         0: undecoded frames stay as they are; 1: they are dropped
//   plans        n Plan (32 bytes each), written for every frame
//   keep_len     n int32, written for every frame: the output frame's length, 0 for a dropped frame
//                and for one left to the host
//   counters     5 uint32, zeroed by the caller: decoded events, decode errors, other topics (the
//                host's frames are in none of the three), the length of `overflow`, and the events
//                that a later emit finds rewritten
//   overflow     n int32: the frames left to the host, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_normalise_classify(
    const void* buf, const void* offs, int n, int dialect, int drop, void* plans, void* keep_len, void* counters,
    void* overflow, void* stream) {
  if (n <= 0) return 0;
  if ((dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) || (drop != 0 && drop != 1) || !buf || !offs ||
      !plans || !keep_len || !counters || !overflow)
    return static_cast<int>(hipErrorInvalidValue);
  const int grid = blocks_of(n, BLOCK);
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* pl = static_cast<Plan*>(plans);
  auto* kl = static_cast<int32_t*>(keep_len);
  auto* c = static_cast<uint32_t*>(counters);
  auto* ov = static_cast<int32_t*>(overflow);
  if (dialect == DIALECT_PROTOBUFJS)
    hipLaunchKernelGGL(nm_classify<DIALECT_PROTOBUFJS>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, drop, pl, kl, c, ov);
  else
    hipLaunchKernelGGL(nm_classify<DIALECT_UPB>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, drop, pl, kl, c, ov);
  return static_cast<int>(hipGetLastError());
}

// emit, after the scan over keep_len (with the host's lengths scattered in).
//   plans        classify's
//   pos          n uint64, the scan's: output index << 32 | output byte offset of every frame
//   out          the output buffer, exactly the scan's total of bytes: a planned frame m is written
//                at [pos[m], pos[m] + plans[m].out_len), which the scan placed inside it
//   counters     classify's; [4] counts the rewritten events
extern "C" __attribute__((visibility("default"))) int bh_normalise_emit(
    const void* buf, const void* offs, int n, const void* plans, const void* pos, void* out, void* counters,
    void* stream) {
  if (n <= 0) return 0;
  if (!buf || !offs || !plans || !pos || !out || !counters) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(nm_emit, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(buf), static_cast<const int32_t*>(offs),
                     static_cast<const Plan*>(plans), static_cast<const uint64_t*>(pos), n, static_cast<uint8_t*>(out),
                     static_cast<uint32_t*>(counters));
  return static_cast<int>(hipGetLastError());
}
