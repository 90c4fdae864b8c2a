// Drop the progress events that repeat their media's step, on the GPU (gfx950): the device half of
// `python -m beholder_amd thin --device gpu` (beholder_amd/thin.py, ops/gpu_thin.py).
//
// Input is what the fold takes (telemetry_fold.hip): the capture as it lies in the file and
// `offs[n + 1]`, the frame starts from the host's one pass over the length headers. What comes back
// is a cut: keep_len[m], the frame's whole length where it is kept and 0 where it is dropped, which
// the extract's scan and gather (telemetry_select.hip) turn into the output stream.
//
// Whether a progress event is kept depends on its media's neighbouring progress event in stream
// order, so one media's events must lie next to each other and in stream order: the transitions'
// stable sort by media (telemetry_transitions.hip), called as it is. The stages, each a launch or a
// few on one stream:
//
//  classify, th_classify, one lane per frame. Every frame's keep_len is its whole length. A topic-2
//    frame is read as a TelemetryProgress (telemetry_thin.hpp thin_classify, upb in its STRICT form):
//    the lane counts the decode error (per block in LDS, then one atomic), or hands the frame to the
//    host through the overflow list with its atomic cursor, or writes the event's row
//    {hash, id_off, id_len, status, TR_EVENT}, its mark word marks[m] and is_event[m] = 1. Other
//    topics are not read.
//  claim, rank, compact and sort are the transitions' and the extract's entry points
//    (bh_transitions_claim, bh_select_scan over slot_used and over is_event, bh_transitions_compact,
//    bh_transitions_sort_pass): keys[k] is the media number of the k-th event by media and stream
//    order, vals[k] >> 32 its frame.
//  mark, th_mark, one lane per sorted position k. Its neighbour is k + 1 under `last` and k - 1 under
//    `first`; where that is in range, has the same key and its frame's mark word equals this
//    frame's, the lane stores keep_len[frame] = 0. A frame has one sorted position, so every
//    keep_len word has exactly one writer in this launch; marks[] and keys[] are only read. The
//    neighbour across a block or wave edge is read from global memory like any other. Dropped lanes
//    are counted by wave ballot and one atomic add per wave: one per dropped element would send
//    most of a capture's events to one word.
//
// Visibility is the fold's rule: within a launch workgroups meet only in atomics (the cursor, the
// counts); every plain load reads what an earlier launch or the host wrote. No kernel waits for
// another workgroup. Every lane's loops are bounded by the frame's own length.
#include "launch_grid.hpp"
#include "telemetry_thin.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;  // threads per block

// counters[]: ops/gpu_thin.py reads the same layout; the first two are the transitions'
constexpr int C_PROGRESS_ERR = 0, C_OVERFLOW = 1, C_DROPPED = 2;

template <int DIALECT>
__global__ __launch_bounds__(BLOCK) void th_classify(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                     int n, int32_t step, StatusEvent* __restrict__ rows,
                                                     int32_t* __restrict__ is_event, uint64_t* __restrict__ marks,
                                                     int32_t* __restrict__ keep_len, uint32_t* __restrict__ counters,
                                                     int32_t* __restrict__ overflow) {
  __shared__ uint32_t errors;
  if (threadIdx.x == 0) errors = 0;
  __syncthreads();
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n) {
    const int head = offs[m], end = offs[m + 1];
    StatusEvent ev;
    uint64_t mark;
    const int kind = thin_classify<DIALECT>(buf, head, end, step, ev, mark);
    if (kind == TH_HOST) overflow[atomicAdd(&counters[C_OVERFLOW], 1u)] = m;  // at most one per frame: stays below n
    if (kind == TH_ERROR) atomicAdd(&errors, 1u);
    rows[m] = ev;
    marks[m] = mark;
    is_event[m] = kind == TH_EVENT ? 1 : 0;
    keep_len[m] = end - head;
  }
  __syncthreads();
  if (threadIdx.x == 0 && errors) atomicAdd(&counters[C_PROGRESS_ERR], errors);
}

template <bool FIRST>
__global__ __launch_bounds__(BLOCK) void th_mark(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ vals,
                                                 int events, int n, const uint64_t* __restrict__ marks,
                                                 int32_t* __restrict__ keep_len, uint32_t* __restrict__ counters) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  bool drop = false;
  if (k < events) {
    const int nb = FIRST ? k - 1 : k + 1;
    if (nb >= 0 && nb < events && keys[nb] == keys[k]) {
      const uint32_t frame = static_cast<uint32_t>(vals[k] >> 32), other = static_cast<uint32_t>(vals[nb] >> 32);
      // always: the frames are the event scan's indices, all below n
      if (frame < static_cast<uint32_t>(n) && other < static_cast<uint32_t>(n) && marks[frame] == marks[other]) {
        keep_len[frame] = 0;
        drop = true;
      }
    }
  }
  const unsigned long long dropped = __ballot(drop);  // every lane of the wave is here: no lane left early
  if ((threadIdx.x & 63) == 0 && dropped) atomicAdd(&counters[C_DROPPED], static_cast<uint32_t>(__popcll(dropped)));
}

}  // namespace

// C ABI for ctypes (ops/gpu_thin.py). All pointers are device pointers from torch tensors on the
// caller's device; `stream` is the torch stream (hipStream_t). Each returns a hipError_t and launches
// nothing for a count <= 0.

// classify.
//   dialect      0 = upb, 1 = protobufjs
//   step         the width of a bucket, >= 1
//   rows         n StatusEvent, written for every frame
//   is_event     n int32, written for every frame: 1 for a progress event, else 0
//   marks        n uint64, written for every frame: the event's mark word, else 0
//   keep_len     n int32, written for every frame: its whole length
//   counters     3 uint32, zeroed by the caller: progress decode errors, the length of `overflow`,
//                and the frames that a later mark drops
//   overflow     n int32: the frames left to the host, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_thin_classify(
    const void* buf, const void* offs, int n, int dialect, int step, void* rows, void* is_event, void* marks,
    void* keep_len, void* counters, void* overflow, void* stream) {
  if (n <= 0) return 0;
  if ((dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) || step < 1 || !buf || !offs || !rows || !is_event ||
      !marks || !keep_len || !counters || !overflow)
    return static_cast<int>(hipErrorInvalidValue);
  const int grid = blocks_of(n, BLOCK);
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* rw = static_cast<StatusEvent*>(rows);
  auto* ie = static_cast<int32_t*>(is_event);
  auto* mk = static_cast<uint64_t*>(marks);
  auto* kl = static_cast<int32_t*>(keep_len);
  auto* c = static_cast<uint32_t*>(counters);
  auto* ov = static_cast<int32_t*>(overflow);
  if (dialect == DIALECT_PROTOBUFJS)
    hipLaunchKernelGGL(th_classify<DIALECT_PROTOBUFJS>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, step, rw, ie, mk, kl, c,
                       ov);
  else
    hipLaunchKernelGGL(th_classify<DIALECT_UPB>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, step, rw, ie, mk, kl, c, ov);
  return static_cast<int>(hipGetLastError());
}

// mark, over the sorted keys and vals.
//   keys, vals   `events` uint32 and uint64: the media number, and frame << 32 | status
//   n            the frame count: every frame in vals is below it
//   first        0: an event is dropped where its successor repeats its mark; 1: where its predecessor does
//   marks        n uint64, classify's
//   keep_len     n int32: 0 is stored for a dropped frame
//   counters     classify's; [2] counts the dropped frames
extern "C" __attribute__((visibility("default"))) int bh_thin_mark(
    const void* keys, const void* vals, int events, int n, int first, const void* marks, void* keep_len, void* counters,
    void* stream) {
  if (events <= 0) return 0;
  if (events > n || (first != 0 && first != 1) || !keys || !vals || !marks || !keep_len || !counters)
    return static_cast<int>(hipErrorInvalidValue);
  const int grid = blocks_of(events, BLOCK);
  auto st = static_cast<hipStream_t>(stream);
  const auto* k = static_cast<const uint32_t*>(keys);
  const auto* v = static_cast<const uint64_t*>(vals);
  const auto* mk = static_cast<const uint64_t*>(marks);
  auto* kl = static_cast<int32_t*>(keep_len);
  auto* c = static_cast<uint32_t*>(counters);
  if (first)
    hipLaunchKernelGGL(th_mark<true>, dim3(grid), dim3(BLOCK), 0, st, k, v, events, n, mk, kl, c);
  else
    hipLaunchKernelGGL(th_mark<false>, dim3(grid), dim3(BLOCK), 0, st, k, v, events, n, mk, kl, c);
  return static_cast<int>(hipGetLastError());
}
