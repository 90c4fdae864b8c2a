// Replace a capture's media ids and host names by keyed pseudonyms on the GPU (gfx950): the device
// half of `python -m beholder_amd anonymise --device gpu` (beholder_amd/anonymise.py,
// ops/gpu_anonymise.py).
//
// Input is what the normalise takes (telemetry_normalise.hip): the capture as it lies in the file and
// `offs[n + 1]`, the frame starts from the host's one pass over the length headers. Output is a
// framed stream of canonical frames whose chosen strings are pseudonyms (telemetry_anonymise.hpp).
//
// Two kernels, with the extract's scan (telemetry_select.hip, bh_select_scan) between them, in the
// normalise's shape:
//
//  classify, an_classify, one lane per frame. Reads the frame as the normalise does (anon_classify
//    calls norm_classify), hashes the chosen strings with keyed BLAKE2s from the two states after the
//    key block, which arrive by value and are scalars, and stores the 64-byte plan and keep_len[m],
//    the output frame's length. A frame the device does not write (NM_HOST: the normalise's rule, or
//    a chosen string above 4,096 bytes) goes to the overflow list through an atomic cursor with
//    keep_len 0; the host asks anonymise.anon_of and scatters the lengths of its frames into keep_len
//    before the scan. Events, decode errors and other topics are counted per block in LDS, then by
//    one atomic each. The hash's arrays are indexed by constants only and live in registers.
//  emit, an_emit, nm_emit's walk: a wave takes 64 frames and writes the ones the device plans one
//    after the other, lane b producing bytes b, b + 64, ... of the frame at its output offset pos[m].
//    The plan of the frame in hand is read from its lane into scalar registers, digest words
//    included; a digit of a replaced string is a shift and a select on them, and nothing of the
//    input is read for it. Host frames have a span in the output that this kernel leaves alone.
//
// The launcher computes the two states on the host from the key (anon_midstates): the key itself is
// never copied to the device.
//
// Visibility is the fold's rule: within a launch workgroups meet only in atomics (the cursor, the
// counts); every plain load reads what an earlier launch or the host wrote. No kernel waits for
// another workgroup. Every lane's loops are bounded by the frame's own length, and the hash's by
// 4,096 bytes.
#include "launch_grid.hpp"
#include "telemetry_anonymise.hpp"
#include "wave_lane.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;  // threads per block

// counters[]: ops/gpu_anonymise.py reads the same layout
constexpr int C_EVENTS = 0, C_ERRORS = 1, C_OTHER = 2, C_OVERFLOW = 3;

template <int DIALECT>
__global__ __launch_bounds__(BLOCK) void an_classify(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                     int n, int drop, int fields, const Midstates mids,
                                                     AnonPlan* __restrict__ plans, int32_t* __restrict__ keep_len,
                                                     uint32_t* __restrict__ counters, int32_t* __restrict__ overflow) {
  __shared__ uint32_t local[3];
  if (threadIdx.x < 3) local[threadIdx.x] = 0;
  __syncthreads();
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n) {
    const int head = offs[m], end = offs[m + 1];
    AnonPlan plan;
    const int kind = anon_classify<DIALECT>(buf, head, end, drop != 0, fields, mids, plan);
    if (kind == NM_HOST) overflow[atomicAdd(&counters[C_OVERFLOW], 1u)] = m;  // at most one per frame: stays below n
    else if (kind == NM_STATUS || kind == NM_PROGRESS) atomicAdd(&local[C_EVENTS], 1u);
    else {
      const uint32_t topic = buf[head + 4];
      atomicAdd(&local[topic == 1 || topic == 2 ? C_ERRORS : C_OTHER], 1u);
    }
    plans[m] = plan;
    keep_len[m] = plan.p.out_len;
  }
  __syncthreads();
  if (threadIdx.x < 3 && local[threadIdx.x]) atomicAdd(&counters[threadIdx.x], local[threadIdx.x]);
}

// One wave per 64 frames; pos[m] & 0xffffffff is frame m's output byte offset.
__global__ __launch_bounds__(BLOCK) void an_emit(const uint8_t* __restrict__ buf, const AnonPlan* __restrict__ plans,
                                                 const uint64_t* __restrict__ pos, int n, uint8_t* __restrict__ out) {
  const int m = blockIdx.x * BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  AnonPlan mine{{0, 0, 0, 0, 0, 0, NM_DROP, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  int my_dst = 0;
  if (m < n) {
    mine = plans[m];
    my_dst = static_cast<int>(pos[m] & 0xffffffffull);
  }
  unsigned long long todo = __ballot(mine.p.kind == NM_COPY || mine.p.kind == NM_STATUS || mine.p.kind == NM_PROGRESS);
  while (todo) {  // wave-uniform
    const int i = __ffsll(todo) - 1;
    todo &= todo - 1;
    // the frame in hand is lane i's: its plan goes to scalar registers
    const AnonPlan plan{
        {from_lane(mine.p.id_off, i), from_lane(mine.p.id_len, i), from_lane(mine.p.status, i),
         from_lane(mine.p.progress, i), from_lane(mine.p.host_off, i), from_lane(mine.p.host_len, i),
         from_lane(mine.p.kind, i), from_lane(mine.p.out_len, i)},
        {from_lane(mine.id_digest[0], i), from_lane(mine.id_digest[1], i), from_lane(mine.id_digest[2], i),
         from_lane(mine.id_digest[3], i)},
        {from_lane(mine.host_digest[0], i), from_lane(mine.host_digest[1], i), from_lane(mine.host_digest[2], i),
         from_lane(mine.host_digest[3], i)}};
    const int d = from_lane(my_dst, i);
    const int L = plan.p.out_len;
    if (plan.p.kind == NM_COPY) {
      const int s = plan.p.id_off;
      for (int b = lane; b < L; b += 64) out[d + b] = buf[s + b];
      continue;
    }
    for (int b = lane; b < L; b += 64) out[d + b] = static_cast<uint8_t>(anon_byte(buf, plan, b));
  }
}

}  // namespace

// C ABI for ctypes (ops/gpu_anonymise.py). Device pointers come from torch tensors on the caller's
// device; `stream` is the torch stream (hipStream_t). Each returns a hipError_t and launches nothing
// for n <= 0.

// classify.
//   dialect      0 = upb, 1 = protobufjs
//   drop         0: undecoded frames stay as they are; 1: they are dropped
//   fields       1: replace mediaId, 2: replace host, 3: both
//   key, keylen  host memory, 16 to 32 bytes: read here, on the host, into the two states after the
//                key block, which the kernel gets by value; never copied to the device
//   plans        n AnonPlan (64 bytes each), written for every frame
//   keep_len     n int32, written for every frame: the output frame's length, 0 for a dropped frame
//                and for one left to the host
//   counters     4 uint32, zeroed by the caller: decoded events, decode errors, other topics (the
//                host's frames are in none of the three) and the length of `overflow`
//   overflow     n int32: the frames left to the host, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_anonymise_classify(
    const void* buf, const void* offs, int n, int dialect, int drop, int fields, const void* key, int keylen,
    void* plans, void* keep_len, void* counters, void* overflow, void* stream) {
  if (n <= 0) return 0;
  Midstates mids;
  if ((dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) || (drop != 0 && drop != 1) || fields < 1 ||
      fields > (AN_MEDIA | AN_HOST) || !buf || !offs || !plans || !keep_len || !counters || !overflow ||
      !anon_midstates(static_cast<const uint8_t*>(key), keylen, mids))
    return static_cast<int>(hipErrorInvalidValue);
  const int grid = blocks_of(n, BLOCK);
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* pl = static_cast<AnonPlan*>(plans);
  auto* kl = static_cast<int32_t*>(keep_len);
  auto* c = static_cast<uint32_t*>(counters);
  auto* ov = static_cast<int32_t*>(overflow);
  if (dialect == DIALECT_PROTOBUFJS)
    hipLaunchKernelGGL(an_classify<DIALECT_PROTOBUFJS>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, drop, fields, mids, pl,
                       kl, c, ov);
  else
    hipLaunchKernelGGL(an_classify<DIALECT_UPB>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, drop, fields, mids, pl, kl, c,
                       ov);
  return static_cast<int>(hipGetLastError());
}

// emit, after the scan over keep_len (with the host's lengths scattered in).
//   plans        classify's
//   pos          n uint64, the scan's: output index << 32 | output byte offset of every frame
//   out          the output buffer, exactly the scan's total of bytes: a planned frame m is written
//                at [pos[m], pos[m] + plans[m].p.out_len), which the scan placed inside it
extern "C" __attribute__((visibility("default"))) int bh_anonymise_emit(const void* buf, int n, const void* plans,
                                                                        const void* pos, void* out, void* stream) {
  if (n <= 0) return 0;
  if (!buf || !plans || !pos || !out) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(an_emit, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(buf), static_cast<const AnonPlan*>(plans),
                     static_cast<const uint64_t*>(pos), n, static_cast<uint8_t*>(out));
  return static_cast<int>(hipGetLastError());
}
