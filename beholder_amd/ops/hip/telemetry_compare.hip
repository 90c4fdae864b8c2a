// Two captures matched frame for frame on the GPU (gfx950): the device half of
// `python -m beholder_amd compare --device gpu` (beholder_amd/compare.py, ops/gpu_compare.py).
//
// Input is the two captures as one joined stream, A's n_a frames first and then B's, and
// `offs[n + 1]`, the frame starts from the host's pass over both captures' length headers with B's
// shifted by A's size. The side of frame m is m >= n_a. What comes back are two cuts, keep_a[m] and
// keep_b[m] (the frame's whole length where it is only in its capture, else 0), which the extract's
// scan and gather (telemetry_select.hip) turn into the two output streams, and a handful of counts.
//
// A frame's fate depends on its rank among the frames of its content on its own side, so one
// content's frames must lie next to each other, A's in stream order and then B's: the transitions'
// claim and stable sort (telemetry_transitions.hip), called as they are over rows that carry a
// content where theirs carry a media id. The stages, each a launch or a few on one stream:
//
//  classify, cmp_classify, one lane per joined frame (telemetry_compare.hpp cmp_row). A frame
//    whose topic is not selected is skipped and counted per side; only its topic byte is read. A
//    content above DEDUPE_DEVICE_MAX goes to the overflow list through its atomic cursor: the host
//    pairs those. Every other frame gets the row {hash, content start, content length, side,
//    TR_EVENT} and is_event[m] = 1. Every frame's keep_a, keep_b and is_matched word is zeroed.
//  claim, rank, compact and sort are the transitions' and the extract's entry points
//    (bh_transitions_claim, bh_select_scan, bh_transitions_compact, bh_transitions_sort_pass):
//    keys[p] is the content number of sorted position p, vals[p] its frame << 32 | side.
//  bounds, cmp_bounds, one lane per sorted position writes its content's run_start, side_start and
//    run_end where it is the one position that knows them (cmp_bounds_at): plain stores, one writer
//    each, as tr_pairs writes its run bounds.
//  match, cmp_match, one lane per sorted position, a launch of its own because it reads the bounds
//    that other workgroups wrote. cmp_verdict gives matched or not and the partner's position. An
//    unmatched frame's length goes to keep_a[m] or keep_b[m]; a matched A frame sets is_matched[m]
//    and partner[m], its partner's joined frame index. A frame has one sorted position, so each of
//    these words has exactly one writer. The pairs, and at every run's first position the contents
//    of A, of B and of both, are counted by wave ballot, summed per block in LDS and flushed with
//    one global atomic per counter and block.
//  breaks, cmp_breaks, after the extract's scan over is_matched has listed A's matched frames in
//    stream order: one lane per listed position k >= 1 tests partner[idx[k]] < partner[idx[k - 1]];
//    ballot, LDS, one atomic per block.
//
// Visibility is media_table.hpp's rule: within a launch workgroups meet only in atomics (the cursor,
// the counts); every plain load reads what an earlier launch or the host wrote. No kernel waits for
// another workgroup. The one loop over bytes, the hash, is bounded by DEDUPE_DEVICE_MAX.
#include "launch_grid.hpp"
#include "telemetry_compare.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;  // threads per block

// counters[]: ops/gpu_compare.py reads the same layout; [1] is where the transitions keep theirs
constexpr int C_SKIPPED_A = 0, C_OVERFLOW = 1, C_SKIPPED_B = 2, C_MATCHED = 3, C_DISTINCT_A = 4, C_DISTINCT_B = 5,
              C_COMMON = 6, C_BREAKS = 7;

// Adds the wave's votes to the block's sum: one LDS atomic per wave. Every lane of the wave calls it.
__device__ __forceinline__ void wave_count(const bool vote, uint32_t* sum) {
  const unsigned long long votes = __ballot(vote);
  if ((threadIdx.x & 63) == 0 && votes) atomicAdd(sum, static_cast<uint32_t>(__popcll(votes)));
}

__global__ __launch_bounds__(BLOCK) void cmp_classify(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                      int n, int n_a, const DedupeParams s,
                                                      StatusEvent* __restrict__ rows, int32_t* __restrict__ is_event,
                                                      int32_t* __restrict__ keep_a, int32_t* __restrict__ keep_b,
                                                      int32_t* __restrict__ is_matched,
                                                      uint32_t* __restrict__ counters, int32_t* __restrict__ overflow) {
  __shared__ uint32_t skipped[2];
  if (threadIdx.x < 2) skipped[threadIdx.x] = 0u;
  __syncthreads();
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  int kind = DK_ROW;
  const int32_t side = m >= n_a ? SIDE_B : SIDE_A;
  if (m < n) {
    StatusEvent ev;
    kind = cmp_row(buf, offs[m], offs[m + 1], side, s, ev);
    if (kind == DK_HOST) overflow[atomicAdd(&counters[C_OVERFLOW], 1u)] = m;  // at most one per frame: stays below n
    rows[m] = ev;
    is_event[m] = kind == DK_ROW ? 1 : 0;
    keep_a[m] = 0;
    keep_b[m] = 0;
    is_matched[m] = 0;
  }
  wave_count(kind == DK_KEEP && side == SIDE_A, &skipped[0]);  // every lane of the wave is here: no lane left early
  wave_count(kind == DK_KEEP && side == SIDE_B, &skipped[1]);
  __syncthreads();
  if (threadIdx.x == 0 && skipped[0]) atomicAdd(&counters[C_SKIPPED_A], skipped[0]);
  if (threadIdx.x == 1 && skipped[1]) atomicAdd(&counters[C_SKIPPED_B], skipped[1]);
}

__global__ __launch_bounds__(BLOCK) void cmp_bounds(const uint32_t* __restrict__ keys,
                                                    const uint64_t* __restrict__ vals, int events, uint32_t groups,
                                                    int32_t* __restrict__ run_start,
                                                    int32_t* __restrict__ side_start, int32_t* __restrict__ run_end) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p < events) cmp_bounds_at(keys, vals, events, groups, p, run_start, side_start, run_end);
}

__global__ __launch_bounds__(BLOCK) void cmp_match(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ vals,
                                                   int events, uint32_t groups, const int32_t* __restrict__ offs, int n,
                                                   const int32_t* __restrict__ run_start,
                                                   const int32_t* __restrict__ side_start,
                                                   const int32_t* __restrict__ run_end, int32_t* __restrict__ keep_a,
                                                   int32_t* __restrict__ keep_b, int32_t* __restrict__ is_matched,
                                                   int32_t* __restrict__ partner, uint32_t* __restrict__ counters) {
  __shared__ uint32_t sums[4];  // pairs, contents of A, of B, of both
  if (threadIdx.x < 4) sums[threadIdx.x] = 0u;
  __syncthreads();
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  CmpVerdict v{false, SIDE_A, -1, false, false, false};
  if (p < events) {
    v = cmp_verdict(keys, vals, events, groups, p, run_start, side_start, run_end);
    const uint32_t m = cmp_frame_of(vals[p]);
    if (m < static_cast<uint32_t>(n)) {  // always: the frames are the event scan's indices, all below n
      if (!v.matched) {
        (v.side == SIDE_B ? keep_b : keep_a)[m] = offs[m + 1] - offs[m];
      } else if (v.side == SIDE_A) {
        is_matched[m] = 1;
        partner[m] = static_cast<int32_t>(cmp_frame_of(vals[v.partner]));  // v.partner is in [0, events)
      }
    }
  }
  wave_count(v.matched && v.side == SIDE_A, &sums[0]);  // every lane of the wave is here
  wave_count(v.run_head && v.in_a, &sums[1]);
  wave_count(v.run_head && v.in_b, &sums[2]);
  wave_count(v.run_head && v.in_a && v.in_b, &sums[3]);
  __syncthreads();
  if (threadIdx.x < 4 && sums[threadIdx.x]) atomicAdd(&counters[C_MATCHED + threadIdx.x], sums[threadIdx.x]);
}
static_assert(C_DISTINCT_A == C_MATCHED + 1 && C_DISTINCT_B == C_MATCHED + 2 && C_COMMON == C_MATCHED + 3,
              "cmp_match flushes sums[k] into counters[C_MATCHED + k]");

__global__ __launch_bounds__(BLOCK) void cmp_breaks(const int32_t* __restrict__ idx, int count,
                                                    const int32_t* __restrict__ partner, int n,
                                                    uint32_t* __restrict__ counters) {
  __shared__ uint32_t sum;
  if (threadIdx.x == 0) sum = 0u;
  __syncthreads();
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  bool descent = false;
  if (k >= 1 && k < count) {
    const uint32_t here = static_cast<uint32_t>(idx[k]), before = static_cast<uint32_t>(idx[k - 1]);
    // always: the indices are the scan's, all below n
    if (here < static_cast<uint32_t>(n) && before < static_cast<uint32_t>(n)) descent = partner[here] < partner[before];
  }
  wave_count(descent, &sum);  // every lane of the wave is here
  __syncthreads();
  if (threadIdx.x == 0 && sum) atomicAdd(&counters[C_BREAKS], sum);
}

}  // namespace

// C ABI for ctypes (ops/gpu_compare.py). All pointers but `params` are device pointers from torch
// tensors on the caller's device; `stream` is the torch stream (hipStream_t). Each returns a
// hipError_t and launches nothing for a count <= 0.

// classify.
//   buf, offs    the joined stream and its n + 1 frame starts (host-checked)
//   n_a          A's frame count, 0..n: frame m is B's where m >= n_a
//   params       host pointer to a DedupeParams (ops/gpu_dedupe.py dedupe_params), copied into the
//                kernel's arguments; only its topics are read here
//   rows         n StatusEvent, written for every frame
//   is_event     n int32, written for every frame: 1 where it takes part on the device, else 0
//   keep_a, keep_b, is_matched   n int32 each, zeroed here
//   counters     8 uint32, zeroed by the caller: skipped frames of A, the length of `overflow`,
//                skipped frames of B; the rest belongs to match and breaks
//   overflow     n int32: the frames left to the host, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_compare_classify(
    const void* buf, const void* offs, int n, int n_a, const void* params, void* rows, void* is_event, void* keep_a,
    void* keep_b, void* is_matched, void* counters, void* overflow, void* stream) {
  if (n <= 0) return 0;
  if (n_a < 0 || n_a > n || !buf || !offs || !params || !rows || !is_event || !keep_a || !keep_b || !is_matched ||
      !counters || !overflow)
    return static_cast<int>(hipErrorInvalidValue);
  const DedupeParams s = *static_cast<const DedupeParams*>(params);
  hipLaunchKernelGGL(cmp_classify, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(buf), static_cast<const int32_t*>(offs), n, n_a, s,
                     static_cast<StatusEvent*>(rows), static_cast<int32_t*>(is_event), static_cast<int32_t*>(keep_a),
                     static_cast<int32_t*>(keep_b), static_cast<int32_t*>(is_matched), static_cast<uint32_t*>(counters),
                     static_cast<int32_t*>(overflow));
  return static_cast<int>(hipGetLastError());
}

// bounds, over the sorted keys and vals.
//   keys, vals   `events` uint32 and uint64: the content number, and frame << 32 | side
//   groups       the content count: every key is below it
//   run_start, side_start, run_end   `groups` int32 each, written for every content
extern "C" __attribute__((visibility("default"))) int bh_compare_bounds(
    const void* keys, const void* vals, int events, int groups, void* run_start, void* side_start, void* run_end,
    void* stream) {
  if (events <= 0) return 0;
  if (groups < 1 || groups > events || !keys || !vals || !run_start || !side_start || !run_end)
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(cmp_bounds, dim3(blocks_of(events, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint32_t*>(keys), static_cast<const uint64_t*>(vals), events,
                     static_cast<uint32_t>(groups), static_cast<int32_t*>(run_start), static_cast<int32_t*>(side_start),
                     static_cast<int32_t*>(run_end));
  return static_cast<int>(hipGetLastError());
}

// match, after bounds.
//   offs, n      the joined stream's frame starts and frame count: every frame in vals is below n
//   keep_a, keep_b   n int32 each: an unmatched frame's whole length is stored into its side's
//   is_matched   n int32: 1 is stored for a matched frame of A
//   partner      n int32: a matched frame of A gets its partner's joined frame index
//   counters     classify's; [3..6] count the pairs and the contents of A, of B and of both
extern "C" __attribute__((visibility("default"))) int bh_compare_match(
    const void* keys, const void* vals, int events, int groups, const void* offs, int n, const void* run_start,
    const void* side_start, const void* run_end, void* keep_a, void* keep_b, void* is_matched, void* partner,
    void* counters, void* stream) {
  if (events <= 0) return 0;
  if (groups < 1 || groups > events || events > n || !keys || !vals || !offs || !run_start || !side_start || !run_end ||
      !keep_a || !keep_b || !is_matched || !partner || !counters)
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(cmp_match, dim3(blocks_of(events, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint32_t*>(keys), static_cast<const uint64_t*>(vals), events,
                     static_cast<uint32_t>(groups), static_cast<const int32_t*>(offs), n,
                     static_cast<const int32_t*>(run_start), static_cast<const int32_t*>(side_start),
                     static_cast<const int32_t*>(run_end), static_cast<int32_t*>(keep_a), static_cast<int32_t*>(keep_b),
                     static_cast<int32_t*>(is_matched), static_cast<int32_t*>(partner),
                     static_cast<uint32_t*>(counters));
  return static_cast<int>(hipGetLastError());
}

// breaks, after the scan over is_matched.
//   idx          the scan's indices: the first `count` are A's matched frames in stream order
//   partner      n int32, match's (and the host's, for its own pairs)
//   counters     classify's; [7] counts the adjacent descents
extern "C" __attribute__((visibility("default"))) int bh_compare_breaks(
    const void* idx, int count, const void* partner, int n, void* counters, void* stream) {
  if (count <= 1) return 0;
  if (count > n || !idx || !partner || !counters) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(cmp_breaks, dim3(blocks_of(count, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const int32_t*>(idx), count, static_cast<const int32_t*>(partner), n,
                     static_cast<uint32_t*>(counters));
  return static_cast<int>(hipGetLastError());
}
