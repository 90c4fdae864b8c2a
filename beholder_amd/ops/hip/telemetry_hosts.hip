// What every worker host did in a framed telemetry stream, on the GPU (gfx950): the device half of
// `python -m beholder_amd hosts --device gpu` (beholder_amd/hosts.py, ops/gpu_hosts.py).
//
// Input is what the fold takes (telemetry_fold.hip): the capture as it lies in the file and
// `offs[n + 1]`, the frame starts from the host's one pass over the length headers. What comes back
// is a reduction whose size is not known before the run: one row of counters per worker, the run
// bounds per media, and one count per (media, worker) pair that occurs.
//
// A worker's stints, handovers and rewinds depend on the order of one media's progress events, so
// they must lie next to each other and in stream order: the transitions' stable sort by media
// (telemetry_transitions.hip), called as it is. The stages, each a launch or a few on one stream:
//
//  classify, ho_classify, one lane per frame. A topic-2 frame is read as a TelemetryProgress
//    (telemetry_hosts.hpp hosts_classify, upb in its STRICT form): the lane counts the decode error
//    (per block in LDS, then one atomic), or hands the frame to the CPU through the overflow list
//    with its atomic cursor, or writes the event: a row keyed by its id, a row keyed by its worker
//    string, its progress and is_event[m] = 1. Other topics are not read.
//  claim, rank, compact and sort are the transitions' and the extract's entry points over the id
//    rows: keys[k] is the media number of the k-th event by media and stream order, vals[k] its
//    frame << 32 | status. The same claim and slot scan over the worker rows, in a table of their
//    own, give every worker string a dense number.
//  number, ho_number, one lane per sorted position k: worker_of[k] is the worker number of the
//    event's frame and prog[k] its progress, so the two launches below read their own event and
//    their neighbour's from consecutive words and compare integers only.
//  pairs, ho_pairs, one lane per sorted position: the event's key is media number << 32 | worker
//    number, and the lane finds that key's slot in one more table of media_table.hpp (claim_slot;
//    the home slot is finalise64(key) & hash_mask & slot_mask; two events have the same key where
//    the two integers of the claimant's position equal the lane's own). The table counts the events
//    per pair: a wave adds up every stretch of neighbouring lanes that found the same slot, which a
//    stint is, and makes one global atomic add per stretch. The claimant sets pair_used[slot]; the
//    extract's scan over pair_used compacts the claimed slots.
//  walk, ho_walk, one lane per sorted position, laid out as tr_pairs is (a block takes eight tiles
//    of 256). Where the previous position holds the same media the lane decides between a handover
//    (the workers differ: one `taken` for its own worker, one `lost` for the other), a rewind (the
//    same worker, the same raw status, a smaller progress) and neither; where it does not, the
//    position starts the media's run: one `starts` for its worker, and run_start[media] with a
//    plain store. The position that ends the run stores run_end[media]. Every event adds 1 to its
//    worker's word of its status class (class_of). The position before a block's first is read
//    from global memory like any other.
//
//    The per-worker counters are summed on chip first. Of the two ways to do that, this is the
//    per-block LDS table: workers numbered below LDS_WORKERS have their row of WORKER_WORDS words
//    in LDS, flushed with one global atomic add per non-zero word when the block is done; workers
//    at or above it add to the global rows directly. A real capture has a handful of workers, so
//    its every add is an LDS atomic, as in tr_pairs; a stream with many workers spreads its global
//    adds over as many rows, which is where global atomics are cheap. The wave-level merge needs a
//    loop over the distinct workers of a wave whose trip count depends on the data; the table has
//    none, and the shape of tr_pairs is the one already measured here. All sums are of integers:
//    the result is exact for any number of workers, and the same from run to run.
//
// Visibility is media_table.hpp's rule: within a launch workgroups meet only in atomics (the claims,
// the cursor, the counts); every plain load reads what an earlier launch or the host wrote, which is
// why number is a launch of its own before pairs. No kernel waits for another workgroup. Every
// lane's loops are bounded by the frame's own length or by the table's size.
#include "launch_grid.hpp"
#include "telemetry_hosts.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;        // threads per block
constexpr int TILES = 8;          // a block of the walk takes TILES * BLOCK consecutive positions, as tr_pairs does
constexpr int LDS_WORKERS = 64;   // workers with a row in the walk's LDS table; ops/gpu_hosts.py LDS_WORKERS

// counters[]: ops/gpu_hosts.py reads the same layout, which is the transitions'
constexpr int C_PROGRESS_ERR = 0, C_OVERFLOW = 1;

template <int DIALECT>
__global__ __launch_bounds__(BLOCK) void ho_classify(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                     int n, StatusEvent* __restrict__ media_rows,
                                                     StatusEvent* __restrict__ worker_rows,
                                                     int32_t* __restrict__ progress, int32_t* __restrict__ is_event,
                                                     uint32_t* __restrict__ counters, int32_t* __restrict__ overflow) {
  __shared__ uint32_t errors;
  if (threadIdx.x == 0) errors = 0;
  __syncthreads();
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n) {
    StatusEvent media, worker;
    int32_t p;
    const int kind = hosts_classify<DIALECT>(buf, offs[m], offs[m + 1], media, worker, p);
    if (kind == HO_HOST) overflow[atomicAdd(&counters[C_OVERFLOW], 1u)] = m;  // at most one per frame: stays below n
    if (kind == HO_ERROR) atomicAdd(&errors, 1u);
    media_rows[m] = media;
    worker_rows[m] = worker;
    progress[m] = p;
    is_event[m] = kind == HO_EVENT ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0 && errors) atomicAdd(&counters[C_PROGRESS_ERR], errors);
}

// position k: vals[k] >> 32 is its frame, slot_of[frame] its worker's slot, slot_rank[slot] >> 32 that
// slot's rank among the claimed slots (the worker table's slot scan's pos).
__global__ __launch_bounds__(BLOCK) void ho_number(const uint64_t* __restrict__ vals, int events, uint32_t n,
                                                   const uint32_t* __restrict__ slot_of,
                                                   const uint64_t* __restrict__ slot_rank, uint32_t slot_mask,
                                                   const int32_t* __restrict__ progress,
                                                   uint32_t* __restrict__ worker_of, int32_t* __restrict__ prog) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= events) return;
  const uint32_t frame = static_cast<uint32_t>(vals[k] >> 32);
  uint32_t worker = 0xffffffffu;  // no worker's number: the walk passes over it
  int32_t p = 0;
  if (frame < n) {  // always: the frames are the event scan's indices
    worker = static_cast<uint32_t>(slot_rank[slot_of[frame] & slot_mask] >> 32);
    p = progress[frame];
  }
  worker_of[k] = worker;
  prog[k] = p;
}

__global__ __launch_bounds__(BLOCK) void ho_pairs(const uint32_t* __restrict__ keys,
                                                  const uint32_t* __restrict__ worker_of, int events,
                                                  uint32_t slot_mask, uint64_t hash_mask,
                                                  unsigned long long* __restrict__ claim,
                                                  int32_t* __restrict__ pair_used, uint32_t* __restrict__ pair_count) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  const int lane = threadIdx.x & 63;
  const bool valid = k < events;
  uint32_t slot = 0xffffffffu;  // no slot: the table has at most 2^30
  if (valid) {
    const uint32_t media = keys[k], worker = worker_of[k];
    const auto same_pair = [&](unsigned long long owner) {
      return owner < static_cast<unsigned long long>(events) && keys[owner] == media && worker_of[owner] == worker;
    };
    const uint32_t home = home_slot(finalise64(pair_key(media, worker)), hash_mask, slot_mask);
    const Claim c = claim_slot(claim, slot_mask, home, static_cast<unsigned long long>(k) + 1ull, same_pair);
    if (c.claimed) pair_used[c.slot] = 1;  // the one writer of pair_used[slot]
    slot = c.slot;
  }
  // one add per stretch of neighbouring lanes with one slot, not one per event. Every lane of the
  // wave is here: none left early.
  const uint32_t left = __shfl_up(slot, 1);
  const bool head = lane == 0 || left != slot;
  const unsigned long long heads = __ballot(head);
  if (head && valid) {
    const unsigned long long above = heads & ~((2ull << lane) - 1ull);  // the heads after this lane
    const int end = above ? __ffsll(above) - 1 : 64;
    atomicAdd(&pair_count[slot], static_cast<uint32_t>(end - lane));
  }
}

__global__ __launch_bounds__(BLOCK) void ho_walk(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ vals,
                                                 const uint32_t* __restrict__ worker_of,
                                                 const int32_t* __restrict__ prog, int events, uint32_t groups,
                                                 uint32_t workers, uint64_t known_mask,
                                                 uint32_t* __restrict__ worker_rows, int32_t* __restrict__ run_start,
                                                 int32_t* __restrict__ run_end) {
  __shared__ uint32_t table[LDS_WORKERS * WORKER_WORDS];
  const uint32_t held = (workers < static_cast<uint32_t>(LDS_WORKERS) ? workers : LDS_WORKERS) * WORKER_WORDS;
  for (uint32_t k = threadIdx.x; k < held; k += BLOCK) table[k] = 0u;
  __syncthreads();
  const auto add = [&](uint32_t worker, uint32_t word) {
    if (worker < static_cast<uint32_t>(LDS_WORKERS)) atomicAdd(&table[worker * WORKER_WORDS + word], 1u);
    else atomicAdd(&worker_rows[static_cast<size_t>(worker) * WORKER_WORDS + word], 1u);
  };
  for (int t = 0; t < TILES; ++t) {
    const long long p = (static_cast<long long>(blockIdx.x) * TILES + t) * BLOCK + threadIdx.x;
    if (p >= events) continue;
    const uint32_t key = keys[p], worker = worker_of[p];
    if (key >= groups || worker >= workers) continue;  // never: both are a claimed slot's rank
    const uint64_t v = vals[p];
    const int32_t status = static_cast<int32_t>(v & 0xffffffffull);
    add(worker, W_CLASS + class_of(status, known_mask));
    if (p > 0 && keys[p - 1] == key) {  // in the previous tile or block as well: read from global memory
      const uint32_t before = worker_of[p - 1];
      if (before != worker) {
        add(worker, W_TAKEN);
        if (before < workers) add(before, W_LOST);
      } else if (static_cast<int32_t>(vals[p - 1] & 0xffffffffull) == status && prog[p] < prog[p - 1]) {
        add(worker, W_REWINDS);
      }
    } else {
      add(worker, W_STARTS);
      run_start[key] = static_cast<int32_t>(p);
    }
    if (p + 1 >= events || keys[p + 1] != key) run_end[key] = static_cast<int32_t>(p + 1);
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < held; k += BLOCK)
    if (table[k]) atomicAdd(&worker_rows[k], table[k]);
}

bool table_size(long long slots, long long least) {
  return slots >= least && slots <= (1ll << 30) && (slots & (slots - 1)) == 0;
}

}  // namespace

// C ABI for ctypes (ops/gpu_hosts.py). All pointers are device pointers from torch tensors on the
// caller's device; `stream` is the torch stream (hipStream_t). Each returns a hipError_t and launches
// nothing for a count <= 0.

// classify.
//   dialect      0 = upb, 1 = protobufjs
//   media_rows   n StatusEvent, written for every frame: the event keyed by its id
//   worker_rows  n StatusEvent, written for every frame: the event keyed by its worker string
//   progress     n int32, written for every frame: the event's progress, else 0
//   is_event     n int32, written for every frame: 1 for a progress event, else 0
//   counters     2 uint32, zeroed by the caller: progress decode errors, the length of `overflow`
//   overflow     n int32: the frames left to the CPU, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_hosts_classify(
    const void* buf, const void* offs, int n, int dialect, void* media_rows, void* worker_rows, void* progress,
    void* is_event, void* counters, void* overflow, void* stream) {
  if (n <= 0) return 0;
  if ((dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) || !buf || !offs || !media_rows || !worker_rows ||
      !progress || !is_event || !counters || !overflow)
    return static_cast<int>(hipErrorInvalidValue);
  const int grid = blocks_of(n, BLOCK);
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* mr = static_cast<StatusEvent*>(media_rows);
  auto* wr = static_cast<StatusEvent*>(worker_rows);
  auto* pr = static_cast<int32_t*>(progress);
  auto* ie = static_cast<int32_t*>(is_event);
  auto* c = static_cast<uint32_t*>(counters);
  auto* ov = static_cast<int32_t*>(overflow);
  if (dialect == DIALECT_PROTOBUFJS)
    hipLaunchKernelGGL(ho_classify<DIALECT_PROTOBUFJS>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, mr, wr, pr, ie, c, ov);
  else
    hipLaunchKernelGGL(ho_classify<DIALECT_UPB>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, mr, wr, pr, ie, c, ov);
  return static_cast<int>(hipGetLastError());
}

// number, over the sorted vals.
//   vals         `events` uint64: frame << 32 | status
//   n            the frame count: every frame in vals is below it
//   slot_of      n uint32: the worker table's slot of every event's frame (bh_transitions_claim)
//   slot_rank    `slots` uint64: the worker table's slot scan's pos, rank << 32 | rank
//   slots        the worker table's size: a power of two, at least 2n and at most 2^30
//   progress     n int32, classify's
//   worker_of    `events` uint32, written: the worker number per sorted position
//   prog         `events` int32, written: the progress per sorted position
extern "C" __attribute__((visibility("default"))) int bh_hosts_number(
    const void* vals, int events, int n, const void* slot_of, const void* slot_rank, long long slots,
    const void* progress, void* worker_of, void* prog, void* stream) {
  if (events <= 0) return 0;
  if (events > n || !table_size(slots, 2ll * n) || !vals || !slot_of || !slot_rank || !progress || !worker_of || !prog)
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(ho_number, dim3(blocks_of(events, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint64_t*>(vals), events, static_cast<uint32_t>(n),
                     static_cast<const uint32_t*>(slot_of), static_cast<const uint64_t*>(slot_rank),
                     static_cast<uint32_t>(slots - 1), static_cast<const int32_t*>(progress),
                     static_cast<uint32_t*>(worker_of), static_cast<int32_t*>(prog));
  return static_cast<int>(hipGetLastError());
}

// pairs, over the sorted keys and number's worker_of.
//   hash_mask    ANDed onto every key's hash before the home slot is taken (all ones in production)
//   claim        `slots` uint64, zeroed by the caller: 0 or 1 + the sorted position that claimed the slot
//   pair_used    `slots` int32, zeroed by the caller: 1 for a claimed slot
//   pair_count   `slots` uint32, zeroed by the caller: the events of the slot's pair
//   slots        a power of two, at least 2 * events and at most 2^30
extern "C" __attribute__((visibility("default"))) int bh_hosts_pairs(
    const void* keys, const void* worker_of, int events, unsigned long long hash_mask, void* claim, void* pair_used,
    void* pair_count, long long slots, void* stream) {
  if (events <= 0) return 0;
  if (!table_size(slots, 2ll * events) || !keys || !worker_of || !claim || !pair_used || !pair_count)
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(ho_pairs, dim3(blocks_of(events, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint32_t*>(keys), static_cast<const uint32_t*>(worker_of), events,
                     static_cast<uint32_t>(slots - 1), hash_mask, static_cast<unsigned long long*>(claim),
                     static_cast<int32_t*>(pair_used), static_cast<uint32_t*>(pair_count));
  return static_cast<int>(hipGetLastError());
}

// walk, over the sorted keys and vals and number's worker_of and prog.
//   groups       the media count: every key is below it
//   workers      the worker count: every worker_of is below it
//   known_mask   bit s set: s is a number of TelemetryStatusEntry
//   worker_rows  workers * WORKER_WORDS (69) uint32, zeroed by the caller: per worker its starts, taken,
//                lost, rewinds and its events per class
//   run_start, run_end   `groups` int32 each: the media's run is [run_start, run_end) of the sorted arrays
extern "C" __attribute__((visibility("default"))) int bh_hosts_walk(
    const void* keys, const void* vals, const void* worker_of, const void* prog, int events, int groups, int workers,
    unsigned long long known_mask, void* worker_rows, void* run_start, void* run_end, void* stream) {
  if (events <= 0) return 0;
  if (groups < 1 || groups > events || workers < 1 || workers > events || !keys || !vals || !worker_of || !prog ||
      !worker_rows || !run_start || !run_end)
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(ho_walk, dim3(blocks_of(events, BLOCK * TILES)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint32_t*>(keys), static_cast<const uint64_t*>(vals),
                     static_cast<const uint32_t*>(worker_of), static_cast<const int32_t*>(prog), events,
                     static_cast<uint32_t>(groups), static_cast<uint32_t>(workers), known_mask,
                     static_cast<uint32_t*>(worker_rows), static_cast<int32_t*>(run_start),
                     static_cast<int32_t*>(run_end));
  return static_cast<int>(hipGetLastError());
}
