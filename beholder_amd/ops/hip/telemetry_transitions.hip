// The status moves of every media of a framed telemetry stream on the GPU (gfx950): the device half
// of `python -m beholder_amd transitions --device gpu` (beholder_amd/transitions.py,
// ops/gpu_transitions.py).
//
// Input is what the fold takes (telemetry_fold.hip): the capture as it lies in the file and
// `offs[n + 1]`, the frame starts from the host's one pass over the length headers. What comes back
// is a reduction: a CLASSES x CLASSES matrix of transition counts and one row per media.
//
// The result depends on the order of one media's status events, so they must lie next to each other
// and in stream order: a stable sort by media over any number of media. The stages, each a launch
// or a few on one stream:
//
//  classify, tr_classify, one lane per frame. A topic-1 frame is read as a TelemetryStatus
//    (telemetry_transitions.hpp classify, upb in its STRICT form): the lane counts the decode error,
//    or hands the frame to the host through the overflow list with its atomic cursor, or writes the
//    event's row {hash, id_off, id_len, status} and is_event[m] = 1. Other topics are not read.
//  claim, tr_claim, one lane per status event finds its id's slot in the fold's table
//    (media_table.hpp claim_slot over `slots` entries, a power of two, >= 2n): ids are the same
//    where length, hash and then the bytes are.
//    Every event learns its slot, slot_of[m]; the claimant also sets slot_used[slot].
//  rank and compact are the extract's scan (telemetry_select.hip bh_select_scan) called as it is,
//    over slot_used (a claimed slot's rank is its dense media number in [0, groups)) and over
//    is_event (the k-th status event's frame, in stream order). tr_compact then writes, per event
//    k, keys[k] = its media number and vals[k] = frame << 32 | status.
//  sort, a stable LSD radix sort of (keys, vals) by key, 8 bits per pass; the host runs
//    ceil(bit_length(groups - 1) / 8) passes. A pass is the shard's three-launch shape:
//      sort_count   per block of 2,048 elements (eight tiles of 256), the per-digit totals, summed in
//                   LDS (integer adds) and written digit-major: totals[d * blocks + b];
//      sort_totals  one block scans all 256 * blocks totals in tiles of 8,192 (32 per thread) with a running carry;
//                   digit-major order is output order, so base[d * blocks + b] is where block b's
//                   elements of digit d start;
//      sort_apply   per block and tile, every element's rank among the earlier lanes of its wave
//                   with the same digit (eight ballots build the mask of those lanes, a popcount
//                   below the lane is the rank), across the tile's waves by per-wave per-digit counts
//                   in LDS (one writer each, the digit's last lane in the wave), across the tiles
//                   by a per-digit running sum in LDS that starts at the block's base.
//    No position depends on the order in which atomics land. The elements arrive in frame order
//    and every pass is stable, so each media's events end up adjacent and in stream order; the
//    frame index is never a sort key.
//  pairs, tr_pairs, one lane per sorted position. Where the previous position holds the same media
//    the lane adds 1 to the cell of the two classes, in a per-block LDS table of CLASSES x CLASSES
//    words that is flushed with one global atomic add per non-zero cell. Where the classes differ
//    the move is one of that media's `changes`: a media's lanes are neighbours, so a wave adds them
//    up by ballot and makes one global atomic add per media it holds (a capture of few media would
//    otherwise send every change to the same few words). A position that starts or ends a media's run writes that
//    media's first or last word and the run's bound with plain stores: each has exactly one writer.
//    The position before a block's first is read from global memory like any other.
//
// Visibility is media_table.hpp's rule. Every lane's loops are bounded by the frame's own length or
// by the table's size.
#include "block_scan.hpp"
#include "launch_grid.hpp"
#include "telemetry_transitions.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;            // threads per block
constexpr int WAVES = BLOCK / 64;
constexpr int TILES = 8;              // a block of sort and pairs takes TILES * BLOCK consecutive elements;
                                      // ops/gpu_transitions.py SORT_BLOCK
constexpr int RADIX = 256;            // 8 bits per pass
constexpr int TOTALS_PER_THREAD = 32; // consecutive totals a thread of sort_totals sums by itself
static_assert(BLOCK == RADIX, "thread d owns digit d of the LDS tables");
static_assert(RADIX % TOTALS_PER_THREAD == 0 && TOTALS_PER_THREAD % 4 == 0, "sort_totals moves whole 16-byte words");

// counters[]: ops/gpu_transitions.py reads the same layout
constexpr int C_STATUS_ERR = 0, C_OVERFLOW = 1;

template <int DIALECT>
__global__ __launch_bounds__(BLOCK) void tr_classify(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                     int n, StatusEvent* __restrict__ rows,
                                                     int32_t* __restrict__ is_event, uint32_t* __restrict__ counters,
                                                     int32_t* __restrict__ overflow) {
  __shared__ uint32_t errors;
  if (threadIdx.x == 0) errors = 0;
  __syncthreads();
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n) {
    StatusEvent ev;
    const int kind = classify<DIALECT>(buf, offs[m], offs[m + 1], ev);
    if (kind == TR_HOST) overflow[atomicAdd(&counters[C_OVERFLOW], 1u)] = m;  // at most one per frame: stays below n
    if (kind == TR_ERROR) atomicAdd(&errors, 1u);
    rows[m] = ev;
    is_event[m] = kind == TR_EVENT ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0 && errors) atomicAdd(&counters[C_STATUS_ERR], errors);
}

__global__ __launch_bounds__(BLOCK) void tr_claim(const uint8_t* __restrict__ buf, const StatusEvent* __restrict__ rows,
                                                  int n, uint32_t slot_mask, uint64_t hash_mask,
                                                  unsigned long long* __restrict__ claim,
                                                  int32_t* __restrict__ slot_used, uint32_t* __restrict__ slot_of) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const StatusEvent row = rows[m];
  if (row.kind != TR_EVENT) return;
  const unsigned long long me = static_cast<unsigned long long>(m) + 1ull;
  const auto same_id = [&](unsigned long long owner) {
    const StatusEvent o = rows[owner];
    return o.id_len == row.id_len && o.hash == row.hash && bytes_equal(buf + o.id_off, buf + row.id_off, row.id_len);
  };
  const Claim c = claim_slot(claim, slot_mask, home_slot(row.hash, hash_mask, slot_mask), me, same_id);
  if (c.claimed) slot_used[c.slot] = 1;  // the one writer of slot_used[slot]
  slot_of[m] = c.slot;
}

// event k: frame[k] is its frame (the event scan's indices), slot_rank[slot] >> 32 its slot's rank
// among the claimed slots (the slot scan's pos).
__global__ __launch_bounds__(BLOCK) void tr_compact(const StatusEvent* __restrict__ rows,
                                                    const int32_t* __restrict__ frame,
                                                    const uint32_t* __restrict__ slot_of,
                                                    const uint64_t* __restrict__ slot_rank, int events,
                                                    uint32_t* __restrict__ keys, uint64_t* __restrict__ vals) {
  const int k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= events) return;
  const int m = frame[k];
  keys[k] = static_cast<uint32_t>(slot_rank[slot_of[m]] >> 32);
  vals[k] = (static_cast<uint64_t>(static_cast<uint32_t>(m)) << 32) | static_cast<uint32_t>(rows[m].status);
}

__global__ __launch_bounds__(BLOCK) void sort_count(const uint32_t* __restrict__ keys, int events, int shift,
                                                    uint32_t* __restrict__ totals) {
  __shared__ uint32_t tot[RADIX];
  tot[threadIdx.x] = 0u;
  __syncthreads();
  BH_UNROLL
  for (int t = 0; t < TILES; ++t) {
    const long long i = (static_cast<long long>(blockIdx.x) * TILES + t) * BLOCK + threadIdx.x;
    if (i < events) atomicAdd(&tot[(keys[i] >> shift) & (RADIX - 1)], 1u);
  }
  __syncthreads();
  totals[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x] = tot[threadIdx.x];
}

// One block. base[i] = totals[0] + ... + totals[i - 1] for i in [0, count).
__global__ __launch_bounds__(BLOCK) void sort_totals(const uint32_t* __restrict__ totals, long long count,
                                                     uint32_t* __restrict__ base) {
  __shared__ uint64_t wave_sums[WAVES];
  uint64_t carry = 0;
  // count is a multiple of RADIX and so of TOTALS_PER_THREAD: a thread's run lies inside or outside as
  // a whole, and it is read and written as 16-byte words (the arrays are torch allocations)
  for (long long tile = 0; tile < count; tile += BLOCK * TOTALS_PER_THREAD) {  // the same trip count for every thread
    const long long first = tile + static_cast<long long>(threadIdx.x) * TOTALS_PER_THREAD;
    const bool inside = first < count;
    uint4 v[TOTALS_PER_THREAD / 4];
    uint64_t sum = 0;
    BH_UNROLL
    for (int k = 0; k < TOTALS_PER_THREAD / 4; ++k) {
      v[k] = inside ? *reinterpret_cast<const uint4*>(totals + first + 4 * k) : make_uint4(0u, 0u, 0u, 0u);
      sum += static_cast<uint64_t>(v[k].x) + v[k].y + v[k].z + v[k].w;
    }
    uint64_t total;
    uint32_t run = static_cast<uint32_t>(carry + block_scan<BLOCK>(sum, wave_sums, total) - sum);  // below `events`
    BH_UNROLL
    for (int k = 0; k < TOTALS_PER_THREAD / 4; ++k) {
      const uint4 out = make_uint4(run, run + v[k].x, run + v[k].x + v[k].y, run + v[k].x + v[k].y + v[k].z);
      if (inside) *reinterpret_cast<uint4*>(base + first + 4 * k) = out;
      run = out.w + v[k].w;
    }
    carry += total;
  }
}

__global__ __launch_bounds__(BLOCK) void sort_apply(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ vals,
                                                    int events, int shift, const uint32_t* __restrict__ base,
                                                    uint32_t* __restrict__ keys_out, uint64_t* __restrict__ vals_out) {
  __shared__ uint32_t wave_tot[WAVES][RADIX];  // this tile's count per wave and digit
  __shared__ uint32_t before[RADIX];           // where the tile's elements of a digit start
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;
  before[threadIdx.x] = base[static_cast<size_t>(threadIdx.x) * gridDim.x + blockIdx.x];
  for (int t = 0; t < TILES; ++t) {  // the same trip count for every thread: no lane leaves before the end
    // thread d owns column d of wave_tot and before[d] between the tiles: it alone rewrites them
    BH_UNROLL
    for (int w = 0; w < WAVES; ++w) wave_tot[w][threadIdx.x] = 0u;
    __syncthreads();
    const long long i = (static_cast<long long>(blockIdx.x) * TILES + t) * BLOCK + threadIdx.x;
    const bool valid = i < events;
    const uint32_t key = valid ? keys[i] : 0u;
    const uint32_t d = (key >> shift) & (RADIX - 1);
    unsigned long long peers = __ballot(valid);  // ends as the valid lanes of this wave with the digit d
    BH_UNROLL
    for (int b = 0; b < 8; ++b) {
      const bool bit = (d >> b) & 1u;
      const unsigned long long set = __ballot(valid && bit);
      peers &= bit ? set : ~set;
    }
    const uint32_t rank = static_cast<uint32_t>(__popcll(peers & below));
    if (valid && (peers >> lane) == 1ull) wave_tot[wave][d] = static_cast<uint32_t>(__popcll(peers));  // the digit's last lane
    __syncthreads();
    if (valid) {
      uint32_t p = before[d] + rank;
      for (int w = 0; w < WAVES; ++w)
        if (w < wave) p += wave_tot[w][d];
      if (p < static_cast<uint32_t>(events)) {  // always: the totals count these very elements
        keys_out[p] = key;
        vals_out[p] = vals[i];
      }
    }
    __syncthreads();  // every lane has read before[] and wave_tot[][]
    uint32_t sum = 0u;
    BH_UNROLL
    for (int w = 0; w < WAVES; ++w) sum += wave_tot[w][threadIdx.x];
    before[threadIdx.x] += sum;
  }
}

__global__ __launch_bounds__(BLOCK) void tr_pairs(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ vals,
                                                  int events, uint32_t groups, uint64_t known_mask,
                                                  uint32_t* __restrict__ matrix, uint64_t* __restrict__ first,
                                                  uint64_t* __restrict__ last, int32_t* __restrict__ run_start,
                                                  int32_t* __restrict__ run_end, uint32_t* __restrict__ changes) {
  __shared__ uint32_t cells[CLASSES * CLASSES];
  for (int k = threadIdx.x; k < static_cast<int>(CLASSES * CLASSES); k += BLOCK) cells[k] = 0u;
  __syncthreads();
  const int lane = threadIdx.x & 63;
  for (int t = 0; t < TILES; ++t) {  // the same trip count for every thread: the wave votes below
    const long long p = (static_cast<long long>(blockIdx.x) * TILES + t) * BLOCK + threadIdx.x;
    uint32_t key = p < events ? keys[p] : 0xffffffffu;
    const bool valid = key < groups;  // every key is: it is a claimed slot's rank
    if (!valid) key = 0xffffffffu;
    bool change = false;
    if (valid) {
      const uint64_t v = vals[p];
      const uint32_t to = class_of(static_cast<int32_t>(v & 0xffffffffull), known_mask);
      if (p > 0 && keys[p - 1] == key) {  // in the previous tile or block as well: read from global memory
        const uint32_t from = class_of(static_cast<int32_t>(vals[p - 1] & 0xffffffffull), known_mask);
        atomicAdd(&cells[from * CLASSES + to], 1u);
        change = from != to;
      } else {
        first[key] = v;
        run_start[key] = static_cast<int32_t>(p);
      }
      if (p + 1 >= events || keys[p + 1] != key) {
        last[key] = v;
        run_end[key] = static_cast<int32_t>(p + 1);
      }
    }
    // changes: one add per wave and media, not one per change. A media's lanes are neighbours, so
    // the first lane of every stretch of one key adds the stretch's changes.
    const uint32_t left = __shfl_up(key, 1);
    const bool head = lane == 0 || left != key;
    const unsigned long long heads = __ballot(head);
    const unsigned long long changed = __ballot(change);
    if (head && valid) {
      const unsigned long long above = heads & ~((2ull << lane) - 1ull);  // the heads after this lane
      const int end = above ? __ffsll(above) - 1 : 64;
      const unsigned long long stretch = (end == 64 ? ~0ull : (1ull << end) - 1ull) & ~((1ull << lane) - 1ull);
      const uint32_t count = static_cast<uint32_t>(__popcll(changed & stretch));
      if (count) atomicAdd(&changes[key], count);
    }
  }
  __syncthreads();
  for (int k = threadIdx.x; k < static_cast<int>(CLASSES * CLASSES); k += BLOCK)
    if (cells[k]) atomicAdd(&matrix[k], cells[k]);
}

}  // namespace

// C ABI for ctypes (ops/gpu_transitions.py). All pointers are device pointers from torch tensors on
// the caller's device; `stream` is the torch stream (hipStream_t). Each returns a hipError_t and
// launches nothing for a count <= 0.

// classify.
//   dialect      0 = upb, 1 = protobufjs
//   rows         n StatusEvent, written for every frame
//   is_event     n int32, written for every frame: 1 for a status event, else 0
//   counters     2 uint32, zeroed by the caller: status decode errors, the length of `overflow`
//   overflow     n int32: the frames left to the host, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_transitions_classify(
    const void* buf, const void* offs, int n, int dialect, void* rows, void* is_event, void* counters, void* overflow,
    void* stream) {
  if (n <= 0) return 0;
  if ((dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) || !buf || !offs || !rows || !is_event || !counters ||
      !overflow)
    return static_cast<int>(hipErrorInvalidValue);
  const int grid = blocks_of(n, BLOCK);
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* rw = static_cast<StatusEvent*>(rows);
  auto* ie = static_cast<int32_t*>(is_event);
  auto* c = static_cast<uint32_t*>(counters);
  auto* ov = static_cast<int32_t*>(overflow);
  if (dialect == DIALECT_PROTOBUFJS)
    hipLaunchKernelGGL(tr_classify<DIALECT_PROTOBUFJS>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, rw, ie, c, ov);
  else
    hipLaunchKernelGGL(tr_classify<DIALECT_UPB>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, rw, ie, c, ov);
  return static_cast<int>(hipGetLastError());
}

// claim, over the rows of an earlier classify.
//   hash_mask    ANDed onto every hash before the home slot is taken (all ones in production)
//   claim        `slots` uint64, zeroed by the caller: 0 or 1 + the frame that claimed the slot
//   slot_used    `slots` int32, zeroed by the caller: 1 for a claimed slot
//   slot_of      n uint32: the slot of every status event's media; the other frames' are not written
//   slots        a power of two, at least 2n and at most 2^30 (the slot scan counts them in an int)
extern "C" __attribute__((visibility("default"))) int bh_transitions_claim(
    const void* buf, const void* rows, int n, unsigned long long hash_mask, void* claim, void* slot_used, void* slot_of,
    long long slots, void* stream) {
  if (n <= 0) return 0;
  if (slots < 2ll * n || slots > (1ll << 30) || (slots & (slots - 1)) != 0 || !buf || !rows || !claim || !slot_used ||
      !slot_of)
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(tr_claim, dim3(blocks_of(n, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint8_t*>(buf), static_cast<const StatusEvent*>(rows), n,
                     static_cast<uint32_t>(slots - 1), hash_mask, static_cast<unsigned long long*>(claim),
                     static_cast<int32_t*>(slot_used), static_cast<uint32_t*>(slot_of));
  return static_cast<int>(hipGetLastError());
}

// compact, after the two scans.
//   frame        the event scan's indices: the first `events` are the status events' frames in stream order
//   slot_rank    the slot scan's pos, `slots` uint64: rank << 32 | rank
//   keys, vals   `events` uint32 and uint64, written: the media number, and frame << 32 | status
extern "C" __attribute__((visibility("default"))) int bh_transitions_compact(
    const void* rows, const void* frame, const void* slot_of, const void* slot_rank, int events, void* keys, void* vals,
    void* stream) {
  if (events <= 0) return 0;
  if (!rows || !frame || !slot_of || !slot_rank || !keys || !vals) return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(tr_compact, dim3(blocks_of(events, BLOCK)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const StatusEvent*>(rows), static_cast<const int32_t*>(frame),
                     static_cast<const uint32_t*>(slot_of), static_cast<const uint64_t*>(slot_rank), events,
                     static_cast<uint32_t*>(keys), static_cast<uint64_t*>(vals));
  return static_cast<int>(hipGetLastError());
}

// One pass of the sort over bits [shift, shift + 8) of the keys. With blocks = ceil(events / 2048):
//   totals, base   256 * blocks uint32 each, scratch, 16-byte aligned
//   keys_out, vals_out   `events` each, written; they must not be the inputs
//   stages       bit 0 count, bit 1 totals, bit 2 apply; the probe times them apart, everything else
//                passes 7. A later stage reads what the earlier ones of an earlier call wrote.
extern "C" __attribute__((visibility("default"))) int bh_transitions_sort_pass(
    const void* keys, const void* vals, int events, int shift, void* totals, void* base, void* keys_out, void* vals_out,
    int stages, void* stream) {
  if (events <= 0) return 0;
  if (shift < 0 || shift > 24 || (shift & 7) || stages < 1 || stages > 7 || !keys || !vals || !totals || !base ||
      !keys_out || !vals_out || keys == keys_out || vals == vals_out ||
      ((reinterpret_cast<uintptr_t>(totals) | reinterpret_cast<uintptr_t>(base)) & 15u))
    return static_cast<int>(hipErrorInvalidValue);
  const int blocks = blocks_of(events, BLOCK * TILES);
  auto st = static_cast<hipStream_t>(stream);
  const auto* k = static_cast<const uint32_t*>(keys);
  auto* tt = static_cast<uint32_t*>(totals);
  auto* bs = static_cast<uint32_t*>(base);
  hipError_t err = hipSuccess;
  if (stages & 1) {
    hipLaunchKernelGGL(sort_count, dim3(blocks), dim3(BLOCK), 0, st, k, events, shift, tt);
    err = hipGetLastError();
    if (err != hipSuccess) return static_cast<int>(err);
  }
  if (stages & 2) {
    hipLaunchKernelGGL(sort_totals, dim3(1), dim3(BLOCK), 0, st, tt, static_cast<long long>(RADIX) * blocks, bs);
    err = hipGetLastError();
    if (err != hipSuccess) return static_cast<int>(err);
  }
  if (stages & 4) {
    hipLaunchKernelGGL(sort_apply, dim3(blocks), dim3(BLOCK), 0, st, k, static_cast<const uint64_t*>(vals), events, shift,
                       bs, static_cast<uint32_t*>(keys_out), static_cast<uint64_t*>(vals_out));
    err = hipGetLastError();
  }
  return static_cast<int>(err);
}

// pairs, over the sorted keys and vals.
//   groups       the media count: every key is below it
//   known_mask   bit s set: s is a number of TelemetryStatusEntry
//   matrix       65 * 65 uint32, zeroed by the caller: cell [from * 65 + to]
//   first, last  `groups` uint64 each: frame << 32 | status of the media's first and last status event
//   run_start, run_end   `groups` int32 each: the media's run is [run_start, run_end) of the sorted arrays
//   changes      `groups` uint32, zeroed by the caller
extern "C" __attribute__((visibility("default"))) int bh_transitions_pairs(
    const void* keys, const void* vals, int events, int groups, unsigned long long known_mask, void* matrix, void* first,
    void* last, void* run_start, void* run_end, void* changes, void* stream) {
  if (events <= 0) return 0;
  if (groups < 1 || groups > events || !keys || !vals || !matrix || !first || !last || !run_start || !run_end || !changes)
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(tr_pairs, dim3(blocks_of(events, BLOCK * TILES)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint32_t*>(keys), static_cast<const uint64_t*>(vals), events,
                     static_cast<uint32_t>(groups), known_mask, static_cast<uint32_t*>(matrix),
                     static_cast<uint64_t*>(first), static_cast<uint64_t*>(last), static_cast<int32_t*>(run_start),
                     static_cast<int32_t*>(run_end), static_cast<uint32_t*>(changes));
  return static_cast<int>(hipGetLastError());
}
