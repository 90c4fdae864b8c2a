// Both topics of a framed telemetry stream joined per media, on the GPU (gfx950): the device half of
// `python -m beholder_amd stages --device gpu` (beholder_amd/stages.py, ops/gpu_stages.py).
//
// Input is what the fold takes (telemetry_fold.hip): the capture as it lies in the file and
// `offs[n + 1]`, the frame starts from the host's one pass over the length headers. What comes back
// is a reduction: three tables of counts by status class, one row per media, and the lead events.
//
// What a progress event adds depends on the latest earlier status event of its media, at any
// distance. The events of both topics go through the transitions' stable sort by media
// (telemetry_transitions.hip), called as it is: a media's events of both topics then lie next to each
// other in stream order, and "the latest earlier status event" becomes a value carried forward along
// the sorted positions. The stages, each a launch or a few on one stream:
//
//  classify, st_classify, one lane per frame (telemetry_stages.hpp stages_classify): a topic-1 frame
//    is read as the transitions read it, a topic-2 frame as the thin reads it. The lane counts the
//    decode error under its topic (per block in LDS, then one atomic each), or hands the frame to the
//    CPU through the overflow list with its atomic cursor, or writes the event's row, is_event[m] = 1
//    and aux[m]: the progress, and a bit for a status event. Other topics are not read.
//  claim, rank, compact and sort are the transitions' and the extract's entry points over the rows
//    of both topics: keys[p] is the media number of the p-th event by media and stream order,
//    vals[p] its frame << 32 | status.
//  carry, three launches: an inclusive scan with `max` over the sorted positions, of two components:
//      A[p] = (p + 1) << 32 | uint32(status) where position p holds a status event, else 0;
//      B[p] = p + 1 where p is the first position of its media's run, else 0.
//    max over A picks the status event with the largest position at or before p and brings its
//    status along in the low half; max over B the latest run start, which is p's own run's.
//      carry_reduce  per block of 256 positions: gathers saux[p] = aux[frame of p], so that every
//                    later read is of consecutive words, and writes the block's two maxima;
//      carry_totals  one block scans the blocks' maxima in tiles of 256 with a running carry, so any
//                    number of blocks takes one launch; base[b] is the inclusive maximum over the
//                    blocks 0..b;
//      carry_apply   per block, the scan of its 256 positions (64-lane waves with __shfl_up, then
//                    the four waves' maxima through LDS) joined with base[b - 1]: stand[p] is the
//                    position of the latest status event at or before p or -1, stood[p] that
//                    event's status, head[p] the first position of p's run.
//    The scan is over the whole array and not segmented by media. It need not be: a run is a
//    contiguous range, so every position in [head[p], p] belongs to p's media and every position
//    below head[p] to another. The latest status position at or before p is therefore p's media's
//    iff it is >= head[p]; where it is smaller, no status event of p's media lies at or before p at
//    all, since that one would be later than the one found. stand[p] is valid iff stand[p] >= head[p].
//  settle, st_settle, one lane per sorted position, laid out as tr_pairs is (a block takes eight
//    tiles of 256), reading its own words and its successor's only. A status event adds to
//    entered[class]. A progress event with a valid stand adds to matrix[class of stood][its own
//    class]; one without is a lead event and sets lead_flag[p]. A position with a valid stand whose
//    successor is a status event of the same run closes a stage of p - stand[p] progress events into
//    closed[class of stood][bucket_of]. The three tables are summed per block in LDS
//    (65 * 65 + 65 + 65 * 14 words, 20,800 bytes) and flushed with one global atomic add per non-zero
//    word. The lead event whose successor is not one writes its media's lead count and last
//    progress; the run's last position writes the run's bounds, the open stage's position and the
//    last progress. Each of these words has exactly one writer.
//
// Visibility is media_table.hpp's rule: within a launch workgroups meet only in atomics; every plain
// load reads what an earlier launch or the host wrote, which is why the carry is three launches and
// not a single look-back pass. No kernel waits for another workgroup. All sums and maxima are of
// integers: the result is exact and the same from run to run.
#include "launch_grid.hpp"
#include "telemetry_stages.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;  // threads per block; positions per block of the carry: ops/gpu_stages.py CARRY_BLOCK
constexpr int WAVES = BLOCK / 64;
constexpr int TILES = 8;    // a block of the settle takes TILES * BLOCK consecutive positions, as tr_pairs does

// counters[]: ops/gpu_stages.py reads the same layout; the first two are the transitions'
constexpr int C_STATUS_ERR = 0, C_OVERFLOW = 1, C_PROGRESS_ERR = 2;

constexpr uint32_t T_MATRIX = 0, T_ENTERED = CLASSES * CLASSES, T_CLOSED = T_ENTERED + CLASSES,
                   T_WORDS = T_CLOSED + CLASSES * BUCKETS;  // the settle's tables, one after the other

template <int DIALECT>
__global__ __launch_bounds__(BLOCK) void st_classify(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                     int n, StatusEvent* __restrict__ rows,
                                                     uint64_t* __restrict__ aux, int32_t* __restrict__ is_event,
                                                     uint32_t* __restrict__ counters, int32_t* __restrict__ overflow) {
  __shared__ uint32_t errors[2];
  if (threadIdx.x < 2) errors[threadIdx.x] = 0;
  __syncthreads();
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n) {
    StatusEvent ev;
    uint64_t a;
    const int head = offs[m];
    const int kind = stages_classify<DIALECT>(buf, head, offs[m + 1], ev, a);
    if (kind == ST_HOST) overflow[atomicAdd(&counters[C_OVERFLOW], 1u)] = m;  // at most one per frame: stays below n
    if (kind == ST_ERROR) atomicAdd(&errors[buf[head + 4] == 1 ? 0 : 1], 1u);
    rows[m] = ev;
    aux[m] = a;
    is_event[m] = kind == ST_EVENT ? 1 : 0;
  }
  __syncthreads();
  if (threadIdx.x == 0 && errors[0]) atomicAdd(&counters[C_STATUS_ERR], errors[0]);
  if (threadIdx.x == 1 && errors[1]) atomicAdd(&counters[C_PROGRESS_ERR], errors[1]);
}

// The two components of the carry, joined by max each. The identity is {0, 0}.
struct Carry {
  uint64_t a;  // (position + 1) << 32 | uint32(status) of a status event
  uint32_t b;  // position + 1 of a run's first position
};

__device__ __forceinline__ Carry join(Carry x, Carry y) {
  return Carry{x.a > y.a ? x.a : y.a, x.b > y.b ? x.b : y.b};
}

// Inclusive max-scan of one Carry per thread over the block; `total` is the block's maximum. wave_a
// and wave_b hold one entry per wave. Every thread of the block must call it.
__device__ __forceinline__ Carry block_scan_max(Carry x, uint64_t* wave_a, uint32_t* wave_b, Carry& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int d = 1; d < 64; d <<= 1) {
    const Carry y{__shfl_up(x.a, d), __shfl_up(x.b, d)};
    if (lane >= d) x = join(x, y);
  }
  __syncthreads();  // the previous call's readers are done with wave_a and wave_b
  if (lane == 63) {
    wave_a[wave] = x.a;
    wave_b[wave] = x.b;
  }
  __syncthreads();
  Carry before{0, 0}, all{0, 0};
  for (int w = 0; w < WAVES; ++w) {
    const Carry t{wave_a[w], wave_b[w]};
    if (w < wave) before = join(before, t);
    all = join(all, t);
  }
  total = all;
  return join(x, before);
}

// What position p puts into the scan: saux[p] is its aux word.
__device__ __forceinline__ Carry carry_of(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ vals,
                                          uint64_t saux, long long p) {
  const uint64_t at = static_cast<uint64_t>(p + 1);
  Carry x{0, 0};
  if (aux_is_status(saux)) x.a = (at << 32) | (vals[p] & 0xffffffffull);
  if (p == 0 || keys[p - 1] != keys[p]) x.b = static_cast<uint32_t>(at);  // in the previous block as well
  return x;
}

__global__ __launch_bounds__(BLOCK) void carry_reduce(const uint32_t* __restrict__ keys,
                                                      const uint64_t* __restrict__ vals, int events, uint32_t n,
                                                      const uint64_t* __restrict__ aux, uint64_t* __restrict__ saux,
                                                      uint64_t* __restrict__ totals) {
  __shared__ uint64_t wave_a[WAVES];
  __shared__ uint32_t wave_b[WAVES];
  const long long p = static_cast<long long>(blockIdx.x) * BLOCK + threadIdx.x;
  Carry x{0, 0};
  if (p < events) {
    const uint32_t frame = static_cast<uint32_t>(vals[p] >> 32);
    const uint64_t a = frame < n ? aux[frame] : 0ull;  // always inside: the frames are the event scan's indices
    saux[p] = a;
    x = carry_of(keys, vals, a, p);
  }
  Carry total;
  block_scan_max(x, wave_a, wave_b, total);
  if (threadIdx.x == 0) {
    totals[2 * static_cast<size_t>(blockIdx.x)] = total.a;
    totals[2 * static_cast<size_t>(blockIdx.x) + 1] = total.b;
  }
}

// One block. base[b] = max(totals[0], ..., totals[b]) per component, for b in [0, blocks).
__global__ __launch_bounds__(BLOCK) void carry_totals(const uint64_t* __restrict__ totals, int blocks,
                                                      uint64_t* __restrict__ base) {
  __shared__ uint64_t wave_a[WAVES];
  __shared__ uint32_t wave_b[WAVES];
  Carry carry{0, 0};
  for (int tile = 0; tile < blocks; tile += BLOCK) {  // the trip count is the same for every thread
    const int b = tile + threadIdx.x;
    Carry x{0, 0};
    if (b < blocks) x = Carry{totals[2 * static_cast<size_t>(b)], static_cast<uint32_t>(totals[2 * static_cast<size_t>(b) + 1])};
    Carry total;
    const Carry incl = join(carry, block_scan_max(x, wave_a, wave_b, total));
    if (b < blocks) {
      base[2 * static_cast<size_t>(b)] = incl.a;
      base[2 * static_cast<size_t>(b) + 1] = incl.b;
    }
    carry = join(carry, total);
  }
}

__global__ __launch_bounds__(BLOCK) void carry_apply(const uint32_t* __restrict__ keys,
                                                     const uint64_t* __restrict__ vals, int events,
                                                     const uint64_t* __restrict__ saux,
                                                     const uint64_t* __restrict__ base, int32_t* __restrict__ stand,
                                                     int32_t* __restrict__ stood, int32_t* __restrict__ head) {
  __shared__ uint64_t wave_a[WAVES];
  __shared__ uint32_t wave_b[WAVES];
  const long long p = static_cast<long long>(blockIdx.x) * BLOCK + threadIdx.x;
  Carry x{0, 0};
  if (p < events) x = carry_of(keys, vals, saux[p], p);
  Carry total;
  Carry incl = block_scan_max(x, wave_a, wave_b, total);
  if (blockIdx.x > 0) {
    const size_t b = static_cast<size_t>(blockIdx.x) - 1;
    incl = join(incl, Carry{base[2 * b], static_cast<uint32_t>(base[2 * b + 1])});
  }
  if (p >= events) return;
  stand[p] = static_cast<int32_t>(incl.a >> 32) - 1;  // -1: no status event at or before p
  stood[p] = static_cast<int32_t>(static_cast<uint32_t>(incl.a & 0xffffffffull));
  head[p] = static_cast<int32_t>(incl.b) - 1;         // position 0 starts a run, so never -1
}

__global__ __launch_bounds__(BLOCK) void st_settle(const uint32_t* __restrict__ keys, const uint64_t* __restrict__ vals,
                                                   const uint64_t* __restrict__ saux, const int32_t* __restrict__ stand,
                                                   const int32_t* __restrict__ stood, const int32_t* __restrict__ head,
                                                   int events, uint32_t groups, uint64_t known_mask,
                                                   uint32_t* __restrict__ tables, int32_t* __restrict__ media_rows,
                                                   int32_t* __restrict__ lead_flag) {
  __shared__ uint32_t cells[T_WORDS];
  for (uint32_t k = threadIdx.x; k < T_WORDS; k += BLOCK) cells[k] = 0u;
  __syncthreads();
  for (int t = 0; t < TILES; ++t) {
    const long long p = (static_cast<long long>(blockIdx.x) * TILES + t) * BLOCK + threadIdx.x;
    if (p >= events) continue;
    const uint32_t key = keys[p];
    const int32_t st = stand[p], hd = head[p];
    // never: a key is a claimed slot's rank, and the carry's positions lie in [0, p]
    if (key >= groups || hd < 0 || hd > p || st > p) {
      lead_flag[p] = 0;
      continue;
    }
    const uint64_t a = saux[p];
    const bool is_status = aux_is_status(a);
    const int32_t progress = aux_progress(a);
    const bool standing = st >= hd;
    const uint32_t mine = class_of(static_cast<int32_t>(vals[p] & 0xffffffffull), known_mask);
    const uint32_t under = class_of(stood[p], known_mask);  // read only where `standing`
    if (is_status) atomicAdd(&cells[T_ENTERED + mine], 1u);
    else if (standing) atomicAdd(&cells[T_MATRIX + under * CLASSES + mine], 1u);
    lead_flag[p] = !is_status && !standing ? 1 : 0;
    const bool run_ends = p + 1 >= events || keys[p + 1] != key;
    const bool status_next = !run_ends && aux_is_status(saux[p + 1]);
    const uint32_t count = standing ? static_cast<uint32_t>(p - st) : 0u;
    int32_t* row = media_rows + static_cast<size_t>(key) * MEDIA_WORDS;
    if (standing && status_next) atomicAdd(&cells[T_CLOSED + under * BUCKETS + bucket_of(count, progress)], 1u);
    if (!standing && (run_ends || status_next)) {  // the last lead event of the media
      row[M_LEAD] = static_cast<int32_t>(p - hd + 1);
      row[M_LEAD_LAST] = progress;
    }
    if (run_ends) {
      row[M_START] = hd;
      row[M_END] = static_cast<int32_t>(p + 1);
      row[M_OPEN] = standing ? st + 1 : 0;
      row[M_LAST] = progress;
    }
  }
  __syncthreads();
  for (uint32_t k = threadIdx.x; k < T_WORDS; k += BLOCK)
    if (cells[k]) atomicAdd(&tables[k], cells[k]);
}

}  // namespace

// C ABI for ctypes (ops/gpu_stages.py). All pointers are device pointers from torch tensors on the
// caller's device; `stream` is the torch stream (hipStream_t). Each returns a hipError_t and launches
// nothing for a count <= 0.

// classify.
//   dialect      0 = upb, 1 = protobufjs
//   rows         n StatusEvent, written for every frame
//   aux          n uint64, written for every frame: the progress of a progress event in the low half,
//                bit 32 for a status event, 0 for a frame that is no event
//   is_event     n int32, written for every frame: 1 for an event of either topic, else 0
//   counters     3 uint32, zeroed by the caller: status decode errors, the length of `overflow`,
//                progress decode errors
//   overflow     n int32: the frames left to the CPU, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_stages_classify(
    const void* buf, const void* offs, int n, int dialect, void* rows, void* aux, void* is_event, void* counters,
    void* overflow, void* stream) {
  if (n <= 0) return 0;
  if ((dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) || !buf || !offs || !rows || !aux || !is_event ||
      !counters || !overflow)
    return static_cast<int>(hipErrorInvalidValue);
  const int grid = blocks_of(n, BLOCK);
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* rw = static_cast<StatusEvent*>(rows);
  auto* ax = static_cast<uint64_t*>(aux);
  auto* ie = static_cast<int32_t*>(is_event);
  auto* c = static_cast<uint32_t*>(counters);
  auto* ov = static_cast<int32_t*>(overflow);
  if (dialect == DIALECT_PROTOBUFJS)
    hipLaunchKernelGGL(st_classify<DIALECT_PROTOBUFJS>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, rw, ax, ie, c, ov);
  else
    hipLaunchKernelGGL(st_classify<DIALECT_UPB>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, rw, ax, ie, c, ov);
  return static_cast<int>(hipGetLastError());
}

// carry, over the sorted keys and vals. With blocks = ceil(events / 256):
//   n            the frame count: every frame in vals is below it
//   aux          n uint64, classify's
//   saux         `events` uint64, written: aux in sorted order
//   totals, base 2 * blocks uint64 each, scratch
//   stand        `events` int32, written: the position of the latest status event at or before the
//                position, -1 where there is none; the media's own iff stand >= head
//   stood        `events` int32, written: that event's status (0 where stand is -1)
//   head         `events` int32, written: the first position of the position's run
extern "C" __attribute__((visibility("default"))) int bh_stages_carry(
    const void* keys, const void* vals, int events, int n, const void* aux, void* saux, void* totals, void* base,
    void* stand, void* stood, void* head, void* stream) {
  if (events <= 0) return 0;
  if (events > n || !keys || !vals || !aux || !saux || !totals || !base || !stand || !stood || !head)
    return static_cast<int>(hipErrorInvalidValue);
  const int blocks = blocks_of(events, BLOCK);
  auto st = static_cast<hipStream_t>(stream);
  const auto* k = static_cast<const uint32_t*>(keys);
  const auto* v = static_cast<const uint64_t*>(vals);
  auto* sa = static_cast<uint64_t*>(saux);
  auto* tt = static_cast<uint64_t*>(totals);
  auto* bs = static_cast<uint64_t*>(base);
  hipLaunchKernelGGL(carry_reduce, dim3(blocks), dim3(BLOCK), 0, st, k, v, events, static_cast<uint32_t>(n),
                     static_cast<const uint64_t*>(aux), sa, tt);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return static_cast<int>(err);
  hipLaunchKernelGGL(carry_totals, dim3(1), dim3(BLOCK), 0, st, tt, blocks, bs);
  err = hipGetLastError();
  if (err != hipSuccess) return static_cast<int>(err);
  hipLaunchKernelGGL(carry_apply, dim3(blocks), dim3(BLOCK), 0, st, k, v, events, sa, bs, static_cast<int32_t*>(stand),
                     static_cast<int32_t*>(stood), static_cast<int32_t*>(head));
  return static_cast<int>(hipGetLastError());
}

// settle, over the sorted keys and vals and the carry's outputs.
//   groups       the media count: every key is below it
//   known_mask   bit s set: s is a number of TelemetryStatusEntry
//   tables       65 * 65 + 65 + 65 * 14 uint32, zeroed by the caller: matrix[standing * 65 + reported],
//                entered[class], closed[class * 14 + bucket]
//   media_rows   groups * 6 int32, zeroed by the caller: M_* of telemetry_stages.hpp
//   lead_flag    `events` int32, written: 1 for a lead event, else 0
extern "C" __attribute__((visibility("default"))) int bh_stages_settle(
    const void* keys, const void* vals, const void* saux, const void* stand, const void* stood, const void* head,
    int events, int groups, unsigned long long known_mask, void* tables, void* media_rows, void* lead_flag,
    void* stream) {
  if (events <= 0) return 0;
  if (groups < 1 || groups > events || !keys || !vals || !saux || !stand || !stood || !head || !tables || !media_rows ||
      !lead_flag)
    return static_cast<int>(hipErrorInvalidValue);
  hipLaunchKernelGGL(st_settle, dim3(blocks_of(events, BLOCK * TILES)), dim3(BLOCK), 0, static_cast<hipStream_t>(stream),
                     static_cast<const uint32_t*>(keys), static_cast<const uint64_t*>(vals),
                     static_cast<const uint64_t*>(saux), static_cast<const int32_t*>(stand),
                     static_cast<const int32_t*>(stood), static_cast<const int32_t*>(head), events,
                     static_cast<uint32_t>(groups), known_mask, static_cast<uint32_t*>(tables),
                     static_cast<int32_t*>(media_rows), static_cast<int32_t*>(lead_flag));
  return static_cast<int>(hipGetLastError());
}
