// Drop the byte-identical repeat frames of a framed telemetry stream on the GPU (gfx950): the device
// half of `python -m beholder_amd dedupe --device gpu` (beholder_amd/dedupe.py, ops/gpu_dedupe.py).
//
// Input is what the fold, the extract and the coalesce take (telemetry_fold.hip): the capture as it
// lies in the file and `offs[n + 1]`, the frame starts from the host's one pass over the length
// headers. The key of a frame is its own bytes: its content, the topic byte and the body. So there
// is no protobuf decode, no dialect and no "id is not ASCII" host path. The kernels here end at
// keep_len[m], the frame's length where it is kept and 0 where it is not; the prefix sum and the
// gather over keep_len are the extract's (telemetry_select.hip), called as they are.
//
// Three launches on one stream:
//
//  hash, dedupe_hash, one lane per frame (telemetry_dedupe.hpp dedupe_kind). A frame whose topic
//    is not selected is KEEP; only its topic byte is read. A frame whose content is longer than
//    DEDUPE_DEVICE_MAX goes to an overflow list through an atomic cursor: the host decides those.
//    Every other frame gets its 64-bit content hash. Writes one 16-byte row {hash, off, len}:
//    len is the content's length, 0 for KEEP and -1 for a host frame.
//  claim, dedupe_claim, one lane per frame that takes part finds its content's slot in the table
//    (media_table.hpp claim_slot over `slots` entries, a power of two, >= 2n): contents are the same
//    where length, then hash, then the bytes are, so nothing depends on the hash (hash_mask = 0
//    stays exact). Then one atomic max on the slot's winner word, of m + 1 under
//    keep=last and of n - m under keep=first: the winner is the content's last or first frame by
//    index, not by arrival, so every result is the same from run to run, and the table starts from
//    zeros either way. The lane writes its slot to slot_of[m].
//  mark, dedupe_mark, one lane per frame. keep_len[m] = offs[m + 1] - offs[m] where the frame is
//    KEEP or the winner of its slot, else 0. Host frames get 0 here; the host decides them by
//    content in a plain dict and scatters their lengths into keep_len before the scan.
//
// A host frame is longer than the cap and a device frame is not, so the two never share a content:
// unlike the coalesce there is no step that resolves host against device.
//
// Every loop over bytes is bounded by DEDUPE_DEVICE_MAX, the walk by the table's size.
//
// Visibility is media_table.hpp's rule: claim reads the rows of hash and the stream, mark reads
// slot_of and the winners of claim.
#include "telemetry_dedupe.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;

struct DedupeRow {
  uint64_t hash;
  int32_t off;  // the content's start in buf: the frame's start + 4
  int32_t len;  // the content's length; 0: KEEP, -1: left to the host
};
static_assert(sizeof(DedupeRow) == 16, "ops/gpu_dedupe.py views the rows as (n, 2) int64");

template <bool WIDE>
__global__ __launch_bounds__(BLOCK) void dedupe_hash(const uint8_t* __restrict__ buf,
                                                     const int32_t* __restrict__ offs, int n, const DedupeParams s,
                                                     DedupeRow* __restrict__ rows, uint32_t* __restrict__ cursor,
                                                     int32_t* __restrict__ overflow) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const int head = offs[m];
  const int end = offs[m + 1];
  const int kind = dedupe_kind(buf, head, end, s);
  DedupeRow row{0, head + 4, 0};
  if (kind == DK_HOST) {
    row.len = -1;
    overflow[atomicAdd(cursor, 1u)] = m;  // at most one per frame: stays below n
  } else if (kind == DK_ROW) {
    row.len = end - head - 4;  // 1..DEDUPE_DEVICE_MAX
    row.hash = content_hash<WIDE>(buf + row.off, row.len);
  }
  rows[m] = row;
}

template <bool WIDE>
__global__ __launch_bounds__(BLOCK) void dedupe_claim(const uint8_t* __restrict__ buf,
                                                      const DedupeRow* __restrict__ rows, int n, uint32_t slot_mask,
                                                      uint64_t hash_mask, uint32_t first,
                                                      unsigned long long* __restrict__ claim,
                                                      uint32_t* __restrict__ winner, int32_t* __restrict__ slot_of) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const DedupeRow row = rows[m];
  if (row.len <= 0) return;
  const unsigned long long me = static_cast<unsigned long long>(m) + 1ull;
  const auto same_content = [&](unsigned long long owner) {
    const DedupeRow o = rows[owner];  // a row with len > 0: only such lanes claim
    return o.len == row.len && o.hash == row.hash && content_equal<WIDE>(buf + o.off, buf + row.off, row.len);
  };
  const uint32_t slot = claim_slot(claim, slot_mask, home_slot(row.hash, hash_mask, slot_mask), me, same_content).slot;
  // n < 2^31; both values are in 1..n, so 0 stays "no frame"
  atomicMax(&winner[slot], first ? static_cast<uint32_t>(n - m) : static_cast<uint32_t>(me));
  slot_of[m] = static_cast<int32_t>(slot);
}

__global__ __launch_bounds__(BLOCK) void dedupe_mark(const int32_t* __restrict__ offs,
                                                     const DedupeRow* __restrict__ rows, int n,
                                                     const uint32_t* __restrict__ winner,
                                                     const int32_t* __restrict__ slot_of, uint32_t slot_mask,
                                                     uint32_t first, int32_t* __restrict__ keep_len) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const int32_t len = rows[m].len;
  bool keep = len == 0;
  // masked: a slot_of that claim did not write must not index past the table
  if (len > 0)
    keep = winner[static_cast<uint32_t>(slot_of[m]) & slot_mask] ==
           (first ? static_cast<uint32_t>(n - m) : static_cast<uint32_t>(m) + 1u);
  keep_len[m] = keep ? offs[m + 1] - offs[m] : 0;
}

}  // namespace

// C ABI for ctypes (ops/gpu_dedupe.py). All pointers but `params` are device pointers from torch
// tensors on the caller's device; `stream` is the torch stream (hipStream_t). Returns a hipError_t
// (hipErrorInvalidValue for a bad table size or `stages`). n <= 0 launches nothing.
//   buf, offs    the framed stream and its n + 1 frame starts (host-checked, see above)
//   params       host pointer to a DedupeParams, copied into the kernels' arguments;
//                params->slot_mask + 1 = slots, a power of two, at least 2n
//   rows         n DedupeRow, written by hash
//   cursor       one uint32, zeroed by the caller: the length of `overflow` afterwards
//   overflow     n int32: the frames left to the host, in no particular order
//   claim        `slots` uint64, zeroed by the caller: 0 or 1 + the frame that claimed the slot
//   winner       `slots` uint32, zeroed by the caller: 0, or 1 + the last frame of the slot's
//                content (keep=last), or n - the first frame (keep=first)
//   slot_of      n int32: written for frames that take part on the device only
//   keep_len     n int32, written for every frame
//   stages       bit 0 hash, bit 1 claim, bit 2 mark; the probe times them apart, everything else
//                passes 7. A later stage reads what the earlier ones of an earlier call wrote.
extern "C" __attribute__((visibility("default"))) int bh_dedupe_mark(
    const void* buf, const void* offs, int n, const void* params, void* rows, void* cursor, void* overflow,
    void* claim, void* winner, void* slot_of, void* keep_len, int stages, void* stream) {
  if (n <= 0) return 0;
  if (!params || stages < 1 || stages > 7) return static_cast<int>(hipErrorInvalidValue);
  const DedupeParams s = *static_cast<const DedupeParams*>(params);
  const long long slots = static_cast<long long>(s.slot_mask) + 1;
  if (slots < 2ll * n || (slots & (slots - 1)) != 0) return static_cast<int>(hipErrorInvalidValue);
  if (!buf || !offs || !rows || !cursor || !overflow || !claim || !winner || !slot_of || !keep_len)
    return static_cast<int>(hipErrorInvalidValue);
  const int grid = (n + BLOCK - 1) / BLOCK;
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* rw = static_cast<DedupeRow*>(rows);
  auto* cu = static_cast<uint32_t*>(cursor);
  auto* ov = static_cast<int32_t*>(overflow);
  auto* cl = static_cast<unsigned long long*>(claim);
  auto* wi = static_cast<uint32_t*>(winner);
  auto* so = static_cast<int32_t*>(slot_of);
  const bool wide = (s.flags & DF_WIDE) != 0;
  const uint32_t first = (s.flags & DF_FIRST) ? 1u : 0u;
  hipError_t err = hipSuccess;
  if (stages & 1) {
    if (wide) hipLaunchKernelGGL(dedupe_hash<true>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, s, rw, cu, ov);
    else hipLaunchKernelGGL(dedupe_hash<false>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, s, rw, cu, ov);
    err = hipGetLastError();
    if (err != hipSuccess) return static_cast<int>(err);
  }
  if (stages & 2) {
    if (wide)
      hipLaunchKernelGGL(dedupe_claim<true>, dim3(grid), dim3(BLOCK), 0, st, b, rw, n, s.slot_mask, s.hash_mask, first,
                         cl, wi, so);
    else
      hipLaunchKernelGGL(dedupe_claim<false>, dim3(grid), dim3(BLOCK), 0, st, b, rw, n, s.slot_mask, s.hash_mask, first,
                         cl, wi, so);
    err = hipGetLastError();
    if (err != hipSuccess) return static_cast<int>(err);
  }
  if (stages & 4) {
    hipLaunchKernelGGL(dedupe_mark, dim3(grid), dim3(BLOCK), 0, st, o, rw, n, wi, so, s.slot_mask, first,
                       static_cast<int32_t*>(keep_len));
    err = hipGetLastError();
  }
  return static_cast<int>(err);
}
