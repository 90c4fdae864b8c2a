// Cut a framed telemetry stream down to the frames that set its end state on the GPU (gfx950): the
// device half of `python -m beholder_amd coalesce --device gpu` (beholder_amd/coalesce.py,
// ops/gpu_coalesce.py).
//
// Input is what the fold and the extract take (telemetry_fold.hip): the capture as it lies in the
// file and `offs[n + 1]`, the frame starts from the host's one pass over the length headers. The
// kernels here end at keep_len[m], the frame's length where it is kept and 0 where it is not; the
// prefix sum and the gather over keep_len are the extract's (telemetry_select.hip), called as they are.
//
// Three launches on one stream:
//
//  classify, coalesce_classify, one lane per frame. Reads the frame by its topic
//    (telemetry_readers.hpp, upb in its STRICT form) and decides it (telemetry_coalesce.hpp classify):
//    drop, keep, keyed, or left to the host. Writes one 24-byte row
//      {hash, id_off, id_len, status, kind | topic}
//    Frames left to the host go to an overflow list through an atomic cursor.
//  claim, coalesce_claim, one lane per keyed frame finds its key's slot in the group table
//    (media_table.hpp claim_slot over `slots` entries, a power of two, >= 2n): keys are the same
//    where topic, status, length, hash and then the id's bytes are.
//    Then an atomic max of m + 1 on the slot's winner word: the winner is the key's last frame by
//    index, not by arrival, so every result is the same from run to run. The lane writes its slot
//    to slot_of[m].
//  mark, coalesce_mark, one lane per frame. keep_len[m] = offs[m + 1] - offs[m] where the frame is
//    kept (kind keep, or keyed and winner[slot_of[m]] == m + 1), else 0; keyed[m] = 1 for a keyed
//    frame. Host frames get 0 here; the host decides them and scatters their lengths into keep_len
//    before the scan.
//
// Visibility is media_table.hpp's rule: claim reads the rows of classify, mark reads slot_of and the
// winners of claim.
#include "telemetry_coalesce.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;

struct CoalesceRow {
  uint64_t hash;
  int32_t id_off;
  int32_t id_len;
  int32_t status;
  uint32_t flags;  // CL_* in the low two bits, R_STATUS
};
static_assert(sizeof(CoalesceRow) == 24, "ops/gpu_coalesce.py views the rows as (n, 6) int32");

constexpr uint32_t R_KIND = 3;    // mask of the CL_* kind
constexpr uint32_t R_STATUS = 4;  // topic 1 (else topic 2); keyed rows only

template <int DIALECT>
__global__ __launch_bounds__(BLOCK) void coalesce_classify(const uint8_t* __restrict__ buf,
                                                           const int32_t* __restrict__ offs, int n,
                                                           const CoalesceParams s, CoalesceRow* __restrict__ rows,
                                                           uint32_t* __restrict__ cursor,
                                                           int32_t* __restrict__ overflow) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const int head = offs[m];
  const int end = offs[m + 1];
  CoalesceKey key{0, 0, 0, 0, 0};
  const int kind = classify<DIALECT>(buf, head, end, s, key);
  CoalesceRow row{0, 0, 0, 0, static_cast<uint32_t>(kind)};
  if (kind == CL_HOST) {
    overflow[atomicAdd(cursor, 1u)] = m;  // at most one per frame: stays below n
  } else if (kind == CL_KEYED) {
    row.hash = key.hash;
    row.id_off = key.id_off;
    row.id_len = key.id_len;
    row.status = key.status;
    if (key.topic == 1) row.flags |= R_STATUS;
  }
  rows[m] = row;
}

__global__ __launch_bounds__(BLOCK) void coalesce_claim(const uint8_t* __restrict__ buf,
                                                        const CoalesceRow* __restrict__ rows, int n,
                                                        uint32_t slot_mask, uint64_t hash_mask,
                                                        unsigned long long* __restrict__ claim,
                                                        uint32_t* __restrict__ winner, int32_t* __restrict__ slot_of) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const CoalesceRow row = rows[m];
  if ((row.flags & R_KIND) != CL_KEYED) return;
  const unsigned long long me = static_cast<unsigned long long>(m) + 1ull;
  const auto same_key = [&](unsigned long long owner) {
    const CoalesceRow o = rows[owner];  // a keyed row: only keyed lanes claim
    return o.flags == row.flags && o.status == row.status && o.id_len == row.id_len && o.hash == row.hash &&
           bytes_equal(buf + o.id_off, buf + row.id_off, row.id_len);
  };
  const uint32_t slot = claim_slot(claim, slot_mask, home_slot(row.hash, hash_mask, slot_mask), me, same_key).slot;
  atomicMax(&winner[slot], static_cast<uint32_t>(me));  // n < 2^31
  slot_of[m] = static_cast<int32_t>(slot);
}

__global__ __launch_bounds__(BLOCK) void coalesce_mark(const int32_t* __restrict__ offs,
                                                       const CoalesceRow* __restrict__ rows, int n,
                                                       const uint32_t* __restrict__ winner,
                                                       const int32_t* __restrict__ slot_of, uint32_t slot_mask,
                                                       int32_t* __restrict__ keep_len, uint8_t* __restrict__ keyed) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const uint32_t kind = rows[m].flags & R_KIND;
  bool keep = kind == CL_KEEP;
  // masked: a slot_of that claim did not write must not index past the table
  if (kind == CL_KEYED) keep = winner[static_cast<uint32_t>(slot_of[m]) & slot_mask] == static_cast<uint32_t>(m) + 1u;
  keep_len[m] = keep ? offs[m + 1] - offs[m] : 0;
  keyed[m] = kind == CL_KEYED ? 1 : 0;
}

}  // namespace

// C ABI for ctypes (ops/gpu_coalesce.py). All pointers but `params` are device pointers from torch
// tensors on the caller's device; `stream` is the torch stream (hipStream_t). Returns a hipError_t
// (hipErrorInvalidValue for an unknown dialect, a bad table size or `stages`). n <= 0 launches nothing.
//   buf, offs    the framed stream and its n + 1 frame starts (host-checked, see above)
//   dialect      0 = upb, 1 = protobufjs
//   params       host pointer to a CoalesceParams, copied into the kernels' arguments;
//                params->slot_mask + 1 = slots, a power of two, at least 2n
//   rows         n CoalesceRow, written by classify
//   cursor       one uint32, zeroed by the caller: the length of `overflow` afterwards
//   overflow     n int32: the frames left to the host, in no particular order
//   claim        `slots` uint64, zeroed by the caller: 0 or 1 + the frame that claimed the slot
//   winner       `slots` uint32, zeroed by the caller: 0 or 1 + the last frame of the slot's key
//   slot_of      n int32: written for keyed frames only
//   keep_len     n int32, written for every frame; keyed: n uint8, written for every frame
//   stages       bit 0 classify, bit 1 claim, bit 2 mark; the probe times them apart, everything
//                else passes 7. A later stage reads what the earlier ones of an earlier call wrote.
extern "C" __attribute__((visibility("default"))) int bh_coalesce_mark(
    const void* buf, const void* offs, int n, int dialect, const void* params, void* rows, void* cursor,
    void* overflow, void* claim, void* winner, void* slot_of, void* keep_len, void* keyed, int stages, void* stream) {
  if (n <= 0) return 0;
  if ((dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) || !params || stages < 1 || stages > 7)
    return static_cast<int>(hipErrorInvalidValue);
  const CoalesceParams s = *static_cast<const CoalesceParams*>(params);
  const long long slots = static_cast<long long>(s.slot_mask) + 1;
  if (slots < 2ll * n || (slots & (slots - 1)) != 0) return static_cast<int>(hipErrorInvalidValue);
  if (!buf || !offs || !rows || !cursor || !overflow || !claim || !winner || !slot_of || !keep_len || !keyed)
    return static_cast<int>(hipErrorInvalidValue);
  const int grid = (n + BLOCK - 1) / BLOCK;
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* rw = static_cast<CoalesceRow*>(rows);
  auto* cu = static_cast<uint32_t*>(cursor);
  auto* ov = static_cast<int32_t*>(overflow);
  auto* wi = static_cast<uint32_t*>(winner);
  auto* so = static_cast<int32_t*>(slot_of);
  hipError_t err = hipSuccess;
  if (stages & 1) {
    if (dialect == DIALECT_PROTOBUFJS)
      hipLaunchKernelGGL(coalesce_classify<DIALECT_PROTOBUFJS>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, s, rw, cu, ov);
    else
      hipLaunchKernelGGL(coalesce_classify<DIALECT_UPB>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, s, rw, cu, ov);
    err = hipGetLastError();
    if (err != hipSuccess) return static_cast<int>(err);
  }
  if (stages & 2) {
    hipLaunchKernelGGL(coalesce_claim, dim3(grid), dim3(BLOCK), 0, st, b, rw, n, s.slot_mask, s.hash_mask,
                       static_cast<unsigned long long*>(claim), wi, so);
    err = hipGetLastError();
    if (err != hipSuccess) return static_cast<int>(err);
  }
  if (stages & 4) {
    hipLaunchKernelGGL(coalesce_mark, dim3(grid), dim3(BLOCK), 0, st, o, rw, n, wi, so, s.slot_mask,
                       static_cast<int32_t*>(keep_len), static_cast<uint8_t*>(keyed));
    err = hipGetLastError();
  }
  return static_cast<int>(err);
}
