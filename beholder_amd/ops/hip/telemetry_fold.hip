// Fold a framed telemetry stream into its end state on the GPU (gfx950): the device half of
// `python -m beholder_amd summarise --device gpu` (beholder_amd/replay.py, ops/gpu_fold.py).
//
// Input is the capture as it lies in the file, `u32 L | u8 topic | body` per frame
// (transport/framing.py), and `offs[n + 1]`, the frame starts from the host's one pass over the
// length headers (`frame_index`, ops/csrc/py_codec.cpp; offs[n] = bytes in buf, every frame holds
// its 5 header bytes). Frame m: topic = buf[offs[m] + 4], body = [offs[m] + 5, offs[m + 1]).
//
// Two launches on one stream; nothing per event goes back to the host.
//
//  Pass A, fold_decode, one lane per frame. Topic 1 is read as a TelemetryStatus, topic 2 as a
//    TelemetryProgress (telemetry_readers.hpp; upb in its STRICT form, so it agrees with the CPU
//    codec on every byte string it decides itself). The lane writes one 24-byte row
//      {hash64(id), id_off, id_len, status, flags}
//    and counts: decode errors per topic, progress frames whose status is no known enum number,
//    other topic bytes, and a 64-bin histogram of known progress statuses. Counts are summed per
//    block in LDS; one global atomic per block and non-zero bin.
//    Frames the device does not decide go to an overflow list through an atomic cursor and are
//    folded by the host with the service's codec, counters and all: an id with a byte >= 0x80
//    (its identity is the decoded string, U+FFFD for invalid UTF-8, which the device does not
//    model), and in the upb dialect a non-ASCII host (upb rejects invalid UTF-8) or a start-group.
//  Pass B, fold_group, one lane per frame with the group flag finds its id's slot in the group
//    table (media_table.hpp claim_slot over `slots` entries, a power of two, >= 2n): ids are the
//    same where length, hash and then the bytes are.
//    Group updates: integer atomic adds for the three counts, and last-writer-wins by frame index,
//    not by arrival, through an atomic max on (m + 1) << 32 | status. Every result is therefore the
//    same from run to run.
//
// Visibility is media_table.hpp's rule: in pass B every plain load reads buf, offs or the rows of
// pass A. That is why the passes are two kernels and not one.
#include "media_table.hpp"

namespace {

using namespace bh;

struct FoldRow {
  uint64_t hash;
  int32_t id_off;
  int32_t id_len;
  int32_t status;
  uint32_t flags;
};
static_assert(sizeof(FoldRow) == 24, "ops/gpu_fold.py views the rows as (n, 6) int32");

constexpr uint32_t F_GROUP = 1;   // the frame takes part in pass B
constexpr uint32_t F_STATUS = 2;  // topic 1 (else topic 2)
constexpr uint32_t F_KNOWN = 4;   // progress: status is a known enum number

// counters[]: ops/gpu_fold.py reads the same layout
constexpr int C_STATUS_ERR = 0, C_PROGRESS_ERR = 1, C_UNKNOWN_STATUS = 2, C_OTHER_TOPIC = 3, C_OVERFLOW = 4;
constexpr int C_HIST = 8, N_COUNTERS = C_HIST + 64;
static_assert(N_COUNTERS == 72, "ops/gpu_fold.py allocates N_COUNTERS = 72 counters");

constexpr int TOPIC_STATUS = 1, TOPIC_PROGRESS = 2;

template <int DIALECT>
__global__ __launch_bounds__(256) void fold_decode(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                   int n, uint64_t known_mask, FoldRow* __restrict__ rows,
                                                   uint32_t* __restrict__ counters, int32_t* __restrict__ overflow) {
  __shared__ uint32_t local[N_COUNTERS];
  for (int k = threadIdx.x; k < N_COUNTERS; k += blockDim.x) local[k] = 0;
  __syncthreads();
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m < n) {
    const int head = offs[m];
    const int start = head + 5;
    const int end = offs[m + 1];
    const int topic = buf[head + 4];
    FoldRow row{0, 0, 0, 0, 0};
    if (topic != TOPIC_STATUS && topic != TOPIC_PROGRESS) {
      atomicAdd(&local[C_OTHER_TOPIC], 1u);
    } else {
      const bool is_status = topic == TOPIC_STATUS;
      Row r;
      read_message<DIALECT, true>(buf, start, end, is_status, r);
      bool to_host = r.ok == OK_HOST;
      if (r.ok == OK_DECODED) {
        uint32_t high;
        row.hash = hash64_bytes(buf + r.id_off, r.id_len, high);
        to_host = high != 0;
        if (DIALECT == DIALECT_UPB && !is_status && !to_host)
          to_host = has_high_byte(buf + r.host_off, r.host_len);
      }
      if (to_host) {
        overflow[atomicAdd(&counters[C_OVERFLOW], 1u)] = m;  // at most one per frame: stays below n
      } else if (r.ok == OK_ERROR) {
        atomicAdd(&local[is_status ? C_STATUS_ERR : C_PROGRESS_ERR], 1u);
      } else {
        row.id_off = r.id_off;
        row.id_len = r.id_len;
        row.status = r.status;
        row.flags = F_GROUP | (is_status ? F_STATUS : 0u);
        if (!is_status) {
          const uint32_t s = static_cast<uint32_t>(r.status);
          if (s < 64u && ((known_mask >> s) & 1ull)) {
            row.flags |= F_KNOWN;
            atomicAdd(&local[C_HIST + s], 1u);
          } else {
            atomicAdd(&local[C_UNKNOWN_STATUS], 1u);
          }
        }
      }
    }
    rows[m] = row;
  }
  __syncthreads();
  for (int k = threadIdx.x; k < N_COUNTERS; k += blockDim.x)
    if (local[k]) atomicAdd(&counters[k], local[k]);
}

__global__ __launch_bounds__(256) void fold_group(const uint8_t* __restrict__ buf, const FoldRow* __restrict__ rows,
                                                  int n, uint32_t slot_mask, uint64_t hash_mask,
                                                  unsigned long long* __restrict__ claim,
                                                  unsigned long long* __restrict__ last,
                                                  uint32_t* __restrict__ counts) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const FoldRow row = rows[m];
  if (!(row.flags & F_GROUP)) return;
  const unsigned long long me = static_cast<unsigned long long>(m) + 1ull;
  const auto same_id = [&](unsigned long long owner) {
    const FoldRow o = rows[owner];
    return o.id_len == row.id_len && o.hash == row.hash && bytes_equal(buf + o.id_off, buf + row.id_off, row.id_len);
  };
  const uint32_t slot = claim_slot(claim, slot_mask, home_slot(row.hash, hash_mask, slot_mask), me, same_id).slot;
  if (row.flags & F_STATUS) {
    atomicAdd(&counts[3 * slot], 1u);
    atomicMax(&last[slot], (me << 32) | static_cast<uint32_t>(row.status));
  } else {
    atomicAdd(&counts[3 * slot + 1], 1u);
    if (row.flags & F_KNOWN) atomicAdd(&counts[3 * slot + 2], 1u);
  }
}

}  // namespace

// C ABI for ctypes (ops/gpu_fold.py). All pointers are device pointers from torch tensors on the
// caller's device; `stream` is the torch stream (hipStream_t); `dialect` 0 = upb, 1 = protobufjs.
//   buf, offs    the framed stream and its n + 1 frame starts (host-checked, see above)
//   known_mask   bit s set: s is a number of TelemetryStatusEntry (numbers outside 0-63 are unknown)
//   hash_mask    ANDed onto every hash before the home slot is taken (all ones in production;
//                tests pass small masks so that every probe chain collides)
//   rows         n FoldRow, written by pass A
//   counters     72 uint32, zeroed by the caller: errors, unknown, other, overflow count, histogram
//   overflow     n int32: the frames left to the host, in no particular order
//   claim, last  `slots` uint64 each, zeroed by the caller; counts: 3 * slots uint32, zeroed
//   slots        a power of two, at least 2n
//   passes       1 = pass A only, 2 = pass B only (over rows of an earlier call), 3 = both; the
//                probe times them apart, everything else passes 3
// Returns a hipError_t (hipErrorInvalidValue for an unknown dialect or a bad table size or `passes`).
// n == 0 launches nothing.
extern "C" __attribute__((visibility("default"))) int bh_fold_telemetry(
    const void* buf, const void* offs, int n, int dialect, unsigned long long known_mask,
    unsigned long long hash_mask, void* rows, void* counters, void* overflow, void* claim, void* last, void* counts,
    long long slots, int passes, void* stream) {
  if (n <= 0) return 0;
  if (dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) return static_cast<int>(hipErrorInvalidValue);
  if (slots < 2ll * n || slots > (1ll << 32) || (slots & (slots - 1)) != 0 || passes < 1 || passes > 3)
    return static_cast<int>(hipErrorInvalidValue);
  const int block = 256;
  const int grid = (n + block - 1) / block;
  auto s = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* rw = static_cast<FoldRow*>(rows);
  auto* c = static_cast<uint32_t*>(counters);
  auto* ov = static_cast<int32_t*>(overflow);
  if (passes & 1) {
    if (dialect == DIALECT_PROTOBUFJS)
      hipLaunchKernelGGL(fold_decode<DIALECT_PROTOBUFJS>, dim3(grid), dim3(block), 0, s, b, o, n, known_mask, rw, c,
                         ov);
    else
      hipLaunchKernelGGL(fold_decode<DIALECT_UPB>, dim3(grid), dim3(block), 0, s, b, o, n, known_mask, rw, c, ov);
  }
  hipError_t err = hipGetLastError();
  if (err != hipSuccess || !(passes & 2)) return static_cast<int>(err);
  hipLaunchKernelGGL(fold_group, dim3(grid), dim3(block), 0, s, b, rw, n, static_cast<uint32_t>(slots - 1), hash_mask,
                     static_cast<unsigned long long*>(claim), static_cast<unsigned long long*>(last),
                     static_cast<uint32_t*>(counts));
  return static_cast<int>(hipGetLastError());
}
