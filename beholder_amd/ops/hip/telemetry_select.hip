// Cut a framed telemetry stream down to selected frames on the GPU (gfx950): the device half of
// `python -m beholder_amd extract --device gpu` (beholder_amd/extract.py, ops/gpu_extract.py).
//
// Input is what the fold takes (telemetry_fold.hip): the capture as it lies in the file and
// `offs[n + 1]`, the frame starts from the host's one pass over the length headers. Output is a
// framed stream again: the kept frames byte for byte, in stream order, and their input indices.
//
// Three stages, each its own launch (or launches) on one stream:
//
//  mark, select_mark, one lane per frame. Reads the frame by its topic (telemetry_readers.hpp, upb in
//    its STRICT form) and evaluates the selector (telemetry_select.hpp decide). Writes
//    keep_len[m] = offs[m + 1] - offs[m] for a kept frame and 0 for a dropped one. Frames the device
//    does not decide go to an overflow list through an atomic cursor with keep_len 0; the host
//    decides them and scatters their lengths into keep_len before the scan.
//  scan, three launches: an exclusive prefix sum over (kept ? 1 : 0, keep_len[m]), both in one
//    64-bit add as count << 32 | bytes (the input is below 2^31 bytes and a frame holds at least 5).
//      scan_reduce   per block of 256 frames, the block's total;
//      scan_totals   one block scans the totals in tiles of 256 with a running carry, so any number
//                    of totals takes one launch; base[b] is block b's exclusive prefix, base[blocks]
//                    the grand total, which is all the host reads back before it sizes the output;
//      scan_apply    per block, the scan of its 256 frames in LDS plus base[b]: pos[m] is frame m's
//                    (output index << 32 | output byte offset); a kept frame also writes the
//                    compacted out_offs[k] and indices[k], the last frame out_offs[kept].
//  gather, one launch, two shapes (ops/gpu_extract.py picks; scripts/gpu_extract_probe.py times both):
//      gather_search one lane per 16 output bytes. The lane finds its frame by binary search in
//                    out_offs, walks on where its 16 bytes cross frame ends (frames hold at least 5
//                    bytes, so at most 3 times), and stores one aligned 16-byte word; only the last
//                    lane of the output stores bytes. Every lane of a wave writes, whatever the
//                    selectivity.
//      gather_walk   a wave takes 64 frames and copies the kept ones one after the other, lane b
//                    moving bytes b, b + 64, ... of the frame: consecutive lanes, consecutive bytes.
//    Both read source bytes one by one (source and destination are mutually misaligned) and only
//    bytes of kept frames, and write only [0, kept_bytes).
//
// Visibility is the fold's rule: within a launch workgroups meet only in atomics (the overflow
// cursor); every plain load reads what an earlier launch or the host wrote. No kernel waits for
// another workgroup, which is why the scan is three launches and not a single look-back pass.
#include "block_scan.hpp"
#include "telemetry_select.hpp"

namespace {

using namespace bh;

constexpr int BLOCK = 256;  // frames per block in mark and scan; ops/gpu_extract.py SCAN_BLOCK

template <int DIALECT>
__global__ __launch_bounds__(BLOCK) void select_mark(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                     int n, const SelectParams s,
                                                     const MediaEntry* __restrict__ table,
                                                     const uint8_t* __restrict__ blob, int32_t* __restrict__ keep_len,
                                                     uint32_t* __restrict__ cursor, int32_t* __restrict__ overflow) {
  const int m = blockIdx.x * blockDim.x + threadIdx.x;
  if (m >= n) return;
  const int head = offs[m];
  const int end = offs[m + 1];
  const int d = decide<DIALECT>(buf, head, end, s, table, blob);
  if (d == DECIDE_HOST) overflow[atomicAdd(cursor, 1u)] = m;  // at most one per frame: stays below n
  keep_len[m] = d == DECIDE_KEEP ? end - head : 0;
}

__device__ __forceinline__ uint64_t packed(int32_t len) {
  return len > 0 ? (1ull << 32) | static_cast<uint32_t>(len) : 0ull;
}

__global__ __launch_bounds__(BLOCK) void scan_reduce(const int32_t* __restrict__ keep_len, int n,
                                                     uint64_t* __restrict__ totals) {
  __shared__ uint64_t wave_sums[BLOCK / 64];
  const int m = blockIdx.x * BLOCK + threadIdx.x;
  uint64_t total;
  block_scan<BLOCK>(m < n ? packed(keep_len[m]) : 0ull, wave_sums, total);
  if (threadIdx.x == 0) totals[blockIdx.x] = total;
}

// One block. base[b] = totals[0] + ... + totals[b - 1] for b in [0, blocks]; base[blocks] is the sum.
__global__ __launch_bounds__(BLOCK) void scan_totals(const uint64_t* __restrict__ totals, int blocks,
                                                     uint64_t* __restrict__ base) {
  __shared__ uint64_t wave_sums[BLOCK / 64];
  uint64_t carry = 0;
  for (int tile = 0; tile < blocks; tile += BLOCK) {  // the trip count is the same for every thread
    const int b = tile + threadIdx.x;
    const uint64_t x = b < blocks ? totals[b] : 0ull;
    uint64_t total;
    const uint64_t incl = block_scan<BLOCK>(x, wave_sums, total);
    if (b < blocks) base[b] = carry + incl - x;
    carry += total;
  }
  if (threadIdx.x == 0) base[blocks] = carry;
}

__global__ __launch_bounds__(BLOCK) void scan_apply(const int32_t* __restrict__ keep_len, int n,
                                                    const uint64_t* __restrict__ base, uint64_t* __restrict__ pos,
                                                    int32_t* __restrict__ out_offs, int32_t* __restrict__ indices) {
  __shared__ uint64_t wave_sums[BLOCK / 64];
  const int m = blockIdx.x * BLOCK + threadIdx.x;
  const uint64_t x = m < n ? packed(keep_len[m]) : 0ull;
  uint64_t total;
  const uint64_t incl = block_scan<BLOCK>(x, wave_sums, total) + base[blockIdx.x];
  if (m >= n) return;
  const uint64_t excl = incl - x;
  pos[m] = excl;
  if (x) {
    const uint32_t k = static_cast<uint32_t>(excl >> 32);  // below the kept count, which is at most n
    out_offs[k] = static_cast<int32_t>(excl & 0xffffffffull);
    indices[k] = m;
  }
  if (m == n - 1) out_offs[incl >> 32] = static_cast<int32_t>(incl & 0xffffffffull);  // out_offs[kept] = kept bytes
}

// kept >= 1, kept_bytes = out_offs[kept] >= 5. Lane j owns output bytes [16 j, 16 j + 16).
__global__ __launch_bounds__(BLOCK) void gather_search(const uint8_t* __restrict__ buf,
                                                       const int32_t* __restrict__ offs,
                                                       const int32_t* __restrict__ out_offs,
                                                       const int32_t* __restrict__ indices, int kept, int kept_bytes,
                                                       uint8_t* __restrict__ out) {
  const long long first = (static_cast<long long>(blockIdx.x) * BLOCK + threadIdx.x) * 16;
  if (first >= kept_bytes) return;
  const int o0 = static_cast<int>(first);
  int lo = 0, hi = kept;  // out_offs[lo] <= o0 < out_offs[hi]: out_offs[0] = 0, out_offs[kept] = kept_bytes
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if (out_offs[mid] <= o0) lo = mid;
    else hi = mid;
  }
  int k = lo;
  int frame_end = out_offs[k + 1];
  int src = offs[indices[k]] + (o0 - out_offs[k]);
  const int count = kept_bytes - o0 < 16 ? kept_bytes - o0 : 16;
  uint32_t w[4] = {0, 0, 0, 0};
  BH_UNROLL
  for (int b = 0; b < 16; ++b) {
    if (b < count) {
      if (o0 + b == frame_end) {  // o0 + b < kept_bytes, so frame k + 1 exists
        ++k;
        frame_end = out_offs[k + 1];
        src = offs[indices[k]];
      }
      w[b >> 2] |= static_cast<uint32_t>(buf[src++]) << (8 * (b & 3));
    }
  }
  if (count == 16) {
    *reinterpret_cast<uint4*>(out + o0) = make_uint4(w[0], w[1], w[2], w[3]);  // out is 16-byte aligned (host-checked)
  } else {
    BH_UNROLL
    for (int b = 0; b < 16; ++b)
      if (b < count) out[o0 + b] = static_cast<uint8_t>(w[b >> 2] >> (8 * (b & 3)));
  }
}

// One wave per 64 frames; pos[m] & 0xffffffff is frame m's output byte offset.
__global__ __launch_bounds__(BLOCK) void gather_walk(const uint8_t* __restrict__ buf, const int32_t* __restrict__ offs,
                                                     const int32_t* __restrict__ keep_len,
                                                     const uint64_t* __restrict__ pos, int n,
                                                     uint8_t* __restrict__ out) {
  const int m = blockIdx.x * BLOCK + threadIdx.x;
  const int lane = threadIdx.x & 63;
  int len = 0, src = 0, dst = 0;
  if (m < n) {
    len = keep_len[m];
    src = offs[m];
    dst = static_cast<int>(pos[m] & 0xffffffffull);
  }
  unsigned long long todo = __ballot(len > 0);
  while (todo) {  // wave-uniform
    const int i = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int L = __shfl(len, i), s = __shfl(src, i), d = __shfl(dst, i);
    for (int b = lane; b < L; b += 64) out[d + b] = buf[s + b];
  }
}

hipError_t check(const void* a, const void* b) { return a && b ? hipSuccess : hipErrorInvalidValue; }

}  // namespace

// C ABI for ctypes (ops/gpu_extract.py). All pointers but `params` are device pointers from torch
// tensors on the caller's device; `stream` is the torch stream (hipStream_t). Each returns a
// hipError_t and launches nothing for n <= 0.

// mark. `params` is a host pointer to a SelectParams, copied into the kernel's arguments.
//   dialect      0 = upb, 1 = protobufjs
//   table, blob  the media table (params->slot_mask + 1 entries) and its id bytes
//   keep_len     n int32, written for every frame
//   cursor       one uint32, zeroed by the caller: the length of `overflow` afterwards
//   overflow     n int32: the frames left to the host, in no particular order
extern "C" __attribute__((visibility("default"))) int bh_select_mark(
    const void* buf, const void* offs, int n, int dialect, const void* params, const void* table, const void* blob,
    void* keep_len, void* cursor, void* overflow, void* stream) {
  if (n <= 0) return 0;
  if ((dialect != DIALECT_UPB && dialect != DIALECT_PROTOBUFJS) || !params || !table)
    return static_cast<int>(hipErrorInvalidValue);
  const SelectParams s = *static_cast<const SelectParams*>(params);
  if ((s.slot_mask & (s.slot_mask + 1u)) != 0) return static_cast<int>(hipErrorInvalidValue);  // 2^k - 1
  const int grid = (n + BLOCK - 1) / BLOCK;
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  const auto* t = static_cast<const MediaEntry*>(table);
  const auto* bl = static_cast<const uint8_t*>(blob);
  auto* kl = static_cast<int32_t*>(keep_len);
  auto* cu = static_cast<uint32_t*>(cursor);
  auto* ov = static_cast<int32_t*>(overflow);
  if (dialect == DIALECT_PROTOBUFJS)
    hipLaunchKernelGGL(select_mark<DIALECT_PROTOBUFJS>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, s, t, bl, kl, cu, ov);
  else
    hipLaunchKernelGGL(select_mark<DIALECT_UPB>, dim3(grid), dim3(BLOCK), 0, st, b, o, n, s, t, bl, kl, cu, ov);
  return static_cast<int>(hipGetLastError());
}

// scan. With blocks = ceil(n / 256):
//   totals       `blocks` uint64, scratch
//   base         `blocks + 1` uint64; base[blocks] = kept << 32 | kept_bytes afterwards
//   pos          n uint64: output index << 32 | output byte offset of every frame
//   out_offs     n + 1 int32: the first kept + 1 are the output's frame starts
//   indices      n int32: the first `kept` are the kept frames' input indices, ascending
extern "C" __attribute__((visibility("default"))) int bh_select_scan(
    const void* keep_len, int n, void* totals, void* base, void* pos, void* out_offs, void* indices, void* stream) {
  if (n <= 0) return 0;
  if (check(keep_len, totals) != hipSuccess || check(base, pos) != hipSuccess || check(out_offs, indices) != hipSuccess)
    return static_cast<int>(hipErrorInvalidValue);
  const int blocks = (n + BLOCK - 1) / BLOCK;
  auto st = static_cast<hipStream_t>(stream);
  const auto* kl = static_cast<const int32_t*>(keep_len);
  auto* tt = static_cast<uint64_t*>(totals);
  auto* bs = static_cast<uint64_t*>(base);
  hipLaunchKernelGGL(scan_reduce, dim3(blocks), dim3(BLOCK), 0, st, kl, n, tt);
  hipError_t err = hipGetLastError();
  if (err != hipSuccess) return static_cast<int>(err);
  hipLaunchKernelGGL(scan_totals, dim3(1), dim3(BLOCK), 0, st, tt, blocks, bs);
  err = hipGetLastError();
  if (err != hipSuccess) return static_cast<int>(err);
  hipLaunchKernelGGL(scan_apply, dim3(blocks), dim3(BLOCK), 0, st, kl, n, bs, static_cast<uint64_t*>(pos),
                     static_cast<int32_t*>(out_offs), static_cast<int32_t*>(indices));
  return static_cast<int>(hipGetLastError());
}

// gather. kept and kept_bytes are the scan's totals; `out` holds exactly kept_bytes and is 16-byte
// aligned. shape 0 = gather_search (reads out_offs, indices), 1 = gather_walk (reads keep_len, pos).
// kept == 0 launches nothing.
extern "C" __attribute__((visibility("default"))) int bh_select_gather(
    const void* buf, const void* offs, int n, const void* keep_len, const void* pos, const void* out_offs,
    const void* indices, int kept, int kept_bytes, void* out, int shape, void* stream) {
  if (n <= 0 || kept == 0) return 0;
  if (kept < 0 || kept > n || kept_bytes < 5 || !out || (reinterpret_cast<uintptr_t>(out) & 15) != 0 ||
      (shape != 0 && shape != 1))
    return static_cast<int>(hipErrorInvalidValue);
  auto st = static_cast<hipStream_t>(stream);
  const auto* b = static_cast<const uint8_t*>(buf);
  const auto* o = static_cast<const int32_t*>(offs);
  auto* dst = static_cast<uint8_t*>(out);
  if (shape == 0) {
    const long long lanes = (static_cast<long long>(kept_bytes) + 15) / 16;
    const int grid = static_cast<int>((lanes + BLOCK - 1) / BLOCK);
    hipLaunchKernelGGL(gather_search, dim3(grid), dim3(BLOCK), 0, st, b, o, static_cast<const int32_t*>(out_offs),
                       static_cast<const int32_t*>(indices), kept, kept_bytes, dst);
  } else {
    const int grid = (n + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(gather_walk, dim3(grid), dim3(BLOCK), 0, st, b, o, static_cast<const int32_t*>(keep_len),
                       static_cast<const uint64_t*>(pos), n, dst);
  }
  return static_cast<int>(hipGetLastError());
}
