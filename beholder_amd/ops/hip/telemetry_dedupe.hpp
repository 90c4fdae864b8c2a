// The per-frame code of `dedupe` (beholder_amd/dedupe.py): what kind of frame this is, the hash of
// its content and whether two contents are equal bytes. Shared by the kernels
// (telemetry_dedupe.hip) and a host program for CPU tests (tests/native/dedupe_host.cpp): like
// telemetry_coalesce.hpp, this header also compiles with a plain C++17 compiler (BH_FN), so the same
// code runs under ASan/UBSan on a CPU.
//
// A frame is `u32 L | u8 topic | body`; its content is the L bytes after the header. Nothing is
// decoded. dedupe_kind(buf, head, end, params) answers for the frame buf[head, end):
//   DK_KEEP  its topic byte is not selected: kept as it is, equals nothing. Only that byte is read.
//   DK_HOST  its content is longer than DEDUPE_DEVICE_MAX: the host decides it.
//   DK_ROW   it takes part on the device.
// DEDUPE_DEVICE_MAX is a safety condition, not a tuning number: it bounds every lane's hash loop
// and compare loop to 4,096 steps whatever the capture holds. A single frame may otherwise be close
// to 2^31 bytes, and one lane walking it would look like a hang.
//
// content_hash and content_equal exist in two forms that give the same answers. The plain one
// reads byte by byte. The wide one (WIDE) reads 8 bytes at a time at whatever address the content
// starts, through __builtin_memcpy, which gfx950 compiles to one global_load_dwordx2 (the hardware
// takes unaligned global addresses), and finishes the last 0-7 bytes one by one: it never reads a
// byte outside the content, so there is no over-read to reason about at the end of the buffer.
#pragma once
#include "media_table.hpp"

namespace bh {

constexpr int DEDUPE_DEVICE_MAX = 4096;

constexpr int DK_KEEP = 0, DK_ROW = 1, DK_HOST = 2;

// DedupeParams::flags
constexpr uint32_t DF_FIRST = 1;  // keep=first: the smallest index of a content wins (else the largest)
constexpr uint32_t DF_WIDE = 2;   // the 8-byte forms of the hash loop and the compare loop

struct DedupeParams {
  uint64_t topics[4];  // bit t of the 256: frames of topic byte t take part
  uint64_t hash_mask;  // ANDed onto the hash before the home slot is taken (all ones in production)
  uint32_t slot_mask;  // table slots - 1
  uint32_t flags;      // DF_* bits
};
static_assert(sizeof(DedupeParams) == 48, "ops/gpu_dedupe.py DedupeParams mirrors this layout");

BH_FN int dedupe_kind(const uint8_t* __restrict__ buf, const int head, const int end, const DedupeParams& s) {
  const uint32_t topic = buf[head + 4];
  if (((s.topics[topic >> 6] >> (topic & 63u)) & 1ull) == 0) return DK_KEEP;
  return end - head - 4 > DEDUPE_DEVICE_MAX ? DK_HOST : DK_ROW;
}

BH_FN uint64_t load8(const uint8_t* p) {
  uint64_t w;
  __builtin_memcpy(&w, p, 8);  // little-endian: byte k of the content is bits 8k..8k+7
  return w;
}

// The fold's hash (media_table.hpp hash64_bytes) over the n bytes at p: ops/gpu_dedupe.py frame_hash
// is the same. It only orders the probe; no result depends on it.
template <bool WIDE>
BH_FN uint64_t content_hash(const uint8_t* __restrict__ p, const int n) {
  if (!WIDE) {
    uint32_t high;
    return hash64_bytes(p, n, high);
  }
  uint64_t h = 0xcbf29ce484222325ull;
  int k = 0;
  for (; k + 8 <= n; k += 8) {
    uint64_t w = load8(p + k);
    BH_UNROLL
    for (int j = 0; j < 8; ++j) {
      h = (h ^ (w & 0xffu)) * 0x100000001b3ull;
      w >>= 8;
    }
  }
  for (; k < n; ++k) h = (h ^ p[k]) * 0x100000001b3ull;
  return finalise64(h);
}

// Whether the n bytes at a and at b are equal. The two may overlap or be the same bytes.
template <bool WIDE>
BH_FN bool content_equal(const uint8_t* a, const uint8_t* b, const int n) {
  int k = 0;
  if (WIDE) {
    for (; k + 8 <= n; k += 8)
      if (load8(a + k) != load8(b + k)) return false;
  }
  for (; k < n; ++k)
    if (a[k] != b[k]) return false;
  return true;
}

}  // namespace bh
