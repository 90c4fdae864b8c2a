// The per-frame code of `transitions` (beholder_amd/transitions.py), shared by the classify and pairs
// kernels (telemetry_transitions.hip) and a host program for CPU tests
// (tests/native/transitions_host.cpp): like telemetry_select.hpp and telemetry_shard.hpp, this header
// also compiles with a plain C++17 compiler (BH_FN), so the same code runs under ASan/UBSan on a CPU.
//
// classify<DIALECT>(buf, head, end, ev) answers for the frame buf[head, end)
// (`u32 L | u8 topic | body`): TR_SKIP for a frame of another topic than 1, which is not read at all;
// TR_ERROR where the CPU codec raises; TR_HOST where the device does not decide and the host decodes
// instead; TR_EVENT for a status event, with its id span, the fold's hash of the id and its status in
// `ev`. The rule for TR_HOST is the fold's, for a TelemetryStatus: a decoded id with a byte >= 0x80,
// whose identity is the decoded string, and in the upb dialect a start-group.
//
// class_of(status, known_mask) is the class of a status number: the number where its bit is set in
// known_mask (ops/gpu_fold.py known_mask of the enum's numbers, all in 0-63), CLASS_UNKNOWN for every
// other int32.
#pragma once
#include "telemetry_select.hpp"

namespace bh {

constexpr int TR_SKIP = 0, TR_ERROR = 1, TR_HOST = 2, TR_EVENT = 3;
constexpr uint32_t CLASS_UNKNOWN = 64;
constexpr uint32_t CLASSES = 65;  // 0-63 and CLASS_UNKNOWN: the matrix is CLASSES x CLASSES

struct StatusEvent {
  uint64_t hash;   // hash64_bytes of the id bytes
  int32_t id_off;  // absolute in buf
  int32_t id_len;
  int32_t status;
  int32_t kind;    // TR_*
};
static_assert(sizeof(StatusEvent) == 24, "ops/gpu_transitions.py views the rows as (n, 6) int32");

BH_FN uint32_t class_of(int32_t status, uint64_t known_mask) {
  const uint32_t s = static_cast<uint32_t>(status);
  return (s < 64u && ((known_mask >> (s & 63u)) & 1ull)) ? s : CLASS_UNKNOWN;
}

template <int DIALECT>
BH_FN int classify(const uint8_t* __restrict__ buf, const int head, const int end, StatusEvent& ev) {
  ev = StatusEvent{0, 0, 0, 0, TR_SKIP};
  if (buf[head + 4] != 1) return TR_SKIP;
  Row r;
  const int start = head + 5;
  read_message<DIALECT, true>(buf, start, end, true, r);
  int kind = r.ok == OK_HOST ? TR_HOST : r.ok == OK_DECODED ? TR_EVENT : TR_ERROR;
  if (kind == TR_EVENT) {
    uint32_t high;
    ev.hash = hash64_bytes(buf + r.id_off, r.id_len, high);
    if (high) {
      kind = TR_HOST;
      ev.hash = 0;
    } else {
      ev.id_off = r.id_off;
      ev.id_len = r.id_len;
      ev.status = r.status;
    }
  }
  ev.kind = kind;
  return kind;
}

}  // namespace bh
